"""CPU: the route of an LDpred2 Gibbs sweep (viprs_gibbs_route, viprs_amd/csrc/sweep_route.cpp) over everything it depends on,
and viprs_sweep_route / viprs_enet_route answering as before."""
import itertools

import pytest

from tests import test_enet_route as ER
from tests import test_sweep_route as SR
from viprs_amd import _lib as L
from viprs_amd.stats import gibbs as GB


def test_gibbs_route_table():
    assert L.PANEL_GIBBS == 5 and L.BAND_GIBBS == 4
    for ld, dense, ragged, band_ok in itertools.product(SR.LD_TYPES, *[(False, True)] * 3):
        cfg = (ld, dense, ragged, band_ok)
        if ragged and not band_ok:
            with pytest.raises(ValueError, match="Gibbs sweep: windowed LD blocks"):
                L.gibbs_route(*cfg)
            continue
        if dense and ld not in SR.THREE_TYPES:
            with pytest.raises(ValueError, match="dense schedule with unsupported LD dtype"):
                L.gibbs_route(*cfg)
            continue
        if ragged and ld not in SR.THREE_TYPES:
            with pytest.raises(ValueError, match="band schedule with unsupported LD dtype"):
                L.gibbs_route(*cfg)
            continue
        got = L.gibbs_route(*cfg)
        assert got == GB.gibbs_route(*cfg)
        want = dict(dense_family=SR.PANEL if dense else SR.NONE, ragged_family=SR.BAND if ragged else SR.NONE,
                    prologue=int(not (dense and not ragged)), prologue_per_model=1, start_event_by_launcher=int(dense),
                    whole_sweep_events=0, dense_bracketed=1)
        if dense:
            want["dense_model"] = L.PANEL_GIBBS
        if ragged:
            want["ragged_model"] = L.BAND_GIBBS
        for k, v in want.items():
            assert got[k] == v, (cfg, k, got)
        # prologue and events are those of the E-step's grid row for the same lists (as panel items: grid_mfma off), and
        # of the elastic-net route of a grid state
        if dense:
            ref = L.sweep_route(L.F32, L.MODEL_GRID, 3, ld, dense, ragged, True, False)
            for k in ("prologue", "prologue_per_model", "start_event_by_launcher", "whole_sweep_events", "dense_bracketed"):
                assert got[k] == ref[k], (cfg, k)
        enet = L.enet_route(True, ld, dense, ragged, band_ok)
        for k in ("dense_family", "ragged_family", "prologue", "prologue_per_model", "start_event_by_launcher",
                  "whole_sweep_events", "dense_bracketed"):
            assert got[k] == enet[k], (cfg, k)


def test_gibbs_route_rejects_a_null_output():
    assert L.lib.viprs_gibbs_route(L.LD_F32, 1, 0, 1, None) == L.EINVAL


def test_the_other_routes_answer_as_before():
    ER.test_enet_route_table()
    for f32 in (True, False):
        for row, model, width in SR.MODELS:
            SR.test_route_table(f32, row, model, width)
