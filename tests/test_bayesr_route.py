"""CPU: the route of an SBayesR sweep (viprs_bayesr_route, viprs_amd/csrc/sweep_route.cpp) over everything it depends on, and
the other routes answering as before."""
import itertools

import pytest

from tests import test_gibbs_route as GR
from tests import test_sweep_route as SR
from viprs_amd import _lib as L


def test_bayesr_route_table():
    assert L.PANEL_BAYESR == 6 and L.BAND_BAYESR == 5
    for ld, dense, ragged, band_ok in itertools.product(SR.LD_TYPES, *[(False, True)] * 3):
        cfg = (ld, dense, ragged, band_ok)
        if ragged and not band_ok:
            with pytest.raises(ValueError, match="SBayesR sweep: windowed LD blocks"):
                L.bayesr_route(*cfg)
            continue
        if dense and ld not in SR.THREE_TYPES:
            with pytest.raises(ValueError, match="dense schedule with unsupported LD dtype"):
                L.bayesr_route(*cfg)
            continue
        if ragged and ld not in SR.THREE_TYPES:
            with pytest.raises(ValueError, match="band schedule with unsupported LD dtype"):
                L.bayesr_route(*cfg)
            continue
        got = L.bayesr_route(*cfg)
        want = dict(dense_family=SR.PANEL if dense else SR.NONE, ragged_family=SR.BAND if ragged else SR.NONE,
                    prologue=int(not (dense and not ragged)), prologue_per_model=0, start_event_by_launcher=int(dense),
                    whole_sweep_events=0, dense_bracketed=1)
        if dense:
            want["dense_model"] = L.PANEL_BAYESR
        if ragged:
            want["ragged_model"] = L.BAND_BAYESR
        for k, v in want.items():
            assert got[k] == v, (cfg, k, got)
        # prologue and events are those of the E-step's mixture row (K <= 8: panel sweep and band kernel) for the same lists
        # (that row also calls the row-by-row family on an empty windowed list; this route calls nothing)
        if dense:
            ref = L.sweep_route(L.F32, L.MODEL_MIXTURE, 3, ld, dense, ragged, True, False)
            for k in ("dense_family", "prologue", "prologue_per_model", "start_event_by_launcher", "whole_sweep_events",
                      "dense_bracketed"):
                assert got[k] == ref[k], (cfg, k)


def test_bayesr_route_rejects_a_null_output():
    assert L.lib.viprs_bayesr_route(L.LD_F32, 1, 0, 1, None) == L.EINVAL


def test_the_other_routes_answer_as_before():
    GR.test_gibbs_route_table()
    GR.test_the_other_routes_answer_as_before()
