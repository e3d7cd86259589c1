"""CPU: the route of an elastic-net sweep (viprs_enet_route, viprs_amd/csrc/sweep_route.cpp) over everything it depends on,
and viprs_sweep_route answering as before for every configuration tests/test_sweep_route.py enumerates."""
import itertools

import pytest

from tests import test_sweep_route as SR
from viprs_amd import _lib as L


def test_enet_route_table():
    for grid, ld, dense, ragged, band_ok in itertools.product((False, True), SR.LD_TYPES, *[(False, True)] * 3):
        cfg = (grid, ld, dense, ragged, band_ok)
        if ragged and not band_ok:
            with pytest.raises(NotImplementedError, match="elastic-net sweep: windowed LD blocks"):
                L.enet_route(*cfg)
            continue
        if dense and ld not in SR.THREE_TYPES:
            with pytest.raises(ValueError, match="dense schedule with unsupported LD dtype"):
                L.enet_route(*cfg)
            continue
        if ragged and ld not in SR.THREE_TYPES:
            with pytest.raises(ValueError, match="band schedule with unsupported LD dtype"):
                L.enet_route(*cfg)
            continue
        got = L.enet_route(*cfg)
        want = dict(dense_family=SR.PANEL if dense else SR.NONE, ragged_family=SR.BAND if ragged else SR.NONE,
                    prologue=int(not (dense and not ragged)), prologue_per_model=int(grid), start_event_by_launcher=int(dense),
                    whole_sweep_events=int(not grid and not (dense and not ragged)), dense_bracketed=int(grid or dense))
        if dense:
            want["dense_model"] = L.PANEL_ELASTIC_NET
        if ragged:
            want["ragged_model"] = L.BAND_ELASTIC_NET
        for k, v in want.items():
            assert got[k] == v, (cfg, k, got)
        assert L.PANEL_ELASTIC_NET == 4 and L.BAND_ELASTIC_NET == 3
        # prologue and events are those of the E-step's row for the same lists: spike-and-slab for width 1, grid for a grid
        # state (as panel items: grid_mfma off)
        ref = L.sweep_route(L.F32, L.MODEL_GRID if grid else L.MODEL_SPIKE_SLAB, 3 if grid else 1, ld, dense, ragged, True, False)
        if dense or not grid:                    # (a grid state without dense blocks: the E-step calls the generic launcher)
            for k in ("prologue", "prologue_per_model", "start_event_by_launcher", "whole_sweep_events", "dense_bracketed"):
                assert got[k] == ref[k], (cfg, k)
        assert got["whole_sweep_events"] or got["dense_bracketed"], cfg


def test_enet_route_rejects_a_null_output():
    assert L.lib.viprs_enet_route(0, L.LD_F32, 1, 0, 1, None) == L.EINVAL


@pytest.mark.parametrize("f32", [True, False], ids=["f32", "f64"])
@pytest.mark.parametrize("row, model, width", SR.MODELS, ids=[f"{m[0]}-{m[2]}" for m in SR.MODELS])
def test_sweep_route_answers_as_before(f32, row, model, width):
    SR.test_route_table(f32, row, model, width)


def test_sweep_route_still_refuses_model_kind_3():
    SR.test_route_rejects_bad_arguments()
    with pytest.raises(ValueError, match="model kind"):
        L.sweep_route(L.F32, 3, 1, L.LD_F32, 1, 0)
