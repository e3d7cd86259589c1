"""CPU: the route of an E-step sweep (viprs_sweep_route, viprs_amd/csrc/sweep_route.cpp) -- which kernel family serves the
dense and the windowed blocks, whether the prologue launch is needed and which HIP events the sweep records -- against the
table written out below, over the full cross product of what the route depends on."""
import itertools

import pytest

from viprs_amd import _lib as L

NONE, GENERIC, TILE_F64, PANEL, BAND, BATCHED = (L.FAMILY_NONE, L.FAMILY_GENERIC, L.FAMILY_TILE_F64, L.FAMILY_PANEL,
                                                 L.FAMILY_BAND, L.FAMILY_GRID_BATCHED)
SPIKE_SLAB, MIXTURE, GRID = L.MODEL_SPIKE_SLAB, L.MODEL_MIXTURE, L.MODEL_GRID
LD_TYPES = (L.LD_I8, L.LD_I16, L.LD_I32, L.LD_I64, L.LD_F32, L.LD_F64)
THREE_TYPES = (L.LD_F32, L.LD_I8, L.LD_I16)                 # what the panel, band and batched grid kernels are built for
# (name of the table row, model kind, width)
MODELS = [("spike_slab", SPIKE_SLAB, 1), ("mixture_narrow", MIXTURE, 1), ("mixture_narrow", MIXTURE, 8),
          ("mixture_wide", MIXTURE, 9), ("mixture_wide", MIXTURE, 31), ("mixture_generic", MIXTURE, 32), ("grid", GRID, 7)]

# fp32 states.  dense: {(dense non-empty, grid_mfma): (family, model constant)}; ragged: {(ragged non-empty, band_ok): ...};
# no_prologue: the (dense non-empty, ragged non-empty, grid_mfma) for which the prologue launch is skipped;
# by_launcher: the (dense non-empty) for which the launcher records the start event.
F32 = {
    "spike_slab": dict(
        dense={(True, False): (PANEL, 0), (True, True): (PANEL, 0), (False, False): (NONE, None), (False, True): (NONE, None)},
        ragged={(True, True): (BAND, 0), (True, False): (GENERIC, SPIKE_SLAB), (False, True): (NONE, None), (False, False): (NONE, None)},
        no_prologue={(True, False, False), (True, False, True)}, by_launcher={True}),
    "mixture_narrow": dict(
        dense={(True, False): (PANEL, 2), (True, True): (PANEL, 2), (False, False): (GENERIC, MIXTURE), (False, True): (GENERIC, MIXTURE)},
        ragged={(True, True): (BAND, 2), (True, False): (GENERIC, MIXTURE), (False, True): (GENERIC, MIXTURE), (False, False): (GENERIC, MIXTURE)},
        no_prologue={(True, False, False), (True, False, True)}, by_launcher={True}),
    "mixture_wide": dict(
        dense={(True, False): (PANEL, 3), (True, True): (PANEL, 3), (False, False): (GENERIC, MIXTURE), (False, True): (GENERIC, MIXTURE)},
        ragged={(True, True): (GENERIC, MIXTURE), (True, False): (GENERIC, MIXTURE), (False, True): (GENERIC, MIXTURE), (False, False): (GENERIC, MIXTURE)},
        no_prologue={(True, False, False), (True, False, True)}, by_launcher={True}),
    "mixture_generic": dict(
        dense={(True, False): (GENERIC, MIXTURE), (True, True): (GENERIC, MIXTURE), (False, False): (GENERIC, MIXTURE), (False, True): (GENERIC, MIXTURE)},
        ragged={(True, True): (GENERIC, MIXTURE), (True, False): (GENERIC, MIXTURE), (False, True): (GENERIC, MIXTURE), (False, False): (GENERIC, MIXTURE)},
        no_prologue=set(), by_launcher=set()),
    "grid": dict(
        dense={(True, False): (PANEL, 1), (True, True): (BATCHED, None), (False, False): (GENERIC, GRID), (False, True): (GENERIC, GRID)},
        ragged={(True, True): (BAND, 1), (True, False): (GENERIC, GRID), (False, True): (GENERIC, GRID), (False, False): (GENERIC, GRID)},
        no_prologue={(True, False, False)}, by_launcher={True}),
}


def expected(f32, row, model, ld, dense, ragged, band_ok, grid_mfma, row_by_row):
    """The route the table gives, or the message of the error it gives."""
    if f32:
        t = F32[row]
        d, r = t["dense"][(dense, grid_mfma)], t["ragged"][(ragged, band_ok)]
        if d[0] in (PANEL, BATCHED) and ld not in THREE_TYPES:
            return "dense schedule with unsupported LD dtype"
        if r[0] == BAND and ld not in THREE_TYPES:
            return "band schedule with unsupported LD dtype"
        prologue = (dense, ragged, grid_mfma) not in t["no_prologue"]
        by_launcher = dense in t["by_launcher"]
    else:
        d = r = (GENERIC if row_by_row else TILE_F64, model)
        prologue, by_launcher = True, False
    if row == "spike_slab":
        # ev[2] .. ev[3] around the dense launcher when there are dense blocks; ev[0] .. ev[1] around everything unless the
        # sweep is fp32 with dense blocks only
        whole, bracketed = not (f32 and dense and not ragged), dense
        by_launcher = by_launcher and dense
    else:
        whole, bracketed = False, True                  # one bracket around all kernels of the call
    return dict(dense_family=d[0], dense_model=d[1], ragged_family=r[0], ragged_model=r[1], prologue=int(prologue),
                prologue_per_model=int(model == GRID), start_event_by_launcher=int(by_launcher),
                whole_sweep_events=int(whole), dense_bracketed=int(bracketed))


@pytest.mark.parametrize("f32", [True, False], ids=["f32", "f64"])
@pytest.mark.parametrize("row, model, width", MODELS, ids=[f"{m[0]}-{m[2]}" for m in MODELS])
def test_route_table(f32, row, model, width):
    n = 0
    for ld, dense, ragged, band_ok, grid_mfma, row_by_row in itertools.product(LD_TYPES, *[(False, True)] * 5):
        cfg = (L.F32 if f32 else L.F64, model, width, ld, dense, ragged, band_ok, grid_mfma, row_by_row)
        want = expected(f32, row, model, ld, dense, ragged, band_ok, grid_mfma, row_by_row)
        if isinstance(want, str):
            with pytest.raises(ValueError, match=want):
                L.sweep_route(*cfg)
            continue
        got = L.sweep_route(*cfg)
        for k, v in want.items():
            assert v is None or got[k] == v, (cfg, k, got, want)
        # what the three predicates of the old schedule were meant to keep
        if got["start_event_by_launcher"]:
            assert got["dense_family"] in (PANEL, BATCHED), cfg
        if not got["prologue"]:
            assert got["dense_family"] == PANEL and (got["ragged_family"] == NONE or not ragged), cfg
        if model != SPIKE_SLAB:
            assert not got["whole_sweep_events"], cfg
        assert got["whole_sweep_events"] or got["dense_bracketed"], cfg      # some bracket stands for the whole sweep
        n += 1
    assert n > 0


def test_route_rejects_bad_arguments():
    for cfg in [(2, SPIKE_SLAB, 1, L.LD_F32, 1, 0), (L.F32, 3, 1, L.LD_F32, 1, 0), (L.F32, MIXTURE, 0, L.LD_F32, 1, 0)]:
        with pytest.raises(ValueError):
            L.sweep_route(*cfg)
