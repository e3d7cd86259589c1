"""CPU: the host side of the spectrum feature (viprs_amd/stats/spectrum.py) -- the ridge penalty from the extremal eigenvalues,
the `LDArrays.set_extremal` path, attaching the extremes to a zarr store (in memory and in its `.zattrs`), and the argument
checks of `lambda_min='compute'` that need no device."""
import json
import os

import numpy as np
import pytest

from viprs_amd.data import ArrayDataLoader, LDArrays
from viprs_amd.io import zarr_ld as Z
from viprs_amd.plan import SpectrumInfo
from viprs_amd.stats import spectrum as S
from viprs_amd.utils import synthetic as syn


def test_lambda_min_from_extremes():
    r = 1e-3
    for lam_min, lam_max in ((-0.25, 40.0), (0.5, 40.0), (0.01, 40.0), (-0.152, 34.1)):
        assert S.lambda_min_from_extremes(lam_min, lam_max) == max(-lam_min, 0.0)
        assert S.lambda_min_from_extremes(lam_min, lam_max, 0.0, "one_plus_r") == max(-lam_min, 0.0)
        assert S.lambda_min_from_extremes(lam_min, None, r) == max(-lam_min, 0.0)           # no maximum: no ratio
        assert S.lambda_min_from_extremes(lam_min, lam_max, r, "one_plus_r") == \
            pytest.approx(max((r * lam_max - lam_min) / (1 + r), 0.0), rel=1e-15)
        x = S.lambda_min_from_extremes(lam_min, lam_max, r, "one_minus_r")
        assert x == pytest.approx(max((r * lam_max - lam_min) / (1 - r), 0.0), rel=1e-15)
        if x > 0.0:                                                                          # what the formula solves
            assert (lam_min + x) == pytest.approx(r * (lam_max + x), rel=1e-12)
        for formula in (None, "something"):
            with pytest.raises(S.UnpinnedLambdaMinError, match="check_store"):
                S.lambda_min_from_extremes(lam_min, lam_max, r, formula)
    assert S.lambda_min_from_extremes(2.0, 2.0) == 0.0                                       # positive definite: no ridge
    assert S.lambda_min_from_extremes(30.0, 40.0, 0.1, "one_minus_r") == 0.0                 # the ratio already holds
    assert Z.UnpinnedLambdaMinError is S.UnpinnedLambdaMinError and issubclass(S.UnpinnedLambdaMinError, NotImplementedError)


def test_ld_arrays_set_extremal():
    sym = syn.make_ld([30, 20], low_memory=False, ld_dtype=np.float32)
    ld = LDArrays(symmetric=(sym.ld_left_bound, sym.ld_indptr, sym.ld_data), lambda_min=0.125)
    assert ld.get_lambda_min() == 0.125 and ld.get_lambda_min(min_max_ratio=0.0) == 0.125    # before: the stored number
    ld.set_extremal(-0.2, 30.0)
    assert ld.get_lambda_min(min_max_ratio=0.0) == 0.2
    with pytest.raises(S.UnpinnedLambdaMinError):
        ld.get_lambda_min()
    assert ld.get_lambda_min(formula="one_plus_r") == pytest.approx((0.03 + 0.2) / 1.001)
    ld.lambda_min_formula = "one_minus_r"
    assert ld.get_lambda_min(min_max_ratio=1e-3) == pytest.approx((0.03 + 0.2) / 0.999)
    assert LDArrays.lambda_min_formula is None


def test_attach_extremal_to_a_store_and_its_zattrs(tmp_path):
    up = syn.make_ld([30, 20], low_memory=True, ld_dtype=np.int8, seed=3)
    path = str(tmp_path / "chr_1")
    Z.write_ld_store(path, up.ld_indptr, up.ld_data, attrs={"Chromosome": 1, "Sample size": 1000})
    m = Z.ZarrLDMatrix(path)
    assert m.get_lambda_min(min_max_ratio=1e-3) == 0.0                                       # no spectrum in the store
    S.attach_extremal(m, -0.25, 40.0)
    assert m.attrs["Spectral properties"]["Extremal"] == {"min": -0.25, "max": 40.0}
    assert m.get_lambda_min() == 0.25 and m.get_lambda_min(min_max_ratio=1e-3, formula="one_plus_r") == \
        pytest.approx((0.04 + 0.25) / 1.001)
    assert "Spectral properties" not in json.load(open(os.path.join(path, ".zattrs")))       # in memory only
    assert Z.ZarrLDMatrix(path).get_lambda_min() == 0.0
    S.attach_extremal(m, -0.25, 40.0, write=True)
    on_disk = json.load(open(os.path.join(path, ".zattrs")))
    assert on_disk == {"Chromosome": 1, "Sample size": 1000, "Spectral properties": {"Extremal": {"min": -0.25, "max": 40.0}}}
    again = Z.ZarrLDMatrix(path)
    assert again.get_lambda_min() == 0.25 and again.chromosome == 1
    assert np.array_equal(again.load().ld_data, up.ld_data)
    # other spectral attributes of a store stay
    S.attach_extremal(again, -0.5, 41.0, write=True)
    again.attrs["Spectral properties"]["Rank"] = 7
    S.attach_extremal(again, -0.5, 42.0)
    assert again.attrs["Spectral properties"] == {"Extremal": {"min": -0.5, "max": 42.0}, "Rank": 7}
    with pytest.raises(ValueError, match="store directory"):
        S.attach_extremal(LDArrays(upper=(up.ld_left_bound, up.ld_indptr, up.ld_data)), 0.0, 1.0, write=True)
    with pytest.raises(TypeError, match="set_extremal"):
        S.attach_extremal(object(), 0.0, 1.0)


def test_spectrum_info_and_plan_summary():
    info = SpectrumInfo([0.5, -0.1, 0.9], [3.0, 9.0, 2.0], [0, 0, 0], [0, 0, 0], [4, 8, 2], [0, 0, 1], ms=1.5)
    assert not info.converged and info.iterations.dtype == np.int32 and "min=-0.1" in repr(info) and info.MAXITER == 1

    class Plan:
        m = 60

        def blocks(self):
            return np.array([0, 10, 30, 60]), np.zeros(3, np.int32)

        def extremal_eigenvalues(self, **kw):
            assert kw == {"rtol": 1e-3}
            return info

    whole = S.plan_spectrum(Plan(), rtol=1e-3)[None]
    assert (whole["min"], whole["max"]) == (-0.1, 9.0) and whole["per_block"].status.tolist() == [0, 0, 1]
    parts = S.plan_spectrum(Plan(), {1: (0, 30), 2: (30, 60), 3: (60, 60)}, rtol=1e-3)
    assert (parts[1]["min"], parts[1]["max"]) == (-0.1, 9.0) and parts[1]["per_block"].converged
    assert (parts[2]["min"], parts[2]["max"]) == (0.9, 2.0) and not parts[2]["per_block"].converged
    assert (parts[3]["min"], parts[3]["max"]) == (1.0, 1.0)


def test_compute_needs_a_device_and_one_rank():
    from viprs_amd.model import VIPRS, VIPRSPerChromosome
    gdl = ArrayDataLoader.synthetic({1: [40, 25], 2: [33]}, ld_dtype=np.int8, kind="longrange")
    for cls in (VIPRS, VIPRSPerChromosome):
        with pytest.raises(RuntimeError, match="HIP device"):
            cls(gdl, lambda_min="compute", e_step_fn=lambda *a: None)

    class TwoRanks:
        world_size, rank = 2, 0
    with pytest.raises(NotImplementedError, match="annotate_spectrum"):
        VIPRS(gdl, lambda_min="compute", comm=TwoRanks())
    # annotated LD: 'infer' reaches every model class through the LD objects, no device involved
    for c, (lo, hi) in {1: (-0.3, 20.0), 2: (0.2, 10.0)}.items():
        gdl.ld[c].set_extremal(lo, hi)
        gdl.ld[c].lambda_min_formula = "one_minus_r"
    hook = lambda *a: None
    assert VIPRS(gdl, lambda_min="infer", e_step_fn=hook).lambda_min == 0.0      # (chromosome 2: 1e-3 x 10 - 0.2 < 0)
    assert VIPRSPerChromosome(gdl, lambda_min="infer", e_step_fn=hook)._lambda_group == \
        [pytest.approx((0.02 + 0.3) / 0.999), 0.0]
