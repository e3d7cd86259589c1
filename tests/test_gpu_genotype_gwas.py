"""Per-genotype-class column sums on the device (`viprs_genotypes_class_sums`, include/viprs_hip.h; kernel:
viprs_amd/csrc/geno_class_sums.h) against the host replay of the header's order (tests/genotype_gwas_reference.py), with `==`;
`association`, `perform_gwas` and the loader form of the pseudo_validation criterion on the device.

Shapes: n straddles a byte, a lane's 16-sample word (15, 16, 17), the 64-sample unit of the row stride (63, 64, 65), a round
of 64 words (1023, 1024, 1025) and reaches a third round (2049); m straddles the R rows of a wavefront and reaches a third
group; n_cols straddles the W columns of the widest instantiation and runs all of W, W / 2 and 1 in one call (2 W + 1 runs
two groups of W and one of 1, W - 1 = 3 one of 2 and one of 1)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import genotype_gwas_reference as R
from viprs_amd import genotypes as G
from viprs_amd.io.plink_bed import pack_codes

pytestmark = pytest.mark.gpu

ROWS, COLS = 4, 4                        # R and W of the kernel (checked against its source below)
N_SIZES = [1, 3, 4, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2049]
M_SIZES = [1, 2, ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 1]
COL_SIZES = [1, 2, 3, COLS, COLS + 1, 2 * COLS + 1]


def _first_difference(got, want):
    if got.dtype != want.dtype or got.shape != want.shape:
        return f"{got.dtype} {got.shape} against {want.dtype} {want.shape}"
    bad = np.argwhere(got != want)
    return None if bad.size == 0 else (f"{bad.shape[0]} of {got.size} differ, first at {tuple(bad[0])}: "
                                       f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")


def test_the_shapes_follow_the_kernels_constants():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "viprs_amd", "csrc",
                            "geno_class_sums.h")).read()
    assert int(re.search(r"kClassSumRows\s*=\s*(\d+)", src).group(1)) == ROWS
    assert int(re.search(r"kClassSumCols\s*=\s*(\d+)", src).group(1)) == COLS


@pytest.mark.parametrize("n", N_SIZES)
def test_device_equals_replay_over_the_cross(gpu, n):
    rng = np.random.default_rng(2000 + n)
    for missing in (0.0, 0.1):
        rows, _ = R.random_case(rng, max(M_SIZES), n, missing)
        Y = rng.standard_normal((n, max(COL_SIZES))) * np.exp(rng.uniform(-2, 2, size=(n, 1)))
        want = R.replay(rows, n, Y)
        for m in M_SIZES:
            g = G.DeviceGenotypes(rows[:m], n)
            for n_cols in COL_SIZES:
                got = g.class_sums(Y[:, :n_cols])
                msg = _first_difference(got, want[:m, :, :n_cols])
                assert msg is None, f"n={n} m={m} n_cols={n_cols} missing={missing}: {msg}"
            g.close()


@pytest.mark.parametrize("n", N_SIZES)
def test_device_equals_int64_for_integer_values(gpu, n):
    rng = np.random.default_rng(3000 + n)
    rows, codes = R.random_case(rng, 7, n)
    Y = rng.integers(-10 ** 6, 10 ** 6, size=(n, 5))
    want = np.stack([(codes == code).astype(np.int64) @ Y for code in R.CODES], axis=1).astype(np.float64)
    g = G.DeviceGenotypes(rows, n)
    assert _first_difference(g.class_sums(Y), want) is None
    assert _first_difference(g.class_sums(Y[:, 2]), want[:, :, 2]) is None
    g.close()


def _raw(g, row0, row1, Y, out):
    L = g._L
    return L.lib.viprs_genotypes_class_sums(g.handle, row0, row1, Y.shape[1], Y.ctypes.data_as(ctypes.c_void_p),
                                            out.ctypes.data_as(ctypes.c_void_p))


def test_independence_of_columns_rows_ranges_and_budget(gpu):
    rng = np.random.default_rng(21)
    n, m = 1500, 23
    rows, _ = R.random_case(rng, m, n)
    Y = np.ascontiguousarray(rng.standard_normal((n, 7)))
    g = G.DeviceGenotypes(rows, n)
    full = g.class_sums(Y)
    assert _first_difference(full, R.replay(rows, n, Y)) is None
    assert np.array_equal(g.class_sums(Y), full)                                   # two calls
    for c in range(7):                                                             # a column alone
        assert np.array_equal(g.class_sums(Y[:, c]), full[:, :, c]), c
    assert np.array_equal(g.class_sums(Y[:, [6, 0, 3]]), full[:, :, [6, 0, 3]])    # among other columns
    for j in (0, 5, m - 1):                                                        # a row alone
        one = G.DeviceGenotypes(rows[j:j + 1], n)
        assert np.array_equal(one.class_sums(Y), full[j:j + 1]), j
        one.close()
        out = np.full((3, 3, 7), 7.5)                                              # a one-row range into the middle of a buffer
        assert _raw(g, j, j + 1, Y, out[1:2]) == 0
        assert np.array_equal(out[1], full[j]) and np.all(out[0] == 7.5) and np.all(out[2] == 7.5), j
    for budget in (1, ROWS * 3 * 7 * 8, 5 * 3 * 7 * 8):                            # one row, one row group, five rows a call
        assert np.array_equal(g.class_sums(Y, max_bytes=budget), full), budget
    out = np.full((m + 2, 3, 7), -1.25)                                            # a range that is no multiple of anything
    assert _raw(g, 6, 6 + 11, Y, out[1:12]) == 0
    assert np.array_equal(out[1:12], full[6:17]) and np.all(out[0] == -1.25) and np.all(out[12:] == -1.25)
    assert g.last_class_sums_ms() > 0.0
    g.close()


def test_never_uploaded_rows_empty_shapes_and_refusals(gpu):
    from viprs_amd import _lib as L
    rng = np.random.default_rng(22)
    n, m = 70, 6
    rows, _ = R.random_case(rng, m, n)
    Y = np.ascontiguousarray(rng.standard_normal((n, 3)))
    # rows 2 .. 3 uploaded, the others never
    h = ctypes.c_void_p()
    L.check(L.lib.viprs_genotypes_create(ctypes.byref(h), n, m, 0))
    part = np.ascontiguousarray(rows[2:4])
    L.check(L.lib.viprs_genotypes_upload_rows(h, 2, 2, part.ctypes.data_as(ctypes.c_void_p)))
    out = np.full((m, 3, 3), 9.0)
    L.check(L.lib.viprs_genotypes_class_sums(h, 0, m, 3, Y.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)))
    assert np.array_equal(out[2:4], R.replay(rows[2:4], n, Y)) and np.all(out[:2] == 0.0) and np.all(out[4:] == 0.0)
    assert not np.any(np.signbit(out[:2]))
    # what needs the object: the row range against m; row0 == row1 is legal and writes nothing
    out[:] = 9.0
    ms = ctypes.c_double(-1.0)
    for r0, r1 in ((-1, 2), (0, m + 1), (m + 1, m + 1)):
        assert L.lib.viprs_genotypes_class_sums(h, r0, r1, 3, Y.ctypes.data_as(ctypes.c_void_p),
                                                out.ctypes.data_as(ctypes.c_void_p)) == L.EINVAL
        assert "rows out of range" in L.last_error()
    for r in (0, 3, m):
        L.check(L.lib.viprs_genotypes_class_sums(h, r, r, 3, Y.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)))
    assert np.all(out == 9.0)
    L.check(L.lib.viprs_genotypes_destroy(h))
    fresh = G.DeviceGenotypes(rows, n)
    with pytest.raises(ValueError, match="no timed class-sums call yet"):
        fresh.last_class_sums_ms()
    with pytest.raises(ValueError, match="NaN or inf"):
        fresh.class_sums(np.full(n, np.inf))
    fresh.close()
    # n = 0 and m = 0
    g0 = G.DeviceGenotypes(np.zeros((4, 0), dtype=np.uint8), 0)
    assert np.array_equal(g0.class_sums(np.zeros((0, 2))), np.zeros((4, 3, 2)))
    assert all(np.array_equal(v, np.zeros(4)) or (f == "A1_FREQ" and np.all(np.isnan(v))) for f, v in g0.association(np.zeros(0)).items())
    g0.close()
    gm = G.DeviceGenotypes(np.zeros((0, G.bytes_per_row(n)), dtype=np.uint8), n)
    assert gm.class_sums(Y).shape == (0, 3, 3) and gm.association(Y[:, 0])["R"].shape == (0,)
    gm.close()


def test_device_is_within_the_headers_bound_of_fsum(gpu):
    rng = np.random.default_rng(23)
    for n in (65, 1025, 2049):
        rows, _ = R.random_case(rng, 5, n)
        Y = rng.standard_normal((n, 2)) * np.exp(rng.uniform(-3, 3, size=(n, 1)))
        g = G.DeviceGenotypes(rows, n)
        err = np.abs(g.class_sums(Y) - R.exact(rows, n, Y))
        assert np.all(err <= R.bound(rows, n, Y)), n
        g.close()


def test_device_association_against_the_host(gpu):
    """Both sides evaluate the same formulas in double on class sums that differ within the header's bound: the CPU test's
    tolerance (`association_rtol`, relative, and absolute in units of the statistic's scale) holds between them."""
    rng = np.random.default_rng(24)
    m, n = 37, 1300
    codes = R.random_codes(rng, m, n, 0.1)
    codes[0], codes[1] = 3, 1
    rows = pack_codes(codes, trailing_bits=rng.integers(0, 256, m))
    dose = np.array([2.0, 0.0, 1.0, 0.0])[codes]
    Y = np.stack([0.4 * dose[5] + rng.standard_normal(n), 0.5 * dose[7] + rng.standard_normal(n) + 30.0], axis=1)
    Y /= Y.std(axis=0)
    Y[rng.random((n, 2)) < 0.05] = np.nan
    keep = rng.random((n, 2)) < 0.7
    tol = R.association_rtol(n)
    dev, host = G.DeviceGenotypes(rows, n), G.HostGenotypes(rows, n)
    for y, kp in ((Y, None), (Y, keep), (np.nan_to_num(Y[:, 0]), None), (np.nan_to_num(Y[:, 1], nan=np.nanmean(Y[:, 1])), keep[:, 0])):
        a, b = dev.association(y, keep=kp), host.association(y, keep=kp)
        assert np.array_equal(a["N"], b["N"]) and np.array_equal(a["A1_FREQ"], b["A1_FREQ"], equal_nan=True)
        for f, scale in (("BETA", 2.4), ("SE", 2.4), ("R", 1.0), ("Z", 4.0 * np.sqrt(n))):
            np.testing.assert_allclose(a[f], b[f], rtol=(4 if f == "Z" else 1) * tol, atol=scale * tol, err_msg=f)
        assert np.all(a["R"][:2] == 0.0) and np.any(np.abs(a["R"]) > 0.2)
    dev.close()


def _cohort(rng, m, n, beta):
    codes = R.random_codes(rng, m, n, 0.02)
    dose = np.array([2.0, 0.0, 1.0, 0.0])[codes]
    g = dose.T @ beta
    y = g + rng.standard_normal(n) * np.sqrt(g.var() * 0.5 / 0.5)               # h2 = 0.5
    return pack_codes(codes, trailing_bits=rng.integers(0, 256, m)), y


def test_from_a_bed_and_a_phenotype_to_scores_and_model_selection(gpu):
    from viprs_amd.data import ArrayDataLoader
    from viprs_amd.model import VIPRS, HyperparameterGrid, VIPRSGrid
    from viprs_amd.model.gridsearch import select_best_model
    rng = np.random.default_rng(25)
    m, n = 300, 600
    beta = rng.standard_normal(m) * (rng.random(m) < 0.1)
    rows, y = _cohort(rng, m, n, beta)
    gdl = ArrayDataLoader({}, {}, genotype={22: (rows, n)}, phenotype=y)
    ss = gdl.perform_gwas()
    host = G.HostGenotypes(rows, n).association(y)
    assert isinstance(gdl.genotype[22], G.DeviceGenotypes) and gdl.shapes == {22: m} and gdl.n == float(host["N"].max())
    np.testing.assert_allclose(ss[22].get_snp_pseudo_corr(), host["R"], rtol=R.association_rtol(n), atol=R.association_rtol(n))
    gdl.compute_ld(("windowed", 50))
    theta = {"pi": 0.1, "sigma_epsilon": 0.6}
    model = VIPRS(gdl).fit(max_iter=30, theta_0=theta)
    prs = model.predict()
    assert prs.shape == (n,) and np.all(np.isfinite(prs)) and np.all(np.isfinite(model.post_mean_beta[22]))
    assert np.corrcoef(prs, y)[0, 1] > 0.3                                        # (in sample: the fit found the signal)
    # a second cohort of the same SNPs validates a grid: the loader after perform_gwas() against the dict by hand
    rows2, y2 = _cohort(rng, m, 400, beta)
    val = ArrayDataLoader({}, {}, genotype={22: (rows2, 400)}, phenotype=y2)
    val.perform_gwas()
    grid = lambda: VIPRSGrid(gdl, HyperparameterGrid(sigma_epsilon_steps=2, pi_steps=3, n_snps=m, h2_est=0.4, h2_se=0.1)
                             ).fit(max_iter=30)
    a = select_best_model(grid(), validation_gdl=val, criterion="pseudo_validation")
    b = select_best_model(grid(), validation_gdl={22: val.sumstats_table[22].get_snp_pseudo_corr()},
                          criterion="pseudo_validation")
    assert a.best_model_idx == b.best_model_idx
    assert np.array_equal(a.validation_result["Pseudo_Validation_R2"], b.validation_result["Pseudo_Validation_R2"])
    assert np.array_equal(a.post_mean_beta[22], b.post_mean_beta[22])
    val.close_genotypes()
    gdl.close_genotypes()
