"""Genotype scoring on the device (`viprs_genotypes_*`, include/viprs_hip.h) against the host references of
tests/genotype_score_reference.py: exact counts, exact integer scores, the header's order bit for bit, the rounding bound,
independence of a column from everything but its own inputs, the argument checks, and the model layer on top.

Shapes: n straddles a byte (3, 4, 5), a lane's 32-bit word (15, 16, 17), the 16-byte stride unit and a wavefront's 64 samples of
one byte column (63, 64, 65), several units (257) and the sample tile of a workgroup (64 lanes x 16 samples = 1024); m straddles
the chunk L; n_cols straddles every column-group width (8, 4, 2, 1 in float32; 4, 2, 1 in float64)."""
import ctypes
import os

import numpy as np
import pytest

from tests import genotype_score_reference as R
from viprs_amd.genotypes import DeviceGenotypes, counts_host, dose_table, score_host

pytestmark = pytest.mark.gpu

L = R.L
TILE = 1024
N_SIZES = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257, TILE - 1, TILE, TILE + 1]
M_SIZES = [1, 2, L - 1, L, L + 1, 2 * L + 1]
COLS = [1, 2, 3, 5, 32, 33]
PRECISIONS = [np.float32, np.float64]


def _assert_equal(got, want, what):
    msg = R.first_difference(got, want)
    assert msg is None, f"{what}: {msg}"


@pytest.mark.parametrize("n", N_SIZES)
def test_counts_and_trailing_bits(gpu, n):
    rng = np.random.default_rng(100 + n)
    for m in M_SIZES:
        packed, codes = R.random_case(rng, n, m)
        want = np.stack([(codes == k).sum(axis=1) for k in range(4)], axis=1).astype(np.int64)
        g = DeviceGenotypes(packed, n)
        got = g.counts()
        assert got.dtype == np.int64 and np.array_equal(got, want), (n, m)
        assert np.array_equal(got.sum(axis=1), np.full(m, n))
        # the same rows with other bits in the unused slots of the last byte: identical counts and scores
        g2 = DeviceGenotypes(R.other_trailing_bits(rng, codes), n)
        assert np.array_equal(g2.counts(), want), (n, m)
        B = rng.normal(size=(m, 3)).astype(np.float32)
        _assert_equal(g2.score(B, "mean"), g.score(B, "mean"), f"trailing bits, n={n} m={m}")
        g.close()
        g2.close()


@pytest.mark.parametrize("n", N_SIZES)
def test_exact_integer_scores(gpu, n):
    """Small-integer B and D: every term and every partial sum is an integer below 2^24 (|term| <= 6, m <= 2049), so every
    order gives the exact sum -- compared with `==` over the cross of the shapes, both precisions and the three ways a table
    reaches the kernel (NULL, a named mode, an explicit table)."""
    rng = np.random.default_rng(200 + n)
    for m in M_SIZES:
        packed, _ = R.random_case(rng, n, m)
        g = DeviceGenotypes(packed, n)
        Dint = rng.integers(-2, 3, size=(m, 4))
        Ball = rng.integers(-3, 4, size=(m, max(COLS)))
        for dose, Dref in ((None, None), ("zero", None), ("table", Dint)):
            want = R.exact_int(packed, n, Ball, Dref)               # (a column's score does not depend on the others)
            for k in COLS:
                for T in PRECISIONS:
                    got = g.score(np.ascontiguousarray(Ball[:, :k]).astype(T), Dint.astype(T) if dose == "table" else dose)
                    assert got.dtype == T and got.shape == (n, k)
                    _assert_equal(got, want[:, :k].astype(T), f"n={n} m={m} cols={k} {np.dtype(T).name} dose={dose}")
        g.close()


@pytest.mark.parametrize("T", PRECISIONS)
@pytest.mark.parametrize("mode", ["mean", "zero", "standardize"])
def test_bits_are_the_headers_order(gpu, T, mode):
    rng = np.random.default_rng(300)
    m = 2 * L + 1
    for n, k in ((17, 33), (257, 33), (TILE + 1, 5)):
        packed, _ = R.random_case(rng, n, m, missing=0.1)
        B = (rng.normal(size=(m, k)) * rng.uniform(0.5, 2.0, size=(m, 1))).astype(T)
        g = DeviceGenotypes(packed, n)
        D = g.dose_table(mode, dtype=T)
        assert np.array_equal(D, dose_table(counts_host(packed, n), mode, dtype=T))
        got = g.score(B, D)
        _assert_equal(got, R.replay(packed, n, B, D, T), f"{mode} {np.dtype(T).name} n={n} cols={k}")
        _assert_equal(g.score(B, mode), got, "named mode against its table")
        g.close()


EDGE_SHAPES = [(1, 1, 1), (3, 2, 2), (4, L - 1, 3), (5, L, 5), (15, L + 1, 32), (16, 2 * L + 1, 33), (17, 1, 33), (63, L, 2),
               (64, L + 1, 1), (65, L - 1, 8), (257, 2, 5), (TILE - 1, L + 1, 2), (TILE, 2, 33), (TILE + 1, L, 3)]


@pytest.mark.parametrize("T", PRECISIONS)
@pytest.mark.parametrize("mode", ["mean", "standardize"])
def test_bits_on_edge_shapes(gpu, T, mode):
    """The two dose modes whose tables are no integers cannot be compared with the integer reference: `==` against the replay
    of the header's order instead, on shapes at every edge of n, m and n_cols."""
    rng = np.random.default_rng(350)
    for n, m, k in EDGE_SHAPES:
        packed, _ = R.random_case(rng, n, m, missing=0.1)
        B = rng.normal(size=(m, k)).astype(T)
        g = DeviceGenotypes(packed, n)
        D = g.dose_table(mode, dtype=T)
        _assert_equal(g.score(B, mode), R.replay(packed, n, B, D, T), f"{mode} {np.dtype(T).name} n={n} m={m} cols={k}")
        g.close()


@pytest.mark.parametrize("T", PRECISIONS)
def test_rounding_bound(gpu, T):
    rng = np.random.default_rng(400)
    for n, m, k in ((65, 2 * L + 1, 5), (TILE + 1, L + 1, 3), (17, L - 1, 33)):
        packed, _ = R.random_case(rng, n, m, missing=0.1)
        B = rng.normal(size=(m, k)).astype(T)
        g = DeviceGenotypes(packed, n)
        D = g.dose_table("mean", dtype=T)
        err = np.abs(g.score(B, D).astype(np.float64) - score_host(packed, n, B, D))
        bound = R.rounding_bound(packed, n, B, D, T)
        print(np.dtype(T).name, (n, m, k), "max error / bound:", float(np.max(err / bound)))
        assert np.all(err <= bound)
        g.close()


@pytest.mark.parametrize("T", PRECISIONS)
def test_independence(gpu, T):
    rng = np.random.default_rng(500)
    n, m, k = 257, 2 * L + 1, 33
    packed, codes = R.random_case(rng, n, m, missing=0.1)
    B = rng.normal(size=(m, k)).astype(T)
    g = DeviceGenotypes(packed, n)
    D = g.dose_table("standardize", dtype=T)
    full = g.score(B, D)
    _assert_equal(g.score(B, D), full, "second call")
    for c in (0, 7, 8, 31, 32):
        _assert_equal(g.score(B[:, c], D), full[:, c], f"column {c} alone")
    perm = rng.permutation(k)
    _assert_equal(g.score(B[:, perm], D)[:, np.argsort(perm)], full, "columns permuted")
    _assert_equal(g.score(B[:, 5:12], D), full[:, 5:12], "a slice of the columns")
    # the chunks cut into ranges of one (the work buffer holds one chunk at a time): the double sums carry on across them
    os.environ["VIPRS_SCORE_WORK_BYTES"] = "1"
    try:
        _assert_equal(g.score(B, D), full, "one chunk per range")
    finally:
        del os.environ["VIPRS_SCORE_WORK_BYTES"]
    # an all-zero B row: present with any dose table, or removed from the genotypes altogether
    rows = np.array([0, L - 1, L, m - 1])
    Bz = B.copy()
    Bz[rows] = 0
    with_rows = g.score(Bz, D)
    D2 = D.copy()
    D2[rows] = rng.normal(size=(4, 4)).astype(T)
    _assert_equal(g.score(Bz, D2), with_rows, "zero rows of B under another dose table")
    # (removing SNPs moves the chunk boundaries, so the comparison is made where it cannot: inside the last chunk)
    keep = np.ones(m, bool)
    keep[m - 1] = False
    Bl = B.copy()
    Bl[m - 1] = 0
    g3 = DeviceGenotypes(np.ascontiguousarray(packed[keep]), n)
    _assert_equal(g3.score(np.ascontiguousarray(Bl[keep]), np.ascontiguousarray(D[keep])), g.score(Bl, D), "zero row removed")
    g3.close()
    g.close()


def test_argument_checks(gpu):
    from viprs_amd import _lib as Lb
    rng = np.random.default_rng(600)
    n, m, k = 21, 9, 2
    packed, _ = R.random_case(rng, n, m)
    g = DeviceGenotypes(packed, n)
    B = np.ascontiguousarray(rng.normal(size=(m, k)).astype(np.float32))
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    score = Lb.lib.viprs_genotypes_score
    out = np.full((n, k), 7.0, dtype=np.float32)
    for args in ((g.handle, 2, k, ptr(B), None, ptr(out)),             # bad dtype code
                 (g.handle, Lb.F32, 0, ptr(B), None, ptr(out)),        # n_cols < 1
                 (g.handle, Lb.F32, -1, ptr(B), None, ptr(out)),
                 (None, Lb.F32, k, ptr(B), None, ptr(out)),            # null object
                 (g.handle, Lb.F32, k, None, None, ptr(out))):         # null effects
        assert score(*args) == Lb.EINVAL and Lb.last_error()
        assert np.all(out == 7.0)
    assert score(g.handle, Lb.F32, k, ptr(B), None, None) == Lb.EINVAL
    counts = np.full((m, 4), -5, dtype=np.int64)
    assert Lb.lib.viprs_genotypes_counts(None, ptr(counts)) == Lb.EINVAL and np.all(counts == -5)
    assert Lb.lib.viprs_genotypes_counts(g.handle, None) == Lb.EINVAL
    before = g.counts().copy()
    up = Lb.lib.viprs_genotypes_upload_rows
    for first, rows in ((-1, 1), (0, m + 1), (m, 1), (2, -1), (m + 1, 0)):
        assert up(g.handle, first, rows, ptr(packed)) == Lb.EINVAL, (first, rows)
    assert up(g.handle, 0, 1, None) == Lb.EINVAL and up(None, 0, 1, ptr(packed)) == Lb.EINVAL
    g._counts = None
    assert np.array_equal(g.counts(), before)
    ms = ctypes.c_double(-1.0)
    assert Lb.lib.viprs_genotypes_last_score_ms(g.handle, None) == Lb.EINVAL
    assert Lb.lib.viprs_genotypes_last_score_ms(g.handle, ctypes.byref(ms)) == Lb.EINVAL        # nothing timed yet
    g.score(B)
    assert g.last_score_ms() > 0.0
    assert Lb.lib.viprs_genotypes_last_counts_ms(g.handle, None) == Lb.EINVAL
    assert g.last_counts_ms() > 0.0
    h = ctypes.c_void_p()
    assert Lb.lib.viprs_genotypes_create(ctypes.byref(h), -1, 3, 0) == Lb.EINVAL
    assert Lb.lib.viprs_genotypes_create(ctypes.byref(h), 3, -1, 0) == Lb.EINVAL
    assert Lb.lib.viprs_genotypes_create(None, 3, 3, 0) == Lb.EINVAL
    assert Lb.lib.viprs_genotypes_create(ctypes.byref(h), 3, 3, 10 ** 6) == Lb.EINVAL and not h
    with pytest.raises(ValueError):
        g.score(B[:-1])
    with pytest.raises(ValueError):
        g.score(B, np.zeros((m, 3), np.float32))
    g.close()
    # a row that was never uploaded reads as "every sample missing"; rows go up in slices
    g = DeviceGenotypes(packed[:0].reshape(0, packed.shape[1]), n)
    g.close()
    h = ctypes.c_void_p()
    Lb.check(Lb.lib.viprs_genotypes_create(ctypes.byref(h), n, m, 0))
    part = np.ascontiguousarray(packed[3:7])
    Lb.check(up(h, 3, 4, ptr(part)))
    c = np.zeros((m, 4), np.int64)
    Lb.check(Lb.lib.viprs_genotypes_counts(h, ptr(c)))
    want = counts_host(packed, n)
    want[[0, 1, 2, 7, 8]] = [0, n, 0, 0]
    assert np.array_equal(c, want)
    Lb.lib.viprs_genotypes_destroy(h)


@pytest.mark.parametrize("T", PRECISIONS)
def test_empty_shapes(gpu, T):
    # m = 0: scores are zeros, no counts; n = 0: nothing to write
    g = DeviceGenotypes(np.zeros((0, 2), np.uint8), 5)
    s = g.score(np.zeros((0, 3), T))
    assert s.shape == (5, 3) and s.dtype == T and not s.any() and not np.signbit(s).any()
    assert g.counts().shape == (0, 4)
    g.close()
    g = DeviceGenotypes(np.zeros((4, 0), np.uint8), 0)
    assert g.score(np.ones((4, 2), T)).shape == (0, 2)
    assert np.array_equal(g.counts(), np.zeros((4, 4), np.int64))
    g.close()


# ---- the model layer ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted_grid(gpu):
    from viprs_amd.data import ArrayDataLoader
    from viprs_amd.model import HyperparameterGrid, VIPRSGrid
    gdl = ArrayDataLoader.synthetic({22: [500, 130]}, seed=3, forms=("upper",), kind="longrange")
    grid = HyperparameterGrid(sigma_epsilon_steps=2, pi_steps=3, n_snps=gdl.m, h2_est=0.2, h2_se=0.1)
    model = VIPRSGrid(gdl, grid, low_memory=True)
    model.fit(batched=True, max_iter=80)
    return gdl, model


def test_model_predict_and_validation(fitted_grid):
    from viprs_amd.data import ArrayDataLoader
    from viprs_amd.eval.continuous_metrics import r2
    from viprs_amd.model import select_best_model
    gdl, model = fitted_grid
    rng = np.random.default_rng(700)
    n, m, c = 257, gdl.m, 22
    packed, _ = R.random_case(rng, n, m, missing=0.05)
    beta = np.asarray(model.post_mean_beta[c])
    assert beta.dtype == np.float32 and beta.shape == (m, model.n_models)
    ok = np.asarray(model.valid_terminated_models)
    planted = int(np.nonzero(ok)[0][len(np.nonzero(ok)[0]) // 2])
    D = dose_table(counts_host(packed, n), "mean", dtype=np.float32)
    host = score_host(packed, n, beta, D)
    y = host[:, planted] + 0.5 * np.std(host[:, planted]) * rng.normal(size=n)
    with pytest.raises(ValueError, match="genotypes"):
        model.predict()
    val = ArrayDataLoader({}, {}, n=n, genotype={c: (packed, n)}, phenotype=y)
    prs = model.predict(test_gdl=val)
    assert prs.shape == (n, model.n_models) and prs.dtype == np.float64
    assert isinstance(val.genotype[c], DeviceGenotypes)
    bound = R.rounding_bound(packed, n, beta, D, np.float32)
    print("predict: max error / bound", float(np.max(np.abs(prs - host) / np.maximum(bound, 1e-300))))
    assert np.all(np.abs(prs - host) <= bound)
    # the training loader's own genotypes
    gdl.genotype = {c: val.genotype[c]}
    assert np.array_equal(model.predict(), prs)
    gdl.genotype = None
    want = np.nan_to_num(np.array([r2(y, prs[:, i]) for i in range(model.n_models)]))
    with pytest.raises(ValueError, match="phenotype"):
        select_best_model(model, validation_gdl=ArrayDataLoader({}, {}, n=n, genotype={c: val.genotype[c]}), criterion="validation")
    sel = select_best_model(model, validation_gdl=val, criterion="validation")
    written = np.asarray(sel.validation_result["Validation_R2"], dtype=np.float64)
    assert np.array_equal(written, want)
    assert sel.best_model_idx == int(np.argmax(np.where(ok, written, -np.inf)))
    assert sel.post_mean_beta[c].shape == (m,) and np.array_equal(sel.post_mean_beta[c], beta[:, sel.best_model_idx])
    assert sel.predict(test_gdl=val).shape == (n,)
    val.close_genotypes()


def test_per_chromosome_predict_is_the_sum_of_its_chromosomes(gpu):
    """`VIPRSPerChromosome.predict`: every chromosome scored on its own genotypes in the model's precision, the chromosomes
    added on the host in double in ascending order -- compared with `==`."""
    from viprs_amd.data import ArrayDataLoader
    from viprs_amd.model import VIPRSPerChromosome
    rng = np.random.default_rng(800)
    gdl = ArrayDataLoader.synthetic({21: [200, 64], 22: [130], 20: [65]}, seed=11, forms=("upper",))
    n = 257
    geno = {c: R.random_case(rng, n, gdl.shapes[c], missing=0.05)[0] for c in gdl.chromosomes}
    gdl.genotype = {c: (geno[c], n) for c in geno}
    model = VIPRSPerChromosome(gdl, low_memory=True).fit(max_iter=30)
    total = model.predict()
    parts = model.predict(per_chromosome=True)
    assert total.shape == (n,) and total.dtype == np.float64 and sorted(parts) == [20, 21, 22]
    assert np.array_equal(total, (parts[20] + parts[21]) + parts[22])
    for c in parts:
        g = DeviceGenotypes(geno[c], n)
        single = g.score(np.asarray(model.post_mean_beta[c]), "mean")
        assert single.dtype == np.float32
        assert np.array_equal(parts[c], single.astype(np.float64))
        g.close()
    gdl.close_genotypes()


def test_ldpredinf_predict(gpu):
    """`LDPredInf.predict`: ValueError before `fit()`, then the device scores of its posterior means within the bound."""
    from viprs_amd.data import ArrayDataLoader
    from viprs_amd.model import LDPredInf, VIPRS
    rng = np.random.default_rng(900)
    gdl = ArrayDataLoader.synthetic({1: [300, 65], 2: [257]}, ld_dtype=np.int8, n=5e4, kind="longrange")
    n = 65
    geno = {c: R.random_case(rng, n, gdl.shapes[c], missing=0.05)[0] for c in gdl.chromosomes}
    val = ArrayDataLoader({}, {}, n=n, genotype={c: (geno[c], n) for c in geno})
    model = LDPredInf(gdl, h2=0.3, dequantize_on_the_fly=True)
    with pytest.raises(ValueError, match="fit"):
        model.predict(test_gdl=val)
    with pytest.raises(ValueError, match="fit"):
        VIPRS(gdl, dequantize_on_the_fly=True).predict(test_gdl=val)
    model.fit()
    with pytest.raises(ValueError, match="genotypes"):
        model.predict()
    prs = model.predict(test_gdl=val)
    assert prs.shape == (n,) and prs.dtype == np.float64 and np.any(prs != 0)
    want, bound = np.zeros(n), np.zeros(n)
    for c in sorted(geno):
        b = np.asarray(model.post_mean_beta[c])
        D = dose_table(counts_host(geno[c], n), "mean", dtype=b.dtype)
        want += score_host(geno[c], n, b, D)
        bound += R.rounding_bound(geno[c], n, b, D, b.dtype)[:, 0]
    assert np.all(np.abs(prs - want) <= bound)
    val.close_genotypes()
