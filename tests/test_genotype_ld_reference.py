"""LD from genotypes on the host (`viprs_amd.genotypes.ld_host`, the definition of `viprs_genotypes_ld` in
include/viprs_hip.h): against an independent float route, the properties the definition promises, and `ld_windows`."""
import numpy as np
import pytest

from viprs_amd import genotypes as G
from viprs_amd.io.plink_bed import pack_codes


def _codes(m, n, missing, seed):
    rng = np.random.default_rng(seed)
    freq = rng.uniform(0.1, 0.9, size=(m, 1))
    dose = (rng.random((m, n)) < freq).astype(np.int64) + (rng.random((m, n)) < freq)
    codes = np.array([3, 2, 0], dtype=np.uint8)[dose]               # dose 0 / 1 / 2 -> code 3 / 2 / 0
    if missing:
        codes[rng.random((m, n)) < missing] = 1
    return codes


def _full(indptr, data, m):
    """The compact upper store as a dense symmetric matrix with a unit diagonal."""
    R = np.eye(m)
    for j in range(m):
        R[j, j + 1:j + 1 + indptr[j + 1] - indptr[j]] = data[indptr[j]:indptr[j + 1]]
    return np.triu(R) + np.triu(R, 1).T


def _corrcoef_route(codes):
    """Decode to float, mean-impute, np.corrcoef: shares nothing with the integer formula."""
    x = np.where(codes == 0, 2.0, np.where(codes == 2, 1.0, 0.0))
    miss = codes == 1
    mu = np.where(miss, 0.0, x).sum(axis=1) / np.maximum((~miss).sum(axis=1), 1)
    return np.corrcoef(np.where(miss, mu[:, None], x))


@pytest.mark.parametrize("m,n,seed", [(40, 300, 1), (23, 77, 2), (70, 129, 3)])
def test_ld_host_equals_corrcoef_of_mean_imputed_doses(m, n, seed):
    """|r| <= 1 and each side is a handful of double roundings of sums of at most 300 terms of magnitude <= 4: the two
    routes agree to a few hundred eps, far inside 1e-12 (derived, not measured)."""
    codes = _codes(m, n, 0.10, seed)
    rows = pack_codes(codes, trailing_bits=np.random.default_rng(seed).integers(0, 256, m))
    ip, data = G.ld_host(rows, n, G.ld_windows(("sample",), m), np.float64)
    assert ip[-1] == m * (m - 1) // 2 and data.dtype == np.float64
    want = _corrcoef_route(codes)
    assert np.max(np.abs(_full(ip, data, m) - want)) <= 1e-12
    # the reference is not symmetric in its operands: U_ij != U_ji under random missingness
    x, p = G._ld_planes(rows, n)
    U = x @ p.T
    assert np.any(U != U.T)


def test_unit_diagonal_through_the_formula():
    """r_ii = nn d / (w w) with w = sqrt(nn d): one rounding in the square root, one in the product, one in the division."""
    codes = _codes(30, 211, 0.10, 5)
    rows = pack_codes(codes)
    R = G.ld_block_host(rows, rows, 211)
    assert np.max(np.abs(np.diag(R) - 1.0)) <= 4 * np.finfo(np.float64).eps
    assert np.array_equal(R, R.T)                       # num is symmetric in exact integers, w_i w_j commutes


def test_full_sample_matrix_is_positive_semidefinite():
    codes = _codes(60, 150, 0.10, 7)
    ip, data = G.ld_host(pack_codes(codes), 150, np.full(60, 60), np.float64)
    assert np.linalg.eigvalsh(_full(ip, data, 60)).min() >= -1e-10


def test_degenerate_snps_give_exact_zeros():
    n = 37
    codes = _codes(6, n, 0.10, 11)
    codes[1] = 0                                        # monomorphic
    codes[3] = 1                                        # all missing
    codes[4] = 1
    codes[4, 5] = 2                                     # a single sample
    for T in (np.float64, np.float32, np.int8, np.int16):
        ip, data = G.ld_host(pack_codes(codes), n, np.full(6, 6), T)
        R = _full(ip, data.astype(np.float64), 6)
        for j in (1, 3, 4):
            assert np.all(np.delete(R[j], j) == 0.0) and np.all(np.delete(R[:, j], j) == 0.0)
        assert R[0, 2] != 0.0
    # one sample in all: every SNP is monomorphic
    ip, data = G.ld_host(pack_codes(_codes(5, 1, 0.0, 1)), 1, np.full(5, 5), np.float64)
    assert data.shape == (10,) and np.all(data == 0.0)


def test_output_types_are_the_stores_quantisation():
    codes = _codes(20, 90, 0.10, 13)
    rows = pack_codes(codes)
    re = G.ld_windows(("windowed", 7), 20)
    ip, r = G.ld_host(rows, 90, re, np.float64)
    assert np.array_equal(np.diff(ip), re - np.arange(1, 21))
    assert np.array_equal(G.ld_host(rows, 90, re, np.float32)[1], r.astype(np.float32))
    assert np.array_equal(G.ld_host(rows, 90, re, np.int8)[1], np.clip(np.rint(r * 127), -127, 127).astype(np.int8))
    assert np.array_equal(G.ld_host(rows, 90, re, np.int16)[1], np.clip(np.rint(r * 32767), -32767, 32767).astype(np.int16))
    assert np.array_equal(G._ld_quantize(np.array([0.5 / 127, 1.5 / 127, -2.5 / 127, 1.0, -1.0]), np.int8),
                          np.array([0, 2, -2, 127, -127], dtype=np.int8))            # ties to even, as np.rint
    assert G.ld_dq_scale(np.int8) == 1 / 127 and G.ld_dq_scale(np.int16) == 1 / 32767 and G.ld_dq_scale(np.float32) == 1.0
    with pytest.raises(ValueError, match="dtype"):
        G.ld_host(rows, 90, re, np.int32)
    # windowed rows are the matching entries of the full matrix
    ipf, rf = G.ld_host(rows, 90, np.full(20, 20), np.float64)
    for j in range(20):
        assert np.array_equal(r[ip[j]:ip[j + 1]], rf[ipf[j]:ipf[j] + ip[j + 1] - ip[j]])


def test_host_genotypes_ld_and_refusals():
    codes = _codes(9, 50, 0.05, 17)
    rows = pack_codes(codes)
    g = G.HostGenotypes(rows, 50)
    ip, data = g.ld(("block", [4]), dtype=np.int16)
    ip2, data2 = G.ld_host(rows, 50, np.array([4, 4, 4, 4, 9, 9, 9, 9, 9]), np.int16)
    assert np.array_equal(ip, ip2) and np.array_equal(data, data2)
    assert np.array_equal(g.ld()[0], G.ld_indptr(np.full(9, 9)))
    for bad, word in (([5, 4] + [9] * 7, "non-decreasing"), ([0] + [9] * 8, r"\[j \+ 1, m\]"), ([10] * 9, r"\[j \+ 1, m\]"),
                      ([9] * 8, "right_end")):
        with pytest.raises(ValueError, match=word):
            g.ld(np.array(bad))
    big = (1 << 19) + 1
    with pytest.raises(ValueError, match="2\\^19"):
        G.ld_host(np.zeros((1, (big + 3) // 4), dtype=np.uint8), big, np.array([1]), np.float32)


def test_ld_windows_for_the_four_estimators():
    m = 10
    assert np.array_equal(G.ld_windows(("sample",), m), np.full(m, m))
    assert np.array_equal(G.ld_windows("sample", m), np.full(m, m))
    assert np.array_equal(G.ld_windows(("windowed", 3), m), [4, 5, 6, 7, 8, 9, 10, 10, 10, 10])
    assert np.array_equal(G.ld_windows(("windowed", 0), m), np.arange(1, m + 1))
    # POS ties: SNPs at one position see each other, and the SNP after them at distance 0 does not
    pos = np.array([100, 100, 100, 150, 200, 200, 900, 901, 901, 5000])
    assert np.array_equal(G.ld_windows(("windowed_bp", 0, pos), m), [3, 3, 3, 4, 6, 6, 7, 9, 9, 10])
    assert np.array_equal(G.ld_windows(("windowed_bp", 100, pos), m), [6, 6, 6, 6, 6, 6, 9, 9, 9, 10])
    with pytest.raises(ValueError, match="sorted"):
        G.ld_windows(("windowed_bp", 10, pos[::-1]), m)
    # ragged blocks, with and without the ends 0 and m, in any order, repeated
    want = [1, 4, 4, 4, 9, 9, 9, 9, 9, 10]
    for b in ([1, 4, 9], [0, 1, 4, 9, 10], [9, 4, 1, 4]):
        assert np.array_equal(G.ld_windows(("block", b), m), want)
    assert np.array_equal(G.ld_windows(("block", []), m), np.full(m, m))
    with pytest.raises(ValueError, match="boundaries"):
        G.ld_windows(("block", [11]), m)
    for bad in (("sample", 3), ("windowed",), ("shrinkage", 1), ("block",)):
        with pytest.raises(ValueError, match="estimator"):
            G.ld_windows(bad, m)
    for est in (("sample",), ("windowed", 2), ("windowed_bp", 60, pos), ("block", [3, 7])):
        re = G.ld_windows(est, m)
        assert re.dtype == np.int64 and np.all(np.diff(re) >= 0) and np.all(re >= np.arange(1, m + 1)) and re[-1] == m
    assert G.ld_windows(("sample",), 0).shape == (0,)


def test_loader_computes_ld_on_the_host_without_a_device(monkeypatch, tmp_path):
    """`compute_ld` through `HostGenotypes`: the LDArrays a model reads, and the store `ZarrLDMatrix` reads back."""
    from viprs_amd.data import ArrayDataLoader
    from viprs_amd.io.zarr_ld import ZarrLDMatrix
    codes = _codes(12, 64, 0.05, 19)
    rows = pack_codes(codes)
    gdl = ArrayDataLoader({}, {}, genotype={7: G.HostGenotypes(rows, 64)})
    gdl.compute_ld(("block", [5]), dtype=np.int8)
    ld = gdl.ld[7]
    assert ld.sample_size == 64 and ld.dq_scale == 1 / 127 and ld.stored_dtype == np.int8
    got = ld.load(return_symmetric=False)
    ip, data = G.ld_host(rows, 64, G.ld_windows(("block", [5]), 12), np.int8)
    assert np.array_equal(got.ld_indptr, ip) and np.array_equal(got.ld_data, data)
    assert np.array_equal(got.leftmost_idx, np.arange(1, 13))
    with pytest.raises(ValueError):
        ld.load(return_symmetric=True)
    # genotypes that do not line up with the summary statistics are refused here, not inside a model
    from viprs_amd.data import SumstatsArrays
    off = ArrayDataLoader({}, {7: SumstatsArrays(np.zeros(11), np.full(11, 1e4))}, genotype={7: G.HostGenotypes(rows, 64)})
    with pytest.raises(ValueError, match="12 genotyped SNPs against 11"):
        off.compute_ld()
    paths = gdl.write_ld_stores(tmp_path)
    z = ZarrLDMatrix(paths[7])
    assert z.ld_estimator == "block" and z.sample_size == 64 and z.chromosome == 7
    back = z.load()
    assert np.array_equal(back.ld_indptr, ip) and np.array_equal(back.ld_data, data) and back.ld_data.dtype == np.int8
