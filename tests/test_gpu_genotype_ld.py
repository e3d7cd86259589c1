"""LD from genotypes on the device (`viprs_genotypes_ld`, include/viprs_hip.h; kernels: viprs_amd/csrc/geno_ld.h) against
`viprs_amd.genotypes.ld_host`, with `==`: every sum of the definition is an exact integer, so no order has to be replayed.

Shapes: n straddles a byte, a lane's 16-sample word (15, 16, 17), a k-step of 32 samples (31, 32, 33), the 16-byte unit of 64
samples and the 128 samples of a K-loop pass (63, 64, 65, 129), and many passes (1025); m straddles a 32-SNP fragment and the
64-SNP tile (31 .. 65) and reaches a third tile (130).  Random missingness makes U_ij != U_ji, so a swapped operand or a
transposed write cannot pass."""
import ctypes

import numpy as np
import pytest

from viprs_amd import genotypes as G
from viprs_amd.io.plink_bed import pack_codes

pytestmark = pytest.mark.gpu

N_SIZES = [1, 3, 4, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129, 1025]
M_SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 130]
MISSING = ["none", "random", "mixed"]
DTYPES = [np.float64, np.float32, np.int8, np.int16]
TILE = 64


def _case(rng, m, n, missing):
    """Packed rows with random trailing bits.  `missing`: "none", "random" (10 % everywhere) or "mixed" (10 % in every other
    tile of 64 SNPs, the first one included: clean and general tile pairs in one call)."""
    freq = rng.uniform(0.1, 0.9, size=(m, 1))
    dose = (rng.random((m, n)) < freq).astype(np.int64) + (rng.random((m, n)) < freq)
    codes = np.array([3, 2, 0], dtype=np.uint8)[dose]
    if missing != "none":
        hit = rng.random((m, n)) < 0.10
        if missing == "mixed":
            hit &= ((np.arange(m) // TILE) % 2 == 0)[:, None]
        codes[hit] = 1
    return pack_codes(codes, trailing_bits=rng.integers(0, 256, m)), codes


def _as(r, T):
    """The stores' quantisation of float64 correlations, written out (tests/test_genotype_ld_reference.py pins `ld_host`'s
    other element types to the same expressions)."""
    if T == np.float64:
        return r
    if T == np.float32:
        return r.astype(np.float32)
    q = 127.0 if T == np.int8 else 32767.0
    return np.clip(np.rint(r * q), -q, q).astype(T)


def _first_difference(got, want):
    if got.dtype != want.dtype or got.shape != want.shape:
        return f"{got.dtype} {got.shape} against {want.dtype} {want.shape}"
    bad = np.nonzero(got != want)[0]
    return None if bad.size == 0 else f"{bad.size} of {got.size} differ, first at {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}"


@pytest.mark.parametrize("n", N_SIZES)
def test_device_equals_host_over_the_cross(gpu, n):
    rng = np.random.default_rng(1000 + n)
    for m in M_SIZES:
        for missing in MISSING:
            rows, codes = _case(rng, m, n, missing)
            g = G.DeviceGenotypes(rows, n)
            ip, want = G.ld_host(rows, n, np.full(m, m), np.float64)
            if missing != "none" and n >= 63 and m >= 31:
                x, p = G._ld_planes(rows, n)
                U = x @ p.T
                assert np.any(U != U.T), "the reference is symmetric here: the case proves nothing about the operand order"
            for T in DTYPES:
                gip, got = g.ld(dtype=T)
                assert np.array_equal(gip, ip)
                msg = _first_difference(got, _as(want, T))
                assert msg is None, f"n={n} m={m} missing={missing} {np.dtype(T).name}: {msg}"
            g.close()


def test_clean_and_general_tiles_meet_in_one_call(gpu):
    """m = 200: tiles 0 and 2 have missing codes, tiles 1 and 3 have none.  The pairs (1, 1), (1, 3), (3, 3) run the clean
    instantiation, the others the general one; every tile row holds both."""
    rng = np.random.default_rng(7)
    rows, codes = _case(rng, 200, 333, "mixed")
    miss = (codes == 1).any(axis=1)
    assert miss[:64].any() and not miss[64:128].any() and miss[128:192].any() and not miss[192:].any()
    g = G.DeviceGenotypes(rows, 333)
    for T in DTYPES:
        ip, want = G.ld_host(rows, 333, np.full(200, 200), T)
        gip, got = g.ld(dtype=T)
        assert np.array_equal(gip, ip) and _first_difference(got, want) is None, np.dtype(T).name
    # a clean pair gives what the general formula gives: the same rows, one missing code added far away, in another SNP
    codes2 = codes.copy()
    codes2[70, 5] = 1                                   # tile 1 is no longer clean; rows 100.. of tile 1 keep their values
    g2 = G.DeviceGenotypes(pack_codes(codes2), 333)
    ip2, got2 = g2.ld(dtype=np.float64)
    sel = np.arange(ip[100], ip[100] + 27)              # r(100, 101 .. 127): inside tile pair (1, 1)
    assert np.array_equal(got2[sel], g.ld(dtype=np.float64)[1][sel])
    g.close()
    g2.close()


def _windows(m):
    j = np.arange(m)
    return {
        "full": np.full(m, m),
        "empty rows": j + 1,
        "one neighbour": np.minimum(j + 2, m),
        "ragged blocks": G.ld_windows(("block", [37, 100, 101, 163]), m),
        "widening then constant": np.minimum(m, j + 1 + np.minimum(2 * j, 50)),
    }


@pytest.mark.parametrize("missing", ["none", "random"])
def test_windows(gpu, missing):
    m, n = 200, 97
    rng = np.random.default_rng(11)
    rows, _ = _case(rng, m, n, missing)
    g = G.DeviceGenotypes(rows, n)
    for name, re in _windows(m).items():
        for T in (np.float32, np.int8):
            ip, want = G.ld_host(rows, n, re, T)
            gip, got = g.ld(re, dtype=T)
            assert np.array_equal(gip, ip) and np.array_equal(np.diff(ip), re - np.arange(1, m + 1)), name
            assert _first_difference(got, want) is None, (name, np.dtype(T).name, _first_difference(got, want))
            if name == "empty rows":
                assert got.size == 0
    g.close()


def test_row_ranges(gpu):
    m, n = 200, 70
    rng = np.random.default_rng(13)
    rows, _ = _case(rng, m, n, "mixed")
    re = G.ld_windows(("windowed", 90), m)
    g = G.DeviceGenotypes(rows, n)
    w = G.ld_stats(g.counts())[2]
    ip, want = G.ld_host(rows, n, re, np.float32)
    # one call
    whole = np.zeros(int(ip[-1]), dtype=np.float32)
    g.ld_rows(0, m, re, w, whole)
    assert _first_difference(whole, want) is None
    assert g.last_ld_ms() > 0.0
    # one row at a time, into a buffer whose other rows must stay as they are
    for j in range(m):
        buf = np.full(int(ip[-1]), -7.0, dtype=np.float32)
        g.ld_rows(j, j + 1, re, w, buf[ip[j]:ip[j + 1]])
        assert np.array_equal(buf[ip[j]:ip[j + 1]], want[ip[j]:ip[j + 1]]), j
        assert np.all(buf[:ip[j]] == -7.0) and np.all(buf[ip[j + 1]:] == -7.0), j
    # ranges that start and end inside tiles and fragments
    for r0, r1 in ((0, 0), (5, 37), (31, 33), (63, 65), (64, 128), (100, 200), (199, 200)):
        buf = np.full(int(ip[r1] - ip[r0]), -7.0, dtype=np.float32)
        g.ld_rows(r0, r1, re, w, buf)
        assert np.array_equal(buf, want[ip[r0]:ip[r1]]), (r0, r1)
    # max_bytes below a tile row: one tile row per call
    gip, got = g.ld(re, dtype=np.float32, max_bytes=1)
    assert np.array_equal(gip, ip) and _first_difference(got, want) is None
    gip, got = g.ld(re, dtype=np.float32, max_bytes=int(ip[128]) * 4)
    assert _first_difference(got, want) is None
    g.close()


def test_refusals_that_need_the_object(gpu):
    from viprs_amd import _lib as L
    m, n = 6, 20
    rows, _ = _case(np.random.default_rng(17), m, n, "random")
    g = G.DeviceGenotypes(rows, n)
    w = G.ld_stats(g.counts())[2]
    out = np.full(15, -7.0, dtype=np.float32)
    for re, word in (([6, 5, 6, 6, 6, 6], "non-decreasing"), ([6, 6, 6, 6, 6, 7], "[j + 1, m]"), ([0, 6, 6, 6, 6, 6], "[j + 1, m]")):
        with pytest.raises(ValueError) as e:
            g.ld_rows(0, 0, np.array(re), w, out[:0])
        assert word in str(e.value)
    full = np.full(m, m, dtype=np.int64)
    args = (full.ctypes.data_as(ctypes.c_void_p), w.ctypes.data_as(ctypes.c_void_p), L.LD_F32, out.ctypes.data_as(ctypes.c_void_p))
    assert L.lib.viprs_genotypes_ld(g.handle, -1, 3, *args) == L.EINVAL and "rows" in L.last_error()
    assert L.lib.viprs_genotypes_ld(g.handle, 0, 7, *args) == L.EINVAL and "rows" in L.last_error()
    assert np.all(out == -7.0)
    ms = ctypes.c_double(-1.0)
    assert L.lib.viprs_genotypes_last_ld_ms(g.handle, ctypes.byref(ms)) == L.EINVAL and "no timed LD call" in L.last_error()
    g.close()
    # n = 0: every SNP is all-missing, the store is zeros
    g0 = G.DeviceGenotypes(np.zeros((5, 0), dtype=np.uint8), 0)
    ip, data = g0.ld(dtype=np.int8)
    assert ip[-1] == 10 and np.all(data == 0)
    g0.close()


def test_rows_uploaded_after_a_call_are_seen(gpu):
    """The per-SNP tables and the clean tiles follow the rows: a clean panel, one LD call, then rows with missing codes."""
    from viprs_amd import _lib as L
    m, n = 70, 90
    rng = np.random.default_rng(29)
    clean, _ = _case(rng, m, n, "none")
    dirty, _ = _case(rng, m, n, "random")
    g = G.DeviceGenotypes(clean, n)
    assert _first_difference(g.ld(dtype=np.float64)[1], G.ld_host(clean, n, np.full(m, m), np.float64)[1]) is None
    L.check(L.lib.viprs_genotypes_upload_rows(g.handle, 0, m, dirty.ctypes.data_as(ctypes.c_void_p)))
    w = G.ld_stats(G.counts_host(dirty, n))[2]
    ip, want = G.ld_host(dirty, n, np.full(m, m), np.float64)
    got = g.ld_rows(0, m, np.full(m, m), w, np.zeros(int(ip[-1])))
    assert _first_difference(got, want) is None
    g.close()


def test_headroom_at_the_sample_limit(gpu):
    """n = 2^19, where the terms of num reach 2^58: SNPs 0 and 1 are all code 0 (w = 0), 2 .. 7 are balanced 0 / 3 -- code 0
    on half the samples, the half shifted by n / 16 from SNP to SNP, so that they correlate strongly -- and half the samples
    of SNPs 4 and 5 are missing.  One more sample is refused."""
    n, m = 1 << 19, 8
    s = np.arange(n)
    codes = np.zeros((m, n), dtype=np.uint8)
    for k in range(2, m):
        codes[k] = np.where((s >= k * n // 16) & (s < k * n // 16 + n // 2), 0, 3)
    codes[4, : n // 2] = 1
    codes[5, (s >> 3) & 1 == 1] = 1
    rows = pack_codes(codes)
    nn, a, w = G.ld_stats(G.counts_host(rows, n))
    assert w[0] == 0.0 and w[1] == 0.0 and np.all(w[2:] > 0.0)
    assert int(nn[2]) * int(nn[3]) * n >= 1 << 56                    # the terms of num are this large
    g = G.DeviceGenotypes(rows, n)
    for T in (np.float64, np.int16):
        ip, want = G.ld_host(rows, n, np.full(m, m), T)
        gip, got = g.ld(dtype=T)
        assert np.array_equal(gip, ip) and _first_difference(got, want) is None, _first_difference(got, want)
    r = G.ld_host(rows, n, np.full(m, m), np.float64)[1]
    assert np.all(r[:13] == 0.0) and np.count_nonzero(r[13:]) >= 3
    g.close()
    big = n + 1
    gb = G.DeviceGenotypes(np.zeros((2, (big + 3) // 4), dtype=np.uint8), big)
    with pytest.raises(ValueError, match=r"2\^19"):
        gb.ld()
    out = np.full(1, -7.0, dtype=np.float32)
    with pytest.raises(ValueError, match=r"2\^19"):                   # the library's own refusal
        gb.ld_rows(0, 2, np.array([2, 2]), np.ones(2), out)
    assert out[0] == -7.0
    gb.close()


def test_host_and_device_classes_agree(gpu):
    rng = np.random.default_rng(19)
    rows, _ = _case(rng, 90, 150, "random")
    h, d = G.HostGenotypes(rows, 150), G.DeviceGenotypes(rows, 150)
    for window in (None, ("windowed", 20), ("block", [33, 70]), ("windowed_bp", 15, np.sort(rng.integers(0, 400, 90)))):
        for T in (np.float32, np.int16):
            (hip_, hd), (dip, dd) = h.ld(window, dtype=T), d.ld(window, dtype=T)
            assert np.array_equal(hip_, dip) and _first_difference(dd, hd) is None, window
    d.close()


def test_loader_computes_ld_and_a_model_fits_on_it(gpu, tmp_path):
    from viprs_amd.data import ArrayDataLoader, LDArrays, SumstatsArrays
    from viprs_amd.io.zarr_ld import ZarrLDMatrix
    from viprs_amd.model import VIPRS
    m, n = 150, 400
    rng = np.random.default_rng(23)
    rows, _ = _case(rng, m, n, "random")
    est = ("block", [60, 101])
    beta_hat = rng.normal(scale=0.01, size=m).astype(np.float32)
    ss = lambda: {1: SumstatsArrays(beta_hat, np.full(m, 5e4))}
    for T in (np.float32, np.int8):
        gdl = ArrayDataLoader({}, ss(), genotype={1: (rows, n)})
        gdl.compute_ld(est, dtype=T)
        ip, data = G.ld_host(rows, n, G.ld_windows(est, m), T)
        got = gdl.ld[1].load(return_symmetric=False)
        assert np.array_equal(got.ld_indptr, ip) and np.array_equal(got.ld_data, data) and got.ld_data.dtype == T
        assert gdl.ld[1].sample_size == n
        direct = ArrayDataLoader({1: LDArrays(upper=(np.arange(1, m + 1, dtype=np.int32), ip, data),
                                              dq_scale=G.ld_dq_scale(T), sample_size=n)}, ss())
        for low_memory in (True, False):
            kw = dict(low_memory=low_memory, dequantize_on_the_fly=T == np.int8 and low_memory)
            theta = {"pi": 0.1, "sigma_epsilon": 0.9}   # (the default starting point is a random draw)
            a = VIPRS(gdl, **kw).fit(max_iter=20, theta_0=theta)
            b = VIPRS(direct, **kw).fit(max_iter=20, theta_0=theta)
            assert np.array_equal(a.post_mean_beta[1], b.post_mean_beta[1])
            assert np.all(np.isfinite(a.post_mean_beta[1])) and np.any(a.post_mean_beta[1] != 0.0)
        paths = gdl.write_ld_stores(tmp_path / np.dtype(T).name)
        z = ZarrLDMatrix(paths[1])
        assert z.ld_estimator == "block" and z.sample_size == n
        back = z.load()
        assert np.array_equal(back.ld_indptr, ip) and np.array_equal(back.ld_data, data) and back.ld_data.dtype == T
        gdl.close_genotypes()
