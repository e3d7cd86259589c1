"""The LD scores `viprs_plan_ld_scores` (include/viprs_hip.h) against the host reference of tests/ld_score_reference.py:
exact cases compared with `==`, random cases against the rounding bound of the header's definition, every bit against the
host replay of the header's order (tests/order_replay.py), independence / determinism, and the model layer
(`LDPredInf(gdl)`, `h2_init="ldsc"`, `annotate_ld_scores`)."""
import ctypes
import functools

import numpy as np
import pytest

from tests import ld_score_reference as SR
from tests import order_replay as OR
from tests.test_gpu_ld_dot import REPLAY_LD, _banded_windows, _float64_sweep, first_difference, replay_case
from viprs_amd.utils import synthetic as syn

pytestmark = pytest.mark.gpu

# block sizes straddling one 16-byte load (4 / 8 / 16 elements), one pass of a wavefront (256 / 512 / 1024 elements) and the
# 64-column padding of the dense squares
DENSE_SIZES = (1, 63, 64, 65, 255, 257, 511, 513, 1023, 1025, 1537, 2305)
SMALL_SIZES = (500, 65, 257)
N_COLS = (1, 2, 3, 5, 32, 33)
KMAX = 15
CORR = 2.0 ** -10
LD_DTYPES = {"int8": np.int8, "int16": np.int16, "fp32": np.float32, "int32": np.int32, "int64": np.int64, "fp64": np.float64}


def _int_blocks(sizes, low_memory, seed):
    """Dense blocks in either form with random integer entries k in [-KMAX, KMAX]: (left_bound, indptr, k as float64)."""
    rng = np.random.default_rng(seed)
    sk = syn.make_ld(sizes, low_memory=low_memory, ld_dtype=np.float32, data=False)
    lb, ip = sk.ld_left_bound, sk.ld_indptr
    ints = np.empty(int(ip[-1]), dtype=np.float64)
    o = 0
    for b in sizes:
        K = np.triu(rng.integers(-KMAX, KMAX + 1, (b, b)), 1)
        K = K + K.T + KMAX * np.eye(b, dtype=np.int64)
        if low_memory:
            for r in range(b - 1):
                ints[o:o + b - 1 - r] = K[r, r + 1:]
                o += b - 1 - r
        else:
            ints[o:o + b * b] = K.ravel()
            o += b * b
    return lb, ip, ints


@functools.lru_cache(maxsize=None)
def _exact_case(kind, low_memory):
    """The windows, the integer entries, integer weights in {0, 1, 2} and the exact sums for them and for unit weights
    (computed once, shared by every LD dtype and state precision, never modified)."""
    if kind == "dense":
        lb, ip, ints = _int_blocks(DENSE_SIZES, low_memory, seed=41)
    elif kind == "small":
        lb, ip, ints = _int_blocks(SMALL_SIZES, low_memory, seed=42)
    else:
        lb, ip = _banded_windows(2500, 90, 140, low_memory, seed=14, jitter=60)
        ints = np.random.default_rng(43).integers(-KMAX, KMAX + 1, int(ip[-1])).astype(np.float64)
    m = lb.shape[0]
    A = np.random.default_rng(44).integers(0, 3, (m, max(N_COLS))).astype(np.float64)
    ref = SR.sums(lb, ip, ints, low_memory, A, mode="int")
    unit = SR.sums(lb, ip, ints, low_memory, None, mode="int")
    # every S2 * 256 and every S0 is an integer below 2^24: any summation order is exact in float32
    for r in (ref, unit):
        assert r["P"].max() < 2 ** 24 and r["Q"].max() < 2 ** 24
    for a in (lb, ip, ints, A, *ref.values(), *unit.values()):
        a.setflags(write=False)
    return lb, ip, ints, A, ref, unit


EXACT_CASES = [(k, l) for k in ("dense", "small", "banded") for l in ("int8", "fp32")] + \
              [(k, l) for k in ("small", "banded") for l in ("int16", "int32", "int64", "fp64")]


@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("low_memory", [False, True])
@pytest.mark.parametrize("kind, ld_name", EXACT_CASES)
def test_exact_arithmetic(gpu, kind, ld_name, low_memory, T):
    """Inputs on which every summation order is exact: a dropped, doubled or misplaced entry, a wrong mirror, a counted
    diagonal or a gap counted as an entry changes the result; nothing else can.  The epilogue is replayed in T."""
    from viprs_amd import _lib as L
    from viprs_amd.plan import LDPlan
    lb, ip, ints, A, ref, unit = _exact_case(kind, low_memory)
    ld_dtype = LD_DTYPES[ld_name]
    floating = np.issubdtype(ld_dtype, np.floating)
    data = (ints / 16.0).astype(ld_dtype) if floating else ints.astype(ld_dtype)
    dq, den = (1.0, 256.0) if floating else (1.0 / 16.0, 1.0)      # S2 as the device holds it: sum of p = (k / 16)^2 or k^2
    m = lb.shape[0]
    corr = np.full(m, CORR)
    plan = LDPlan(lb, ip, data, low_memory)

    def check(storage):
        for n in N_COLS + (None,):
            if n is None:
                An, S2, S0 = None, unit["S2"] / den, unit["S0"]
            elif n == 1:
                An, S2, S0 = A[:, 0].astype(T), ref["S2"][:, 0] / den, ref["S0"][:, 0]
            else:
                An, S2, S0 = A[:, :n].astype(T), ref["S2"][:, :n] / den, ref["S0"][:, :n]
            for c in (None, corr):
                got = plan.ld_scores(An, c, dq_scale=dq, float_precision=np.dtype(T).name)
                want = SR.finish(S2, S0, An, c, dq, T)
                assert got.shape == want.shape and got.dtype == np.dtype(T)
                bad = got != want
                assert not bad.any(), (f"{kind} {ld_name} upper={low_memory} {storage} n_cols={n} corr={c is not None}: "
                                       f"{int(bad.sum())} entries differ, first row {int(np.argwhere(bad)[0][0])}")
    try:
        check("as created")
        if low_memory:
            # the dense blocks in the float64 sweeps' storage (zero lower triangle): entries left of the diagonal are gathered
            # from the column above it
            dense = plan.info(L.INFO_N_DENSE) > 0
            assert not dense or plan.info(L.INFO_UPPER_MIRRORED) == 1
            _float64_sweep(plan)
            assert not dense or plan.info(L.INFO_UPPER_MIRRORED) == 0
            check("zero lower triangle")
            assert not dense or plan.info(L.INFO_UPPER_MIRRORED) == 0, "the call converted the storage"
    finally:
        plan.close()


@functools.lru_cache(maxsize=None)
def _random_case(kind, ld_name, low_memory):
    """Random LD, Gaussian weights with float32 values (exact in both state precisions) and the exact sums for them and
    for unit weights: computed once, shared by both state precisions."""
    ld = syn.make_ld([700, 300, 1537, 64], low_memory=low_memory, ld_dtype=LD_DTYPES[ld_name], kind=kind, seed=5)
    rng = np.random.default_rng(6)
    A = rng.standard_normal((ld.m, 3)).astype(np.float32)
    corr = rng.uniform(0.0, 0.01, ld.m)
    # x = T(stored) is exact for these LD dtypes; the reference squares it in float64
    refs = [SR.sums(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, low_memory, An, mode="fsum") for An in (A, None)]
    return ld, A, corr, refs


@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("low_memory", [False, True])
@pytest.mark.parametrize("kind, ld_name", [("ar1", "fp32"), ("sample", "fp32"), ("sample", "int8"), ("sample", "int16"),
                                           ("ar1", "int16")])
def test_rounding_bound(gpu, kind, ld_name, low_memory, T):
    """Real-valued LD (integer LD at full range: int16 squares above 2^24 round in a float32 state, which is part of the
    definition) and Gaussian weights (signed: the sums cancel), against the bound derived in tests/ld_score_reference.py
    from the header's order."""
    from viprs_amd.plan import LDPlan
    ld, A32, corr, refs = _random_case(kind, ld_name, low_memory)
    A = A32.astype(T)
    item = ld.ld_data.dtype.itemsize
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, low_memory)
    try:
        for An, ref in zip((A, None), refs):
            for c in (None, corr):
                got = plan.ld_scores(An, c, dq_scale=ld.dq_scale, float_precision=np.dtype(T).name).astype(np.float64)
                exact = SR.exact_score(ref, c, ld.dq_scale, T)
                bound = SR.bound(ref, c, ld.dq_scale, T, item)
                err = np.abs(got - exact)
                print(f"rounding {kind} {ld_name} upper={low_memory} {np.dtype(T).name} unit={An is None} "
                      f"corr={c is not None}: worst err/bound = "
                      f"{float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny))):.4f}")
                assert np.all(err <= bound)
                assert np.any(got != (1.0 if An is None else An.astype(np.float64)))
    finally:
        plan.close()


# ---- every bit against the host replay of THE ORDER ------------------------------------------------------------------------
REPLAY_COLS = (1, 3, 7)        # the kernels carry 4, 2 or 1 columns per pass over a row: 7 = 4 + 2 + 1, 3 = 2 + 1


@functools.lru_cache(maxsize=None)
def replay_weights(T):
    """Gaussian weights, (m, 7) column-major in T, and the correction c_j (doubles), shared by every case."""
    m = replay_case("int8", False)[0].shape[0]
    rng = np.random.default_rng(26)
    A = np.asfortranarray(rng.standard_normal((m, max(REPLAY_COLS))).astype(T))
    corr = rng.uniform(0.0, 0.01, m)
    A.setflags(write=False)
    corr.setflags(write=False)
    return A, corr


@functools.lru_cache(maxsize=None)
def replayed_sums(ld_name, low_memory, T):
    """((S2, S0) for the Gaussian weights, (S2, S0) for unit weights) in the header's order: one replay per case."""
    lb, ip, data, _ = replay_case(ld_name, low_memory)
    out = (OR.replay_scores(lb, ip, data, low_memory, replay_weights(T)[0], T),
           OR.replay_scores(lb, ip, data, low_memory, None, T))
    for pair in out:
        for a in pair:
            a.setflags(write=False)
    return out


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
@pytest.mark.parametrize("ld_name", sorted(REPLAY_LD))
def test_bits_are_the_headers_order(gpu, ld_name, low_memory, T):
    """`got == finish(replay)` and nothing else, on the matrix of the product's test: p = fl(x x), S2 by fma(p, a, acc) and
    S0 by plain additions into the slots of THE ORDER, then the header's epilogue operation by operation.  Gaussian and unit
    weights, with and without the correction, both storages of the upper form."""
    from viprs_amd import _lib as L
    from viprs_amd.plan import LDPlan
    lb, ip, data, starts = replay_case(ld_name, low_memory)
    dq = 1.0 if np.issubdtype(data.dtype, np.floating) else 1.0 / np.iinfo(data.dtype).max
    (A, corr), ((S2, S0), (U2, U0)) = replay_weights(T), replayed_sums(ld_name, low_memory, T)
    plan = LDPlan(lb, ip, data, low_memory)

    def check(storage):
        for n in REPLAY_COLS + (None,):
            if n is None:
                An, s2, s0 = None, U2, U0
            elif n == 1:
                An, s2, s0 = A[:, 0], S2[:, 0], S0[:, 0]
            else:
                An, s2, s0 = A[:, :n], S2[:, :n], S0[:, :n]
            for c in (None, corr):
                got = plan.ld_scores(An, c, dq_scale=dq, float_precision=np.dtype(T).name)
                diff = first_difference(got, SR.finish(s2, s0, An, c, dq, T), starts)
                assert not diff, (f"{ld_name} upper={low_memory} {np.dtype(T).name} {storage} n_cols={n} "
                                  f"corr={c is not None}: {diff}")
    try:
        check("as created")
        if low_memory:
            _float64_sweep(plan)
            assert plan.info(L.INFO_N_DENSE) == 0 or plan.info(L.INFO_UPPER_MIRRORED) == 0
            check("zero lower triangle")
    finally:
        plan.close()


@pytest.mark.parametrize("low_memory", [False, True])
def test_independence_and_determinism(gpu, low_memory):
    from viprs_amd.plan import LDPlan
    sizes = [65, 257, 1537, 500, 300, 90]
    ld = syn.make_ld(sizes, low_memory=low_memory, kind="longrange", ld_dtype=np.int8, seed=8)
    m = ld.m
    rng = np.random.default_rng(9)
    A = rng.standard_normal((m, 33)).astype(np.float32)
    corr = rng.uniform(0.0, 0.01, m)
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, low_memory)
    try:
        kw = dict(correction=corr, dq_scale=ld.dq_scale)
        ring = plan.timing_history()
        y = plan.ld_scores(A, **kw)
        assert np.array_equal(y, plan.ld_scores(A, **kw)), "a repeated call changed bits"
        for g in (0, 13, 32):
            assert np.array_equal(plan.ld_scores(A[:, g], **kw), y[:, g]), f"column {g} depends on the other columns"
        unit = plan.ld_scores(None, **kw)
        assert np.array_equal(unit, plan.ld_scores(np.ones(m, dtype=np.float32), **kw)), "unit weights != a column of ones"
        ones = np.ones((m, 5), dtype=np.float32)
        assert np.array_equal(plan.ld_scores(ones, **kw), np.repeat(unit[:, None], 5, axis=1))
        plan.set_active_blocks(np.arange(plan.n_blocks) % 2 == 0)
        assert np.array_equal(plan.ld_scores(A, **kw), y), "the active-block filter of the sweeps reached the call"
        assert np.array_equal(plan.ld_scores(None, **kw), unit)
        plan.set_active_blocks(None)
        assert plan.last_ld_score_ms() > 0.0
        # the sweeps' timing ring never sees the call
        assert plan.timing_history() == ring
    finally:
        plan.close()
    # a block's scores do not depend on the other blocks of the plan
    starts = np.concatenate([[0], np.cumsum(sizes)])
    for bi in (1, 2, 5):
        one = syn.make_ld(sizes, low_memory=low_memory, kind="longrange", ld_dtype=np.int8, seed=8)
        s, e = int(starts[bi]), int(starts[bi + 1])
        ip = one.ld_indptr[s:e + 1] - one.ld_indptr[s]
        lb = np.where(np.diff(ip) > 0, one.ld_left_bound[s:e] - s, np.minimum(one.ld_left_bound[s:e] - s, e - s - 1)).astype(np.int32)
        data = np.ascontiguousarray(one.ld_data[int(one.ld_indptr[s]):int(one.ld_indptr[e])])
        alone = LDPlan(np.ascontiguousarray(lb), np.ascontiguousarray(ip), data, low_memory)
        try:
            assert np.array_equal(alone.ld_scores(np.ascontiguousarray(A[s:e]), corr[s:e], dq_scale=ld.dq_scale), y[s:e])
        finally:
            alone.close()


def test_argument_checks_with_a_plan(gpu):
    from viprs_amd import _lib as L
    from viprs_amd.plan import LDPlan
    ld = syn.make_ld([65, 30], low_memory=True, kind="longrange", ld_dtype=np.int8, seed=8)
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, True)
    try:
        y = np.full(ld.m, 7.0, dtype=np.float32)
        a = np.ones(ld.m, dtype=np.float32)
        py, pa = y.ctypes.data_as(ctypes.c_void_p), a.ctypes.data_as(ctypes.c_void_p)
        ms = ctypes.c_double(-1.0)
        assert L.lib.viprs_plan_last_ld_score_ms(plan.handle, ctypes.byref(ms)) == L.EINVAL and ms.value == -1.0
        for args in ((7, 1, pa, None, py, 1.0), (L.F32, 0, pa, None, py, 1.0), (L.F32, 2, None, None, py, 1.0),
                     (L.F32, 1, pa, None, None, 1.0)):
            assert L.lib.viprs_plan_ld_scores(plan.handle, *args) == L.EINVAL
        assert np.all(y == 7.0)
        with pytest.raises(ValueError):
            plan.ld_scores(np.ones(ld.m + 1, dtype=np.float32))
        with pytest.raises(ValueError):
            plan.ld_scores(correction=np.ones(ld.m + 1))
    finally:
        plan.close()
    empty = LDPlan(np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.int8), True)
    try:
        assert empty.ld_scores().shape == (0,)
        assert L.lib.viprs_plan_ld_scores(empty.handle, L.F32, 1, None, None, py, 1.0) == L.OK and np.all(y == 7.0)
    finally:
        empty.close()


def _gdl():
    from viprs_amd.data import ArrayDataLoader
    return ArrayDataLoader.synthetic({1: [300, 130], 2: [257], 3: [65, 90]}, ld_dtype=np.int8, n=5e4, kind="longrange", ld_sample_size=5e4)


def _host_scores_and_error(gdl, dq_on_the_fly=True):
    """Float64 host scores of every chromosome (corrected, upper form, int8 LD dequantised on the fly) and the bound e_j of
    |float32 device score - host score|: the device's rounding bound (tests/ld_score_reference.py) plus what the definition
    itself rounds -- d = fl32(dq_scale) (relative u32, twice in d^2: eps32 d^2 P) and c = fl32(corr) (u32 |c| (d^2 P + Q))."""
    from viprs_amd.stats import ldsc
    host, err = {}, {}
    eps = float(np.finfo(np.float32).eps)
    for c, ld in gdl.ld.items():
        lop = ld.load(return_symmetric=False, dtype=np.int8)
        m = gdl.shapes[c]
        corr = np.full(m, 1.0 / (ld.sample_size - 2.0))
        dq = ld.dq_scale
        host[c] = ldsc.ld_scores_host(lop.leftmost_idx, lop.ld_indptr, lop.ld_data, True, None, corr, dq)
        ref = SR.sums(lop.leftmost_idx, lop.ld_indptr, lop.ld_data, True, None, mode="fsum")
        err[c] = SR.bound(ref, corr, dq, np.float32, 1) + eps * dq * dq * ref["P"] + \
            0.5 * eps * corr * (dq * dq * ref["P"] + ref["Q"])
    return host, err


def test_model_layer_ldpredinf(gpu):
    """`LDPredInf(gdl)` on the device against `LDPredInf(gdl, h2=simple_ldsc on the host in float64)`.

    h2 = K / mean(l) with K = (mean(chi2) - 1) M / mean(N) formed in float64 on both sides.  The float32 device scores are
    within e_j of the host's (`_host_scores_and_error`), so the means differ by at most E = mean(e_j) and
    |h2_dev - h2_host| <= tol = h2_host E / (mean(l) - E).  Both models then solve with lam = M / (N h2): the two penalties
    differ by at most tol / (h2_host - tol), relatively."""
    from viprs_amd.model import LDPredInf
    from viprs_amd.stats import ldsc
    gdl = _gdl()
    host, err = _host_scores_and_error(gdl)
    h2_host = ldsc.simple_ldsc(gdl, ld_scores=host)
    chroms = sorted(host)
    ell = np.concatenate([host[c] for c in chroms])
    E = float(np.concatenate([err[c] for c in chroms]).mean())
    tol = h2_host * E / (ell.mean() - E)
    dev = LDPredInf(gdl, dequantize_on_the_fly=True)
    print(f"LDPredInf h2: device {dev.h2!r} host {h2_host!r} |diff| {abs(dev.h2 - h2_host):.3e} tol {tol:.3e}")
    assert 0.0 < h2_host <= 1.0 and abs(dev.h2 - h2_host) <= tol
    for c in chroms:
        assert np.all(np.abs(dev.ld_score[c] - host[c]) <= err[c])
    ref = LDPredInf(gdl, h2=h2_host, dequantize_on_the_fly=True)
    dev.fit()
    ref.fit()
    assert dev.solve_info.converged and ref.solve_info.converged
    assert dev.lam == gdl.m / (dev.n * dev.h2) and abs(dev.lam / ref.lam - 1.0) <= tol / (h2_host - tol)
    assert all(np.any(dev.post_mean_beta[c] != 0) for c in chroms)


def test_model_layer_per_chromosome_start(gpu):
    """`VIPRSPerChromosome(h2_init="ldsc")` starts every chromosome at its own clipped estimate (scores of the model's one
    merged plan, float32, within the bound of the host's)."""
    from viprs_amd.model import VIPRSPerChromosome
    from viprs_amd.stats import ldsc
    gdl = _gdl()
    host, err = _host_scores_and_error(gdl)
    model = VIPRSPerChromosome(gdl, dequantize_on_the_fly=True, h2_init="ldsc")
    model.fit(max_iter=2, theta_0={"pi": 0.02})
    ss = gdl.sumstats_table
    for c in model.groups:
        assert np.all(np.abs(model.ld_score[c] - host[c]) <= err[c]) and np.any(model.ld_score[c] != 1.0)
        want = ldsc.ldsc_estimate(ldsc.chisq_statistic(ss[c]), model.ld_score[c], ss[c].n_per_snp)
        assert model.h2_ldsc[c] == want
        h2 = float(np.clip(want, 0.01, 0.99))
        pi, sig, tau = model._theta_for(c, {"pi": 0.02})
        assert sig == 1.0 - h2 and tau == 0.02 * gdl.shapes[c] / h2
        E = float(err[c].mean())
        h2_host = ldsc.ldsc_estimate(ldsc.chisq_statistic(ss[c]), host[c], ss[c].n_per_snp)
        assert abs(want - h2_host) <= abs(h2_host) * E / (host[c].mean() - E)
    assert len({model.h2_ldsc[c] for c in model.groups}) == len(model.groups)
    # the first recorded hyper-parameters come from that start: one M-step away from 1 - h2, not from a random draw
    again = VIPRSPerChromosome(gdl, dequantize_on_the_fly=True, h2_init="ldsc")
    again.fit(max_iter=2, theta_0={"pi": 0.02})
    for c in model.groups:
        assert model.history[c]["ELBO"] == again.history[c]["ELBO"]


def test_annotate_ld_scores(gpu):
    from viprs_amd.stats import ldsc
    gdl = _gdl()
    host, err = _host_scores_and_error(gdl)
    got = ldsc.annotate_ld_scores(gdl, dequantize_on_the_fly=True)
    for c, ld in gdl.ld.items():
        assert ld.ld_score.dtype == np.float64 and np.array_equal(ld.ld_score, got[c])
        assert np.all(np.abs(ld.ld_score - host[c]) <= err[c])
    assert ldsc.simple_ldsc(gdl) == ldsc.simple_ldsc(gdl, ld_scores=got)
    # stratified scores: the columns of an annotation matrix; a column of ones is the unstratified score
    c = 1
    A = np.ones((gdl.shapes[c], 2), dtype=np.float32)
    A[::2, 1] = 0.0
    strat = ldsc.ld_scores(gdl.ld[c], annotation=A, dequantize_on_the_fly=True)[None]
    assert strat.shape == A.shape and np.array_equal(strat[:, 0], got[c]) and np.any(strat[:, 1] != strat[:, 0])


@pytest.mark.parametrize("ld_dtype", [np.int8, np.float32], ids=["int8-on-the-fly", "fp32"])
def test_ld_scores_of_an_upper_only_store_stay_in_the_upper_form(gpu, ld_dtype):
    """`ld_scores(low_memory=False)` of LD objects that hold only the upper-triangular store scores them in that form: the
    upper-form kernels over the same arrays as with ``low_memory=True``, hence the same bits.  Two chromosomes with a
    single-SNP block, a small one and one past 64 SNPs."""
    from viprs_amd.data import ArrayDataLoader
    from viprs_amd.stats import ldsc
    sizes = {1: [1, 5, 33, 70], 2: [3, 66]}
    gdl = ArrayDataLoader.synthetic(sizes, ld_dtype=ld_dtype, forms=("upper",), ld_sample_size=400)
    got = ldsc.ld_scores(gdl, low_memory=False, dequantize_on_the_fly=True)
    want = ldsc.ld_scores(gdl, low_memory=True, dequantize_on_the_fly=True)
    assert sorted(got) == sorted(want) == [1, 2]
    for c in want:
        assert got[c].shape == (sum(sizes[c]),) and np.all(np.isfinite(got[c])) and np.array_equal(got[c], want[c])
        assert got[c][0] == 1.0 if c == 1 else got[c][0] > 1.0      # (the single-SNP block: the diagonal alone)
