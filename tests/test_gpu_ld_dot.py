"""The LD product `viprs_plan_dot` / `viprs_state_dot` (include/viprs_hip.h) against the host reference of
tests/ld_dot_reference.py: exact cases compared with `==`, random cases against the rounding bound the header's order
contract implies, every bit against the host replay of the header's order (tests/order_replay.py), independence /
determinism, the state entry point, consistency with the sweep's own `q`, and the model layer (pseudo-validation against an
external LD panel)."""
import functools
import os

import numpy as np
import pytest

from tests import ld_dot_reference as R
from tests import order_replay as OR
from viprs_amd.utils import synthetic as syn

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# block sizes straddling every edge of the kernels: one 16-byte load (4 / 8 / 16 elements), one pass of a wavefront
# (256 / 512 / 1024 elements), the 64-column padding of the dense squares; one block of several thousand SNPs
RAGGED_SIZES = (1, 63, 64, 65, 255, 257, 511, 513, 1023, 1025, 1537, 2305, 8001)
N_COLS = (1, 2, 3, 4, 5, 31, 32, 33)


def _int_block_ld(sizes, low_memory, ld_dtype, seed, kmax=127):
    """Dense blocks in either form with random integer entries k in [-kmax, kmax] (fp32 LD: k / 128); returns the arrays
    and the entries as integers (float64) for the exact host product."""
    rng = np.random.default_rng(seed)
    sk = syn.make_ld(sizes, low_memory=low_memory, ld_dtype=ld_dtype, data=False)
    lb, ip = sk.ld_left_bound, sk.ld_indptr
    ints = np.empty(int(ip[-1]), dtype=np.float64)
    o = 0
    for b in sizes:
        K = np.triu(rng.integers(-kmax, kmax + 1, (b, b)), 1)
        K = K + K.T + kmax * np.eye(b, dtype=np.int64)
        if low_memory:
            for r in range(b - 1):
                ints[o:o + b - 1 - r] = K[r, r + 1:]
                o += b - 1 - r
        else:
            ints[o:o + b * b] = K.ravel()
            o += b * b
    data = (ints / 128.0).astype(ld_dtype) if np.issubdtype(ld_dtype, np.floating) else ints.astype(ld_dtype)
    return lb, ip, data, ints


def _banded_windows(m, w_left, w_right, low_memory, seed, jitter):
    """Jittered row windows [j - wl_j, j + wr_j] (symmetric form) / [j + 1, j + wr_j] (upper form), as the band tests
    build them."""
    rng = np.random.default_rng(seed)
    j = np.arange(m)
    wl = np.full(m, w_left) - (rng.integers(0, jitter + 1, m) if jitter else 0)
    wr = np.full(m, w_right) - (rng.integers(0, jitter + 1, m) if jitter else 0)
    lo = j + 1 if low_memory else np.maximum(j - np.maximum(wl, 0), 0)
    hi = np.minimum(j + np.maximum(wr, 0) + 1, m)
    length = np.maximum(hi - lo, 0)
    ip = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    lb = np.where(length > 0, lo, np.minimum(lo, m - 1)).astype(np.int32)
    return lb, ip


@functools.lru_cache(maxsize=None)
def _exact_case(kind, ld_name, low_memory):
    ld_dtype = {"int8": np.int8, "int16": np.int16, "fp32": np.float32, "int32": np.int32, "int64": np.int64,
                "fp64": np.float64}[ld_name]
    floating = np.issubdtype(ld_dtype, np.floating)
    bmax, kmax = 8, 127
    if ld_name == "int16":
        bmax, kmax = 1, 32767                      # 32767 * 1 * 500 < 2^24
    if kind == "single":
        lb, ip, data, ints = _int_block_ld((500,), low_memory, ld_dtype, seed=11)
    elif kind == "ragged":
        lb, ip, data, ints = _int_block_ld(RAGGED_SIZES, low_memory, ld_dtype, seed=12)
    elif kind == "small":                          # (LD dtypes without dense squares: these blocks are windowed rows)
        lb, ip, data, ints = _int_block_ld((500, 65, 257), low_memory, ld_dtype, seed=13, kmax=kmax)
    else:
        lb, ip = _banded_windows(2500, 90, 140, low_memory, seed=14, jitter=60)
        ints = np.random.default_rng(15).integers(-kmax, kmax + 1, int(ip[-1])).astype(np.float64)
        data = (ints / 128.0).astype(ld_dtype) if floating else ints.astype(ld_dtype)
    m = lb.shape[0]
    B = np.random.default_rng(16).integers(-bmax, bmax + 1, (m, max(N_COLS))).astype(np.float64)
    ref = R.reference(lb, ip, ints, low_memory, B, mode="int")
    # every product and partial sum is an integer (fp32 LD: a multiple of 1/128) below 2^24: any order is exact in float32
    assert ref["abs_terms"].max() < 2 ** 24
    den = 128.0 if floating else 1.0
    return lb, ip, data, B, ref["exact"] / den


EXACT_CASES = [(k, l, f) for k in ("single", "ragged", "banded") for l in ("int8", "fp32") for f in (False, True)] + \
              [(k, l, f) for k, l in (("small", "int16"), ("banded", "int16"), ("small", "int32"), ("small", "int64"),
                                      ("small", "fp64"), ("banded", "int32")) for f in (False, True)]


def _float64_sweep(plan):
    """One float64 E-step sweep on the plan (the values do not matter): on an upper-form plan it leaves the dense blocks
    with a ZERO lower triangle, the storage the product then has to read in place."""
    from viprs_amd.plan import DeviceState
    m = plan.m
    st = DeviceState(plan, "float64", placement="off")
    try:
        rng = np.random.default_rng(31)
        st.upload("std_beta", 0.01 * rng.standard_normal(m))
        st.upload("u_logs", np.full(m, -4.0))
        st.upload("sqrt_half_var_tau", np.full(m, 200.0))
        st.upload("mu_mult", np.full(m, 0.9))
        st.reset(0.01)
        st.e_step(1e-3)
    finally:
        st.close()


@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("kind, ld_name, low_memory", EXACT_CASES)
def test_exact_arithmetic(gpu, kind, ld_name, low_memory, T):
    """Inputs on which every summation order is exact: a dropped, doubled or misplaced entry, a wrong mirror or a counted
    diagonal changes the result; nothing else can."""
    from viprs_amd import _lib as L
    from viprs_amd.plan import LDPlan
    lb, ip, data, B, S = _exact_case(kind, ld_name, low_memory)
    plan = LDPlan(lb, ip, data, low_memory)

    def check(storage):
        for n in N_COLS:
            Bn = B[:, :n].astype(T) if n > 1 else B[:, 0].astype(T)
            Sn = S[:, :n] if n > 1 else S[:, 0]
            for dq in (1.0, 1.0 / 127.0):
                for inc in (False, True):
                    got = plan.dot(Bn, dq_scale=dq, include_diagonal=inc)
                    want = R.finish(Sn, Bn, dq, inc, T)
                    assert got.shape == Bn.shape and got.dtype == np.dtype(T)
                    bad = got != want
                    assert not bad.any(), (f"{kind} {ld_name} upper={low_memory} {storage} n_cols={n} dq={dq} diag={inc}: "
                                           f"{int(bad.sum())} entries differ, first row {int(np.argwhere(bad)[0][0])}")
    try:
        check("as created")
        if low_memory:
            # the same cases with the dense blocks in the float64 sweeps' storage (zero lower triangle): the product gathers
            # the entries left of the diagonal from the column above it -- a wrong transposed index shows here
            dense = plan.info(L.INFO_N_DENSE) > 0
            assert not dense or plan.info(L.INFO_UPPER_MIRRORED) == 1
            _float64_sweep(plan)
            assert not dense or plan.info(L.INFO_UPPER_MIRRORED) == 0
            check("zero lower triangle")
            assert not dense or plan.info(L.INFO_UPPER_MIRRORED) == 0, "the product converted the storage"
    finally:
        plan.close()


@pytest.mark.parametrize("ld_dtype", [np.float32, np.int8, np.int16])
def test_result_does_not_depend_on_the_upper_storage(gpu, ld_dtype):
    """Random LD, upper form: the product over the mirrored squares (as the first product and the fp32 sweeps leave them)
    and over the zero-lower-triangle storage (as the float64 sweeps leave them) gives the same bits (header contract)."""
    from viprs_amd import _lib as L
    from viprs_amd.plan import LDPlan
    ld, ss, inp = syn.make_problem(sizes=[65, 257, 1537, 500, 2305, 90], low_memory=True, ld_dtype=ld_dtype, seed=8,
                                   kind="longrange")
    rng = np.random.default_rng(10)
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, True)
    try:
        for T in (np.float32, np.float64):
            for B in (rng.standard_normal(ld.m).astype(T), rng.standard_normal((ld.m, 33)).astype(T)):
                st = _sweep_state(plan, inp, np.float32)
                st.e_step(ld.dq_scale)
                st.close()
                assert plan.info(L.INFO_UPPER_MIRRORED) == 1
                y_mirrored = plan.dot(B, dq_scale=ld.dq_scale)
                _float64_sweep(plan)
                assert plan.info(L.INFO_UPPER_MIRRORED) == 0
                y_zero_lower = plan.dot(B, dq_scale=ld.dq_scale)
                assert plan.info(L.INFO_UPPER_MIRRORED) == 0
                assert np.array_equal(y_mirrored, y_zero_lower)
                assert np.any(y_mirrored != B)
    finally:
        plan.close()


@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("low_memory", [False, True])
def test_rounding_bound(gpu, low_memory, T):
    """Random fp32 LD and Gaussian B (signed: the sums cancel).  The header's order puts D(W) additions on the longest
    path of a row, each term enters by one fused multiply-add (one rounding), then one rounded multiply by dq_scale and,
    with the diagonal, one rounded add of B: |got - exact| <= eps_T (D + 2) (sum |r_ji b_i| + |b_j|)."""
    from viprs_amd.plan import LDPlan
    ld = syn.make_ld([700, 300, 1537, 64], low_memory=low_memory, kind="longrange", seed=5)
    m = ld.m
    B = np.random.default_rng(6).standard_normal((m, 3)).astype(T)
    ref = R.reference(ld.ld_left_bound, ld.ld_indptr, ld.ld_data.astype(np.float64), low_memory, B.astype(np.float64))
    D = R.depth(ref["W"], ld.ld_data.dtype.itemsize)[:, None]
    eps = np.finfo(T).eps
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, low_memory)
    try:
        for inc in (False, True):
            got = plan.dot(B, include_diagonal=inc).astype(np.float64)
            exact = ref["exact"] + (B.astype(np.float64) if inc else 0.0)
            bound = eps * (D + 2) * (ref["abs_terms"] + (np.abs(B.astype(np.float64)) if inc else 0.0))
            err = np.abs(got - exact)
            print(f"rounding upper={low_memory} {np.dtype(T).name} diag={inc}: worst err/bound = "
                  f"{float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny))):.4f}")
            assert np.all(err <= bound)
    finally:
        plan.close()


# ---- every bit against the host replay of THE ORDER ------------------------------------------------------------------------
# the smallest sizes that cross every edge of the order: one 16-byte load, one pass of a wavefront at V = 4 / 8 / 16 (256 /
# 512 / 1024 columns) and two, sizes that are no multiple of V or of the dense kernel's rows per wavefront; then one
# jittered windowed component (gaps in the windows of the upper form)
REPLAY_SIZES = (1, 2, 63, 65, 257, 513, 1025, 1537)
REPLAY_LD = {"int8": np.int8, "int16": np.int16, "fp32": np.float32, "int32": np.int32, "fp64": np.float64}
REPLAY_COLS = (1, 3, 33)


def _unrepresentable(ld):
    """Float64 LD whose values are NOT float32 values: every entry (i, j) of a block times 1 + 2^-26 t_ij, t symmetric in
    (-1, 1) -- the conversion to a float32 state rounds."""
    rng = np.random.default_rng(23)
    data = ld.ld_data.astype(np.float64)
    o = 0
    for b in np.diff(ld.block_start):
        b = int(b)
        P = np.triu(rng.uniform(-1.0, 1.0, (b, b)), 1)
        P = 1.0 + 2.0 ** -26 * (P + P.T)
        if ld.low_memory:
            for r in range(b - 1):
                data[o:o + b - 1 - r] *= P[r, r + 1:]
                o += b - 1 - r
        else:
            data[o:o + b * b] *= P.ravel()
            o += b * b
    return data


@functools.lru_cache(maxsize=None)
def replay_case(ld_name, low_memory):
    """(left_bound, indptr, data, block starts): the dense blocks of REPLAY_SIZES with full-range "longrange" LD, then one
    windowed component of 2500 SNPs with uniform entries.  Computed once, never modified."""
    ld_dtype = np.dtype(REPLAY_LD[ld_name])
    ld = syn.make_ld(REPLAY_SIZES, low_memory=low_memory, ld_dtype=np.float32 if ld_name == "fp64" else ld_dtype,
                     kind="longrange", seed=5)
    dense = _unrepresentable(ld) if ld_name == "fp64" else ld.ld_data
    m0 = ld.m
    lb_w, ip_w = _banded_windows(2500, 90, 140, low_memory, seed=14, jitter=60)
    u = np.random.default_rng(24).uniform(-1.0, 1.0, int(ip_w[-1]))
    band = np.rint(u * np.iinfo(ld_dtype).max).astype(ld_dtype) if np.issubdtype(ld_dtype, np.integer) else u.astype(ld_dtype)
    lb = np.concatenate([ld.ld_left_bound, lb_w + m0]).astype(np.int32)
    ip = np.concatenate([np.asarray(ld.ld_indptr, dtype=np.int64), ip_w[1:] + int(ld.ld_indptr[-1])])
    data = np.concatenate([dense, band])
    assert data.dtype == ld_dtype
    if ld_name == "fp64":
        assert np.mean(data.astype(np.float32).astype(np.float64) != data) > 0.9
    starts = np.concatenate([ld.block_start, [m0 + 2500]]).astype(np.int64)
    for a in (lb, ip, data, starts):
        a.setflags(write=False)
    return lb, ip, data, starts


@functools.lru_cache(maxsize=None)
def replay_inputs(T):
    """Gaussian B, (m, 33) column-major in T (float64: full-precision values), shared by every case."""
    m = sum(REPLAY_SIZES) + 2500
    B = np.asfortranarray(np.random.default_rng(25).standard_normal((m, max(REPLAY_COLS))).astype(T))
    B.setflags(write=False)
    return B


@functools.lru_cache(maxsize=None)
def replayed_product(ld_name, low_memory, T):
    """S of every column in the header's order: one replay per case (a column depends on nothing but itself)."""
    lb, ip, data, _ = replay_case(ld_name, low_memory)
    S = OR.replay_dot(lb, ip, data, low_memory, replay_inputs(T))
    S.setflags(write=False)
    return S


def first_difference(got, want, starts):
    """'' if the arrays are equal, else the count, the first differing row, its block and the two values."""
    bad = np.asarray(got) != np.asarray(want)
    if not bad.any():
        return ""
    at = tuple(int(i) for i in np.argwhere(bad)[0])
    block = int(np.searchsorted(starts, at[0], side="right") - 1)
    return (f"{int(bad.sum())} of {bad.size} entries differ, first at {at}: row {at[0] - int(starts[block])} of block "
            f"{block} (size {int(starts[block + 1] - starts[block])}), device {got[at]!r} replay {want[at]!r}")


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
@pytest.mark.parametrize("ld_name", sorted(REPLAY_LD))
def test_bits_are_the_headers_order(gpu, ld_name, low_memory, T):
    """`got == finish(replay)` and nothing else: for finite inputs the header makes the product a fixed function of its
    inputs -- entry e to accumulator e % V of lane (e / V) % 64, one FMA per entry in T, the tree over V, the butterfly over
    the lanes, then two rounded operations.  Random full-range LD and Gaussian B: an unfused multiply-add, a truncating
    conversion (int32 / fp64 LD in a float32 state), another lane assignment or tree changes most rows."""
    from viprs_amd import _lib as L
    from viprs_amd.plan import LDPlan
    lb, ip, data, starts = replay_case(ld_name, low_memory)
    B, S = replay_inputs(T), replayed_product(ld_name, low_memory, T)
    plan = LDPlan(lb, ip, data, low_memory)

    def check(storage):
        for n in REPLAY_COLS:
            Bn, Sn = (B[:, :n], S[:, :n]) if n > 1 else (B[:, 0], S[:, 0])
            for dq in (1.0, 1.0 / 127.0):
                for inc in (False, True):
                    got = plan.dot(Bn, dq_scale=dq, include_diagonal=inc)
                    diff = first_difference(got, R.finish(Sn, Bn, dq, inc, T), starts)
                    assert not diff, (f"{ld_name} upper={low_memory} {np.dtype(T).name} {storage} n_cols={n} dq={dq} "
                                      f"diag={inc}: {diff}")
    try:
        check("as created")
        if low_memory:
            _float64_sweep(plan)
            assert plan.info(L.INFO_N_DENSE) == 0 or plan.info(L.INFO_UPPER_MIRRORED) == 0
            check("zero lower triangle")
    finally:
        plan.close()


def _sweep_state(plan, inp, T):
    from viprs_amd.plan import DeviceState
    st = DeviceState(plan, np.dtype(T).name, placement="off")
    for k in ("std_beta", "u_logs", "sqrt_half_var_tau", "mu_mult", "var_gamma", "var_mu", "eta", "q", "eta_diff"):
        st.upload(k, getattr(inp, k))
    return st


@pytest.mark.parametrize("low_memory", [False, True])
def test_independence_and_determinism(gpu, low_memory):
    from viprs_amd.plan import LDPlan
    ld = syn.make_ld([65, 257, 1537, 500, 300, 90], low_memory=low_memory, kind="longrange", seed=8)
    rng = np.random.default_rng(9)
    B = rng.standard_normal((ld.m, 32)).astype(np.float32)
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, low_memory)
    try:
        y = plan.dot(B)
        assert np.array_equal(y, plan.dot(B)), "a repeated call changed bits"
        for g in (0, 13, 31):
            B2 = rng.standard_normal(B.shape).astype(np.float32)
            B2[:, g] = B[:, g]
            assert np.array_equal(plan.dot(B2)[:, g], y[:, g]), f"column {g} depends on the other columns"
        active = np.arange(plan.n_blocks) % 2 == 0
        plan.set_active_blocks(active)
        assert np.array_equal(plan.dot(B), y), "the active-block filter of the sweeps reached the product"
        plan.set_active_blocks(None)
        assert np.array_equal(plan.dot(B), y)
    finally:
        plan.close()


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_product_between_sweeps_leaves_the_sweeps_alone(gpu, T):
    """Upper form: the fp32 sweeps and the float64 sweeps keep the dense blocks in different storages; a product between
    two sweeps must not disturb what the second one computes."""
    from viprs_amd.plan import LDPlan
    ld, ss, inp = syn.make_problem(sizes=[500, 130, 1700], low_memory=True, seed=3, kind="longrange", float_precision=T)
    out = []
    for with_dot in (False, True):
        plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, True)
        try:
            st = _sweep_state(plan, inp, T)
            st.e_step(ld.dq_scale)
            if with_dot:
                y = st.dot("eta", dq_scale=ld.dq_scale, include_diagonal=False)
                assert np.array_equal(y, plan.dot(st.download("eta"), dq_scale=ld.dq_scale, include_diagonal=False))
            st.e_step(ld.dq_scale)
            out.append({k: st.download(k) for k in ("var_gamma", "var_mu", "eta", "q", "eta_diff")})
        finally:
            plan.close()
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k


@pytest.mark.parametrize("model, width", [("spike_slab", 1), ("mixture", 4), ("grid", 32)])
def test_state_entry_point(gpu, model, width):
    from viprs_amd.plan import DeviceState, LDPlan
    ld = syn.make_ld([300, 700, 65], low_memory=True, kind="longrange", ld_dtype=np.int8, seed=4)
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, True)
    try:
        st = DeviceState(plan, "float32", model=model, width=width, placement="off")
        shape = (ld.m, width) if model == "grid" else (ld.m,)
        eta = np.asarray(0.01 * np.random.default_rng(2).standard_normal(shape), dtype=np.float32,
                         order="F" if model == "grid" else "C")
        st.upload("eta", eta)
        for inc in (False, True):
            y = st.dot("eta", dq_scale=ld.dq_scale, include_diagonal=inc)
            assert y.shape == shape
            assert np.array_equal(y, plan.dot(st.download("eta"), dq_scale=ld.dq_scale, include_diagonal=inc))
        assert np.any(y != eta)
        with pytest.raises(ValueError):
            st.dot("q")
        assert plan.last_dot_ms() > 0.0
    finally:
        plan.close()


@pytest.mark.parametrize("low_memory", [True, False])
def test_sweep_consistency(gpu, low_memory):
    """After 3 sweeps from the standard start, q = (R - I) eta up to rounding.

    The sweep builds q_j as a running sum: in every sweep s, each entry (j, i) of the row adds r_ji * d_i^(s) with
    d^(s) = eta_diff of sweep s (an skipped SNP has d = 0), one rounded multiply-add each: 3 L_j additions whose terms
    have absolute sum A_j = sum_i |r_ji| sum_s |d_i^(s)|, so the recursive sum is within eps32 * 3 L_j * A_j of
    sum_i r_ji sum_s d_i^(s).  eta_i itself is sum_s d_i^(s) up to one rounding per sweep (<= eps32 * 3 * sum_s |d_i^(s)|
    in total, i.e. 3 eps32 A_j after the product), and the product of the final eta is within eps32 * D(L_j) * A_j of
    its exact value (header contract; |eta_i| <= sum_s |d_i^(s)|).  Together:
        |dot(eta)_j - q_j| <= eps32 * (3 L_j + D(L_j) + 3) * A_j,
    with d^(s) taken from the oracle's three sweeps."""
    from tests import helpers as H
    from viprs_amd.plan import LDPlan
    ld, ss, inp = syn.make_problem("cfg2", low_memory=low_memory, kind="longrange")
    st_o, absd = inp.state_copy(), np.zeros(ld.m, dtype=np.float64)
    for _ in range(3):
        st_o = H.run_oracle(ld, inp, st_o, sweeps=1)
        absd += np.abs(st_o["eta_diff"].astype(np.float64))
    ref = R.reference(ld.ld_left_bound, ld.ld_indptr, np.abs(ld.ld_data.astype(np.float64)), low_memory, absd, mode="abs")
    A, L = ref["abs_terms"], ref["L"]
    D = R.depth(ref["W"], ld.ld_data.dtype.itemsize)
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, low_memory)
    try:
        st = _sweep_state(plan, inp, np.float32)
        for _ in range(3):
            st.e_step(ld.dq_scale)
        q = st.download("q").astype(np.float64)
        y = st.dot("eta", dq_scale=ld.dq_scale, include_diagonal=False).astype(np.float64)
    finally:
        plan.close()
    assert np.abs(q).max() > 0
    bound = np.finfo(np.float32).eps * (3 * L + D + 3) * A
    err = np.abs(y - q)
    print(f"sweep consistency upper={low_memory}: worst |dot(eta) - q| / bound = "
          f"{float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny))):.4f}, worst |err| = {err.max():.3e}")
    assert np.all(err <= bound)


def _perturbed_panel(fx, c, seed=21):
    """(left_bound, indptr, data, dq_scale): the training LD of the fixture in the upper form with every entry halved and then changed
    by up to 20 % (a panel with weaker LD) -- the same windows, a different panel."""
    rng = np.random.default_rng(seed)
    if f"ld_upper_data_{c}" in fx:
        ip, data = fx[f"ld_upper_indptr_{c}"], fx[f"ld_upper_data_{c}"]
        lb = np.arange(1, ip.shape[0], dtype=np.int32)
    else:
        up = syn.make_ld(fx[f"sizes_{c}"], low_memory=True, rho=fx[f"rho_{c}"])
        lb, ip, data = up.ld_left_bound, up.ld_indptr, up.ld_data
    pert = data.astype(np.float64) * 0.5 * (1.0 + 0.2 * rng.uniform(-1.0, 1.0, data.shape[0]))
    if np.issubdtype(data.dtype, np.integer):
        return lb, ip, np.clip(np.rint(pert), -127, 127).astype(data.dtype), 1.0 / np.iinfo(data.dtype).max
    return lb, ip, pert.astype(data.dtype), 1.0


def test_model_layer_external_panel(gpu):
    """`VIPRSGrid.pseudo_validate(validation_ld=...)` and `select_best_model(..., validation_ld=...)` against the host.

    Propagation of the product's bound: rb = sum r b is formed on the host in float64 on both sides; bsb = sum_j b_j (Rb)_j
    inherits |d(Rb)_j| <= e_j = eps32 (D_j + 3)(A_j + |b_j|) (test_rounding_bound, plus one rounding for dq_scale
    itself, which is rounded to float32 first; dq_scale is folded into A), so |d bsb| <= E = sum_j |b_j| e_j and
    |d(rb^2 / bsb)| <= (rb^2 / bsb) * E / (bsb - E).  The two float64 evaluations of rb and bsb differ by their summation
    order: m 2^-52 of the absolute sums, added to the tolerance."""
    from tests.test_fit import loader_from_fixture
    from viprs_amd.model import HyperparameterGrid, VIPRSGrid, select_best_model
    fx = np.load(os.path.join(HERE, "golden", "fitgrid_independent.npz"))
    c = 22
    gdl = loader_from_fixture(fx)
    grid = HyperparameterGrid(sigma_epsilon_steps=2, pi_steps=3, n_snps=gdl.m, h2_est=0.2, h2_se=0.1)
    model = VIPRSGrid(gdl, grid, low_memory=True)
    model.fit(batched=True, max_iter=80)
    lb, ip, pert, dq = _perturbed_panel(fx, c)
    vb = {c: fx[f"validation_std_beta_{c}"]}
    beta = np.asarray(model.post_mean_beta[c])
    b64 = beta.astype(np.float64)
    ref = R.reference(lb, ip, pert.astype(np.float64), True, b64)
    Rb = dq * ref["exact"] + b64
    rb = b64.T @ np.asarray(vb[c], dtype=np.float64)
    bsb = np.sum(b64 * Rb, axis=0)
    host = rb ** 2 / bsb
    D = R.depth(ref["W"], pert.dtype.itemsize)[:, None]
    E = np.sum(np.abs(b64) * np.finfo(np.float32).eps * (D + 3) * (dq * ref["abs_terms"] + np.abs(b64)), axis=0)
    u64 = b64.shape[0] * 2.0 ** -52
    E = E + u64 * np.sum(np.abs(b64) * (dq * ref["abs_terms"] + np.abs(b64)), axis=0)
    d_rb = u64 * (np.abs(b64).T @ np.abs(np.asarray(vb[c], dtype=np.float64)))
    tol = host * E / (bsb - E) + 2 * np.abs(rb) * d_rb / (bsb - E)
    ok = np.asarray(model.valid_terminated_models)
    order = np.argsort(np.where(ok, host, -np.inf))
    best, second = int(order[-1]), int(order[-2])
    assert host[best] - host[second] > 20 * (tol[best] + tol[second]), "the host scores do not separate the two best models"
    got = np.asarray(model.pseudo_validate(vb, validation_ld={c: (lb, ip, pert, True)}), dtype=np.float64)
    print("pseudo R2 host", host, "device", got, "tol", tol)
    assert np.all(np.abs(got - host) <= tol)
    # ... and not the training panel's scores
    assert np.any(np.abs(np.asarray(model.pseudo_validate(vb), dtype=np.float64) - host) > tol)
    sel = select_best_model(model, validation_gdl=vb, criterion="pseudo_validation", validation_ld={c: (lb, ip, pert, True)})
    assert sel.best_model_idx == best
    assert np.all(np.abs(np.asarray(sel.validation_result["Pseudo_Validation_R2"], dtype=np.float64) - host) <= tol)
