"""The ridge solve `viprs_plan_solve_ridge` (include/viprs_hip.h) on the device against the host model of
tests/ridge_reference.py and a dense float64 solve: accuracy through the TRUE residual, indefinite systems, per-block
stopping, zero right-hand sides, windowed LD, every bit against the host model driven by the replays of the header's
orders (tests/order_replay.py), determinism / independence, warm starts, the model layer (`LDPredInf`) and solves between
sweeps of the same plan.

The bounds: a block is accepted when its true residual ||b - A x|| / ||b||, evaluated in float64 from the dense block, is at
most 2 rtol -- the solver stops on its own estimate <= rtol, the host model's estimate equals its true residual to within
10 % on these inputs, and the factor 2 pays for the device's different summation order in the product.  The error bound
||x - x*|| / ||x*|| <= kappa(A) 2 rtol follows from the residual bound.  `maxiter` = twice the host model's largest
per-block count keeps a slow or stagnating kernel from passing."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests import order_replay as OR
from tests import ridge_reference as RR
from tests.test_gpu_ld_dot import REPLAY_SIZES
from viprs_amd.utils import synthetic as syn

pytestmark = pytest.mark.gpu

# one 16-byte load (4 / 2 elements), one wavefront (256 / 128), one pass of a workgroup (1024 / 512), several passes
SIZES = (1, 2, 63, 64, 65, 257, 513, 1025, 2305)
SMALL = (63, 65, 257)
RTOL = {np.float32: 1e-5, np.float64: 1e-10}
CASES = {"ar1-fp32-sym": ("ar1", np.float32, False), "ar1-fp32-upper": ("ar1", np.float32, True),
         "longrange-int8-sym": ("longrange", np.int8, False), "longrange-int8-upper": ("longrange", np.int8, True),
         "sample-fp32-sym": ("sample", np.float32, False)}


@functools.lru_cache(maxsize=None)
def _ld(case, sizes=SIZES):
    kind, ld_dtype, low_memory = CASES[case]
    sym = syn.make_ld(sizes, low_memory=False, ld_dtype=ld_dtype, kind=kind)
    ld = syn.make_ld(sizes, low_memory=True, ld_dtype=ld_dtype, kind=kind) if low_memory else sym
    return ld, syn.make_sumstats(sym).std_beta.astype(np.float64)


def _arrays(ld):
    return ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory


@functools.lru_cache(maxsize=None)
def _base(case, T, sizes=SIZES):
    """The unshifted systems of a case and their eigenvalues (a scalar shift moves every eigenvalue by fl_T(shift))."""
    ld, _ = _ld(case, sizes)
    systems = RR.block_systems(*_arrays(ld), 0.0, ld.dq_scale, T)
    return systems, [np.linalg.eigvalsh(A) for _, _, A in systems]


@functools.lru_cache(maxsize=None)
def _reference(case, shift, T, rtol, sizes=SIZES):
    ld, b64 = _ld(case, sizes)
    b = b64.astype(T)
    base, eigs = _base(case, T, sizes)
    sh = float(np.dtype(T).type(shift))
    systems = [(s, e, A + sh * np.eye(e - s)) for s, e, A in base]
    kappa = np.array([np.abs(ev + sh).max() / np.abs(ev + sh).min() for ev in eigs])
    x, info = RR.solve(*_arrays(ld), b, shift, ld.dq_scale, rtol)
    assert np.all(info.status == 0)
    return SimpleNamespace(ld=ld, b=b, systems=systems, kappa=kappa, x_host=x, info_host=info,
                           x_star=RR.dense_solve(systems, b))


def _plan(ld):
    from viprs_amd.plan import LDPlan
    return LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory)


def _check_blocks(ref, x, info, rtol, T):
    res = RR.true_residuals(ref.systems, ref.b, x)
    err = np.array([np.linalg.norm(x[s:e] - ref.x_star[s:e]) / np.linalg.norm(ref.x_star[s:e]) for s, e, _ in ref.systems])
    print("iterations", info.iterations.tolist(), "host", ref.info_host.iterations.tolist())
    print("true residual / rtol", np.round(res / rtol, 3).tolist())
    print("relres / rtol", np.round(info.relres / rtol, 3).tolist())
    print("error / (kappa 2 rtol)", np.round(err / (ref.kappa * 2 * rtol), 4).tolist())
    assert x.dtype == T and np.all(np.isfinite(x))
    assert np.all(info.status == 0), info.status
    assert np.all(res <= 2 * rtol)
    assert np.all(err <= ref.kappa * 2 * rtol)
    seen = res > 100 * np.finfo(T).eps
    assert np.all(info.relres[seen] <= 2 * res[seen]) and np.all(res[seen] <= 2 * info.relres[seen])


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shift", [0.05, 5.0])
@pytest.mark.parametrize("case", sorted(CASES))
def test_accuracy(gpu, case, shift, T):
    rtol = RTOL[T]
    ref = _reference(case, shift, T, rtol)
    plan = _plan(ref.ld)
    try:
        x, info = plan.solve_ridge(ref.b, shift, dq_scale=ref.ld.dq_scale, rtol=rtol,
                                   maxiter=2 * int(ref.info_host.iterations.max()))
        ms, launched = plan.last_solve_ms()
    finally:
        plan.close()
    _check_blocks(ref, x, info, rtol, T)
    assert info.iterations[0] == 1                      # a single SNP: one step exhausts its Krylov space
    assert info.converged and info.ms == ms > 0.0 and launched >= info.iterations.max()


def test_indefinite_matrix(gpu):
    rtol = 1e-8
    ref = _reference("ar1-fp32-sym", -1.0, np.float64, rtol, SMALL)
    assert all((np.linalg.eigvalsh(A) < 0).sum() >= 45 for _, _, A in ref.systems)
    plan = _plan(ref.ld)
    try:
        x, info = plan.solve_ridge(ref.b, -1.0, rtol=rtol, maxiter=4 * 257)
    finally:
        plan.close()
    res = RR.true_residuals(ref.systems, ref.b, x)
    print("iterations", info.iterations.tolist(), "host", ref.info_host.iterations.tolist(), "true residual / rtol",
          np.round(res / rtol, 3).tolist())
    assert np.all(info.status == 0) and np.all(res <= 2 * rtol)


def test_per_block_stopping_and_max_iter(gpu):
    ld, b64 = _ld("ar1-fp32-sym", SMALL)
    b = b64.copy()
    shift = np.concatenate([np.full(63 + 65, 5.0), np.full(257, -1.0)])
    systems = RR.block_systems(*_arrays(ld), shift, 1.0, np.float64)
    plan = _plan(ld)
    try:
        x, info = plan.solve_ridge(b, shift, rtol=1e-8, maxiter=20)
        x_long, info_long = plan.solve_ridge(b, shift, rtol=1e-8, maxiter=1000)
    finally:
        plan.close()
    res = RR.true_residuals(systems, b, x)
    print("iterations", info.iterations.tolist(), "status", info.status.tolist(), "relres", info.relres.tolist(),
          "true", res.tolist())
    assert info.status.tolist() == [0, 0, 1] and not info.converged
    assert info.iterations[0] <= 10 and info.iterations[1] <= 10 and info.iterations[2] == 20
    assert np.all(np.isfinite(x))
    assert res[2] <= 2 * info.relres[2] and info.relres[2] <= 2 * res[2]
    assert np.all(res[:2] <= 2e-8)
    # the easy blocks do not see what the hard one does
    assert np.array_equal(x[:128], x_long[:128])
    assert np.array_equal(info.iterations[:2], info_long.iterations[:2])
    assert np.array_equal(info.relres[:2], info_long.relres[:2])
    assert info_long.status.tolist() == [0, 0, 0]


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
def test_zero_right_hand_side_on_one_block(gpu, T):
    ld, b64 = _ld("longrange-int8-upper")
    b = b64.astype(T)
    bz = b.copy()
    s, e = int(ld.block_start[5]), int(ld.block_start[6])
    bz[s:e] = 0.0
    plan = _plan(ld)
    try:
        x, info = plan.solve_ridge(b, 0.5, dq_scale=ld.dq_scale)
        xz, iz = plan.solve_ridge(bz, 0.5, dq_scale=ld.dq_scale)
    finally:
        plan.close()
    assert iz.status[5] == 2 and iz.iterations[5] == 0 and iz.relres[5] == 0.0 and np.all(xz[s:e] == 0.0)
    assert iz.converged and np.any(x[s:e] != 0.0)
    others = np.arange(len(SIZES)) != 5
    assert np.array_equal(xz[:s], x[:s]) and np.array_equal(xz[e:], x[e:])
    assert np.array_equal(iz.iterations[others], info.iterations[others])
    assert np.array_equal(iz.relres[others], info.relres[others]) and np.all(iz.status[others] == 0)


@functools.lru_cache(maxsize=None)
def _banded(low_memory):
    lb, ip, data = RR.banded_ar1(2500, 0.95, 40, low_memory)
    b = np.random.default_rng(31).standard_normal(2500)
    systems = RR.block_systems(lb, ip, data, low_memory, 0.5, 1.0, np.float64)
    assert len(systems) == 1
    return lb, ip, data, b, systems


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_windowed_ld(gpu, low_memory, T):
    """A truncated AR(1) band is not positive definite (smallest eigenvalue about -0.15 before the shift)."""
    from viprs_amd.plan import LDPlan
    lb, ip, data, b64, systems = _banded(low_memory)
    assert np.linalg.eigvalsh(systems[0][2]).min() < 0.5
    b = b64.astype(T)
    rtol = RTOL[T]
    _, host = RR.solve(lb, ip, data, low_memory, b, 0.5, 1.0, rtol)
    plan = LDPlan(lb, ip, data, low_memory)
    try:
        x, info = plan.solve_ridge(b, 0.5, rtol=rtol, maxiter=2 * int(host.iterations.max()))
    finally:
        plan.close()
    res = RR.true_residuals(systems, b, x)
    print("iterations", info.iterations.tolist(), "host", host.iterations.tolist(), "true residual / rtol", res / rtol)
    assert info.status.tolist() == [0] and res[0] <= 2 * rtol


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
def test_determinism_and_independence(gpu, T):
    from viprs_amd.plan import LDPlan
    ld, b64 = _ld("longrange-int8-upper")
    b = b64.astype(T)
    plan = _plan(ld)
    try:
        x, info = plan.solve_ridge(b, 0.05, dq_scale=ld.dq_scale)
        x2, info2 = plan.solve_ridge(b, 0.05, dq_scale=ld.dq_scale)
        assert np.array_equal(x, x2) and np.array_equal(info.relres, info2.relres), "a repeated call changed bits"
        for ce in (1, 7):
            xc, ic = plan.solve_ridge(b, 0.05, dq_scale=ld.dq_scale, check_every=ce)
            assert np.array_equal(xc, x) and np.array_equal(ic.iterations, info.iterations), f"check_every={ce}"
            assert np.array_equal(ic.relres, info.relres) and np.array_equal(ic.status, info.status)
        plan.set_active_blocks(np.arange(plan.n_blocks) % 2 == 0)
        xa, _ = plan.solve_ridge(b, 0.05, dq_scale=ld.dq_scale)
        plan.set_active_blocks(None)
        assert np.array_equal(xa, x), "the active-block filter of the sweeps reached the solve"
    finally:
        plan.close()
    # the 257-SNP block in a plan of its own (it starts at SNP 195 above, at 0 here)
    one = syn.make_ld(SIZES, low_memory=True, ld_dtype=np.int8, kind="longrange")
    s, e = int(one.block_start[5]), int(one.block_start[6])
    o0, o1 = int(one.ld_indptr[s]), int(one.ld_indptr[e])
    lb = (one.ld_left_bound[s:e] - s).astype(np.int32)
    ip = (one.ld_indptr[s:e + 1] - o0).astype(np.int64)
    alone = LDPlan(lb, ip, np.ascontiguousarray(one.ld_data[o0:o1]), True)
    try:
        xs, infos = alone.solve_ridge(np.ascontiguousarray(b[s:e]), 0.05, dq_scale=ld.dq_scale, maxiter=5 * 2305)
    finally:
        alone.close()
    assert np.array_equal(xs, x[s:e]) and infos.iterations[0] == info.iterations[5] and infos.relres[0] == info.relres[5]


def test_warm_start(gpu):
    ld, b64 = _ld("ar1-fp32-upper")
    b = b64.astype(np.float32)
    plan = _plan(ld)
    try:
        x, info = plan.solve_ridge(b, 0.05)
        x1, info1 = plan.solve_ridge(b, 0.05, x0=x)
    finally:
        plan.close()
    print("iterations", info.iterations.tolist(), "warm", info1.iterations.tolist())
    assert np.all(info.status == 0) and np.all(info1.status == 0)
    assert info1.iterations.max() <= 2
    systems = RR.block_systems(*_arrays(ld), 0.05, 1.0, np.float32)
    assert np.all(RR.true_residuals(systems, b, x1) <= 2e-5)
    untouched = info1.iterations == 0
    for k in np.nonzero(untouched)[0]:
        s, e = int(ld.block_start[k]), int(ld.block_start[k + 1])
        assert np.array_equal(x1[s:e], x[s:e])


def test_model_layer(gpu):
    from viprs_amd.data import ArrayDataLoader
    from viprs_amd.model import LDPredInf
    gdl = ArrayDataLoader.synthetic({1: [300, 65], 2: [257]}, ld_dtype=np.int8, n=5e4, kind="longrange")
    dev = LDPredInf(gdl, h2=0.3, dequantize_on_the_fly=True).fit()
    seen = {}

    def solve_fn(*args):
        seen["args"] = args
        return RR.solve(*args)

    host = LDPredInf(gdl, h2=0.3, dequantize_on_the_fly=True, solve_fn=solve_fn).fit()
    lb, ip, data, low_memory, b, shift, dq_scale = seen["args"][:7]
    assert data.dtype == np.int8 and low_memory and dq_scale == 1.0 / 127 and shift == dev.lam == 622 / (5e4 * 0.3)
    assert {c: v.shape for c, v in dev.post_mean_beta.items()} == {1: (365,), 2: (257,)}
    assert dev.post_mean_beta[1].dtype == np.float32 and dev.solve_info.converged
    systems = RR.block_systems(lb, ip, data, True, shift, dq_scale, np.float32)
    kappa = RR.condition_numbers(systems)
    x_star = RR.dense_solve(systems, b)
    cat = lambda mdl: np.concatenate([mdl.post_mean_beta[c] for c in (1, 2)])
    for name, x in (("device", cat(dev)), ("host", cat(host))):
        res = RR.true_residuals(systems, b, x)
        print(name, "true residual / rtol", (res / 1e-5).tolist())
        assert np.all(res <= 2e-5)
        for k, (s, e, _) in enumerate(systems):
            assert np.linalg.norm(x[s:e] - x_star[s:e]) / np.linalg.norm(x_star[s:e]) <= kappa[k] * 2e-5


def _sweep_state(plan, inp, T):
    from viprs_amd.plan import DeviceState
    st = DeviceState(plan, np.dtype(T).name, placement="off")
    for k in ("std_beta", "u_logs", "sqrt_half_var_tau", "mu_mult", "var_gamma", "var_mu", "eta", "q", "eta_diff"):
        st.upload(k, getattr(inp, k))
    return st


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
def test_solve_between_sweeps_leaves_the_sweeps_alone(gpu, T):
    """Upper form: the fp32 and the float64 sweeps keep the dense blocks in different storages; a solve between two sweeps
    reads whichever is there, like the product, and must not disturb what the second sweep computes."""
    from viprs_amd.plan import LDPlan
    ld, ss, inp = syn.make_problem(sizes=[500, 130, 1700], low_memory=True, seed=3, kind="longrange", float_precision=T)
    systems = RR.block_systems(*_arrays(ld), 0.5, ld.dq_scale, np.float32)
    b = np.asarray(inp.std_beta, dtype=np.float32)
    out = []
    for with_solve in (False, True):
        plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, True)
        try:
            st = _sweep_state(plan, inp, T)
            st.e_step(ld.dq_scale)
            if with_solve:
                x, info = plan.solve_ridge(b, 0.5, dq_scale=ld.dq_scale)
                assert np.all(info.status == 0) and np.all(RR.true_residuals(systems, b, x) <= 2e-5)
            st.e_step(ld.dq_scale)
            out.append({k: st.download(k) for k in ("var_gamma", "var_mu", "eta", "q", "eta_diff")})
        finally:
            plan.close()
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k


# ---- every bit against the replayed host model ----------------------------------------------------------------------------
# REPLAY_SIZES (test_gpu_ld_dot): one 16-byte load, one wavefront pass of the product, one and two passes of the 256-thread
# dot product in both precisions (1024 / 512 elements), sizes that are no multiple of the chunk
REPLAY_CASES = ("ar1-fp32-sym", "longrange-int8-upper", "banded-sym", "banded-upper")
# "to convergence": every block of every case below stops with status 0 well below this (asserted on the replayed model)
REPLAY_MAXITER = 120


@functools.lru_cache(maxsize=None)
def replay_system(case):
    """(left_bound, indptr, data, low_memory, dq_scale, b as float64, block starts) of a replay case."""
    if case.startswith("banded"):
        lb, ip, data, b, _ = _banded(case.endswith("upper"))
        return lb, ip, data, case.endswith("upper"), 1.0, b, np.array([0, 2500])
    ld, b = _ld(case, REPLAY_SIZES)
    return ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory, ld.dq_scale, b, np.asarray(ld.block_start)


def replay_shift(kind, starts):
    """0.5 (the single windowed block: 2.0 -- the truncated AR(1) band has condition number 110 at 0.5 and needs more than 100
    iterations in float64), or a per-SNP vector whose sign alternates from block to block, the first one negative: +[0.4,
    0.6] and -[8, 12].  A negative shift of the positive one's size leaves a block indefinite AND nearly singular (the
    eigenvalues of an LD block are dense around 0.5: hundreds of iterations, the large blocks more than 600).  At -[8, 12]
    every block converges within 40 iterations: the AR(1) blocks are negative definite there, the 257- and 1025-SNP
    long-range blocks indefinite (their two factor eigenvalues stay positive).  The single windowed block takes the signs by
    halves, +-[80, 120] (1250 negative and 1250 positive eigenvalues): its spectrum is dense up to 39, so the negative half
    has to clear it."""
    if kind == "scalar":
        return 0.5 if len(starts) > 2 else 2.0
    m = int(starts[-1])
    mag = np.random.default_rng(33).uniform(0.4, 0.6, m)
    edges = starts if len(starts) > 2 else np.array([0, m // 2, m])
    sign = np.concatenate([np.full(int(e - s), -1.0 if k % 2 == 0 else 1.0)
                           for k, (s, e) in enumerate(zip(edges[:-1], edges[1:]))])
    if len(starts) == 2:
        return 200.0 * sign * mag
    return np.where(sign < 0, 20.0, 1.0) * sign * mag


def _same_solve(name, got, want, starts):
    (x, info), (xr, ir) = got, want
    for field in ("iterations", "status", "relres"):
        a, b = getattr(info, field), getattr(ir, field)
        assert np.array_equal(a, b), (f"{name}: {field} of blocks {np.nonzero(a != b)[0].tolist()}: device {a.tolist()} "
                                      f"replay {b.tolist()}")
    bad = x != xr
    if bad.any():
        at = int(np.argwhere(bad)[0][0])
        block = int(np.searchsorted(starts, at, side="right") - 1)
        raise AssertionError(f"{name}: x differs in {int(bad.sum())} entries, first at SNP {at} (block {block}, size "
                             f"{int(starts[block + 1] - starts[block])}): device {x[at]!r} replay {xr[at]!r}")


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shift_kind", ["scalar", "vector"])
@pytest.mark.parametrize("case", REPLAY_CASES)
def test_bits_are_the_replayed_model(gpu, case, shift_kind, T):
    """`x`, `iterations`, `relres` and `status` `==` the host model with the product in the header's order and the dot
    products in the 256-thread order: every operation of the solver is then the device's.  The ladder of `maxiter` compares
    the state after each of the first iterations (a failure points at the iteration where the two part), then the run to
    convergence (status 0 in every block, asserted) under both `check_every`, then a warm start from a perturbed solution
    (a few iterations remain)."""
    from viprs_amd.plan import LDPlan
    lb, ip, data, low_memory, dq, b64, starts = replay_system(case)
    b = b64.astype(T)
    shift = replay_shift(shift_kind, starts)
    rtol = RTOL[T]
    replay = lambda **kw: OR.replayed_solve(lb, ip, data, low_memory, b, shift, dq, rtol, **kw)
    name = f"{case} {shift_kind} {np.dtype(T).name}"
    plan = LDPlan(lb, ip, data, low_memory)
    try:
        device = lambda **kw: plan.solve_ridge(b, shift, dq_scale=dq, rtol=rtol, **kw)
        for k in (1, 2, 3, 5, 8):
            _same_solve(f"{name} maxiter={k}", device(maxiter=k, check_every=1), replay(maxiter=k), starts)
        want = replay(maxiter=REPLAY_MAXITER)
        print(name, "iterations", want[1].iterations.tolist(), "status", want[1].status.tolist())
        assert np.all(want[1].status == 0) and 8 < want[1].iterations.max() < REPLAY_MAXITER
        for ce in (1, 7):
            _same_solve(f"{name} check_every={ce}", device(maxiter=REPLAY_MAXITER, check_every=ce), want, starts)
        x0 = (want[0] * (1 + T(1e-3) * np.random.default_rng(34).standard_normal(b.shape[0]).astype(T))).astype(T)
        warm = replay(maxiter=REPLAY_MAXITER, x0=x0)
        print(name, "warm start iterations", warm[1].iterations.tolist())
        assert np.all(warm[1].status == 0) and warm[1].iterations.max() > 0
        assert np.all(warm[1].iterations <= want[1].iterations)
        for ce in (1, 7):
            _same_solve(f"{name} x0 check_every={ce}", device(maxiter=REPLAY_MAXITER, check_every=ce, x0=x0), warm, starts)
    finally:
        plan.close()
