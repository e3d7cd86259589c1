"""The extremal eigenvalues `viprs_plan_extremal_eigenvalues` (include/viprs_hip.h) on the device against
`np.linalg.eigvalsh` of the dense blocks and the host model of tests/lanczos_reference.py: accuracy at both ends, windowed
LD with a negative eigenvalue, the status at maxiter, every bit against the host model driven by the replays of the header's
orders (tests/order_replay.py), determinism / independence, calls between sweeps of the same plan and the model layer
(`annotate_spectrum`, `lambda_min='compute'`).

The bounds: a block stops when its two residual bounds are <= rtol * scale, and a Ritz value lies within its residual bound
of an eigenvalue, so |theta - lambda| <= rtol * max(|lambda_min|, |lambda_max|) at both ends once the Ritz values have
reached the EXTREME eigenvalues -- which the comparison with `eigvalsh` checks.  rtol: 1e-4 (float32), 1e-6 (float64).
`maxiter` = twice the host model's largest per-block count: the device sums its products in another order, which may flip
one decision at a check (the checks are at k = 1, 2, 4, ...: one flip doubles the count), and no more."""
import functools

import numpy as np
import pytest

from tests import lanczos_reference as LR
from tests import order_replay as OR
from tests import ridge_reference as RR
from tests.test_gpu_ld_dot import REPLAY_SIZES
from viprs_amd.utils import synthetic as syn

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 257, 513, 1025, 2305)
SMALL = (63, 65, 257)
RTOL = {np.float32: 1e-4, np.float64: 1e-6}
CASES = {"ar1-fp32-sym": ("ar1", np.float32, False), "ar1-fp32-upper": ("ar1", np.float32, True),
         "longrange-int8-sym": ("longrange", np.int8, False), "longrange-int8-upper": ("longrange", np.int8, True),
         "sample-fp32-sym": ("sample", np.float32, False)}


@functools.lru_cache(maxsize=None)
def _ld(case, sizes=SIZES):
    kind, ld_dtype, low_memory = CASES[case]
    return syn.make_ld(sizes, low_memory=low_memory, ld_dtype=ld_dtype, kind=kind)


def _arrays(ld):
    return ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory


@functools.lru_cache(maxsize=None)
def _host(kind, ld_dtype, T, sizes):
    """Host model (maxiter 5 x size per block) and dense spectra of a matrix: the same for both of its forms."""
    ld = syn.make_ld(sizes, low_memory=False, ld_dtype=ld_dtype, kind=kind)
    info, eigs = LR.run_blocks(_arrays(ld), ld.dq_scale, T, RTOL[T])
    assert np.all(info.status == 0)
    return info, eigs


def _reference(case, T, sizes=SIZES):
    kind, ld_dtype, _ = CASES[case]
    return _host(kind, ld_dtype, T, sizes)


def _plan(ld):
    from viprs_amd.plan import LDPlan
    return LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory)


def _check(info, eigs, rtol):
    assert np.all(np.isfinite(info.lambda_min)) and np.all(np.isfinite(info.lambda_max))
    assert np.all(np.isfinite(info.resid_min)) and np.all(np.isfinite(info.resid_max))
    worst = LR.check_against_dense(info, eigs, rtol)
    print("worst error / (rtol scale)", round(worst, 4))


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_accuracy(gpu, case, T):
    sizes = SMALL if (T == np.float64 and CASES[case][0] == "ar1") else SIZES
    rtol = RTOL[T]
    host, eigs = _reference(case, T, sizes)
    ld = _ld(case, sizes)
    plan = _plan(ld)
    try:
        info = plan.extremal_eigenvalues(dq_scale=ld.dq_scale, rtol=rtol, maxiter=2 * int(host.iterations.max()),
                                         float_precision=T)
        ms, launched, host_ms = plan.last_spectrum_ms()
    finally:
        plan.close()
    print("iterations", info.iterations.tolist(), "host", host.iterations.tolist(), "ms", round(ms, 3), "host ms",
          round(host_ms, 3))
    _check(info, eigs, rtol)
    assert info.converged and info.ms == ms > 0.0 and launched >= info.iterations.max() and 0.0 <= host_ms
    if sizes[0] == 1:                                   # a single SNP: one step exhausts its Krylov space
        assert info.iterations[0] == 1 and info.lambda_min[0] == info.lambda_max[0] == 1.0
        assert info.resid_min[0] == info.resid_max[0] == 0.0


@functools.lru_cache(maxsize=None)
def _banded(low_memory):
    lb, ip, data = RR.banded_ar1(2500, 0.95, 40, low_memory)
    eigs = [np.linalg.eigvalsh(A) for _, _, A in RR.block_systems(lb, ip, data, low_memory, 0.0, 1.0, np.float64)]
    assert len(eigs) == 1 and eigs[0][0] < -0.15
    return lb, ip, data, eigs


@functools.lru_cache(maxsize=None)
def _banded_host(T):
    lb, ip, data, _ = _banded(False)
    return LR.run_blocks((lb, ip, data, False), 1.0, T, RTOL[T])[0]


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_windowed_ld(gpu, low_memory, T):
    """A truncated AR(1) band is not positive definite: lambda_min is about -0.152."""
    from viprs_amd.plan import LDPlan
    lb, ip, data, eigs = _banded(low_memory)
    host = _banded_host(T)
    plan = LDPlan(lb, ip, data, low_memory)
    try:
        info = plan.extremal_eigenvalues(rtol=RTOL[T], maxiter=2 * int(host.iterations.max()), float_precision=T)
    finally:
        plan.close()
    print("iterations", info.iterations.tolist(), "host", host.iterations.tolist(), info.lambda_min, info.lambda_max)
    _check(info, eigs, RTOL[T])
    assert info.lambda_min[0] < -0.1


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
def test_max_iter_status(gpu, T):
    ld = _ld("ar1-fp32-sym", SMALL)
    rtol = RTOL[T]
    host = LR.extremal_eigenvalues(*_arrays(ld), rtol=rtol, maxiter=16, float_precision=T)
    _, eigs = _reference("ar1-fp32-sym", T, SMALL)
    plan = _plan(ld)
    try:
        info = plan.extremal_eigenvalues(rtol=rtol, maxiter=16, float_precision=T)
        long = plan.extremal_eigenvalues(rtol=rtol, maxiter=4096, float_precision=T)
    finally:
        plan.close()
    print("status", info.status.tolist(), "host", host.status.tolist(), "iterations", info.iterations.tolist())
    assert np.array_equal(info.status, host.status) and info.converged == bool(np.all(host.status == 0))
    assert np.all(info.iterations[info.status == 1] == 16) and np.all(long.status == 0)
    # the bounds of an unconverged block are still bounds: an eigenvalue lies within resid of each Ritz value
    systems = RR.block_systems(*_arrays(ld), 0.0, 1.0, T)
    for k, (ev, (_, _, A)) in enumerate(zip(eigs, systems)):
        slack = 64 * np.finfo(T).eps * np.abs(A).sum(axis=1).max()
        for theta, resid in ((info.lambda_min[k], info.resid_min[k]), (info.lambda_max[k], info.resid_max[k])):
            assert np.isfinite(theta) and np.isfinite(resid)
            assert resid >= np.abs(ev - theta).min() - slack, (k, theta, resid)
    done = info.status == 0
    for name in ("lambda_min", "lambda_max", "resid_min", "resid_max", "iterations"):
        assert np.array_equal(getattr(info, name)[done], getattr(long, name)[done]), name


def _same(a, b):
    return all(np.array_equal(getattr(a, n), getattr(b, n))
               for n in ("lambda_min", "lambda_max", "resid_min", "resid_max", "iterations", "status"))


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
def test_determinism_and_independence(gpu, T):
    from viprs_amd.plan import LDPlan
    ld = _ld("longrange-int8-upper")
    kw = dict(dq_scale=ld.dq_scale, rtol=RTOL[T], float_precision=T)
    plan = _plan(ld)
    try:
        info = plan.extremal_eigenvalues(**kw)
        assert _same(plan.extremal_eigenvalues(**kw), info), "a repeated call changed bits"
        plan.set_active_blocks(np.arange(plan.n_blocks) % 2 == 0)
        filtered = plan.extremal_eigenvalues(**kw)
        plan.set_active_blocks(None)
        assert _same(filtered, info), "the active-block filter of the sweeps reached the spectrum"
    finally:
        plan.close()
    assert info.converged
    # the 257-SNP block in a plan of its own (it starts at SNP 195 above, at 0 here)
    s, e = int(ld.block_start[5]), int(ld.block_start[6])
    o0, o1 = int(ld.ld_indptr[s]), int(ld.ld_indptr[e])
    lb = (ld.ld_left_bound[s:e] - s).astype(np.int32)
    ip = (ld.ld_indptr[s:e + 1] - o0).astype(np.int64)
    alone = LDPlan(lb, ip, np.ascontiguousarray(ld.ld_data[o0:o1]), True)
    try:
        one = alone.extremal_eigenvalues(**kw)
    finally:
        alone.close()
    for name in ("lambda_min", "lambda_max", "resid_min", "resid_max", "iterations", "status"):
        assert getattr(one, name)[0] == getattr(info, name)[5], name


def _sweep_state(plan, inp, T):
    from viprs_amd.plan import DeviceState
    st = DeviceState(plan, np.dtype(T).name, placement="off")
    for k in ("std_beta", "u_logs", "sqrt_half_var_tau", "mu_mult", "var_gamma", "var_mu", "eta", "q", "eta_diff"):
        st.upload(k, getattr(inp, k))
    return st


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
def test_between_sweeps(gpu, T):
    """Upper form: the fp32 and the float64 sweeps keep the dense blocks in different storages; a spectrum call between two
    sweeps reads whichever is there, like the product, and must not disturb what the second sweep computes."""
    from viprs_amd.plan import LDPlan
    ld, ss, inp = syn.make_problem(sizes=[500, 130, 1700], low_memory=True, seed=3, kind="longrange", float_precision=T)
    eigs = [np.linalg.eigvalsh(A) for _, _, A in RR.block_systems(*_arrays(ld), 0.0, ld.dq_scale, np.float32)]
    out = []
    for with_spectrum in (False, True):
        plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, True)
        try:
            st = _sweep_state(plan, inp, T)
            st.e_step(ld.dq_scale)
            if with_spectrum:
                _check(plan.extremal_eigenvalues(dq_scale=ld.dq_scale), eigs, 1e-4)
            st.e_step(ld.dq_scale)
            out.append({k: st.download(k) for k in ("var_gamma", "var_mu", "eta", "q", "eta_diff")})
        finally:
            plan.close()
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k


def test_model_layer(gpu):
    from viprs_amd.data import ArrayDataLoader
    from viprs_amd.model import VIPRS, VIPRSPerChromosome
    from viprs_amd.stats.spectrum import UnpinnedLambdaMinError, annotate_spectrum, lambda_min_from_extremes
    make = lambda: ArrayDataLoader.synthetic({1: [300, 65], 2: [257]}, ld_dtype=np.int8, kind="longrange")
    gdl = make()
    kw = dict(dequantize_on_the_fly=True)
    # what the parent commit gives: None, a number, 'infer' on LD without a spectrum
    assert VIPRS(gdl, **kw).lambda_min == 0.0 and VIPRS(gdl, lambda_min=0.25, **kw).lambda_min == 0.25
    assert VIPRS(gdl, lambda_min="infer", **kw).lambda_min == 0.0
    assert VIPRSPerChromosome(gdl, lambda_min="infer", **kw)._lambda_group == [0.0, 0.0]

    rtol, r = 1e-4, 1e-3
    ext = {}
    for c in (1, 2):
        up = gdl.ld[c].load(return_symmetric=False)
        ev = [np.linalg.eigvalsh(A) for _, _, A in RR.block_systems(up.leftmost_idx, up.ld_indptr, up.ld_data, True, 0.0,
                                                                    1.0 / 127, np.float32)]
        ext[c] = (min(e[0] for e in ev), max(e[-1] for e in ev))
    bound = {c: rtol * max(abs(lo), abs(hi)) for c, (lo, hi) in ext.items()}

    # 'compute': the r = 0 rule on the model's device; VIPRS keeps the last chromosome's value, the batch one per chromosome
    model = VIPRS(gdl, lambda_min="compute", **kw)
    want = {c: lambda_min_from_extremes(*ext[c]) for c in ext}
    print("extremes", ext, "computed", model.lambda_min_computed)
    assert abs(model.lambda_min - want[2]) <= bound[2] and sorted(model.lambda_min_computed) == [1, 2]
    assert all(s["per_block"].converged for s in model.spectrum.values())
    assert abs(model.spectrum[1]["min"] - ext[1][0]) <= bound[1] and abs(model.spectrum[1]["max"] - ext[1][1]) <= bound[1]
    model.fit(max_iter=1, theta_0={"pi": 0.02, "sigma_epsilon": 0.85})
    per = VIPRSPerChromosome(gdl, lambda_min="compute", **kw)
    assert all(abs(per._lambda_group[g] - want[c]) <= bound[c] for g, c in enumerate((1, 2)))
    per.fit(max_iter=1, theta_0={"pi": 0.02, "sigma_epsilon": 0.85})
    assert VIPRS(gdl, lambda_min="compute", merge_chromosomes=False, **kw).lambda_min_computed == model.lambda_min_computed

    # annotate, then 'infer': refused without a formula, the chosen formula applied to the extremes with one
    spectrum = annotate_spectrum(gdl, dequantize_on_the_fly=True)
    assert sorted(spectrum) == [1, 2] and all(s["per_block"].converged for s in spectrum.values())
    with pytest.raises(UnpinnedLambdaMinError, match="chromosome 1"):
        VIPRS(gdl, lambda_min="infer", **kw)
    for formula in ("one_plus_r", "one_minus_r"):
        for c in (1, 2):
            gdl.ld[c].lambda_min_formula = formula
        got = VIPRS(gdl, lambda_min="infer", **kw).lambda_min
        assert abs(got - lambda_min_from_extremes(*ext[2], r, formula)) <= (1 + r) * bound[2] / (1 - r)
        groups = VIPRSPerChromosome(gdl, lambda_min="infer", **kw)._lambda_group
        assert all(abs(groups[g] - lambda_min_from_extremes(*ext[c], r, formula)) <= (1 + r) * bound[c] / (1 - r)
                   for g, c in enumerate((1, 2)))
    # 'compute' needs the device
    with pytest.raises(RuntimeError, match="HIP device"):
        VIPRS(make(), lambda_min="compute", e_step_fn=lambda *a: None)


# ---- every bit against the replayed host model ----------------------------------------------------------------------------
REPLAY_CASES = ("ar1-fp32-sym", "longrange-int8-upper", "banded-sym", "banded-upper")
# the run to convergence: `==` needs no accurate eigenvalue, so the tolerance is one that every block -- the windowed band
# included -- meets at one of the check points k = 16, 32, 64, 128 (status 0 in every block, asserted on the replayed model);
# maxiter lies above the last of them and is no power of two
REPLAY_RTOL = 1e-3
REPLAY_MAXITER = 160
FIELDS = ("iterations", "status", "lambda_min", "lambda_max", "resid_min", "resid_max")


@functools.lru_cache(maxsize=None)
def replay_matrix(case):
    if case.startswith("banded"):
        lb, ip, data, _ = _banded(case.endswith("upper"))
        return lb, ip, data, case.endswith("upper"), 1.0
    ld = _ld(case, REPLAY_SIZES)
    return ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory, ld.dq_scale


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", REPLAY_CASES)
def test_bits_are_the_replayed_model(gpu, case, T):
    """All six outputs `==` the host model with the product in the header's order, the dot products (the norm of the start
    vector included) in the 256-thread order and the library's own QL routine for the Ritz pairs.  The ladder of `maxiter`
    compares the coefficients' consequences after the first steps (3 and 5 fall between the check points), then the run
    to convergence: every block stops with status 0 at a check point between the ladder and `maxiter`."""
    from viprs_amd.plan import LDPlan
    lb, ip, data, low_memory, dq = replay_matrix(case)
    name = f"{case} {np.dtype(T).name}"
    plan = LDPlan(lb, ip, data, low_memory)
    try:
        for k in (1, 2, 3, 5, 16, REPLAY_MAXITER):
            want = OR.replayed_spectrum(lb, ip, data, low_memory, dq, REPLAY_RTOL, k, T)
            got = plan.extremal_eigenvalues(dq_scale=dq, rtol=REPLAY_RTOL, maxiter=k, float_precision=T)
            for field in FIELDS:
                a, b = getattr(got, field), getattr(want, field)
                assert np.array_equal(a, b), (f"{name} maxiter={k}: {field} of blocks {np.nonzero(a != b)[0].tolist()}: "
                                              f"device {a.tolist()} replay {b.tolist()}")
        print(name, "iterations", want.iterations.tolist(), "status", want.status.tolist())
        assert np.all(want.status == 0) and 16 < want.iterations.max() < REPLAY_MAXITER
    finally:
        plan.close()


@pytest.mark.parametrize("ld_dtype", [np.int8, np.float32], ids=["int8-on-the-fly", "fp32"])
def test_ld_spectrum_mirrors_an_upper_only_store_on_the_device(gpu, ld_dtype):
    """`ld_spectrum(low_memory=False)` of LD objects that hold only the upper-triangular store: mirrored on the device
    (`LDPlan.from_upper`, documented as bit-identical to the symmetric plan), so every figure `==` the one of objects that
    hand out the symmetric form themselves.  Two chromosomes with a single-SNP block, a small one and one past 64 SNPs."""
    from viprs_amd.data import ArrayDataLoader
    from viprs_amd.stats.spectrum import ld_spectrum
    sizes = {1: [1, 5, 33, 70], 2: [3, 66]}
    kw = dict(low_memory=False, dequantize_on_the_fly=True)
    got = ld_spectrum(ArrayDataLoader.synthetic(sizes, ld_dtype=ld_dtype, forms=("upper",)), **kw)
    want = ld_spectrum(ArrayDataLoader.synthetic(sizes, ld_dtype=ld_dtype), **kw)
    assert sorted(got) == sorted(want) == [1, 2]
    for c in want:
        assert got[c]["min"] == want[c]["min"] and got[c]["max"] == want[c]["max"]
        assert got[c]["per_block"].status.shape == (len(sizes[c]),) and got[c]["per_block"].converged
        for field in FIELDS:
            assert np.array_equal(getattr(got[c]["per_block"], field), getattr(want[c]["per_block"], field)), (c, field)
