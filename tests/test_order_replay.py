"""CPU: the host replays of tests/order_replay.py -- what the GPU tests of the LD product, the LD scores, the ridge solve and
the extremal eigenvalues compare with `==` -- checked on their own: exact on inputs where every order is exact, within the
header's bound of the exact sums on the random inputs of the GPU tests, different from a plain float32 matrix product on
those inputs (so that `==` with the replay says something), and, driving the two host models, as good as the float64-product
models by the acceptance criteria of test_ridge_reference.py / test_lanczos_reference.py."""
import math
import time

import numpy as np
import pytest

from viprs_amd.plan import SpectrumInfo
from viprs_amd.utils import synthetic as syn

from . import lanczos_reference as LR
from . import ld_dot_reference as R
from . import ld_score_reference as SR
from . import order_replay as OR
from . import ridge_reference as RR
from . import test_gpu_ld_dot as GD
from . import test_gpu_ld_score as GS

EPS = {np.float32: float(np.finfo(np.float32).eps), np.float64: float(np.finfo(np.float64).eps)}
TINY = np.finfo(np.float64).tiny


# ---- exact inputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("low_memory", [False, True])
@pytest.mark.parametrize("kind, ld_name", [("single", "fp32"), ("small", "int16"), ("small", "fp64"), ("banded", "int8"),
                                           ("banded", "int32")])
def test_product_replay_is_exact_on_integer_inputs(kind, ld_name, low_memory, T):
    lb, ip, data, B, S = GD._exact_case(kind, ld_name, low_memory)
    got = OR.replay_dot(lb, ip, data, low_memory, B[:, :5].astype(T))
    assert got.dtype == T and np.array_equal(got, S[:, :5])
    assert np.array_equal(OR.replay_dot(lb, ip, data, low_memory, B[:, 3].astype(T)), S[:, 3])


@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("low_memory", [False, True])
@pytest.mark.parametrize("kind, ld_name", [("dense", "int8"), ("small", "fp32"), ("banded", "int16"), ("banded", "fp64")])
def test_score_replay_is_exact_on_integer_inputs(kind, ld_name, low_memory, T):
    lb, ip, ints, A, ref, unit = GS._exact_case(kind, low_memory)
    floating = ld_name.startswith("fp")
    data = (ints / 16.0).astype(GS.LD_DTYPES[ld_name]) if floating else ints.astype(GS.LD_DTYPES[ld_name])
    den = 256.0 if floating else 1.0
    S2, S0 = OR.replay_scores(lb, ip, data, low_memory, A[:, :3].astype(T), T)
    assert np.array_equal(S2, ref["S2"][:, :3] / den) and np.array_equal(S0, ref["S0"][:, :3])
    U2, U0 = OR.replay_scores(lb, ip, data, low_memory, None, T)
    assert U2.shape == (lb.shape[0],) and np.array_equal(U2, unit["S2"] / den) and np.array_equal(U0, unit["S0"])
    assert np.array_equal(U0, ref["L"])                  # unit weights: S0 is the number of entries of the row


# ---- the header's bound on the random inputs of the GPU tests -------------------------------------------------------------
def _converted(data, T):
    """x = T(stored element) as float64: the header converts first, the sums are over the converted values."""
    return np.asarray(data).astype(T).astype(np.float64)


# every LD dtype in both forms in a float32 state (the header's bound verbatim), three of them in a float64 state
BOUND_CASES = [(l, f, np.float32) for l in sorted(GD.REPLAY_LD) for f in (False, True)] + \
              [("fp64", False, np.float64), ("fp64", True, np.float64), ("int8", False, np.float64)]


@pytest.mark.parametrize("ld_name, low_memory, T", BOUND_CASES)
def test_product_replay_within_the_headers_bound(ld_name, low_memory, T):
    """|S - exact| <= eps_T D sum |r b| (header; D counts W for a window with gaps).  The reference: `fsum` over float64
    products -- exact products in a float32 state (24-bit factors): the header's bound verbatim.  In a float64 state each
    product of the reference is rounded once, at most 2^-53 of its magnitude: the bound there is the header's with D + 1, a
    derived allowance for the reference, not the header's own figure."""
    lb, ip, data, _ = GD.replay_case(ld_name, low_memory)
    B = GD.replay_inputs(T)[:, :3]
    t0 = time.perf_counter()
    S = OR.replay_dot(lb, ip, data, low_memory, B)
    ms = 1e3 * (time.perf_counter() - t0)
    ref = R.reference(lb, ip, _converted(data, T), low_memory, B.astype(np.float64), mode="fsum")
    D = R.depth(ref["W"], data.dtype.itemsize)[:, None] + (1 if T == np.float64 else 0)
    err = np.abs(S.astype(np.float64) - ref["exact"])
    bound = EPS[T] * D * ref["abs_terms"]
    print(f"product replay {ld_name} upper={low_memory} {np.dtype(T).name}: worst err/bound = "
          f"{float(np.max(err / np.maximum(bound, TINY))):.4f}, replay of 3 columns {ms:.0f} ms")
    assert np.all(err <= bound) and np.any(err > 0)


@pytest.mark.parametrize("ld_name, low_memory, T", [("int8", False, np.float32), ("int8", True, np.float64),
                                                     ("int16", False, np.float64), ("int16", True, np.float32),
                                                     ("int32", False, np.float32), ("int32", True, np.float32),
                                                     ("fp32", False, np.float64), ("fp32", True, np.float32),
                                                     ("fp64", False, np.float32), ("fp64", True, np.float64)])
def test_score_replay_within_the_headers_bound(ld_name, low_memory, T):
    """S2 within eps_T (D + 1) sum p |A| of the exact sum of the squares, S0 within eps_T D sum |A| (header, ROUNDING):
    every LD dtype in both forms.  Float64 state: one more unit of D for the reference's own rounded products, as above (in
    a float32 state the reference's squares and products are exact and the bound is the header's verbatim)."""
    lb, ip, data, _ = GD.replay_case(ld_name, low_memory)
    A, _ = GS.replay_weights(T)
    A = A[:, :2]
    t0 = time.perf_counter()
    S2, S0 = OR.replay_scores(lb, ip, data, low_memory, A, T)
    U2, U0 = OR.replay_scores(lb, ip, data, low_memory, None, T)
    ms = 1e3 * (time.perf_counter() - t0)
    own = 1 if T == np.float64 else 0
    for name, (s2, s0), ref in (("gaussian", (S2, S0), SR.sums(lb, ip, _converted(data, T), low_memory, A, mode="fsum")),
                                ("unit", (U2, U0), SR.sums(lb, ip, _converted(data, T), low_memory, None, mode="fsum"))):
        D = R.depth(ref["W"], data.dtype.itemsize).astype(np.float64)
        D = D[:, None] if s2.ndim == 2 else D
        e2, e0 = np.abs(s2.astype(np.float64) - ref["S2"]), np.abs(s0.astype(np.float64) - ref["S0"])
        b2, b0 = EPS[T] * (D + 1 + own) * ref["P"], EPS[T] * (D + own) * ref["Q"]
        print(f"score replay {ld_name} upper={low_memory} {np.dtype(T).name} {name}: worst S2 err/bound = "
              f"{float(np.max(e2 / np.maximum(b2, TINY))):.4f}, S0 {float(np.max(e0 / np.maximum(b0, TINY))):.4f}"
              f" (both replays {ms:.0f} ms)")
        assert np.all(e2 <= b2) and np.all(e0 <= b0)
        # (unit weights: sums of integer squares below 2^24 / 2^53 are exact in any order -- no rounding to see there)
        assert name == "unit" or np.any(e2 > 0)
    assert np.array_equal(U0, np.asarray(ref["L"], dtype=T))


# ---- discriminating power: a condition on the inputs of the GPU tests -----------------------------------------------------
@pytest.mark.parametrize("low_memory", [False, True])
@pytest.mark.parametrize("ld_name", sorted(GD.REPLAY_LD))
def test_a_plain_float32_product_differs_from_the_replay(ld_name, low_memory):
    """If a float32 `R @ B` gave the replay's bits, `==` with the replay would not tell the header's order from any other:
    it must differ in at least half of the rows of every block of 257 SNPs or more."""
    lb, ip, data, starts = GD.replay_case(ld_name, low_memory)
    B = GD.replay_inputs(np.float32)[:, 0]
    S = OR.replay_dot(lb, ip, data, low_memory, B)
    x = _converted(data, np.float32)
    shares = []
    for s, e in zip(starts[:-1], starts[1:]):
        s, e = int(s), int(e)
        if e - s < 257:
            continue
        Rb, _ = R.block_matrix(lb, ip, x, low_memory, s, e)
        plain = Rb.astype(np.float32) @ np.ascontiguousarray(B[s:e])
        assert plain.dtype == np.float32
        shares.append(float(np.mean(plain != S[s:e])))
    print(f"plain float32 product vs replay, {ld_name} upper={low_memory}: share of differing rows per block "
          f"{[round(v, 2) for v in shares]}")
    assert len(shares) == 5 and min(shares) >= 0.5


# ---- the solvers' dot product ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 511, 513, 1023, 1025, 2500])
def test_ordered_dot(n, T):
    V = 16 // np.dtype(T).itemsize
    rng = np.random.default_rng(n)
    # float32 values in either dtype: the float64 products are exact, `fsum` of them is the exact dot product
    a = rng.standard_normal(n).astype(np.float32).astype(T)
    b = rng.standard_normal(n).astype(np.float32).astype(T)
    terms = a.astype(np.float64) * b.astype(np.float64)
    got = OR.ordered_dot(a, b)
    assert isinstance(got, float) and abs(got - math.fsum(terms)) <= n * 2.0 ** -53 * float(np.abs(terms).sum())
    # the chunk width is T's, whatever the operands
    assert got == OR.dot_for(T)(a.astype(np.float64), b.astype(np.float64))
    # integers: every order is exact
    ai, bi = rng.integers(-1000, 1001, n).astype(T), rng.integers(-1000, 1001, n).astype(T)
    assert OR.ordered_dot(ai, bi) == float(np.dot(ai.astype(np.int64), bi.astype(np.int64)))
    # the block's partial last chunk belongs to thread (n // V) % 256, behind that thread's whole chunks
    tail = np.zeros(n, dtype=T)
    tail[n - n % V:] = 1.0
    part = OR.thread_partials(tail, tail)
    want = np.zeros(OR.N_THREADS)
    want[(n // V) % OR.N_THREADS] = n % V
    assert np.array_equal(part, want)
    # element e to thread (e // V) % 256
    e = np.arange(n)
    count = np.bincount((e // V) % OR.N_THREADS, minlength=OR.N_THREADS).astype(np.float64)
    assert np.array_equal(OR.thread_partials(np.ones(n, dtype=T), np.ones(n, dtype=T)), count)


def test_the_reduction_is_a_tree_over_the_lanes_then_the_wavefronts_in_order():
    """Accumulators on which the order of the reduction shows."""
    lanes = np.zeros(OR.N_THREADS)
    lanes[:4] = [2.0 ** 53, 1.0, 1.0, -2.0 ** 53]
    # butterfly: (2^53 + 1) + (1 - 2^53) = 2^53 - (2^53 - 1) = 1; a serial sum gives ((2^53 + 1) + 1) - 2^53 = 0
    assert OR.reduce_threads(lanes) == 1.0
    waves = np.zeros(OR.N_THREADS)
    waves[[0, 64, 128, 192]] = [2.0 ** 53, 1.0, 1.0, -2.0 ** 53]         # wavefronts in order: ((2^53 + 1) + 1) - 2^53 = 0
    assert OR.reduce_threads(waves) == 0.0
    waves[[0, 64, 128, 192]] = [1.0, 1.0, 2.0 ** 53, -2.0 ** 53]         # ((1 + 1) + 2^53) - 2^53 = 2
    assert OR.reduce_threads(waves) == 2.0
    # a thread adds its elements in ascending order: 2^53, then 1 (lost), then -2^53; V = 2: elements 0, 1 and 512
    a = np.zeros(1024)
    a[[0, 1, 512]] = [2.0 ** 53, 1.0, -2.0 ** 53]
    assert OR.thread_partials(a, np.ones(1024))[0] == 0.0 and OR.ordered_dot(a, np.ones(1024)) == 0.0


# ---- the replay-driven host models meet the criteria of the float64-product ones -----------------------------------------
SIZES = (1, 2, 63, 64, 65, 257)


@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("kind, ld_dtype, low_memory, shift", [("ar1", np.float32, False, 0.05),
                                                               ("ar1", np.float32, True, 5.0),
                                                               ("longrange", np.int8, True, 0.05),
                                                               ("sample", np.float32, False, 5.0)])
def test_replayed_minres_against_the_dense_solve(kind, ld_dtype, low_memory, shift, T):
    """The criteria of test_ridge_reference.py::test_host_model_against_the_dense_solve."""
    sym = syn.make_ld(SIZES, low_memory=False, ld_dtype=ld_dtype, kind=kind)
    ld = syn.make_ld(SIZES, low_memory=True, ld_dtype=ld_dtype, kind=kind) if low_memory else sym
    b = syn.make_sumstats(sym).std_beta.astype(T)
    rtol = {np.float32: 1e-5, np.float64: 1e-10}[T]
    args = (ld.ld_left_bound, ld.ld_indptr, ld.ld_data, low_memory)
    x, info = OR.replayed_solve(*args, b, shift, ld.dq_scale, rtol)
    systems = RR.block_systems(*args, shift, ld.dq_scale, T)
    assert x.dtype == T and np.all(info.status == 0) and info.converged
    assert info.iterations[0] == 1 and info.iterations.max() <= 106
    res = RR.true_residuals(systems, b, x)
    assert np.all(res <= 2 * rtol), res / rtol
    xs = RR.dense_solve(systems, b)
    kappa = RR.condition_numbers(systems)
    for k, (s, e, _) in enumerate(systems):
        err = np.linalg.norm(x[s:e] - xs[s:e]) / np.linalg.norm(xs[s:e])
        assert err <= kappa[k] * 2 * rtol, (k, err, kappa[k])
    seen = res > 100 * np.finfo(T).eps
    assert np.all(np.abs(info.relres[seen] / res[seen] - 1.0) < 0.1)
    # the seams' defaults are the model as it was: the replayed run is another rounding of the same recurrences
    x_def, info_def = RR.solve(*args, b, shift, ld.dq_scale, rtol)
    assert np.all(np.abs(info.iterations - info_def.iterations) <= 2)


def test_replayed_minres_zero_rhs_maxiter_and_warm_start():
    """The criteria of test_ridge_reference.py::test_host_model_indefinite_zero_rhs_maxiter_and_warm_start."""
    ld = syn.make_ld((63, 65, 257), low_memory=False, ld_dtype=np.float32, kind="ar1")
    b = syn.make_sumstats(ld).std_beta.astype(np.float64)
    args = (ld.ld_left_bound, ld.ld_indptr, ld.ld_data, False)
    systems = RR.block_systems(*args, -1.0, 1.0, np.float64)
    x, info = OR.replayed_solve(*args, b, -1.0, 1.0, 1e-8, 4 * 257)
    assert np.all(info.status == 0) and np.all(RR.true_residuals(systems, b, x) <= 2e-8)
    shift = np.concatenate([np.full(63 + 65, 5.0), np.full(257, -1.0)])
    _, i20 = OR.replayed_solve(*args, b, shift, 1.0, 1e-8, 20)
    assert i20.status.tolist() == [0, 0, 1] and i20.iterations[2] == 20 and not i20.converged
    bz = b.copy()
    bz[63:128] = 0.0
    xz, iz = OR.replayed_solve(*args, bz, 5.0, 1.0, 1e-10)
    assert iz.status.tolist() == [0, 2, 0] and iz.iterations[1] == 0 and np.all(xz[63:128] == 0.0)
    b32 = b.astype(np.float32)
    x0, _ = OR.replayed_solve(*args, b32, 0.05, 1.0, 1e-5)
    _, i1 = OR.replayed_solve(*args, b32, 0.05, 1.0, 1e-5, x0=x0)
    assert i1.iterations.max() <= 2 and np.all(i1.status == 0)


def _replayed_blocks(args, dq_scale, T, rtol, factor=5):
    """`lanczos_reference.run_blocks` with the replays in the seams."""
    lb, ip, data, low_memory = args
    product, dot = OR.BlockProduct(lb, ip, data, low_memory), OR.dot_for(T)
    dq = np.dtype(T).type(dq_scale)
    rows, eigs = [], []
    for s, e, A in RR.block_systems(*args, 0.0, dq_scale, T):
        rows.append(LR.lanczos_block(None, dq, rtol, factor * (e - s), T, product(s, e), dot, OR.ritz_extremes, e - s))
        eigs.append(np.linalg.eigvalsh(A))
    return SpectrumInfo(*zip(*rows)), eigs


@pytest.mark.parametrize("T, rtol", [(np.float32, 1e-4), (np.float64, 1e-6)])
@pytest.mark.parametrize("kind, ld_dtype, low_memory, sizes", [("ar1", np.float32, False, (63, 65, 257)),
                                                               ("longrange", np.int8, True, SIZES)])
def test_replayed_lanczos_against_the_dense_spectrum(kind, ld_dtype, low_memory, sizes, T, rtol):
    """The criteria of test_lanczos_reference.py: status 0, both ends within rtol * scale of `eigvalsh`, both residual
    bounds below rtol * scale (`check_against_dense`)."""
    ld = syn.make_ld(sizes, low_memory=low_memory, ld_dtype=ld_dtype, kind=kind)
    info, eigs = _replayed_blocks((ld.ld_left_bound, ld.ld_indptr, ld.ld_data, low_memory), ld.dq_scale, T, rtol)
    worst = LR.check_against_dense(info, eigs, rtol)
    print(kind, np.dtype(T).name, "iterations", info.iterations.tolist(), "worst error / (rtol scale)", round(worst, 4))
    assert info.iterations.max() <= 512
    if sizes[0] == 1:
        assert info.iterations[0] == 1 and info.lambda_min[0] == info.lambda_max[0] == 1.0
        assert info.resid_min[0] == info.resid_max[0] == 0.0


@pytest.mark.parametrize("low_memory", [False, True])
def test_replayed_lanczos_on_the_windowed_band_and_at_maxiter(low_memory):
    lb, ip, data = RR.banded_ar1(600, 0.95, 40, low_memory)
    info, eigs = _replayed_blocks((lb, ip, data, low_memory), 1.0, np.float32, 1e-4)
    LR.check_against_dense(info, eigs, 1e-4)
    assert info.lambda_min[0] < -0.1
    cut = OR.replayed_spectrum(lb, ip, data, low_memory, rtol=1e-4, maxiter=12)
    assert cut.status.tolist() == [1] and cut.iterations.tolist() == [12] and not cut.converged
    assert np.isfinite(cut.lambda_min[0]) and cut.resid_min[0] > 1e-4 * cut.lambda_max[0]


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_each_seam_changes_the_solvers_bits(T):
    """The `==` of the GPU tests means something only if the orders matter: with the float64 matrix product in place of the
    product's replay the replayed MINRES and Lanczos give other bits in both state precisions, with `np.dot` in place of the
    256-thread order in a float64 state."""
    ld = syn.make_ld((257, 513), low_memory=True, ld_dtype=np.int8, kind="longrange")
    args = (ld.ld_left_bound, ld.ld_indptr, ld.ld_data, True)
    b = syn.make_sumstats(syn.make_ld((257, 513), low_memory=False, ld_dtype=np.int8, kind="longrange")).std_beta.astype(T)
    product, dot = OR.BlockProduct(*args), OR.dot_for(T)
    x, info = OR.replayed_solve(*args, b, 0.5, ld.dq_scale, maxiter=8)
    assert np.array_equal(x, OR.replayed_solve(*args, b, 0.5, ld.dq_scale, maxiter=8)[0])
    x1, i1 = RR.solve(*args, b, 0.5, ld.dq_scale, None, 8, dot=dot)                     # another product
    assert np.mean(x1 != x) > 0.5 and np.all(i1.relres != info.relres)
    x2, i2 = RR.solve(*args, b, 0.5, ld.dq_scale, None, 8, off_product=product)         # another dot product
    sp = OR.replayed_spectrum(*args, ld.dq_scale, 1e-3, 8, T)
    s1 = LR.extremal_eigenvalues(*args, ld.dq_scale, 1e-3, 8, T, dot=dot, ritz=OR.ritz_extremes)
    assert np.all(s1.lambda_min != sp.lambda_min) and np.all(s1.resid_max != sp.resid_max)
    s2 = LR.extremal_eigenvalues(*args, ld.dq_scale, 1e-3, 8, T, off_product=product, ritz=OR.ritz_extremes)
    if T == np.float64:
        assert np.all(i2.relres != info.relres) and np.mean(x2 != x) > 0.5
        assert np.all(s2.lambda_min != sp.lambda_min) and np.all(s2.resid_max != sp.resid_max)
    # (float32 state: the products of float32 values are exact in float64 and the sums of a few hundred of them nearly so;
    # what is left of the order disappears when the coefficients are rounded to float32.  The float64 state is where the
    # `==` tests pin the order of the dot products.)
