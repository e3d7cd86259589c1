"""CPU: the host model of the extremal-eigenvalue computation (tests/lanczos_reference.py) against `np.linalg.eigvalsh` of
the dense blocks, and the C library's implicit-QL routine (`viprs_tridiagonal_extremes`) against `np.linalg.eigh`.

The bound: a Ritz value theta with residual bound r has an eigenvalue of A within r (to O(eps ||A||)); the stopping rule
asks r <= rtol * scale, so |theta - lambda| <= rtol * max(|lambda_min|, |lambda_max|) at both ends -- provided the Ritz
value has converged to the EXTREME eigenvalue and not to an interior one, which is what the comparison with `eigvalsh`
checks.  Every block gets maxiter = 5 x its size (scipy's default for Krylov solvers).

Both forms of one (kind, LD dtype) stand for the same matrix: the dense blocks rebuilt from the two are compared bit for bit,
the recurrence runs on one."""
import ctypes
import functools

import numpy as np
import pytest

from viprs_amd import _lib as L
from viprs_amd.utils import synthetic as syn

from . import lanczos_reference as LR
from . import ridge_reference as RR

SIZES = (1, 2, 63, 64, 65, 257, 513, 1025, 2305)
SMALL = (63, 65, 257)
LD_DTYPES = {"fp32": np.float32, "int8": np.int8, "int16": np.int16}
RTOL = {np.float32: 1e-4, np.float64: 1e-6}


@functools.lru_cache(maxsize=None)
def _ld(kind, ld_name, low_memory, sizes=SIZES):
    return syn.make_ld(sizes, low_memory=low_memory, ld_dtype=LD_DTYPES[ld_name], kind=kind)


def _arrays(ld):
    return ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory


@functools.lru_cache(maxsize=None)
def host_case(kind, ld_name, T, sizes=SIZES):
    ld = _ld(kind, ld_name, False, sizes)
    return LR.run_blocks(_arrays(ld), ld.dq_scale, T, RTOL[T])


def test_start_vector():
    u = LR.start_vector(4096)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u) and np.all(u != 0.0) and np.all(np.abs(u) < 0.5)
    assert np.array_equal(np.rint(u * 2.0 ** 25) % 2, np.ones(4096))             # odd multiples of 2^-25
    assert abs(u.mean()) < 0.02 and abs(u.std() - 12 ** -0.5) < 0.01
    # a function of the index alone; the first entry from the definition, in Python integers
    assert np.array_equal(LR.start_vector(5), u[:5])
    h = 0x9E3779B97F4A7C15
    h = ((h ^ (h >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
    h = ((h ^ (h >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
    h ^= h >> 31
    assert u[0] == (h >> 40) * 2.0 ** -24 - 0.5 + 2.0 ** -25
    assert LR.check_points(1) == [1] and LR.check_points(16) == [1, 2, 4, 8, 16] and LR.check_points(20) == [1, 2, 4, 8, 16, 20]


@pytest.mark.parametrize("ld_name", sorted(LD_DTYPES))
@pytest.mark.parametrize("kind", ["ar1", "longrange", "sample"])
def test_host_model_float32(kind, ld_name):
    sym, up = _ld(kind, ld_name, False), _ld(kind, ld_name, True)
    a = RR.block_systems(*_arrays(sym), 0.0, sym.dq_scale, np.float32)
    b = RR.block_systems(*_arrays(up), 0.0, up.dq_scale, np.float32)
    assert all(np.array_equal(x[2], y[2]) for x, y in zip(a, b)) and len(a) == len(b) == len(SIZES)
    info, eigs = host_case(kind, ld_name, np.float32)
    worst = LR.check_against_dense(info, eigs, 1e-4)
    print(kind, ld_name, "iterations", info.iterations.tolist(), "worst error / (rtol scale)", round(worst, 4))
    assert info.iterations[0] == 1 and info.lambda_min[0] == info.lambda_max[0] == 1.0
    assert info.resid_min[0] == info.resid_max[0] == 0.0
    assert info.iterations.max() <= 512


@pytest.mark.parametrize("kind,sizes", [("ar1", SMALL), ("longrange", SIZES), ("sample", SIZES)])
def test_host_model_float64(kind, sizes):
    info, eigs = host_case(kind, "int8" if kind == "longrange" else "fp32", np.float64, sizes)
    worst = LR.check_against_dense(info, eigs, 1e-6)
    print(kind, "iterations", info.iterations.tolist(), "worst error / (rtol scale)", round(worst, 4))


def test_small_ar1_blocks_need_more_steps_than_they_have_snps():
    """In finite precision the Ritz values at k = size are not the eigenvalues: stopping there would miss lambda_min."""
    for T in (np.float32, np.float64):
        info, eigs = host_case("ar1", "fp32", T, (63, 64, 65))
        LR.check_against_dense(info, eigs, RTOL[T])
        assert np.all(info.iterations > np.array([63, 64, 65])), (T, info.iterations.tolist())


@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("low_memory", [False, True])
def test_windowed_band_has_a_negative_eigenvalue(low_memory, T):
    lb, ip, data = RR.banded_ar1(2500, 0.95, 40, low_memory)
    info, eigs = LR.run_blocks((lb, ip, data, low_memory), 1.0, T, RTOL[T])
    assert len(eigs) == 1 and abs(eigs[0][0] + 0.152) < 1e-3
    LR.check_against_dense(info, eigs, RTOL[T])
    assert info.lambda_min[0] < -0.1
    print("band", np.dtype(T).name, "iterations", info.iterations.tolist(), info.lambda_min, info.lambda_max)


def test_whole_panel_entry_point_and_maxiter_status():
    ld = _ld("ar1", "fp32", True, SMALL)
    full = LR.extremal_eigenvalues(*_arrays(ld), rtol=1e-4, maxiter=1024)
    cut = LR.extremal_eigenvalues(*_arrays(ld), rtol=1e-4, maxiter=16)
    assert full.converged and np.all(full.iterations > 16)
    assert cut.status.tolist() == [1, 1, 1] and not cut.converged and cut.iterations.tolist() == [16, 16, 16]
    assert np.all(np.isfinite(cut.lambda_min)) and np.all(cut.resid_min > 1e-4 * cut.lambda_max)


def _ql(alpha, beta):
    out = np.zeros(4)
    a = np.ascontiguousarray(alpha, dtype=np.float64)
    b = np.ascontiguousarray(beta, dtype=np.float64)
    vp = ctypes.c_void_p
    rc = L.lib.viprs_tridiagonal_extremes(len(a), a.ctypes.data_as(vp), b.ctypes.data_as(vp) if len(b) else None,
                                          out.ctypes.data_as(vp))
    assert rc == L.OK
    return out


@pytest.mark.parametrize("k", [1, 2, 3, 64, 500])
def test_library_ql_routine_against_eigh(k):
    """Eigenvalues to 1e-12 ||T||; the last components |s| to the perturbation bound of an eigenvector under a backward
    error of 1e-12 ||T||: 1e-12 ||T|| / gap (+ the same for eigh's own)."""
    rng = np.random.default_rng(100 + k)
    for trial in range(4):
        a = rng.standard_normal(k) * (1.0 if trial % 2 else 3.0) + trial
        b = np.abs(rng.standard_normal(max(k - 1, 0))) + 0.1
        T = np.diag(a) + np.diag(b, 1) + np.diag(b, -1)
        theta, S = np.linalg.eigh(T)
        norm = np.abs(T).sum(axis=1).max()
        got = _ql(a, b)
        assert abs(got[0] - theta[0]) <= 1e-12 * norm and abs(got[1] - theta[-1]) <= 1e-12 * norm
        gap_lo = theta[1] - theta[0] if k > 1 else np.inf
        gap_hi = theta[-1] - theta[-2] if k > 1 else np.inf
        assert abs(got[2] - abs(S[-1, 0])) <= 2e-12 * norm / gap_lo + 1e-15
        assert abs(got[3] - abs(S[-1, -1])) <= 2e-12 * norm / gap_hi + 1e-15
        # what the stopping rule multiplies by beta_{k+1}: the same as the host model's
        lo, hi, r_lo, r_hi = LR.ritz_extremes(list(a), list(b) + [0.7])
        assert abs(0.7 * got[2] - r_lo) <= 2e-12 * norm / gap_lo + 1e-15 and abs(0.7 * got[3] - r_hi) <= 2e-12 * norm / gap_hi + 1e-15


def test_library_ql_routine_on_lanczos_coefficients_and_bad_arguments():
    """The coefficients the recurrence really produces (ghost copies: clusters of nearly equal Ritz values)."""
    ld = _ld("ar1", "fp32", False, SMALL)
    _, _, A = RR.block_systems(*_arrays(ld), 0.0, 1.0, np.float32)[2]
    R = A - np.eye(A.shape[0])
    v = LR.start_vector(A.shape[0])
    v = (v / np.linalg.norm(v)).astype(np.float32)
    v_prev, b, al, be = np.zeros_like(v), 0.0, [], []
    for _ in range(400):
        w = (R @ v.astype(np.float64)).astype(np.float32) + v - np.float32(b) * v_prev
        a = float(np.dot(v.astype(np.float64), w.astype(np.float64)))
        w = w - np.float32(a) * v
        b = float(np.sqrt(np.dot(w.astype(np.float64), w.astype(np.float64))))
        al.append(a)
        be.append(b)
        v_prev, v = v, (w.astype(np.float64) / b).astype(np.float32)
    for k in (1, 2, 16, 128, 400):
        lo, hi, r_lo, r_hi = LR.ritz_extremes(al[:k], be[:k])
        got = _ql(al[:k], be[:k - 1])
        scale = max(abs(lo), abs(hi))
        assert abs(got[0] - lo) <= 1e-12 * scale and abs(got[1] - hi) <= 1e-12 * scale
        # the bounds agree wherever they can decide a stop at rtol >= 1e-8
        assert abs(be[k - 1] * got[2] - r_lo) <= 1e-9 * scale and abs(be[k - 1] * got[3] - r_hi) <= 1e-9 * scale
    out = np.zeros(4)
    assert L.lib.viprs_tridiagonal_extremes(0, None, None, out.ctypes.data_as(ctypes.c_void_p)) == L.EINVAL
    assert L.lib.viprs_plan_extremal_eigenvalues(None, L.F32, 1.0, 1e-4, 16, None, None, None, None, None, None) == L.EINVAL
    ms = ctypes.c_double(0.0)
    assert L.lib.viprs_plan_last_spectrum_ms(None, ctypes.byref(ms), None, None) == L.EINVAL
