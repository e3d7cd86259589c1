"""Host replay of the elastic-net sweep (tests/enet_replay.c through ctypes: libm `fmaf` for the q updates) -- what the `==`
tests of `viprs_state_enet_sweep` and of `viprs_amd.stats.enet.enet_sweep_host` compare with -- and the small shared pieces
of those tests: the KKT violation of a solution against the dense blocks, the sweep-to-a-fixed-point loop, the bound."""
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "enet_replay.c")
_SUFFIX = {np.dtype(np.float32): "f32", np.dtype(np.int8): "i8", np.dtype(np.int16): "i16"}
_vp = ctypes.c_void_p

# The KKT violation of a fixed point of the replay, measured on make_problem(sizes=[1601, 130, 64, 1], seed=53,
# kind="longrange"), symmetric float32 LD (EXPERIMENTS.md, "Lassosum"), per (s, lambda); fixed points after 136 and 104
# sweeps.  The bound of a case is 4 x its measurement: room for the order of the q sums, three orders of magnitude below the
# penalties -- a violation anywhere near `pen` means the update is wrong.  Other cases take 4 x the larger measurement.
KKT_MEASURED = {(0.9, 0.005): 2.15e-6, (0.9, 0.012): 1.33e-6}
KKT_BOUND = {k: 4 * v for k, v in KKT_MEASURED.items()}
KKT_BOUND_ANY = 4 * max(KKT_MEASURED.values())


@functools.lru_cache(maxsize=None)
def _lib():
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    out = os.path.join(tempfile.mkdtemp(prefix="enet_replay_"), "libenetreplay.so")
    subprocess.run([cc, "-O2", "-ffp-contract=off", "-fPIC", "-shared", _SRC, "-o", out, "-lm"], check=True)
    lib = ctypes.CDLL(out)
    for sfx in _SUFFIX.values():
        f = getattr(lib, f"enet_replay_sweep_{sfx}")
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_int64, _vp, _vp, _vp, ctypes.c_int] + [_vp] * 8 + [ctypes.c_float]
    return lib


def _p(a):
    return a.ctypes.data_as(_vp)


def replay_sweep(lb, ip, data, low_memory, std_beta, mult, penalty, eta, q, dq_scale=1.0):
    """`enet_sweep_host`'s signature and contract (eta, q float32 ``(m,)`` or Fortran-ordered ``(m, G)``, updated in place;
    returns eta_diff, var_mu, var_gamma), by the C file."""
    data = np.ascontiguousarray(data)
    fn = getattr(_lib(), f"enet_replay_sweep_{_SUFFIX[data.dtype]}")
    lb = np.ascontiguousarray(lb, dtype=np.int32)
    ip = np.ascontiguousarray(ip, dtype=np.int64)
    m = lb.shape[0]
    beta = np.ascontiguousarray(std_beta, dtype=np.float32)
    assert eta.dtype == q.dtype == np.float32 and eta.shape == q.shape and eta.shape[0] == m
    shape = eta.shape
    outs = [np.zeros(shape, dtype=np.float32, order="F") for _ in range(3)]
    cols = lambda a: np.asarray(a).reshape(m, -1)
    C, Pn, E, Q = cols(mult), cols(penalty), cols(eta), cols(q)
    O = [cols(o) for o in outs]
    for g in range(E.shape[1]):
        c, pen = (np.ascontiguousarray(a[:, g], dtype=np.float32) for a in (C, Pn))
        e, qq = np.array(E[:, g]), np.array(Q[:, g])
        o = [np.zeros(m, dtype=np.float32) for _ in range(3)]
        rc = fn(m, _p(lb), _p(ip), _p(data), int(bool(low_memory)), _p(beta), _p(c), _p(pen), _p(e), _p(qq), _p(o[0]), _p(o[1]),
                _p(o[2]), float(np.float32(dq_scale)))
        assert rc == 0
        E[:, g], Q[:, g] = e, qq
        for dst, src in zip(O, o):
            dst[:, g] = src
    return tuple(outs)


def to_fixed_point(sweep, ld, std_beta, mult, penalty, max_sweeps=400, eta=None, q=None):
    """Sweeps from eta = q = 0 (or the given start) until a sweep changes nothing: (eta, q, sweeps run, the last included)."""
    m = ld.m
    eta = np.zeros(m, dtype=np.float32) if eta is None else eta.copy()
    q = np.zeros(m, dtype=np.float32) if q is None else q.copy()
    for k in range(1, max_sweeps + 1):
        ed, _, _ = sweep(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory, std_beta, mult, penalty, eta, q, ld.dq_scale)
        if np.max(np.abs(ed)) == 0:
            return eta, q, k
    raise AssertionError(f"no fixed point within {max_sweeps} sweeps")


def dense_matrix(lb, ip, data, low_memory, dq_scale=1.0):
    """The float64 matrix the arrays stand for (unit diagonal)."""
    lb, ip = np.asarray(lb, dtype=np.int64), np.asarray(ip, dtype=np.int64)
    m = lb.shape[0]
    R = np.zeros((m, m))
    x = np.asarray(data, dtype=np.float64) * float(dq_scale)
    for j in range(m):
        n = int(ip[j + 1] - ip[j])
        R[j, lb[j]:lb[j] + n] = x[ip[j]:ip[j + 1]]
    if low_memory:
        R = R + R.T
    np.fill_diagonal(R, 1.0)
    return R


def kkt_violation(R, std_beta, beta, s, pen):
    """max over SNPs of |g_j - pen sign(beta_j)| on the support and max(|g_j| - pen, 0) off it, g = beta_hat - ((1 - s) R + s I)
    beta, all in float64."""
    b = np.asarray(beta, dtype=np.float64)
    g = np.asarray(std_beta, dtype=np.float64) - ((1.0 - s) * (R @ b) + s * b)
    pen = np.broadcast_to(np.asarray(pen, dtype=np.float64), b.shape)
    on = b != 0
    v = np.where(on, np.abs(g - pen * np.sign(b)), np.maximum(np.abs(g) - pen, 0.0))
    return float(v.max())


# ---- the two-chromosome case of the model tests -------------------------------------------------------------------------------
MODEL_CHROMS = {1: [130, 64], 2: [200, 1]}
MODEL_S = (0.5, 1.0)
MODEL_LAMBDAS = (0.012, 0.005, 0.002)
MODEL_TOL = 1e-6


def model_gdl():
    from viprs_amd.data import ArrayDataLoader
    return ArrayDataLoader.synthetic(MODEL_CHROMS, ld_dtype=np.int8, n=5e4, kind="longrange", h2=0.5)


@functools.lru_cache(maxsize=None)
def model_fit(device=False):
    """`Lassosum.fit()` on the case, on the device or by `enet_sweep_host`.  tol = 1e-6: the upper form (the model's
    default) re-forms the second-pass sums in every sweep and idles at changes of ~6e-8 instead of reaching a sweep that
    changes nothing.  Cached: a test that changes the model (`select_best`) works on a copy."""
    from viprs_amd.model import Lassosum
    from viprs_amd.stats.enet import enet_sweep_host
    return Lassosum(model_gdl(), s=MODEL_S, lambdas=MODEL_LAMBDAS, tol=MODEL_TOL, dequantize_on_the_fly=True,
                    sweep_fn=None if device else enet_sweep_host).fit()
