"""Host replay of the LDpred2 Gibbs sweep (tests/gibbs_replay.c through ctypes: libm `expf` in the sigmoid, libm `fmaf` for the
q updates) -- what the `==` tests of `viprs_state_gibbs_sweep` and of `viprs_amd.stats.gibbs.gibbs_sweep_host` compare with --
and the small shared pieces of those tests: the inputs of a chain, the case of the model tests."""
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gibbs_replay.c")
_SUFFIX = {np.dtype(np.float32): "f32", np.dtype(np.int8): "i8", np.dtype(np.int16): "i16"}
_vp = ctypes.c_void_p


@functools.lru_cache(maxsize=None)
def _lib():
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    out = os.path.join(tempfile.mkdtemp(prefix="gibbs_replay_"), "libgibbsreplay.so")
    subprocess.run([cc, "-O2", "-ffp-contract=off", "-fPIC", "-shared", _SRC, "-o", out, "-lm"], check=True)
    lib = ctypes.CDLL(out)
    for sfx in _SUFFIX.values():
        f = getattr(lib, f"gibbs_replay_sweep_{sfx}")
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_int64, _vp, _vp, _vp, ctypes.c_int] + [_vp] * 11 + [ctypes.c_float]
    return lib


def _p(a):
    return a.ctypes.data_as(_vp)


def replay_sweep(lb, ip, data, low_memory, std_beta, mu_mult, half_var_tau, u_logs, unif, noise, eta, q, dq_scale=1.0):
    """`gibbs_sweep_host`'s signature and contract (eta, q float32 ``(m,)`` or Fortran-ordered ``(m, G)``, updated in place;
    returns eta_diff, var_mu, var_gamma), by the C file."""
    data = np.ascontiguousarray(data)
    fn = getattr(_lib(), f"gibbs_replay_sweep_{_SUFFIX[data.dtype]}")
    lb = np.ascontiguousarray(lb, dtype=np.int32)
    ip = np.ascontiguousarray(ip, dtype=np.int64)
    m = lb.shape[0]
    beta = np.ascontiguousarray(std_beta, dtype=np.float32)
    assert eta.dtype == q.dtype == np.float32 and eta.shape == q.shape and eta.shape[0] == m
    shape = eta.shape
    outs = [np.zeros(shape, dtype=np.float32, order="F") for _ in range(3)]
    cols = lambda a: np.asarray(a).reshape(m, -1)
    ins = [cols(a) for a in (mu_mult, half_var_tau, u_logs, unif, noise)]
    E, Q = cols(eta), cols(q)
    O = [cols(o) for o in outs]
    for g in range(E.shape[1]):
        col = [np.ascontiguousarray(a[:, g], dtype=np.float32) for a in ins]
        e, qq = np.array(E[:, g]), np.array(Q[:, g])
        o = [np.zeros(m, dtype=np.float32) for _ in range(3)]
        rc = fn(m, _p(lb), _p(ip), _p(data), int(bool(low_memory)), _p(beta), *[_p(a) for a in col], _p(e), _p(qq), _p(o[0]),
                _p(o[1]), _p(o[2]), float(np.float32(dq_scale)))
        assert rc == 0
        E[:, g], Q[:, g] = e, qq
        for dst, src in zip(O, o):
            dst[:, g] = src
    return tuple(outs)


def chain_inputs(n_per_snp, pairs, m_total=None):
    """``mu_mult, half_var_tau, u_logs`` (float32, Fortran ``(m, G)``) of the chains ``pairs = ((p, h2), ...)``: what
    `prep_columns` writes for LDpred2's parameters (`viprs_amd.stats.gibbs.gibbs_prep_host`)."""
    from viprs_amd.stats.gibbs import gibbs_prep_host
    m = n_per_snp.shape[0]
    out = [np.zeros((m, len(pairs)), dtype=np.float32, order="F") for _ in range(3)]
    for g, (p, h2) in enumerate(pairs):
        for o, v in zip(out, gibbs_prep_host(n_per_snp, m if m_total is None else m_total, p, h2)):
            o[:, g] = v
    return tuple(out)


# ---- the two-chromosome case of the model tests -------------------------------------------------------------------------------
MODEL_CHROMS = {1: [130, 64], 2: [200, 1]}
MODEL_H2 = 0.5


def model_gdl(chroms=None, n=5e4):
    from viprs_amd.data import ArrayDataLoader
    return ArrayDataLoader.synthetic(MODEL_CHROMS if chroms is None else chroms, ld_dtype=np.int8, n=n, kind="longrange",
                                     h2=MODEL_H2)
