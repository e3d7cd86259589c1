"""Host replay of the SBayesR sweep (tests/bayesr_replay.c through ctypes: libm `expf` in the softmax, libm `fmaf` where the
header writes an fma) -- what the `==` tests of `viprs_state_bayesr_sweep` and of `viprs_amd.stats.bayesr.bayesr_sweep_host`
compare with -- and the small shared pieces of those tests: the inputs of a chain, the case of the model tests."""
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bayesr_replay.c")
_SUFFIX = {np.dtype(np.float32): "f32", np.dtype(np.int8): "i8", np.dtype(np.int16): "i16"}
_vp = ctypes.c_void_p


@functools.lru_cache(maxsize=None)
def _lib():
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    out = os.path.join(tempfile.mkdtemp(prefix="bayesr_replay_"), "libbayesrreplay.so")
    subprocess.run([cc, "-O2", "-ffp-contract=off", "-fPIC", "-shared", _SRC, "-o", out, "-lm"], check=True)
    lib = ctypes.CDLL(out)
    for sfx in _SUFFIX.values():
        f = getattr(lib, f"bayesr_replay_sweep_{sfx}")
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_int64, ctypes.c_int, _vp, _vp, _vp, ctypes.c_int] + [_vp] * 13 + [ctypes.c_float]
    return lib


def _p(a):
    return a.ctypes.data_as(_vp)


def replay_sweep(lb, ip, data, low_memory, std_beta, mu_mult, sqrt_half_var_tau, u_logs, log_null_pi, unif, z, eta, q,
                 dq_scale=1.0):
    """`bayesr_sweep_host`'s signature and contract (eta, q float32 ``(m,)``, updated in place; returns eta_diff, var_mu,
    var_gamma, kstar), by the C file."""
    data = np.ascontiguousarray(data)
    fn = getattr(_lib(), f"bayesr_replay_sweep_{_SUFFIX[data.dtype]}")
    lb = np.ascontiguousarray(lb, dtype=np.int32)
    ip = np.ascontiguousarray(ip, dtype=np.int64)
    m = lb.shape[0]
    K = np.asarray(mu_mult).shape[1]
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    ins = [f(a) for a in (std_beta, mu_mult, sqrt_half_var_tau, u_logs, log_null_pi, unif, z)]
    assert eta.dtype == q.dtype == np.float32 and eta.shape == q.shape == (m,) and eta.flags.c_contiguous and q.flags.c_contiguous
    ed, mu, gam = np.zeros(m, np.float32), np.zeros((m, K), np.float32), np.zeros((m, K), np.float32)
    ks = np.zeros(m, np.int32)
    rc = fn(m, K, _p(lb), _p(ip), _p(data), int(bool(low_memory)), *[_p(a) for a in ins], _p(eta), _p(q), _p(ed), _p(mu), _p(gam),
            _p(ks), float(np.float32(dq_scale)))
    assert rc == 0
    return ed, mu, gam, ks


def chain_inputs(n_per_snp, pi, gamma, sigma2_beta, sigma2_e=1.0):
    """``mu_mult, sqrt_half_var_tau, u_logs`` (float32 ``(m, K)``) and ``log_null_pi`` (``(m,)``) of a chain: what `prep_mixture`
    writes for SBayesR's parameters (`viprs_amd.stats.bayesr.bayesr_prep_host`)."""
    from viprs_amd.stats.bayesr import bayesr_prep_host
    return bayesr_prep_host(n_per_snp, pi, gamma, sigma2_beta, sigma2_e)


# Parameters under which every outcome k* = 0 .. K turns up in every block of 64 or more SNPs of the per-SNP-input tests: a null
# weight of one half and component variances of the order of the squared marginal effects, so that no weight is negligible.
SPREAD_PI = {1: (0.5, 0.5), 3: (0.4, 0.2, 0.2, 0.2)}
SPREAD_GAMMA = {1: (1.0,), 3: (0.25, 1.0, 4.0)}

SPREAD_SIGMA2_BETA = 1e-5


def spread_inputs(m, K, seed=None):
    """The four inputs under the parameters above with the per-SNP sample sizes n_j of tests/per_snp_inputs.py and a null
    weight that varies along the SNPs as well (pi_0 sqrt(w_j)): no input is one value repeated."""
    from tests import per_snp_inputs as PS
    dr = PS.Draws(m, PS.SEED if seed is None else seed)
    mm, sv, ul, lnp = chain_inputs(dr.n, SPREAD_PI[K], SPREAD_GAMMA[K], SPREAD_SIGMA2_BETA)
    return mm, sv, ul, (lnp.astype(np.float64) + 0.5 * np.log(dr.w)).astype(np.float32)


def every_outcome_in_every_block(kstar, block_start, K, min_size=64):
    bs = np.asarray(block_start)
    return all(np.bincount(kstar[int(s):int(e)], minlength=K + 1).min() > 0 for s, e in zip(bs[:-1], bs[1:]) if e - s >= min_size)


# ---- the three-chromosome case of the model tests -----------------------------------------------------------------------------
MODEL_CHROMS = {1: [130, 64], 2: [200, 1], 3: [96]}
MODEL_H2 = 0.5


def model_gdl(chroms=None, n=5e4, seed=None):
    from viprs_amd.data import ArrayDataLoader
    kw = {} if seed is None else {"seed": seed}
    return ArrayDataLoader.synthetic(MODEL_CHROMS if chroms is None else chroms, ld_dtype=np.int8, n=n, kind="longrange",
                                     h2=MODEL_H2, **kw)
