#!/usr/bin/env python3
"""Fingerprint of the seven summary-statistics models (development tool; one JSON object on stdout, also written to --out).

    python tools/model_fingerprint.py --backend host|device [--out FILE]

Builds `ClumpThreshold`, `LDPredInf`, `Lassosum`, `LDpred2` (grid and auto), `PRSCS`, `SBayesR` and `SuSiE` through their
public constructors only -- so the same file runs on any commit that has the seven classes -- on one small synthetic loader
(two chromosomes, LD blocks of [130, 64] and [200, 1] SNPs, int8 long-range LD with a panel size, so that the LD-score
estimate of h2 runs where a model has one), fits each with small grids and at most 20 sweeps per chain, and reports for every
model the sha256 of the bytes of each ``post_mean_beta[c]`` and, where the model has them, of ``pip[c]``, ``index_of[c]``,
every numeric `grid_table` column (as float64) and ``h2`` / ``h2_init``, with shapes and dtypes.  Two runs of two commits on
the same machine are compared as files: a refactor of the model layer leaves them byte-identical.

``--backend host``: the package's host definitions as hooks (for `LDPredInf` a dense ``numpy.linalg.solve`` per merged
matrix, defined here).  ``--backend device``: no hooks, everything on HIP device 0.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHROMS = {1: [130, 64], 2: [200, 1]}


def digest(a):
    a = np.ascontiguousarray(a)
    return dict(sha256=hashlib.sha256(a.tobytes()).hexdigest(), shape=list(a.shape), dtype=a.dtype.name)


def dense_solve(lb, ip, data, low_memory, b, shift, dq_scale, rtol, maxiter, x0):
    """``(R + shift I) x = b`` by a dense solve in float64 over the merged matrix (the `solve_fn` hook of `LDPredInf`)."""
    from viprs_amd.model.ClumpThreshold import _host_dot
    from viprs_amd.plan import RidgeInfo
    m = b.shape[0]
    R = _host_dot(lb, ip, data, low_memory, np.eye(m), dq_scale)
    x = np.linalg.solve(R + shift * np.eye(m), b.astype(np.float64)).astype(b.dtype)
    return x, RidgeInfo([0], [0.0], [RidgeInfo.CONVERGED])


def models(host):
    """``{name: constructor}``; every constructor takes the loader."""
    from viprs_amd.model import LDpred2, Lassosum, PRSCS, SBayesR
    from viprs_amd.model.ClumpThreshold import ClumpThreshold
    from viprs_amd.model.LDPredInf import LDPredInf
    from viprs_amd.model.SuSiE import SuSiE
    from viprs_amd.stats.clump import clump_host
    from viprs_amd.stats.enet import enet_sweep_host
    from viprs_amd.stats.gibbs import gibbs_sweep_host
    from viprs_amd.stats.susie import susie_host
    hook = lambda name, fn: {name: fn} if host else {}
    deq = dict(dequantize_on_the_fly=True)
    return {
        "ClumpThreshold": lambda g: ClumpThreshold(g, r2=(0.1, 0.5), p_thresholds=(1e-4, 0.05, 1.0), **deq,
                                                   **hook("clump_fn", clump_host)),
        "LDPredInf": lambda g: LDPredInf(g, h2=None, **deq, **hook("solve_fn", dense_solve)),
        "Lassosum": lambda g: Lassosum(g, s=(0.5, 1.0), lambdas=(0.012, 0.005, 0.002), max_sweeps=20, **deq,
                                       **hook("sweep_fn", enet_sweep_host)),
        "LDpred2_grid": lambda g: LDpred2(g, mode="grid", p=(0.05, 1.0), h2_init="ldsc", burn_in=5, num_iter=10, seed=3, **deq,
                                          **hook("sweep_fn", gibbs_sweep_host)),
        "LDpred2_auto": lambda g: LDpred2(g, mode="auto", n_chains=3, h2_init="ldsc", burn_in=10, num_iter=10, seed=3, **deq,
                                          **hook("sweep_fn", gibbs_sweep_host)),
        "PRSCS": lambda g: PRSCS(g, phi=(1e-2, None), n_iter=20, n_burnin=10, thin=2, seed=3, **deq,
                                 **hook("sweep_fn", gibbs_sweep_host)),
        "SBayesR": lambda g: SBayesR(g, h2_init="ldsc", n_iter=20, n_burnin=8, n_chains=2, seed=3, **deq,
                                     **hook("backend", "host")),
        "SuSiE": lambda g: SuSiE(g, L=3, **deq, **hook("fit_fn", susie_host)),
    }


def fingerprint(model, fit_kw):
    model.fit(**fit_kw)
    out = {"post_mean_beta": {str(c): digest(b) for c, b in model.post_mean_beta.items()}}
    for name in ("pip", "index_of"):
        per_chromosome = getattr(model, name, None)
        if per_chromosome is not None:
            out[name] = {str(c): digest(a) for c, a in per_chromosome.items()}
    table = getattr(model, "grid_table", None)
    if table is not None:
        out["grid_table"] = {str(k): digest(table[k].to_numpy(dtype=np.float64)) for k in table.columns
                             if np.issubdtype(table[k].dtype, np.number) or table[k].dtype == bool}
    for name in ("h2", "h2_init"):
        v = getattr(model, name, None)
        if v is not None:
            out[name] = digest(np.asarray(v, dtype=np.float64))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", choices=("host", "device"), required=True)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from viprs_amd.data import ArrayDataLoader
    host = args.backend == "host"
    if not host:
        from viprs_amd import _lib
        if _lib.device_count() < 1:
            raise SystemExit("model_fingerprint: no HIP device visible")
    result = {"tool": "model_fingerprint", "backend": args.backend, "models": {}}
    for name, make in models(host).items():
        gdl = ArrayDataLoader.synthetic(CHROMS, ld_dtype=np.int8, n=5e4, kind="longrange", h2=0.5, ld_sample_size=5000)
        result["models"][name] = fingerprint(make(gdl), dict(max_iter=20) if name == "SuSiE" else {})
    text = json.dumps(result, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
