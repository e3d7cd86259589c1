#!/usr/bin/env python3
"""One PATHWISE grid search per chromosome (the reference CLI's default with --hyp-search GS / BMA): the 22 chromosomes'
32-point grids in ONE lock-step batch (`VIPRSGridPathwisePerChromosome`: one prep, one sweep, one reduction per EM round,
a chromosome at one grid point at a time) against 22 `VIPRSGrid(...).fit(pathwise=True)` fits run one after the other.
The workload of tools/grid_per_chromosome_bench.py: cfg3 split into 22 chromosomes (bench.split_into_chromosomes),
upper-triangular fp32 LD, the 32-point grid of BASELINE configs[4] for every chromosome.  Stopping is held off
(`min_iter` and `patience` above G x max_iter): every grid point runs `--iters-per-point` iterations, every chromosome
G x that many rounds, and the batch and the sequential fits do the same work.

Prints one JSON line: ms per EM round of the batch and of the 22 sequential fits (median round; total wall time per
round as well), the sweep kernels' mean time, the commit call's time, and whether every chromosome's ELBO trajectory was
identical in the two.

    python tools/grid_pathwise_per_chromosome_bench.py [--iters-per-point 4] [--config cfg3] [--symmetric]
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                                                 # noqa: E402
from bench import split_into_chromosomes                                     # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters-per-point", type=int, default=4)
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--symmetric", action="store_true", help="symmetric LD (default: upper-triangular, as bench.py)")
    ap.add_argument("--grid-models", type=int, default=32)
    ap.add_argument("--seed", type=int, default=7209)
    args = ap.parse_args()

    from viprs_amd.model import HyperparameterGrid, VIPRSGrid, VIPRSGridPathwisePerChromosome
    from viprs_amd.utils import synthetic as syn

    lm = not args.symmetric
    sizes = bench.config_sizes(args.config, args.seed)
    ld, ss, _, _ = bench.build_workload(SimpleNamespace(ld_kind="longrange", host_ld=True), sizes, None, args.seed, lm,
                                        np.dtype("float32"), data=True)
    gdl, chrom_sizes = split_into_chromosomes(ld, ss)
    sig, pi = syn.grid_points(args.grid_models)
    n_pi = 8 if args.grid_models % 8 == 0 and args.grid_models >= 8 else args.grid_models
    grid = HyperparameterGrid(sigma_epsilon_steps=args.grid_models // n_pi, pi_steps=n_pi, h2_est=0.1, h2_se=0.1, n_snps=1_100_000)
    tab = grid.to_table()
    assert np.array_equal(tab["sigma_epsilon"].to_numpy(), sig) and np.array_equal(tab["pi"].to_numpy(), pi)
    G, K = args.grid_models, args.iters_per_point
    hold = G * K + 10                            # > every chromosome's whole history: no stopping rule fires
    fit_kw = dict(max_iter=K, min_iter=hold, patience=hold)

    out = {"name": "22 per-chromosome PATHWISE grid searches (VIPRSGrid per chromosome, pathwise mode): lock-step batch vs "
                   "one VIPRSGrid(...).fit(pathwise=True) after the other",
           "unit": "ms per EM round (one iteration of every chromosome at its current grid point)", "config": args.config,
           "low_memory": lm, "snps": int(ld.m), "chromosomes": 22, "grid_models": G, "iterations_per_point": K,
           "rounds": G * K}
    stamps = []
    model = VIPRSGridPathwisePerChromosome(gdl, {c: grid for c in chrom_sizes}, low_memory=lm)
    t0 = time.perf_counter()
    model.fit(on_iteration=lambda i: stamps.append(time.perf_counter()), **fit_kw)
    wall = time.perf_counter() - t0
    assert len(stamps) == G * K, len(stamps)
    d = np.diff(np.array(stamps))
    k = model._plans["*"].timing_history(which=0)
    # the commit call on its own: every chromosome into one column, host-timed around a synchronisation (launch included)
    ds, store = model._dstate["*"], model._store
    C = len(model.groups)
    tc = []
    for r in range(12):
        ds.synchronize()
        t = time.perf_counter()
        store.commit_groups(ds, np.arange(C), np.full(C, r % G))
        store.synchronize()
        tc.append(time.perf_counter() - t)
    out["batched"] = {"ms_per_round": float(np.median(d)) * 1e3, "ms_per_round_wall": wall / (G * K) * 1e3,
                      "sweep_kernels_ms_avg": float(np.mean(k)) if k else None,
                      "commit_call_ms_median": float(np.median(tc[2:])) * 1e3,
                      "nit_per_point": sorted({r.nit for rs in model.optim_results.values() for r in rs})}
    hist = {c: list(model.history[c]["ELBO"]) for c in model.groups}
    del model, ds, store

    per_chrom, per_chrom_wall, sweep_k, same = [], [], [], True
    for c, sub in gdl.split_by_chromosome().items():
        st = []
        one = VIPRSGrid(sub, grid, low_memory=lm)
        t0 = time.perf_counter()
        one.fit(pathwise=True, on_iteration=lambda i: st.append(time.perf_counter()), **fit_kw)
        per_chrom_wall.append((time.perf_counter() - t0) / (G * K) * 1e3)
        per_chrom.append(float(np.median(np.diff(np.array(st)))) * 1e3)
        kk = next(iter(one._plans.values())).timing_history(which=0)
        sweep_k.append(float(np.mean(kk)) if kk else float("nan"))
        same = same and one.history["ELBO"] == hist[c]
        del one
    out["sequential"] = {"ms_per_round": float(np.sum(per_chrom)), "ms_per_round_wall": float(np.sum(per_chrom_wall)),
                         "ms_per_iteration_per_chromosome": [round(x, 4) for x in per_chrom],
                         "sweep_kernels_ms_sum": float(np.sum(sweep_k))}
    out["elbo_trajectories_identical"] = bool(same)
    out["speedup_batched_over_sequential"] = out["sequential"]["ms_per_round"] / out["batched"]["ms_per_round"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
