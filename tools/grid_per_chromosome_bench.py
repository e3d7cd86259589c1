#!/usr/bin/env python3
"""One grid search per chromosome (the reference CLI's default with --hyp-search GS / BMA): the 22 chromosomes' 32-point
grids in ONE lock-step batch (`VIPRSGridPerChromosome`: one prep, one masked sweep, one reduction per EM round) against
22 `VIPRSGrid(batched=True)` fits run one after the other.  Mirrors bench.py:measure_per_chromosome: the cfg3 workload
split into 22 chromosomes (bench.split_into_chromosomes), the 32-point grid of BASELINE configs[4]
(synthetic.grid_points), stopping rules held off (`min_iter`) so that every round updates every pair.

Prints one JSON line: ms per EM round of the batch and of the sequential fits, the sweep kernels' mean time, and
whether every pair's ELBO trajectory was identical in the two.

    python tools/grid_per_chromosome_bench.py [--iters 8] [--warmup 3] [--config cfg3] [--symmetric]
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
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--symmetric", action="store_true", help="symmetric LD (default: upper-triangular, as bench.py)")
    ap.add_argument("--grid-models", type=int, default=32)
    ap.add_argument("--seed", type=int, default=7209)
    args = ap.parse_args()

    from viprs_amd.model import HyperparameterGrid, VIPRSGrid, VIPRSGridPerChromosome
    from viprs_amd.model import _lockstep
    from viprs_amd.utils import synthetic as syn

    lm = not args.symmetric
    sizes = bench.config_sizes(args.config, args.seed)
    ld, ss, _, _ = bench.build_workload(SimpleNamespace(ld_kind="longrange", host_ld=True), sizes, None, args.seed, lm,
                                        np.dtype("float32"), data=True)
    gdl, chrom_sizes = split_into_chromosomes(ld, ss)
    # the grid of synthetic.grid_points (BASELINE configs[4]), the same for every chromosome (a {chromosome: grid} dict)
    sig, pi = syn.grid_points(args.grid_models)
    n_pi = 8 if args.grid_models % 8 == 0 and args.grid_models >= 8 else args.grid_models
    grid = HyperparameterGrid(sigma_epsilon_steps=args.grid_models // n_pi, pi_steps=n_pi, h2_est=0.1, h2_se=0.1, n_snps=1_100_000)
    tab = grid.to_table()
    assert np.array_equal(tab["sigma_epsilon"].to_numpy(), sig) and np.array_equal(tab["pi"].to_numpy(), pi)
    n_it = args.warmup + args.iters

    # every LockstepEM.update's ELBO vector, in call order (the trajectories compared below)
    record = []
    update = _lockstep.LockstepEM.update

    def recording_update(self, a, s, i):
        code = update(self, a, s, i)
        record.append(self.elbos.copy())
        return code
    _lockstep.LockstepEM.update = recording_update

    out = {"name": "22 per-chromosome grid searches (VIPRSGrid per chromosome, independent mode): lock-step batch vs one "
                   "VIPRSGrid(batched=True) after the other",
           "unit": "ms per EM round (one iteration of all 22 x G pairs)", "config": args.config, "low_memory": lm,
           "snps": int(ld.m), "chromosomes": 22, "grid_models": args.grid_models, "iterations": args.iters,
           "warmup_iterations": args.warmup}
    stamps = []
    model = VIPRSGridPerChromosome(gdl, {c: grid for c in chrom_sizes}, low_memory=lm)
    record.clear()
    model.fit(pathwise=False, max_iter=n_it, min_iter=n_it + 1, on_iteration=lambda i: stamps.append(time.perf_counter()))
    d = np.diff(np.array(stamps))[args.warmup - 1:]
    k = model._plans["*"].timing_history(which=0)
    G = model.n_models
    batch_elbos = {c: [r[gi * G:(gi + 1) * G] for r in record] for gi, c in enumerate(model.groups)}
    out["batched"] = {"ms_per_round": float(np.median(d)) * 1e3, "ms_per_round_all": [round(float(x) * 1e3, 4) for x in d],
                      "sweep_kernels_ms_avg": float(np.mean(k[-args.iters:])) if k else None}
    groups = list(model.groups)
    del model

    per_chrom, sweep_k, same = [], [], True
    for c, sub in gdl.split_by_chromosome().items():
        st = []
        one = VIPRSGrid(sub, grid, low_memory=lm)
        record.clear()
        one.fit(batched=True, max_iter=n_it, min_iter=n_it + 1, on_iteration=lambda i: st.append(time.perf_counter()))
        dd = np.diff(np.array(st))[args.warmup - 1:]
        per_chrom.append(float(np.median(dd)) * 1e3)
        kk = next(iter(one._plans.values())).timing_history(which=0)
        sweep_k.append(float(np.mean(kk[-args.iters:])) if kk else float("nan"))
        same = same and len(record) == len(batch_elbos[c]) and all(np.array_equal(x, y) for x, y in zip(record, batch_elbos[c]))
        del one
    assert groups == sorted(chrom_sizes)
    _lockstep.LockstepEM.update = update
    out["sequential"] = {"ms_per_round": float(np.sum(per_chrom)), "ms_per_iteration_per_chromosome": [round(x, 4) for x in per_chrom],
                         "sweep_kernels_ms_sum": float(np.sum(sweep_k))}
    out["elbo_trajectories_identical"] = bool(same)
    out["speedup_batched_over_sequential"] = out["sequential"]["ms_per_round"] / out["batched"]["ms_per_round"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
