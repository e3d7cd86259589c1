#!/usr/bin/env python3
"""Time the LDpred2 Gibbs sweep (`viprs_state_gibbs_sweep`) next to the elastic-net sweep and the grid-column E-step sweep of
the same plan, its draws kernel, and `LDpred2(mode="auto")` per iteration (development tool; one JSON line, also written to
--out).

    python tools/gibbs_bench.py [--config cfg3] [--ld-dtypes float32,int8] [--rounds 6] [--per-round 5] [--no-fit] [--chains 30]

Per LD dtype: the workload in the upper form, "longrange" LD generated on the device, ONE plan (created with
VIPRS_GRID_MFMA=0, so the grid-column E-step runs as (block, model) items of the panel sweep, the path the Gibbs policy
shares) and on it: an elastic-net state of width 1 and one of 3 columns (the states of tools/enet_bench.py), and grid states
of width 1 and 3 prepared for LDpred2's (p, h2) = (0.5, 0.2), (0.01, 0.2), (0.9, 0.4), swept once by the E-step (`e_step`) and
once by the Gibbs sweep.  Every timed sweep starts from eta = q = 0.  After a warm-up the kinds alternate, `--per-round`
sweeps each, for `--rounds` rounds in ONE process; sweep times are the plan's own HIP events (`viprs_plan_last_kernel_ms`,
which = 0: the draws kernel is outside them), the draws kernel's is `viprs_plan_last_gibbs_draws_ms`.  Reported per kind:
median, min and max in ms; the ratios of the Gibbs medians to the elastic-net and the grid-column medians of the same width.

`fit`: `LDpred2(mode="auto")` with `--chains` chains, 20 + 10 iterations, on the same plan (int8 LD unless --fit-ld says
otherwise): wall time per iteration.  The model is put on the device-generated plan directly (`LDpred2.from_plan`; no LD on
the host).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

os.environ.setdefault("VIPRS_GRID_MFMA", "0")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viprs_amd.utils import synthetic as syn             # noqa: E402

ENET = ((0.2, 0.005), (0.5, 0.002), (0.9, 0.005))
PAIRS = ((0.5, 0.2), (0.01, 0.2), (0.9, 0.4))


def stats(t):
    t = np.asarray(t, dtype=np.float64)
    return dict(median_ms=round(float(np.median(t)), 4), min_ms=round(float(t.min()), 4), max_ms=round(float(t.max()), 4),
                n=int(t.shape[0]))


def sweep_times(plan, skel, ss, inp, rounds, per_round):
    from viprs_amd.plan import DeviceState
    from viprs_amd.stats.gibbs import gibbs_prep_rows
    m, dq = plan.m, skel.dq_scale
    f32 = np.float32
    e1 = DeviceState(plan, "float32", placement="off")
    e1.upload("std_beta", inp.std_beta)
    e1.upload("mu_mult", np.full(m, f32(0.5)))
    e1.upload("sqrt_half_var_tau", np.full(m, f32(0.002)))
    e3 = DeviceState(plan, "float32", model="grid", width=3, placement="off")
    e3.upload("std_beta", inp.std_beta)
    e3.upload("mu_mult", np.asfortranarray(np.repeat(np.array([[1.0 - s for s, _ in ENET]], dtype=f32), m, axis=0)))
    e3.upload("half_var_tau", np.asfortranarray(np.repeat(np.array([[lam for _, lam in ENET]], dtype=f32), m, axis=0)))
    grid = {}
    for w in (1, 3):
        st = DeviceState(plan, "float32", model="grid", width=w, placement="off")
        st.upload("std_beta", inp.std_beta)
        st.set_n_per_snp(ss.n_per_snp)
        st.prep_columns(gibbs_prep_rows(np.arange(w), m, [p for p, _ in PAIRS[:w]], [h for _, h in PAIRS[:w]]))
        grid[w] = st
    count = {"i": 0}

    def gibbs(st):
        count["i"] += 1
        st.gibbs_sweep(dq, seed=1, draw_index=count["i"])
    kinds = {"enet_width1": (e1, lambda: e1.enet_sweep(dq)), "enet_grid3": (e3, lambda: e3.enet_sweep(dq)),
             "grid_column_width1": (grid[1], lambda: grid[1].e_step(dq)), "grid_column_grid3": (grid[3], lambda: grid[3].e_step(dq)),
             "gibbs_width1": (grid[1], lambda: gibbs(grid[1])), "gibbs_grid3": (grid[3], lambda: gibbs(grid[3]))}
    times = {k: [] for k in kinds}
    draws = {"gibbs_width1": [], "gibbs_grid3": []}

    def run(name, n, keep):
        st, fn = kinds[name]
        for _ in range(n):
            st.reset(inp.pi)
            fn()
            if keep:
                times[name].append(plan.last_kernel_ms(0))
                if name in draws:
                    draws[name].append(plan.last_gibbs_draws_ms())
    for name in kinds:                                       # warm-up: code objects, clocks
        run(name, 10, False)
    for _ in range(rounds):
        for name in kinds:
            run(name, per_round, True)
    nonzero = [float(v) for v in np.count_nonzero(grid[3].download("eta"), axis=0) / m]
    for st in (e1, e3, grid[1], grid[3]):
        st.close()
    out = {k: stats(v) for k, v in times.items()}
    for w in ("width1", "grid3"):
        g = out[f"gibbs_{w}"]
        g["draws_kernel"] = stats(draws[f"gibbs_{w}"])
        g["ratio_to_enet"] = round(g["median_ms"] / out[f"enet_{w}"]["median_ms"], 4)
        g["ratio_to_grid_column"] = round(g["median_ms"] / out[f"grid_column_{w}"]["median_ms"], 4)
        g["draws_over_sweep"] = round(g["draws_kernel"]["median_ms"] / g["median_ms"], 4)
    out["eta_nonzero_after_one_gibbs_sweep"] = nonzero
    return out


def auto_on_plan(plan, skel, ss, std_beta, chains, burn_in=20, num_iter=10):
    """`LDpred2(mode="auto").fit()` on a plan that exists on the device only."""
    from viprs_amd.model import LDpred2

    model = LDpred2.from_plan(plan, std_beta, ss.n_per_snp, skel.dq_scale, 0.2, mode="auto", burn_in=burn_in, num_iter=num_iter,
                              n_chains=chains, seed=1)
    t0 = time.perf_counter()
    model.fit()
    wall = time.perf_counter() - t0
    t = model.grid_table
    return dict(chains=chains, iterations=burn_in + num_iter, wall_s=round(wall, 3),
                wall_ms_per_iteration=round(1e3 * wall / (burn_in + num_iter), 3), diverged=int(t["diverged"].sum()),
                kept=int(t["kept"].sum()), p_est_median=float(np.nanmedian(model.p_est)),
                h2_est_median=float(np.nanmedian(model.h2_est)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--ld-dtypes", default="float32,int8")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--per-round", type=int, default=5)
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--fit-ld", default="int8")
    ap.add_argument("--chains", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from viprs_amd import _lib as L
    from viprs_amd.plan import LDPlan
    if L.device_count() < 1:
        raise SystemExit("gibbs_bench: no HIP device visible")
    result = {"tool": "gibbs_bench", "config": args.config, "sweeps": {}}
    sizes = syn.block_sizes(args.config)
    for ld_name in dict.fromkeys(args.ld_dtypes.split(",") + ([] if args.no_fit else [args.fit_ld])):
        skel = syn.make_ld(sizes, low_memory=True, ld_dtype=np.dtype(ld_name), kind="longrange", data=False)
        ss = syn.make_sumstats(skel)
        inp = syn.make_inputs(ss)
        plan = LDPlan.synthetic(skel)
        if ld_name in args.ld_dtypes.split(","):
            result["sweeps"][ld_name] = sweep_times(plan, skel, ss, inp, args.rounds, args.per_round)
            print(json.dumps({ld_name: result["sweeps"][ld_name]}), file=sys.stderr, flush=True)
        if not args.no_fit and ld_name == args.fit_ld:
            result["auto"] = dict(ld=ld_name, m=int(plan.m), **auto_on_plan(plan, skel, ss, inp.std_beta, args.chains))
            print(json.dumps(result["auto"]), file=sys.stderr, flush=True)
        plan.close()
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
