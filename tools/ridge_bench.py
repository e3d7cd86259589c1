#!/usr/bin/env python3
"""Time the ridge solve (`LDPlan.solve_ridge`, the solve of `LDPredInf.fit`) on the cfg3 synthetic workload next to the LD
product of the same plan (development tool; one JSON line).

    python tools/ridge_bench.py [--config cfg3] [--calls 5] [--ld-dtypes float32,int8] [--h2 0.3] [--n 3.5e5]

Upper-form LD generated on the device, simulated summary statistics as the right-hand side, shift = m / (n h2).  Per LD
dtype and state precision: a warm-up solve, then `--calls` solves; `solve_ms` is the HIP-event time from the first to the
last kernel of a solve (the loop's read-backs included), `iter_ms` = solve_ms / launched iterations, `dot_ms` the event time
of the last product of the same plan.  The per-block iteration counts are reported as min / median / max and as the share
of block-iterations that ran on blocks still iterating (`live_share`: 1 - the work a block-dropping product would save).

What the fused kernel alone costs is read from a kernel trace of this tool, in a run of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/ridge_bench.py --ld-dtypes float32 --states float32 --calls 3
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viprs_amd.plan import LDPlan                        # noqa: E402
from viprs_amd.utils import synthetic as syn             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--ld-dtypes", default="float32,int8")
    ap.add_argument("--states", default="float32,float64")
    ap.add_argument("--h2", type=float, default=0.3)
    ap.add_argument("--n", type=float, default=3.5e5)
    ap.add_argument("--check-every", type=int, default=4)
    args = ap.parse_args()
    sizes = syn.block_sizes(args.config)
    rows = []
    for ld_name in args.ld_dtypes.split(","):
        skel = syn.make_ld(sizes, low_memory=True, ld_dtype=np.dtype(ld_name), kind="longrange", data=False)
        ss = syn.make_sumstats(skel, n=args.n, h2=args.h2)
        plan = LDPlan.synthetic(skel)
        m = plan.m
        lam = m / (args.n * args.h2)
        for T in args.states.split(","):
            b = ss.std_beta.astype(T)
            x, info = plan.solve_ridge(b, lam, dq_scale=skel.dq_scale, check_every=args.check_every)      # warm-up
            t, launched = [], 0
            for _ in range(args.calls):
                x, info = plan.solve_ridge(b, lam, dq_scale=skel.dq_scale, check_every=args.check_every)
                ms, launched = plan.last_solve_ms()
                t.append(ms)
            it = info.iterations.astype(np.int64)
            rows.append({"ld": ld_name, "state": T, "m": int(m), "blocks": int(it.shape[0]), "max_block": int(np.max(sizes)),
                         "lam": round(lam, 4), "converged": bool(info.converged), "launched": int(launched),
                         "iters_min": int(it.min()), "iters_median": float(np.median(it)), "iters_max": int(it.max()),
                         "live_share": round(float((it * np.diff(plan.blocks()[0])).sum() / (launched * m)), 3),
                         "relres_max": float(info.relres.max()),
                         "solve_ms": round(float(np.mean(t)), 4), "solve_ms_min": round(float(np.min(t)), 4),
                         "iter_ms": round(float(np.mean(t)) / launched, 4), "dot_ms": round(plan.last_dot_ms(), 4)})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
        plan.close()
    print(json.dumps({"tool": "ridge_bench", "config": args.config, "calls": args.calls, "h2": args.h2, "n": args.n,
                      "check_every": args.check_every, "rows": rows}))


if __name__ == "__main__":
    main()
