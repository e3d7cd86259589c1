#!/usr/bin/env python3
"""Time SuSiE fine-mapping (`LDPlan.susie`, the fit of `SuSiE.fit`) on the cfg3 synthetic workload next to the 1-column LD
product of the same plan, and `susie_host` on cfg2 as the host baseline (development tool; one JSON line, also written to
profiles/susie_bench.json).

    python tools/susie_bench.py [--config cfg3] [--calls 3] [--ld-dtypes float32,int8] [--L 1,10] [--max-iter 100]
                                [--host-config cfg2 | --no-host] [--out profiles/susie_bench.json]

Upper-form LD generated on the device, z = sqrt(n) x simulated standardised effects.  Per LD dtype and L: a warm-up call,
then `--calls` calls; `total_ms` is the HIP-event time from the first to the last kernel of a call (the loop's read-backs
included), `step_kernel_ms` the event time of ONE step kernel (effect L - 1 of iteration 1: every block still running),
`dot_ms` the event time of a 1-column product of the same plan in the same process.  `frozen_share` is the share of the
products' LD entries that belong to blocks already frozen when the product ran -- INFERRED from the per-block iteration counts
and the block sizes (entries ~ size^2), not measured: what a row filter could save.  The host baseline runs pinned to one
core (`os.sched_setaffinity`)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viprs_amd.plan import LDPlan                        # noqa: E402
from viprs_amd.utils import synthetic as syn             # noqa: E402


def device_rows(args):
    sizes = syn.block_sizes(args.config)
    rows = []
    for ld_name in args.ld_dtypes.split(","):
        skel = syn.make_ld(sizes, low_memory=True, ld_dtype=np.dtype(ld_name), kind="longrange", data=False)
        ss = syn.make_sumstats(skel, n=args.n, h2=args.h2)
        z = np.sqrt(np.asarray(ss.n_per_snp, dtype=np.float64)) * np.asarray(ss.std_beta, dtype=np.float64)
        plan = LDPlan.synthetic(skel)
        m = plan.m
        size = np.diff(plan.blocks()[0]).astype(np.float64)
        one = np.ones(m, dtype=np.float32)
        for L in (int(v) for v in args.L.split(",")):
            kw = dict(L=L, dq_scale=skel.dq_scale, tol=args.tol, max_iter=args.max_iter, check_every=args.check_every)
            info = plan.susie(z, **kw)                                   # warm-up
            t, st, steps = [], [], 0
            for _ in range(args.calls):
                info = plan.susie(z, **kw)
                ms, steps, step_ms = plan.last_susie_ms()
                t.append(ms)
                st.append(step_ms)
            d = []
            for _ in range(args.calls):
                plan.dot(one, dq_scale=skel.dq_scale)
                d.append(plan.last_dot_ms())
            it = info.iterations.astype(np.float64)
            launched = steps // L
            rows.append({"ld": ld_name, "state": "float32", "L": L, "m": int(m), "blocks": int(it.shape[0]),
                         "max_block": int(size.max()), "max_iter": args.max_iter, "tol": args.tol,
                         "iterations_launched": int(launched), "steps": int(steps),
                         "iters_min": int(it.min()), "iters_median": float(np.median(it)), "iters_max": int(it.max()),
                         "converged_share": round(float(np.mean(info.status == 0)), 4),
                         "frozen_share": round(float(1.0 - (it * size * size).sum() / (launched * (size * size).sum())), 4),
                         "total_ms": round(float(np.mean(t)), 3), "total_ms_min": round(float(np.min(t)), 3),
                         "step_ms": round(float(np.mean(t)) / steps, 4),
                         "step_kernel_ms": round(float(np.mean(st)), 4), "step_kernel_ms_min": round(float(np.min(st)), 4),
                         "dot_ms": round(float(np.mean(d)), 4), "dot_ms_min": round(float(np.min(d)), 4),
                         "step_kernel_over_dot": round(float(np.mean(st) / np.mean(d)), 3)})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
        plan.close()
    return rows


def host_row(args):
    from viprs_amd.stats.susie import susie_host
    try:
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
    except (AttributeError, OSError):
        pass
    ld = syn.make_ld(syn.block_sizes(args.host_config), low_memory=True, ld_dtype=np.float32, kind="longrange")
    ss = syn.make_sumstats(ld, n=args.n, h2=args.h2)
    z = np.sqrt(np.asarray(ss.n_per_snp, dtype=np.float64)) * np.asarray(ss.std_beta, dtype=np.float64)
    t0 = time.perf_counter()
    info = susie_host(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, True, z, L=10, dq_scale=ld.dq_scale, tol=args.tol,
                      max_iter=args.max_iter)
    sec = time.perf_counter() - t0
    return {"config": args.host_config, "m": int(z.shape[0]), "blocks": int(info.status.shape[0]), "L": 10,
            "iters_max": int(info.iterations.max()), "converged_share": round(float(np.mean(info.status == 0)), 4),
            "seconds": round(sec, 3), "cores": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--ld-dtypes", default="float32,int8")
    ap.add_argument("--L", default="1,10")
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--check-every", type=int, default=4)
    ap.add_argument("--h2", type=float, default=0.3)
    ap.add_argument("--n", type=float, default=3.5e5)
    ap.add_argument("--host-config", default="cfg2")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-device", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "susie_bench.json"))
    args = ap.parse_args()
    result = {"tool": "susie_bench", "config": args.config, "calls": args.calls, "h2": args.h2, "n": args.n,
              "check_every": args.check_every, "rows": [] if args.no_device else device_rows(args),
              "host": None if args.no_host else host_row(args)}
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
