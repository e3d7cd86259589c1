#!/usr/bin/env python3
"""What the extremal eigenvalues of a synthetic panel cost (`LDPlan.extremal_eigenvalues`; development tool; one JSON line).

    python tools/spectrum_workload.py [--configs cfg2,cfg3] [--ld-dtypes float32,int8] [--states float32]
                                      [--rtol 1e-4] [--maxiter 2048] [--calls 2]

Upper-form "longrange" LD generated on the device.  Per config, LD dtype and state precision, after a warm-up call:
`ms` the HIP-event time of a call from its first to its last kernel (the checks of the stopping rule included), `products`
the LD products it launched (one per iteration), `host_ms` / `host_share` the time the host spent inside the checks
(downloading the coefficients, the implicit-QL eigenproblems), the histogram of the per-block iteration counts (they are
check points: powers of two, or maxiter), the blocks left at status 1 with their sizes, the iteration count of the largest
block, and the extremes over the panel.
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
    ap.add_argument("--configs", default="cfg2,cfg3")
    ap.add_argument("--ld-dtypes", default="float32,int8")
    ap.add_argument("--states", default="float32")
    ap.add_argument("--rtol", type=float, default=1e-4)
    ap.add_argument("--maxiter", type=int, default=2048)
    ap.add_argument("--calls", type=int, default=2)
    args = ap.parse_args()
    rows = []
    for config in args.configs.split(","):
        sizes = np.asarray(syn.block_sizes(config))
        for ld_name in args.ld_dtypes.split(","):
            skel = syn.make_ld(sizes, low_memory=True, ld_dtype=np.dtype(ld_name), kind="longrange", data=False)
            plan = LDPlan.synthetic(skel)
            block_size = np.diff(plan.blocks()[0])
            for T in args.states.split(","):
                kw = dict(dq_scale=skel.dq_scale, rtol=args.rtol, maxiter=args.maxiter, float_precision=T)
                info = plan.extremal_eigenvalues(**kw)                                      # warm-up
                t, host, launched = [], [], 0
                for _ in range(args.calls):
                    info = plan.extremal_eigenvalues(**kw)
                    ms, launched, host_ms = plan.last_spectrum_ms()
                    t.append(ms)
                    host.append(host_ms)
                it = info.iterations.astype(np.int64)
                counts, n = np.unique(it, return_counts=True)
                stuck = np.nonzero(info.status == 1)[0]
                rows.append({"config": config, "ld": ld_name, "state": T, "m": int(plan.m), "blocks": int(it.shape[0]),
                             "max_block": int(block_size.max()), "rtol": args.rtol, "maxiter": args.maxiter,
                             "ms": round(float(np.mean(t)), 3), "ms_min": round(float(np.min(t)), 3),
                             "products": int(launched), "ms_per_product": round(float(np.mean(t)) / max(launched, 1), 4),
                             "dot_ms": round(plan.last_dot_ms(), 4),
                             "host_ms": round(float(np.mean(host)), 3),
                             "host_share": round(float(np.mean(host)) / float(np.mean(t)), 3),
                             "iterations_histogram": {int(c): int(k) for c, k in zip(counts, n)},
                             "iterations_of_largest_block": int(it[np.argmax(block_size)]),
                             "status_1_blocks": int(stuck.shape[0]),
                             "status_1_sizes": sorted(int(s) for s in block_size[stuck])[-8:],
                             "live_share": round(float((it * block_size).sum() / (max(launched, 1) * plan.m)), 3),
                             "lambda_min": float(info.lambda_min.min()), "lambda_max": float(info.lambda_max.max()),
                             "worst_resid_over_scale": float(np.max(np.maximum(info.resid_min, info.resid_max) /
                                                                    np.maximum(np.abs(info.lambda_min), np.abs(info.lambda_max))))})
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
            plan.close()
    print(json.dumps({"tool": "spectrum_workload", "calls": args.calls, "rows": rows}))


if __name__ == "__main__":
    main()
