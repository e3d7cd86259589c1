#!/usr/bin/env python3
"""Time the LD scores (`viprs_plan_ld_scores`) next to the LD product of the same plan on the cfg3 synthetic workload
(development tool; one JSON line).

    python tools/ld_score_bench.py [--config cfg3] [--calls 30]

For {fp32, int8} LD x {upper, symmetric}, float32 state: unit-weight scores against `LDPlan.dot` with one column, and 32
annotation columns against the 32-column product.  Both read the same LD bytes; the product reads B as well.  After a
warm-up of both, the two calls ALTERNATE `--calls` times in one process; times are the kernels' own HIP events
(`last_ld_score_ms` / `last_dot_ms`: no upload, no download inside the bracket).  `ratio` = median score / median product.
bytes = stored LD bytes of the device layout + the vectors read and written; `frac_peak` is against 8 TB/s."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viprs_amd import _lib as L                          # noqa: E402
from viprs_amd.plan import LDPlan                        # noqa: E402
from viprs_amd.utils import synthetic as syn             # noqa: E402

PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--ld-dtypes", default="float32,int8")
    args = ap.parse_args()
    if L.device_count() < 1:
        raise SystemExit("ld_score_bench: no HIP device visible")
    sizes = syn.block_sizes(args.config)
    rows = []
    for ld_name in args.ld_dtypes.split(","):
        for low_memory in (True, False):
            skel = syn.make_ld(sizes, low_memory=low_memory, ld_dtype=np.dtype(ld_name), kind="longrange", data=False)
            plan = LDPlan.synthetic(skel)
            m = plan.m
            ld_bytes = plan.info(L.INFO_LD_BYTES_DEVICE)
            rng = np.random.default_rng(12345)
            corr = np.full(m, 1.0 / (5e4 - 2.0))
            for n_cols in (1, 32):
                B = rng.standard_normal(m if n_cols == 1 else (m, n_cols)).astype(np.float32)
                A = None if n_cols == 1 else np.asfortranarray(B)
                for _ in range(3):
                    plan.dot(B, dq_scale=skel.dq_scale)
                    plan.ld_scores(A, corr, dq_scale=skel.dq_scale)
                t_dot, t_score = [], []
                for _ in range(args.calls):
                    plan.dot(B, dq_scale=skel.dq_scale)
                    t_dot.append(plan.last_dot_ms())
                    plan.ld_scores(A, corr, dq_scale=skel.dq_scale)
                    t_score.append(plan.last_ld_score_ms())
                dot_ms, score_ms = float(np.median(t_dot)), float(np.median(t_score))
                score_bytes = ld_bytes + m * 8 + m * n_cols * 4 * (1 if A is None else 2)
                rows.append({"ld": ld_name, "form": "upper" if low_memory else "symmetric", "n_cols": n_cols,
                             "weights": "unit" if A is None else "annotation",
                             "score_ms": round(score_ms, 4), "score_ms_min": round(float(np.min(t_score)), 4),
                             "score_ms_max": round(float(np.max(t_score)), 4),
                             "dot_ms": round(dot_ms, 4), "dot_ms_min": round(float(np.min(t_dot)), 4),
                             "dot_ms_max": round(float(np.max(t_dot)), 4),
                             "ratio": round(score_ms / dot_ms, 3), "bytes": int(score_bytes),
                             "frac_peak": round(score_bytes / (score_ms * 1e-3) / PEAK, 3)})
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
            plan.close()
    print(json.dumps({"tool": "ld_score_bench", "config": args.config, "m": int(m), "calls": args.calls, "rows": rows}))


if __name__ == "__main__":
    main()
