#!/usr/bin/env python3
"""Time greedy LD clumping (`viprs_plan_clump`) on the cfg3 synthetic workload and on a 100 000-SNP band (development tool;
one JSON line).

    python tools/clump_bench.py [--config cfg3] [--calls 10] [--ld-dtypes float32,int8] [--no-host] [--no-band]

cfg3, upper form, "longrange" LD generated on the device, chi^2 from `make_sumstats` (order: every SNP by descending chi^2,
every SNP a member); the band: +-250 SNPs around the diagonal in one component, upper form, cubed-uniform entries, chi^2
drawn with 2 % inflated SNPs.  Per LD dtype: r2 = 0.1 alone, then the four columns (0.1, 0.2, 0.5, 0.8).  Reported per run:

* `clump_ms`     the kernels' own HIP events (`last_clump_ms`: no upload, no download inside the bracket), median of
                 `--calls` after a warm-up; min and max beside it
* `host_ms`      `viprs_amd.stats.clump.clump_host` on this machine's CPU, one run, for the runs of up to `--host-cols`
                 columns (default 1: the host loops over the columns, four cost four times one); the device result is
                 compared with it
* `score_ms`     unit-weight `ld_scores` of the same plan: one pass over the same LD bytes, the stream floor
* `steps_max`    index steps of the block with the most of them (SNPs that open a clump in at least one column), the size of
                 that block, and `ns_per_step` = clump_ms / steps_max: the kernel ends with its slowest block
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viprs_amd import _lib as L                          # noqa: E402
from viprs_amd.plan import LDPlan                        # noqa: E402
from viprs_amd.stats.clump import clump_host, clump_order  # noqa: E402
from viprs_amd.utils import synthetic as syn             # noqa: E402

R2_RUNS = ((0.1,), (0.1, 0.2, 0.5, 0.8))


def band_arrays(m, half_width, ld_dtype, seed=14):
    """One windowed component in the upper form: row j holds columns j + 1 .. j + half_width."""
    j = np.arange(m)
    length = np.minimum(j + half_width + 1, m) - (j + 1)
    ip = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    lb = np.minimum(j + 1, m - 1).astype(np.int32)
    u = np.random.default_rng(seed).uniform(-1.0, 1.0, int(ip[-1])).astype(np.float32) ** 3
    if np.issubdtype(ld_dtype, np.floating):
        return lb, ip, u.astype(ld_dtype), 1.0
    qmax = float(np.iinfo(ld_dtype).max)
    return lb, ip, np.round(u * qmax).astype(ld_dtype), 1.0 / qmax


def measure(plan, host_arrays, order, dq, calls, block_start, name, rows, host_cols=1):
    m = plan.m
    for _ in range(3):
        plan.ld_scores(None, None, dq_scale=dq)
    t_score = []
    for _ in range(calls):
        plan.ld_scores(None, None, dq_scale=dq)
        t_score.append(plan.last_ld_score_ms())
    for r2 in R2_RUNS:
        got = plan.clump(order, r2, dq_scale=dq)
        t = []
        for _ in range(calls):
            got = plan.clump(order, r2, dq_scale=dq)
            t.append(plan.last_clump_ms())
        steps = np.add.reduceat((got == np.arange(m, dtype=np.int32)[:, None]).any(axis=1).astype(np.int64), block_start[:-1])
        b = int(np.argmax(steps))
        row = dict(name, n_cols=len(r2), m=int(m), order=int(order.shape[0]),
                   clump_ms=round(float(np.median(t)), 4), clump_ms_min=round(float(np.min(t)), 4),
                   clump_ms_max=round(float(np.max(t)), 4), score_ms=round(float(np.median(t_score)), 4),
                   steps_max=int(steps[b]), steps_max_block_size=int(block_start[b + 1] - block_start[b]),
                   steps_total=int(steps.sum()), index_snps=[int(v) for v in (got == np.arange(m)[:, None]).sum(axis=0)],
                   ns_per_step=round(float(np.median(t)) * 1e6 / max(int(steps[b]), 1), 1))
        if host_arrays is not None and len(r2) <= host_cols:
            lb, ip, data = host_arrays
            t0 = time.perf_counter()
            want = clump_host(lb, ip, data, True, order, r2, None, dq)
            row["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            row["equals_host"] = bool(np.array_equal(got, want))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--ld-dtypes", default="float32,int8")
    ap.add_argument("--band-snps", type=int, default=100_000)
    ap.add_argument("--no-host", action="store_true", help="skip clump_host (cfg3: the LD is then never built on the host)")
    ap.add_argument("--host-cols", type=int, default=1)
    ap.add_argument("--no-band", action="store_true")
    args = ap.parse_args()
    if L.device_count() < 1:
        raise SystemExit("clump_bench: no HIP device visible")
    sizes = syn.block_sizes(args.config)
    rows = []
    for ld_name in args.ld_dtypes.split(","):
        dt = np.dtype(ld_name)
        skel = syn.make_ld(sizes, low_memory=True, ld_dtype=dt, kind="longrange", data=False)
        ss = syn.make_sumstats(skel)
        chisq = np.asarray(ss.n_per_snp, dtype=np.float64) * np.asarray(ss.std_beta, dtype=np.float64) ** 2
        order = clump_order(chisq)
        host = None
        if not args.no_host:
            full = syn.make_ld(sizes, low_memory=True, ld_dtype=dt, kind="longrange")
            host = (full.ld_left_bound, full.ld_indptr, full.ld_data)
        plan = LDPlan.synthetic(skel)
        measure(plan, host, order, skel.dq_scale, args.calls, skel.block_start, {"workload": args.config, "ld": ld_name}, rows,
                args.host_cols)
        plan.close()
        del host
        if args.no_band:
            continue
        lb, ip, data, dq = band_arrays(args.band_snps, 250, dt)
        rng = np.random.default_rng(7)
        chisq = rng.chisquare(1, args.band_snps)
        hot = rng.random(args.band_snps) < 0.02
        chisq[hot] += rng.chisquare(1, int(hot.sum())) * 25.0
        plan = LDPlan(lb, ip, data, True)
        measure(plan, None if args.no_host else (lb, ip, data), clump_order(chisq), dq, args.calls,
                np.array([0, args.band_snps]), {"workload": f"band{args.band_snps}x250", "ld": ld_name}, rows, args.host_cols)
        plan.close()
    print(json.dumps({"tool": "clump_bench", "config": args.config, "calls": args.calls, "rows": rows}))


if __name__ == "__main__":
    main()
