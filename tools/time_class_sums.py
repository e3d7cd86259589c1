#!/usr/bin/env python3
"""Time the per-genotype-class column sums (`viprs_genotypes_class_sums`, viprs_amd/csrc/geno_class_sums.h) on the shapes
EXPERIMENTS.md records (development tool; one JSON line per case).

    python tools/time_class_sums.py [--samples 10000,500] [--snps 200000] [--cols 1,3,32] [--calls 5] [--host-rows 2048]

Random packed rows (the time does not depend on their values).  Per (samples, columns): `ms` = median over `--calls` calls of
the kernels' own HIP events (`last_class_sums_ms`: no upload, no download) after one warm-up call, all SNPs in one row range;
`terms_per_s` = samples x SNPs x columns / time.  Two models, `frac_*` = model / measured:
  bytes   the genotype rows once per column group plus the device copy of Y once per group of R rows, at the 6.3 TB/s copy
          rate (Y stays in L2: the figure is a floor on traffic, not a claim that it comes from HBM)
  valu    vector-ALU issue: the kernel's own instructions per (sample, row, column) term, counted from the ISA of the W = 4
          instantiation's loop (3 v_add_f64 + 6 v_cndmask_b32 + 0.8 v_cmp / s_and per term), x terms / the
          device's issue rate of 256 CUs x 4 SIMDs x 2.4 GHz / 4 cycles per wave64 instruction x 64 lanes
`host_s_scaled`: `class_sums_host` on the first `--host-rows` SNPs x (SNPs / those rows), checked against the device within
the header's bound; `score_ms`: the 1-column float64 score of the same shape through `last_score_ms` (the same number of
terms), for comparison only.  Every case runs in a child process under a time limit; after one that fails nothing more is
started."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.3e12
VALU_LANE_OPS = 256 * 4 * 2.4e9 / 4 * 64          # lane-instructions per second
VALU_PER_TERM = 9.8
ROWS, COLS = 4, 4                                 # R and W of the kernel


def make_rows(m, n, seed=1):
    """Random bytes: the four codes in equal shares (a quarter missing; the kernel does the same work for every code)."""
    return np.random.default_rng(seed).integers(0, 256, size=(m, (n + 3) // 4), dtype=np.uint8)


def n_groups(n_cols):
    g, left = 0, n_cols
    for w in (4, 2, 1):
        g += left // w
        left %= w
    return g


def run_case(n, m, n_cols, calls, host_rows):
    from viprs_amd import _lib as L
    from viprs_amd import genotypes as G
    if L.device_count() < 1:
        raise SystemExit("time_class_sums: no HIP device visible")
    rows = make_rows(m, n)
    rng = np.random.default_rng(2)
    Y = rng.standard_normal((n, n_cols))
    g = G.DeviceGenotypes(rows, n)
    budget = m * 3 * n_cols * 8                    # one row range
    out = g.class_sums(Y, max_bytes=budget)
    times = []
    for _ in range(calls):
        g.class_sums(Y, max_bytes=budget)
        times.append(g.last_class_sums_ms())
    ms = float(np.median(times))
    terms = float(n) * m * n_cols
    stride = ((n + 3) // 4 + 15) // 16 * 16
    y_bytes = -(-stride // 256) * 1024 * 8 * n_cols
    bytes_ms = (m * stride * n_groups(n_cols) + -(-m // ROWS) * y_bytes) / COPY_RATE * 1e3
    valu_ms = VALU_PER_TERM * terms / VALU_LANE_OPS * 1e3
    res = {"tool": "time_class_sums", "n": n, "m": m, "n_cols": n_cols, "calls": calls, "ms": round(ms, 3),
           "ms_min": round(float(np.min(times)), 3), "ms_max": round(float(np.max(times)), 3),
           "terms_per_s": float(f"{terms / ms * 1e3:.4g}"), "model_bytes_ms": round(bytes_ms, 3),
           "model_valu_ms": round(valu_ms, 3), "frac_bytes": round(bytes_ms / ms, 3), "frac_valu": round(valu_ms / ms, 3),
           "bound_by": "valu" if valu_ms > bytes_ms else "bytes"}
    if host_rows > 0:
        k = min(host_rows, m)
        t0 = time.perf_counter()
        host = G.class_sums_host(rows[:k], n, Y)
        host_s = time.perf_counter() - t0
        tol = (16 * -(-n // 1024) + 6) * 2.0 ** -53 * 2.0 * np.abs(Y).sum(axis=0)
        assert np.all(np.abs(host - out[:k]) <= tol), "the device differs from class_sums_host beyond the header's bound"
        res.update(host_rows=k, host_s=round(host_s, 3), host_s_scaled=round(host_s * m / k, 2), host_within_bound=True)
    if n_cols == 1:
        B = rng.standard_normal((m, 1))
        g.score(B, float_precision=np.float64)
        st = []
        for _ in range(calls):
            g.score(B, float_precision=np.float64)
            st.append(g.last_score_ms())
        res["score_ms"] = round(float(np.median(st)), 3)
    g.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="10000,500")
    ap.add_argument("--snps", type=int, default=200000)
    ap.add_argument("--cols", default="1,3,32")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--host-rows", type=int, default=2048)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds a case may take")
    ap.add_argument("--case", default=None, help="(internal) n,n_cols: run this case in this process")
    args = ap.parse_args()
    if args.case:
        n, c = (int(v) for v in args.case.split(","))
        return run_case(n, args.snps, c, args.calls, args.host_rows)
    for n in (int(v) for v in args.samples.split(",")):
        for c in (int(v) for v in args.cols.split(",")):
            cmd = [sys.executable, os.path.abspath(__file__), "--case", f"{n},{c}", "--snps", str(args.snps),
                   "--calls", str(args.calls), "--host-rows", str(args.host_rows)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"time_class_sums: case n={n} n_cols={c} ran out of its {args.limit:.0f} s: nothing more "
                                 "is started")
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-4000:])
                raise SystemExit(f"time_class_sums: case n={n} n_cols={c} ended with status {p.returncode}: nothing more "
                                 "is started")
            print(p.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
