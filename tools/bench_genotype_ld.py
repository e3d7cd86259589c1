#!/usr/bin/env python3
"""Time the LD from genotypes (`viprs_genotypes_ld`, viprs_amd/csrc/geno_ld.h) on the shapes EXPERIMENTS.md records
(development tool; one JSON line).

    python tools/bench_genotype_ld.py [--cases windowed_clean,windowed_missing,dense_clean] [--calls 5] [--host-rows 2048]

Cases (random genotypes; the time does not depend on their values):
  windowed_clean    19 000 SNPs (the benchmark's chr22-like size) x 10 000 samples, a 1 000-SNP window, no missing code
  windowed_missing  the same with 1 % missing: every tile has a missing code, so every pair runs the general instantiation
  dense_clean       one dense block of 13 000 SNPs x 10 000 samples
Every case runs in a child process of its own under a time limit (`--limit` seconds); after a case that fails or runs out
of time nothing more is started.  Per case: `ld_ms` = median over `--calls` calls of the kernels' own HIP events
(`last_ld_ms`: no upload, no download), after one warm-up call; the element type is float32.
`host_s`: `ld_host` on the first `--host-rows` SNPs as a problem of its own under the same estimator (checked `==` against the
device on that problem), and `host_s_scaled` = that time x (entries of the case's store / entries of that problem): the whole
matrix on the host takes minutes (0: skip).
The time model: matrix-core issue time of (tile pairs x quarters x k-steps x products) v_mfma_i32_32x32x32_i8 at the device's
dense int8 rate (2 x the bf16 rate: 5.0e15 op/s, 65 536 op per instruction) plus the HBM time of the packed rows and of the
store at 8 TB/s.  `frac_model` = model / measured."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INT8_OPS = 5.0e15
HBM = 8.0e12
TILE = 64
CASES = {"windowed_clean": (19000, 10000, 1000, 0.0), "windowed_missing": (19000, 10000, 1000, 0.01),
         "dense_clean": (13000, 10000, None, 0.0)}


def make_rows(m, n, missing, seed=1):
    from viprs_amd.io.plink_bed import pack_codes
    rng = np.random.default_rng(seed)
    out = []
    for a in range(0, m, 1000):                          # in slabs: the unpacked codes of all SNPs are not needed at once
        k = min(1000, m - a)
        codes = np.array([3, 2, 0], dtype=np.uint8)[rng.integers(0, 3, size=(k, n))]
        if missing:
            codes[rng.random((k, n)) < missing] = 1
        out.append(pack_codes(codes))
    return np.concatenate(out)


def model_ms(m, n, right_end, clean, elem):
    """(mfma_ms, hbm_ms): the kernels' own tile pairs, quarters and k-steps (a pass of the K loop is 128 samples)."""
    stride = ((n + 3) // 4 + 15) // 16 * 16
    ksteps = ((stride // 16 + 1) // 2) * 4
    pairs = 0
    for I in range((m + TILE - 1) // TILE):
        last = min((I + 1) * TILE, m) - 1
        pairs += (int(right_end[last]) - 1) // TILE - I + 1
    mfma = pairs * 4 * ksteps * (1 if clean else 4)
    nnz = int(np.sum(right_end - np.arange(1, m + 1)))
    return mfma * 65536 / INT8_OPS * 1e3, (m * stride + nnz * elem) / HBM * 1e3, pairs


def run_case(name, calls, host_rows):
    from viprs_amd import _lib as L
    from viprs_amd import genotypes as G
    if L.device_count() < 1:
        raise SystemExit("bench_genotype_ld: no HIP device visible")
    m, n, window, missing = CASES[name]
    rows = make_rows(m, n, missing)
    re = G.ld_windows(("sample",) if window is None else ("windowed", window), m)
    ip = G.ld_indptr(re)
    g = G.DeviceGenotypes(rows, n)
    w = G.ld_stats(g.counts())[2]
    clean = bool(np.all(g.counts()[:, 1] == 0))
    out = np.zeros(int(ip[-1]), dtype=np.float32)
    g.ld_rows(0, m, re, w, out)
    times = []
    for _ in range(calls):
        g.ld_rows(0, m, re, w, out)
        times.append(g.last_ld_ms())
    res = {"case": name, "m": m, "n": n, "window": window, "missing": missing, "clean": clean, "nnz": int(ip[-1]),
           "ld_ms": round(float(np.median(times)), 3), "ld_ms_min": round(float(np.min(times)), 3),
           "ld_ms_max": round(float(np.max(times)), 3)}
    mfma_ms, hbm_ms, pairs = model_ms(m, n, re, clean, 4)
    res.update(tile_pairs=pairs, model_mfma_ms=round(mfma_ms, 3), model_hbm_ms=round(hbm_ms, 3),
               frac_model=round((mfma_ms + hbm_ms) / res["ld_ms"], 3))
    if host_rows > 0:
        # the first k SNPs as a problem of its own under the same estimator, on the host and on the device
        k = min(host_rows, m)
        sub = np.minimum(re[:k], k)
        t0 = time.perf_counter()
        hip_, hdata = G.ld_host(rows[:k], n, sub, np.float32)
        host_s = time.perf_counter() - t0
        g2 = G.DeviceGenotypes(rows[:k], n)
        assert np.array_equal(g2.ld(sub, dtype=np.float32)[1], hdata), "the device differs from ld_host"
        g2.close()
        res.update(host_rows=k, host_s=round(host_s, 3), host_s_scaled=round(host_s * float(ip[-1]) / float(hip_[-1]), 2),
                   host_equal=True)
    g.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--host-rows", type=int, default=2048)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds a case may take")
    ap.add_argument("--case", default=None, help="(internal) run this case in this process")
    args = ap.parse_args()
    if args.case:
        return run_case(args.case, args.calls, args.host_rows)
    rows = []
    for name in args.cases.split(","):
        if name not in CASES:
            raise SystemExit(f"bench_genotype_ld: unknown case {name!r}: {', '.join(CASES)}")
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--calls", str(args.calls),
               "--host-rows", str(args.host_rows)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"bench_genotype_ld: case {name} ran out of its {args.limit:.0f} s: nothing more is started")
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            raise SystemExit(f"bench_genotype_ld: case {name} ended with status {p.returncode}: nothing more is started")
        rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    by = {r["case"]: r for r in rows}
    ratio = None
    if "windowed_clean" in by and "windowed_missing" in by:
        ratio = round(by["windowed_missing"]["ld_ms"] / by["windowed_clean"]["ld_ms"], 3)
    print(json.dumps({"tool": "bench_genotype_ld", "calls": args.calls, "general_over_clean": ratio, "rows": rows}))


if __name__ == "__main__":
    main()
