#!/usr/bin/env python3
"""Time the PRS-CS calls (`viprs_state_cs_variates` / `_update` / `_sums`) next to the Gibbs sweep of the same state and
process (development tool; one JSON line, also written to --out, default profiles/cs_bench.json).

    python tools/bench_cs.py [--config cfg3] [--ld-dtype float32] [--widths 1,5] [--rounds 6] [--per-round 5]

The workload in the upper form, "longrange" LD generated on the device, ONE plan, and per width a grid state that runs the
PRS-CS iteration with sigma2 = 1 and phi = 0.01 held fixed: Gibbs sweep, the two sums calls, update (variates kernel, then
update kernel).  After a warm-up of 10 iterations, `--rounds` x `--per-round` iterations per width, the widths alternating
by round.  The sweep is timed by the plan's HIP events (`viprs_plan_last_kernel_ms`, which = 0), the variates and the update
kernel by theirs (`viprs_plan_last_cs_ms`); the sums call is synchronous and has no event pair of its own: its figure is
the host's wall time around the call (two kernels, the copy of 4 doubles per column and the synchronisation), on an idle
stream.  Reported per width: median, min, max in ms; the ratios of the medians to the sweep's; and the ratio of variates +
update to the stream model of the request -- 60 bytes per (SNP, column) at 6.3 TB/s.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viprs_amd.utils import synthetic as syn             # noqa: E402

STREAM_BYTES, STREAM_TBS = 60.0, 6.3


def stats(t):
    t = np.asarray(t, dtype=np.float64)
    return dict(median_ms=round(float(np.median(t)), 4), min_ms=round(float(t.min()), 4), max_ms=round(float(t.max()), 4),
                n=int(t.shape[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--ld-dtype", default="float32")
    ap.add_argument("--widths", default="1,5")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--per-round", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "cs_bench.json"))
    args = ap.parse_args()
    from viprs_amd import _lib as L
    from viprs_amd.plan import DeviceState, LDPlan
    if L.device_count() < 1:
        raise SystemExit("bench_cs: no HIP device visible")
    widths = [int(w) for w in args.widths.split(",")]
    skel = syn.make_ld(syn.block_sizes(args.config), low_memory=True, ld_dtype=np.dtype(args.ld_dtype), kind="longrange", data=False)
    ss = syn.make_sumstats(skel)
    inp = syn.make_inputs(ss)
    plan = LDPlan.synthetic(skel)
    m, dq = plan.m, skel.dq_scale
    states, it = {}, {w: 0 for w in widths}
    for w in widths:
        st = DeviceState(plan, "float32", model="grid", width=w, placement="off")
        st.upload("std_beta", inp.std_beta)
        st.set_n_per_snp(ss.n_per_snp)
        st.cs_update(np.array([[g, 1.0, 0.01] for g in range(w)]), prepare_only=True)
        states[w] = st
    times = {w: {k: [] for k in ("sweep", "variates", "update", "sums_wall")} for w in widths}

    def iterate(w, n, keep):
        st = states[w]
        params = np.array([[g, 1.0, 0.01] for g in range(w)])
        for _ in range(n):
            it[w] += 1
            st.gibbs_sweep(dq, seed=1, draw_index=it[w])
            st.enet_sums()
            t0 = time.perf_counter()
            st.cs_sums()
            wall = 1e3 * (time.perf_counter() - t0)
            st.cs_update(params, seed=1, draw_index=it[w])
            if keep:
                v, u = plan.last_cs_ms()
                for k, x in (("sweep", plan.last_kernel_ms(0)), ("variates", v), ("update", u), ("sums_wall", wall)):
                    times[w][k].append(x)
    for w in widths:
        iterate(w, 10, False)
    for _ in range(args.rounds):
        for w in widths:
            iterate(w, args.per_round, True)
    result = {"tool": "bench_cs", "config": args.config, "ld_dtype": args.ld_dtype, "m": int(m), "widths": {}}
    for w in widths:
        out = {k: stats(v) for k, v in times[w].items()}
        sweep = out["sweep"]["median_ms"]
        both = out["variates"]["median_ms"] + out["update"]["median_ms"]
        model = 1e3 * STREAM_BYTES * m * w / (STREAM_TBS * 1e12)
        out["update_over_sweep"] = round(out["update"]["median_ms"] / sweep, 4)
        out["variates_over_sweep"] = round(out["variates"]["median_ms"] / sweep, 4)
        out["variates_plus_update_over_sweep"] = round(both / sweep, 4)
        out["sums_wall_over_sweep"] = round(out["sums_wall"]["median_ms"] / sweep, 4)
        out["stream_model_ms"] = round(model, 4)
        out["variates_plus_update_over_stream_model"] = round(both / model, 3)
        psi = states[w].cs_download("psi")
        out["psi_at_the_cap"] = round(float(np.mean(psi == 1.0)), 4)
        out["psi_median"] = float(np.median(psi))
        result["widths"][str(w)] = out
        states[w].close()
    plan.close()
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
