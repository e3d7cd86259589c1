#!/usr/bin/env python3
"""Time the elastic-net sweep (`viprs_state_enet_sweep`) next to the spike-and-slab E-step sweep of the same plan, and a
whole `Lassosum.fit()` (development tool; one JSON line, also written to --out).

    python tools/enet_bench.py [--config cfg3] [--ld-dtypes float32,int8] [--rounds 6] [--per-round 5] [--no-fit] [--host-only]

Per LD dtype: the workload in the upper form, "longrange" LD generated on the device, one plan, three states on it -- a
spike-and-slab state with the inputs of `make_inputs`, an elastic-net state of width 1 and an elastic-net grid state of 3
columns ((s, lambda) = (0.2, 0.005), (0.5, 0.002), (0.9, 0.005)).  Every timed sweep starts from the standard start
(`reset`: eta = q = 0), so every LD entry is streamed -- a sweep near a fixed point skips the strips whose panel has no
change to apply and says nothing about the stream.  After a warm-up the three kinds alternate, `--per-round` sweeps each,
for `--rounds` rounds in ONE process; all times are the plan's own HIP events (`viprs_plan_last_kernel_ms`, which = 0).
Reported per kind: median, min and max in ms; per dtype the ratios of the medians to the spike-and-slab median and the
spike-and-slab sweeps' own (max - min) / median.

`fit`: `Lassosum.fit()` with the default 4 x 20 grid on the same plan (int8 LD unless --fit-ld says otherwise): wall time,
sweeps per lambda and column, total sweeps.  The model is put on the device-generated plan directly (`Lassosum.from_plan`; no
LD on the host).
`host`: the C replay of the sweep (tests/enet_replay.c, one core) on --host-config (cfg2: 19 k SNPs), ms per sweep.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viprs_amd.utils import synthetic as syn             # noqa: E402

GRID = ((0.2, 0.005), (0.5, 0.002), (0.9, 0.005))


def stats(t):
    t = np.asarray(t, dtype=np.float64)
    return dict(median_ms=round(float(np.median(t)), 4), min_ms=round(float(t.min()), 4), max_ms=round(float(t.max()), 4),
                n=int(t.shape[0]))


def host_baseline(config, sweeps=3):
    from tests import enet_replay as ER
    ld, ss, inp = syn.make_problem(config, low_memory=True, kind="longrange")
    m = ld.m
    mult, pen = np.full(m, np.float32(0.5)), np.full(m, np.float32(0.002))
    eta, q = np.zeros(m, dtype=np.float32), np.zeros(m, dtype=np.float32)
    ER.replay_sweep(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, True, inp.std_beta, mult, pen, eta.copy(), q.copy(), 1.0)
    t = []
    for _ in range(sweeps):
        t0 = time.perf_counter()
        ER.replay_sweep(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, True, inp.std_beta, mult, pen, eta, q, 1.0)
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(config=config, m=int(m), nnz=int(ld.nnz), ld="float32", form="upper", cores=1, **stats(t))


def sweep_times(plan, skel, inp, rounds, per_round):
    from viprs_amd.plan import DeviceState
    m, dq = plan.m, skel.dq_scale
    f32 = np.float32
    ss = DeviceState(plan, "float32", placement="off")
    for k in ("std_beta", "u_logs", "sqrt_half_var_tau", "mu_mult"):
        ss.upload(k, getattr(inp, k))
    e1 = DeviceState(plan, "float32", placement="off")
    e1.upload("std_beta", inp.std_beta)
    e1.upload("mu_mult", np.full(m, f32(0.5)))
    e1.upload("sqrt_half_var_tau", np.full(m, f32(0.002)))
    e3 = DeviceState(plan, "float32", model="grid", width=3, placement="off")
    e3.upload("std_beta", inp.std_beta)
    e3.upload("mu_mult", np.asfortranarray(np.repeat(np.array([[1.0 - s for s, _ in GRID]], dtype=f32), m, axis=0)))
    e3.upload("half_var_tau", np.asfortranarray(np.repeat(np.array([[lam for _, lam in GRID]], dtype=f32), m, axis=0)))
    kinds = {"spike_slab": (ss, lambda: ss.e_step(dq)), "enet_width1": (e1, lambda: e1.enet_sweep(dq)),
             "enet_grid3": (e3, lambda: e3.enet_sweep(dq))}
    times = {k: [] for k in kinds}
    nonzero = {}

    def run(name, n, keep):
        st, fn = kinds[name]
        for _ in range(n):
            st.reset(inp.pi)
            fn()
            if keep:
                times[name].append(plan.last_kernel_ms(0))
    for name in kinds:                                       # warm-up: code objects, clocks
        run(name, 10, False)
    for _ in range(rounds):
        for name in kinds:
            run(name, per_round, True)
    nonzero["enet_width1"] = float(np.count_nonzero(e1.download("eta")) / m)
    nonzero["enet_grid3"] = [float(v) for v in np.count_nonzero(e3.download("eta"), axis=0) / m]
    for st, _ in kinds.values():
        st.close()
    out = {k: stats(v) for k, v in times.items()}
    base = out["spike_slab"]
    out["spike_slab_spread"] = round((base["max_ms"] - base["min_ms"]) / base["median_ms"], 4)
    for k in ("enet_width1", "enet_grid3"):
        out[k]["ratio_to_spike_slab"] = round(out[k]["median_ms"] / base["median_ms"], 4)
    out["eta_nonzero_after_one_sweep"] = nonzero
    return out


def fit_on_plan(plan, skel, std_beta):
    """`Lassosum.fit()` with the default grid on a plan that exists on the device only."""
    from viprs_amd.model import Lassosum
    model = Lassosum.from_plan(plan, std_beta, skel.dq_scale)
    t0 = time.perf_counter()
    model.fit()
    wall = time.perf_counter() - t0
    t = model.grid_table
    return dict(wall_s=round(wall, 3), total_sweeps_lockstep=int(t[t["s"] < 1].groupby("lambda")["n_sweeps"].max().sum()),
                sweeps_per_lambda={str(s): [int(v) for v in t[t["s"] == s]["n_sweeps"]] for s in (0.2, 0.5, 0.9)},
                converged=int(t["converged"].sum()), diverged=int(t["diverged"].sum()),
                n_nonzero_last_lambda={str(s): int(t[t["s"] == s]["n_nonzero"].iloc[-1]) for s in (0.2, 0.5, 0.9, 1.0)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--ld-dtypes", default="float32,int8")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--per-round", type=int, default=5)
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--fit-ld", default="int8")
    ap.add_argument("--host-config", default="cfg2")
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = {"tool": "enet_bench", "config": args.config}
    if not args.no_host:
        result["host"] = host_baseline(args.host_config)
        print(json.dumps(result["host"]), file=sys.stderr, flush=True)
    if not args.host_only:
        from viprs_amd import _lib as L
        from viprs_amd.plan import LDPlan
        if L.device_count() < 1:
            raise SystemExit("enet_bench: no HIP device visible")
        sizes = syn.block_sizes(args.config)
        result["sweeps"] = {}
        for ld_name in dict.fromkeys(args.ld_dtypes.split(",") + ([] if args.no_fit else [args.fit_ld])):
            skel = syn.make_ld(sizes, low_memory=True, ld_dtype=np.dtype(ld_name), kind="longrange", data=False)
            inp = syn.make_inputs(syn.make_sumstats(skel))
            plan = LDPlan.synthetic(skel)
            if ld_name in args.ld_dtypes.split(","):
                result["sweeps"][ld_name] = sweep_times(plan, skel, inp, args.rounds, args.per_round)
                print(json.dumps({ld_name: result["sweeps"][ld_name]}), file=sys.stderr, flush=True)
            if not args.no_fit and ld_name == args.fit_ld:
                result["fit"] = dict(ld=ld_name, m=int(plan.m), **fit_on_plan(plan, skel, inp.std_beta))
                print(json.dumps(result["fit"]), file=sys.stderr, flush=True)
            plan.close()
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
