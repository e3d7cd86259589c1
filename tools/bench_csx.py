#!/usr/bin/env python3
"""Time the coupled update of PRS-CSx (`viprs_csx_update`) next to the Gibbs sweeps of its populations and next to the PRS-CS
update of the same sizes (development tool; one JSON line, also written to --out, default profiles/csx_bench.json).

    python tools/bench_csx.py [--config cfg3] [--ld-dtype float32] [--widths 1,5] [--overlaps 1.0,0.5] [--rounds 4] [--per-round 5]

The workload in the upper form, "longrange" LD generated on the device, TWO plans of it (two populations, two streams; the
second population's marginal effects perturbed and its sample a tenth) and per (overlap, width) two grid states under one
`DeviceCoupling`: overlap 1.0 is one SNP set, 0.5 shifts the second population by m / 2 union rows (m_union = 1.5 m, a third of
the union carried by both).  The iteration is the model's, with sigma2 = 1 and phi = 0.01 held fixed: one Gibbs sweep and the
two sums calls per population, the union's sums, one coupled update.  Beside it a third state on the first plan runs
`viprs_state_cs_update` (variates kernel + update kernel) on the same m x width: the parent's cost of the same step.  After a
warm-up of 6 iterations, `--rounds` x `--per-round` iterations per case, the cases alternating by round.  Sweeps, the
PRS-CS kernels and the coupled update are timed by their HIP events.  Reported per case: median, min, max in ms; the
coupled update per (union SNP, chain) in ns next to variates + update per (SNP, chain); its ratio to ONE population's sweep;
the mean attempt count of the draws with two carrying populations and the draws that ended at the attempt cap.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viprs_amd.utils import synthetic as syn             # noqa: E402


def stats(t):
    t = np.asarray(t, dtype=np.float64)
    return dict(median_ms=round(float(np.median(t)), 4), min_ms=round(float(t.min()), 4), max_ms=round(float(t.max()), 4),
                n=int(t.shape[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--ld-dtype", default="float32")
    ap.add_argument("--widths", default="1,5")
    ap.add_argument("--overlaps", default="1.0,0.5")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--per-round", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "csx_bench.json"))
    args = ap.parse_args()
    from viprs_amd import _lib as L
    from viprs_amd.plan import DeviceCoupling, DeviceState, LDPlan
    if L.device_count() < 1:
        raise SystemExit("bench_csx: no HIP device visible")
    widths = [int(w) for w in args.widths.split(",")]
    overlaps = [float(x) for x in args.overlaps.split(",")]
    skel = syn.make_ld(syn.block_sizes(args.config), low_memory=True, ld_dtype=np.dtype(args.ld_dtype), kind="longrange", data=False)
    ss = syn.make_sumstats(skel)
    inp = syn.make_inputs(ss)
    plans = [LDPlan.synthetic(skel), LDPlan.synthetic(skel)]
    m, dq = plans[0].m, skel.dq_scale
    rng = np.random.default_rng(1)
    betas = [inp.std_beta, (inp.std_beta + rng.standard_normal(m) * np.sqrt(10.0 / ss.n)).astype(np.float32)]
    ns = [np.asarray(ss.n_per_snp, dtype=np.float64), 0.1 * np.asarray(ss.n_per_snp, dtype=np.float64)]
    cases, it = {}, {}
    for ov in overlaps:
        shift = int(round((1.0 - ov) * m))
        row_of = np.full((2, m + shift), -1, dtype=np.int64)
        row_of[0, :m] = np.arange(m)
        row_of[1, shift:] = np.arange(m)
        for w in widths:
            states = []
            for k in range(3):                               # two populations, and the PRS-CS state of the comparison
                st = DeviceState(plans[k % 2], "float32", model="grid", width=w, placement="off")
                st.upload("std_beta", betas[k % 2])
                st.set_n_per_snp(ns[k % 2])
                states.append(st)
            cp = DeviceCoupling(states[:2], row_of)
            cp.update(np.array([[g, 0.01, 1.0, 1.0] for g in range(w)]), prepare_only=True)
            states[2].cs_update(np.array([[g, 1.0, 0.01] for g in range(w)]), prepare_only=True)
            cases[(ov, w)] = (states, cp, row_of)
            it[(ov, w)] = 0
    names = ("sweep_0", "sweep_1", "coupled_update", "cs_variates", "cs_update")
    times = {c: {k: [] for k in names} for c in cases}
    capped = {c: 0 for c in cases}

    def iterate(c, n, keep):
        states, cp, _ = cases[c]
        w = c[1]
        par = np.array([[g, 0.01, 1.0, 1.0] for g in range(w)])
        par_cs = np.array([[g, 1.0, 0.01] for g in range(w)])
        for _ in range(n):
            it[c] += 1
            sweeps = []
            for k in range(3):
                states[k].gibbs_sweep(dq, seed=1 + k, draw_index=it[c])
                sweeps.append(plans[k % 2].last_kernel_ms(0))
                states[k].enet_sums()
                states[k].cs_sums()
            cp.sums()
            cp.update(par, seed=1, draw_index=it[c])
            states[2].cs_update(par_cs, seed=1, draw_index=it[c])
            if keep:
                ms, nc = cp.last()
                v, u = plans[0].last_cs_ms()
                capped[c] += nc
                for k, x in zip(names, (sweeps[0], sweeps[1], ms, v, u)):
                    times[c][k].append(x)
    for c in cases:
        iterate(c, 6, False)
    for _ in range(args.rounds):
        for c in cases:
            iterate(c, args.per_round, True)
    result = {"tool": "bench_csx", "config": args.config, "ld_dtype": args.ld_dtype, "m": int(m), "populations": 2, "cases": {}}
    for c, (states, cp, row_of) in cases.items():
        ov, w = c
        out = {k: stats(v) for k, v in times[c].items()}
        mu = row_of.shape[1]
        both = (row_of >= 0).all(axis=0)
        att = cp.download("attempts")
        sweep = 0.5 * (out["sweep_0"]["median_ms"] + out["sweep_1"]["median_ms"])
        cs = out["cs_variates"]["median_ms"] + out["cs_update"]["median_ms"]
        out.update(m_union=int(mu), carried_by_both=int(both.sum()),
                   coupled_ns_per_snp_chain=round(1e6 * out["coupled_update"]["median_ms"] / (mu * w), 4),
                   cs_variates_plus_update_ns_per_snp_chain=round(1e6 * cs / (m * w), 4),
                   coupled_over_cs_variates_plus_update=round(out["coupled_update"]["median_ms"] / cs, 3),
                   coupled_over_one_sweep=round(out["coupled_update"]["median_ms"] / sweep, 4),
                   mean_attempts=round(float(att[both].mean()), 4), longest_run=int(att.max()), n_capped=int(capped[c]),
                   psi_median=float(np.median(cp.download("psi"))))
        result["cases"][f"overlap{ov:g}_width{w}"] = out
        cp.close()
        for st in states:
            st.close()
    for p in plans:
        p.close()
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
