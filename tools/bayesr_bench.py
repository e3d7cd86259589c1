#!/usr/bin/env python3
"""Time the SBayesR sweep (`viprs_state_bayesr_sweep`) next to the mixture E-step sweep and the LDpred2 Gibbs sweep of the same
plan, its draws kernel, its sums call, and `SBayesR.fit()` per iteration (development tool; one JSON line, also written to
--out).

    python tools/bayesr_bench.py [--config cfg3] [--ld-dtypes float32,int8,int16] [--rounds 6] [--per-round 5] [--no-fit]

Per LD dtype: the workload in the upper form, "longrange" LD generated on the device, ONE plan and on it: a mixture state of
K = 4 swept by the E-step (`e_step`: the lane-parallel chain of the panel sweep), a mixture state of K = 3 prepared for
SBayesR's defaults (pi = 0.95, 0.02, 0.02, 0.01; gamma = 0.01, 0.1, 1; h2 = 0.2) swept by `bayesr_sweep`, and a grid state of
width 1 prepared for LDpred2's (p, h2) = (0.5, 0.2) swept by `gibbs_sweep`.  Every timed sweep starts from eta = q = 0.  After
a warm-up the kinds alternate, `--per-round` sweeps each, for `--rounds` rounds in ONE process; sweep times are the plan's own
HIP events (`viprs_plan_last_kernel_ms`, which = 0: the draws kernels are outside them), the draws kernel's is
`viprs_plan_last_bayesr_draws_ms`, the sums call is host wall time around `bayesr_sums` (two launches, one synchronisation).
Reported per kind: median, min and max in ms; the ratios of the SBayesR median to the two others.

`fit`: `SBayesR` with 20 + 10 iterations, one chain (int8 LD unless --fit-ld says otherwise), twice: on the plan of the sweeps
(n = 1e5 samples for 1.1 M SNPs: more SNPs than samples, where the sampler as specified diverges -- DESIGN.md 6.14 -- and
the run records how far it got) and on the same LD with summary statistics of `--fit-n` samples (default 1e7: fewer SNPs than
samples), where the chain runs to the end and the wall time per iteration is taken.  The model is put on the
device-generated plan directly (`SBayesR.from_plan`; no LD on the host).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viprs_amd.utils import synthetic as syn             # noqa: E402

H2 = 0.2


def stats(t):
    t = np.asarray(t, dtype=np.float64)
    return dict(median_ms=round(float(np.median(t)), 4), min_ms=round(float(t.min()), 4), max_ms=round(float(t.max()), 4),
                n=int(t.shape[0]))


def sweep_times(plan, skel, ss, inp, rounds, per_round):
    from viprs_amd.plan import DeviceState
    from viprs_amd.stats import bayesr as B
    from viprs_amd.stats.gibbs import gibbs_prep_rows
    m, dq = plan.m, skel.dq_scale
    mix = DeviceState(plan, "float32", model="mixture", width=4, placement="off")
    fields = syn.make_mixture_inputs(ss, 4, float_precision=np.float32)
    pi0 = fields.pop("pi")
    for k, a in dict(fields, std_beta=inp.std_beta).items():
        mix.upload(k, a)
    br = DeviceState(plan, "float32", model="mixture", width=3, placement="off")
    br.upload("std_beta", inp.std_beta)
    br.set_n_per_snp(ss.n_per_snp)
    br.prep_mixture(*B.bayesr_prep_args(B.DEFAULT_PI, B.DEFAULT_GAMMA,
                                        B.initial_sigma2_beta(H2, m, B.DEFAULT_PI, B.DEFAULT_GAMMA), 1.0 - H2))
    gb = DeviceState(plan, "float32", model="grid", width=1, placement="off")
    gb.upload("std_beta", inp.std_beta)
    gb.set_n_per_snp(ss.n_per_snp)
    gb.prep_columns(gibbs_prep_rows(np.arange(1), m, [0.5], [H2]))
    count = {"i": 0}

    def bayesr():
        count["i"] += 1
        br.bayesr_sweep(dq, seed=1, draw_index=count["i"])

    def gibbs():
        count["i"] += 1
        gb.gibbs_sweep(dq, seed=1, draw_index=count["i"])
    kinds = {"mixture_e_step_K4": (mix, lambda: mix.e_step(dq), pi0), "bayesr_K3": (br, bayesr, 0.0),
             "gibbs_width1": (gb, gibbs, inp.pi)}
    times = {k: [] for k in kinds}
    draws, sums = [], []

    def run(name, n, keep):
        st, fn, pi = kinds[name]
        for _ in range(n):
            st.reset(pi)
            fn()
            if keep:
                times[name].append(plan.last_kernel_ms(0))
                if name == "bayesr_K3":
                    draws.append(plan.last_bayesr_draws_ms())
                    t0 = time.perf_counter()
                    st.bayesr_sums()
                    sums.append(1e3 * (time.perf_counter() - t0))
    for name in kinds:                                       # warm-up: code objects, clocks
        run(name, 10, False)
    br.bayesr_sums()
    for _ in range(rounds):
        for name in kinds:
            run(name, per_round, True)
    counts = [float(v) / m for v in br.bayesr_sums()[:4]]
    for st in (mix, br, gb):
        st.close()
    out = {k: stats(v) for k, v in times.items()}
    b = out["bayesr_K3"]
    b["draws_kernel"] = stats(draws)
    b["sums_call_wall"] = stats(sums)
    b["ratio_to_mixture_e_step_K4"] = round(b["median_ms"] / out["mixture_e_step_K4"]["median_ms"], 4)
    b["ratio_to_gibbs_width1"] = round(b["median_ms"] / out["gibbs_width1"]["median_ms"], 4)
    out["share_of_kstar_after_one_sweep"] = counts
    return out


def fit_on_plan(plan, skel, ss, std_beta, n_iter=30, n_burnin=20):
    """`SBayesR.fit()` on a plan that exists on the device only (`SBayesR.from_plan`).  The time per iteration is wall time over
    the sweeps the chain RAN, and is reported only for a chain that ran to the end."""
    from viprs_amd.model import SBayesR
    model = SBayesR.from_plan(plan, std_beta, ss.n_per_snp, skel.dq_scale, H2, n_iter=n_iter, n_burnin=n_burnin, seed=1)
    t0 = time.perf_counter()
    model.fit()
    wall = time.perf_counter() - t0
    done, diverged = int(model.n_sweeps[0]), bool(model.diverged[0])
    num = lambda v: float(v) if np.isfinite(v) else None          # (a diverged chain has no estimates: null, not NaN)
    return dict(iterations_requested=n_iter, iterations_completed=done, diverged=diverged, wall_s=round(wall, 3),
                wall_ms_per_iteration=None if diverged or done < n_iter else round(1e3 * wall / done, 3),
                h2_est=num(model.h2_est[0]), pi_est=[num(v) for v in model.pi_est[0]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--ld-dtypes", default="float32,int8,int16")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--per-round", type=int, default=5)
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--fit-ld", default="int8")
    ap.add_argument("--fit-n", type=float, default=1e7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from viprs_amd import _lib as L
    from viprs_amd.plan import LDPlan
    if L.device_count() < 1:
        raise SystemExit("bayesr_bench: no HIP device visible")
    result = {"tool": "bayesr_bench", "config": args.config, "sweeps": {}}
    sizes = syn.block_sizes(args.config)
    for ld_name in dict.fromkeys(args.ld_dtypes.split(",") + ([] if args.no_fit else [args.fit_ld])):
        skel = syn.make_ld(sizes, low_memory=True, ld_dtype=np.dtype(ld_name), kind="longrange", data=False)
        ss = syn.make_sumstats(skel)
        inp = syn.make_inputs(ss)
        plan = LDPlan.synthetic(skel)
        if ld_name in args.ld_dtypes.split(","):
            result["sweeps"][ld_name] = sweep_times(plan, skel, ss, inp, args.rounds, args.per_round)
            print(json.dumps({ld_name: result["sweeps"][ld_name]}), file=sys.stderr, flush=True)
        if not args.no_fit and ld_name == args.fit_ld:
            result["fit_more_snps_than_samples"] = dict(ld=ld_name, m=int(plan.m), n=float(np.mean(ss.n_per_snp)),
                                                        **fit_on_plan(plan, skel, ss, inp.std_beta))
            big = syn.make_sumstats(skel, n=args.fit_n)
            result["fit"] = dict(ld=ld_name, m=int(plan.m), n=float(np.mean(big.n_per_snp)),
                                 **fit_on_plan(plan, skel, big, syn.make_inputs(big).std_beta))
            for k in ("fit_more_snps_than_samples", "fit"):
                print(json.dumps({k: result[k]}), file=sys.stderr, flush=True)
        plan.close()
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
