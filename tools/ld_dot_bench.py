#!/usr/bin/env python3
"""Time the LD product (`viprs_state_dot`) on the cfg3 synthetic workload next to the sweep of the same plan
(development tool; one JSON line).

    python tools/ld_dot_bench.py [--config cfg3] [--calls 20] [--sweeps 5]

For {fp32, int8} LD x {upper, symmetric} x n_cols in {1, 32} x {float32, float64}: warm-up, then the mean (and the
median, minimum and maximum) of `last_dot_ms` over `--calls` products through `DeviceState.dot` (B is the resident eta: no
upload inside the bracket) and the mean sweep-kernel time (`plan.timing_history(0)`) of the same state in the same process.  bytes = stored LD bytes of
the device layout + 2 m n_cols sizeof(T); `frac_peak` is against 8 TB/s, `vs_model` = time / (bytes / 6.3 TB/s).
Upper form: a float64 state's sweeps leave the dense blocks with a zero lower triangle, which the product reads in place
(`storage: "zero-lower"`); fp32 states leave them mirrored."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viprs_amd import _lib as L                          # noqa: E402
from viprs_amd.plan import DeviceState, LDPlan           # noqa: E402
from viprs_amd.utils import synthetic as syn             # noqa: E402

PEAK, COPY = 8.0e12, 6.3e12


def make_state(plan, inp, T, n_cols):
    if n_cols == 1:
        st = DeviceState(plan, T, placement="off")
        for k in ("std_beta", "u_logs", "sqrt_half_var_tau", "mu_mult"):
            st.upload(k, getattr(inp, k).astype(T))
        return st, None
    st = DeviceState(plan, T, model="grid", width=n_cols, placement="off")
    scale = np.exp(np.random.default_rng(3).uniform(-0.3, 0.3, size=n_cols))
    st.upload("std_beta", inp.std_beta.astype(T))
    st.upload("u_logs", np.asarray(inp.u_logs[:, None] + np.log(scale)[None, :], dtype=T, order="F"))
    st.upload("half_var_tau", np.asarray((inp.sqrt_half_var_tau.astype(np.float64) ** 2)[:, None] * scale[None, :], dtype=T, order="F"))
    st.upload("mu_mult", np.asarray(inp.mu_mult[:, None] * np.ones((1, n_cols)), dtype=T, order="F"))
    return st, np.arange(n_cols, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--sweeps", type=int, default=5)
    ap.add_argument("--ld-dtypes", default="float32,int8")
    args = ap.parse_args()
    sizes = syn.block_sizes(args.config)
    rows = []
    for ld_name in args.ld_dtypes.split(","):
        for low_memory in (True, False):
            skel = syn.make_ld(sizes, low_memory=low_memory, ld_dtype=np.dtype(ld_name), kind="longrange", data=False)
            plan = LDPlan.synthetic(skel)
            m = plan.m
            beta = (0.01 * np.random.default_rng(12345).standard_normal(m)).astype(np.float32)
            inp = syn.make_inputs(SimpleNamespace(std_beta=beta, n_per_snp=np.full(m, 1e5)))
            ld_bytes = plan.info(L.INFO_LD_BYTES_DEVICE)
            for T in ("float32", "float64"):
                for n_cols in (1, 32):
                    st, active = make_state(plan, inp, T, n_cols)
                    for _ in range(2):
                        st.reset(inp.pi)
                        st.e_step(skel.dq_scale, active)
                    plan.timing_reset()
                    for _ in range(args.sweeps):
                        st.reset(inp.pi)
                        st.e_step(skel.dq_scale, active)
                    sweep_ms = float(np.mean(plan.timing_history(0)))
                    n_ring = len(plan.timing_history(0))
                    for _ in range(3):
                        st.dot("eta", dq_scale=skel.dq_scale)
                    t = []
                    for _ in range(args.calls):
                        st.dot("eta", dq_scale=skel.dq_scale)
                        t.append(plan.last_dot_ms())
                    assert len(plan.timing_history(0)) == n_ring, "a product reached the sweeps' timing ring"
                    dot_ms = float(np.mean(t))
                    nbytes = ld_bytes + 2 * m * n_cols * np.dtype(T).itemsize
                    rows.append({"ld": ld_name, "form": "upper" if low_memory else "symmetric", "state": T, "n_cols": n_cols,
                                 "storage": "zero-lower" if (low_memory and T == "float64") else ("mirrored" if low_memory else "symmetric"),
                                 "dot_ms": round(dot_ms, 4), "dot_ms_min": round(float(np.min(t)), 4),
                                 "dot_ms_median": round(float(np.median(t)), 4), "dot_ms_max": round(float(np.max(t)), 4),
                                 "sweep_ms": round(sweep_ms, 4),
                                 "dot_over_sweep": round(dot_ms / sweep_ms, 3), "bytes": int(nbytes),
                                 "frac_peak": round(nbytes / (dot_ms * 1e-3) / PEAK, 3),
                                 "vs_model": round(dot_ms * 1e-3 / (nbytes / COPY), 2)})
                    print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
                    st.close()
            plan.close()
    print(json.dumps({"tool": "ld_dot_bench", "config": args.config, "m": int(m), "calls": args.calls, "rows": rows}))


if __name__ == "__main__":
    main()
