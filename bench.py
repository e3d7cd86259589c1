#!/usr/bin/env python3
"""bench.py -- SNP-updates/sec of one E-step sweep over synthetic LD blocks on N MI355X GPUs.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N > 1 it is launched as
`python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...`, one rank per GPU
(RANK / LOCAL_RANK / WORLD_SIZE from the environment).  Rank 0 prints ONE JSON line.
A BARE `python bench.py --gpus N` (N > 1, no WORLD_SIZE in the environment) starts the N ranks itself:
the parent -- which never loads the HIP library -- spawns N fresh copies of this script with RANK /
LOCAL_RANK / WORLD_SIZE / MASTER_* / VIPRS_RUN_ID set (one process per GPU, the only parallel axis the
reference has is process-level too: bin/viprs_fit:1079-1086), relays rank 0's line and exits non-zero
if any rank does.  A line is never printed with a world size other than --gpus, nor with more ranks
than HIP devices (`config.rccl_ranks` = the communicator size RCCL itself reports).

A "step" = one pass of the hot path over one batch: the variational state is re-initialised on
the device to the standard start (var_gamma = pi, var_mu = eta = q = eta_diff = 0; the reference's
own benchmark re-initialises before every timed call, benchmarks/benchmark_e_step.py:58-61,
because a converged state takes the skip branch e_step.hpp:410-413 and reads no LD) and one
E-step sweep runs over every LD block of the workload.  LD and the per-SNP inputs are resident in
HBM before the timed region starts.  Before the W warm-up steps the primary workload is swept for
`--prewarm-seconds` (default 0.3 s, untimed; `config.prewarm_s`): the first ~25 sweeps of a fresh process run
~2.5 % slower (clocks, TLBs), and a fit runs hundreds of iterations -- the timed K steps see the steady state.

Workload: BASELINE.json configs[2] -- ~1.1 M SNPs in ~1 700 LD blocks (lognormal block sizes, SURVEY.md 8d;
long-range non-Toeplitz block LD by default, `--ld-kind ar1` for the analytic AR(1) blocks of rounds 1-2),
spike-and-slab prior, fp32 state, fp32 LD in the reference's DEFAULT form (upper-triangular, `low_memory=True`; `--symmetric`
selects the other, which with --full is also the first secondary and is repeated at the top level as `symmetric_ld_form`).
A plain run does only what the headline needs: set-up, warm-up, the K timed steps, the outputs (`--dump-outputs DIR`) and
the line.  Everything else runs only with `--full`: N = 1 then also times, as `config.secondary`, configs[3] (mixture K = 4)
and configs[4] (grid of 32 models) on the same resident LD in both forms, the int8 store format, a float64 state,
math_mode=fast, the EM iteration of the three models, the reference's default OPERATING mode (22 per-chromosome models: one
lock-step batch against 22 fits one after the other), BASELINE configs[0] / configs[1] with the CPU baseline of their own
workloads, the measured chain step (`config.chain_ns_per_snp`) and the CPU baseline of the headline workload
(`cpu_baseline`); N > 1 the other scaling figure.  `metric_definition` stamps what `value`
is (LD form, scaling mode, state placement) so that lines of different rounds are compared like for like.
`--dump-outputs DIR`: the state the last timed step left (var_gamma, var_mu, eta, q, eta_diff: what a caller of the E-step
receives) as DIR/<name>.npy, at most 64 MB in all -- beyond that the same seeded sample of SNPs from every array, whose row
numbers are DIR/sample_rows.npy; N > 1: every rank its own share, DIR/<name>_rank<r>.npy.
N > 1 (default, "strong" = BASELINE.json configs[2], "block-sharded 1/2/4/8 GPUs"): the blocks of ONE 1.1 M-SNP /
1 700-block workload are dealt to the ranks (chain-aware LPT, viprs_amd.parallel.shard_blocks; no data-path
collective) and `value` = that workload's SNPs per max-over-ranks sweep time -- the same quantity as the N = 1 line.
The line carries the time model of every rank and the ceiling the serial chain of the largest LD block puts on this
figure (`strong_scaling_ceiling`).  The WEAK figure (every rank its own 1.1 M-SNP workload, N x the work) is measured
in the same run and reported under `weak_scaling` with its own metric text; `--scaling weak` swaps the two.
Ranks generate their LD ON THE DEVICE (viprs_plan_create_synthetic: the same entries as synthetic.make_ld, bit for bit,
tests/test_synth_device.py), so an 8-rank start-up takes seconds; only the N = 1 headline workload is built on the host
(the CPU baseline runs on it).

No PyTorch: the ranks synchronise and reduce through RCCL via the C ABI (viprs_comm_*).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X HBM3E peak (MI355X_MICROARCH.md: 8 TB/s spec, ~6.3 achievable)
STATE_BYTES_PER_SNP = 68     # lb+indptr (12) + 4 inputs (16) + 5 state reads/writes (40)
SECONDARY_PREWARM_S = 0.1    # untimed sweeps in front of every secondary measurement


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="cfg3", choices=["cfg1", "cfg2", "cfg3", "cfg3max"],
                    help="cfg3max = cfg3 with its largest block replaced by a 6 000-SNP one (BASELINE's clip limit)")
    ap.add_argument("--symmetric", action="store_true",
                    help="symmetric LD (low_memory=False) as the primary workload.  Default: the upper-triangular form, what "
                         "VIPRS() runs by default (low_memory=True, VIPRS.py:75) -- since round 5 its sweep is level with the symmetric one")
    ap.add_argument("--low-memory", action="store_true", help="(the default since round 5; kept so that older command lines still parse)")
    ap.add_argument("--ld-dtype", default="float32", choices=["float32", "int8", "int16"])
    ap.add_argument("--precision", default="float32", choices=["float32", "float64"],
                    help="state type (the reference's float_precision, VIPRS.py:72); float64: spike_slab only, no CPU leg")
    ap.add_argument("--math", default="exact", choices=["exact", "fast"])
    ap.add_argument("--scaling", default="strong", choices=["strong", "weak"],
                    help="N > 1: strong (default, BASELINE configs[2]) = ONE workload sharded by LD block over the ranks; weak = "
                         "one genome-scale workload per rank (N x the work).  The other figure is measured beside `value` in the same run")
    ap.add_argument("--host-ld", action="store_true",
                    help="build every synthetic LD array on the host and upload it (default: on the device, except the N = 1 "
                         "headline workload of a --full run, which the CPU baseline needs on the host)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline: the secondary measurements, the chain-step probe and the "
                         "CPU baseline (a plain run sets up, warms up, times the K steps and prints the line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the state the last timed step left as DIR/<name>.npy (at most 64 MB in all: beyond that a "
                         "fixed, seeded sample of SNPs, DIR/sample_rows.npy)")
    ap.add_argument("--no-secondary", action="store_true",
                    help="with --full: skip the secondary measurements (N = 1: upper-triangular sweep; N > 1: weak scaling)")
    ap.add_argument("--cpu-seconds", type=float, default=20.0, help="with --full: budget of the CPU baseline leg (0 = skip)")
    ap.add_argument("--cpu-threads", type=int, default=0,
                    help="threads of the multi-threaded CPU variants (default: affinity mask capped by the cgroup quota)")
    ap.add_argument("--model", default="spike_slab", choices=["spike_slab", "mixture", "grid"],
                    help="spike_slab = the headline (configs[1..2]); mixture = configs[3] (VIPRSMix); grid = configs[4]")
    ap.add_argument("--width", type=int, default=0, help="mixture components K (default 4) / grid models G (default 32)")
    ap.add_argument("--ld-kind", default="longrange", choices=["ar1", "longrange"],
                    help="synthetic LD blocks (viprs_amd/utils/synthetic.py): longrange = non-Toeplitz blocks whose every "
                         "entry changes the result (the data the full-size parity tests run on); ar1 = rho^|i-j| "
                         "(rounds 1-2; the sweep time does not depend on the values)")
    ap.add_argument("--prewarm-seconds", type=float, default=0.3,
                    help="untimed sweeps of the primary workload BEFORE the --warmup steps (the first ~25 sweeps of a fresh process "
                         "run 2 %% slower: clocks and TLBs; a fit runs hundreds of iterations); reported as config.prewarm_s")
    ap.add_argument("--seed", type=int, default=7209)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.symmetric and args.low_memory:
        ap.error("--symmetric and --low-memory exclude each other")
    args.low_memory = not args.symmetric
    return args


def config_sizes(config, seed):
    from viprs_amd.utils import synthetic as syn
    if config == "cfg3max":
        s = syn.block_sizes("cfg3", seed).copy()
        s[int(np.argmax(s))] = 6000
        return s
    return syn.block_sizes(config, seed)


def shard_blocks_lpt(sizes, n_parts):
    """Blocks of one workload -> ranks (chain-aware LPT, viprs_amd.parallel.shard_blocks); sorted block lists."""
    from viprs_amd.parallel import shard_blocks
    owner = shard_blocks(np.asarray(sizes), n_parts)
    return [sorted(int(i) for i in np.nonzero(owner == r)[0]) for r in range(n_parts)]


# ---- CPU baseline ---------------------------------------------------------------------------------------
def usable_cpus():
    """Hardware threads this process may really use: the scheduler affinity mask, capped by the cgroup CPU quota
    (a container can show 256 CPUs and be allowed 8 -- OpenMP teams sized by os.cpu_count() then spin on each other)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:                       # cgroup v2: "<quota> <period>" or "max <period>"
            q, per = f.read().split()
            if q != "max":
                quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f1, open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f2:
                q, per = float(f1.read()), float(f2.read())
                if q > 0:
                    quota = q / per
        except (OSError, ValueError):
            pass
    if quota is not None:
        n = max(1, min(n, int(quota + 0.5)))
    return n, {"os_cpu_count": os.cpu_count(), "affinity": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None,
               "cgroup_cpu_quota": quota}


def cpu_baseline(ld, inp, budget_s, model="spike_slab", width=1, extra=None, pi0=None, threads_override=0):
    """The reference's own e_step.hpp (oracle/_ref, built from /root/reference by oracle/Makefile) timed on
    this host, state re-initialised before every call:
      1. threads=1 (the parity reference);
      2. its OpenMP path on all hardware threads -- racy Hogwild, e_step.hpp:384-387: the "reference
         multithreaded-CPU" figure, `value`;
      3. exact block-parallel: one threads=1 call per LD block, blocks handed to all hardware threads by a native
         OpenMP loop (what joblib over chromosomes does at a finer grain, bin/viprs_fit:1080-1086) -- spike-and-slab
         only; built with the reference's flags and with -march=x86-64-v3;
      4. variants 1 and 2 from the build with -march=x86-64-v3 (AVX2 + FMA: the portable stand-in for the
         "-march=native" optimistic-CPU line -- the library is built where /root/reference lives, not here).
    `best_exact` names the fastest variant whose results are reproducible (1, 3, 4_single_thread).
    Sample of 1, 2, 4: leading blocks of the same workload sized to the time budget (a mixture / grid SNP-update
    costs `width` times a spike-and-slab one); 3 runs the WHOLE workload (its sweep takes tens of ms)."""
    from oracle import oracle as O
    kind = "reference" if O.have_reference() else "restated"
    cores, host = usable_cpus()
    if threads_override:
        cores = int(threads_override)
    # ~0.2-0.5 M SNP-updates/s single-threaded: size the sample for ~budget/4 per single-thread pass
    target_snps = int(min(ld.m, max(2000, 0.08e6 * budget_s / max(1, width))))
    nb = int(np.searchsorted(ld.block_start, target_snps, side="left"))
    nb = max(1, min(nb, len(ld.block_start) - 1))
    m_s = int(ld.block_start[nb])
    nnz_s = int(ld.ld_indptr[m_s])
    lb = np.ascontiguousarray(ld.ld_left_bound[:m_s])
    ip = np.ascontiguousarray(ld.ld_indptr[:m_s + 1])
    data = ld.ld_data[:nnz_s]
    T = np.float32
    std_beta = np.ascontiguousarray(inp.std_beta[:m_s])
    if model == "spike_slab":
        vec = {k: np.ascontiguousarray(getattr(inp, k)[:m_s]) for k in ("u_logs", "sqrt_half_var_tau", "mu_mult")}
    else:
        order = "F" if model == "grid" else "C"
        vec = {k: np.asarray(v[:m_s], order=order).copy(order=order) for k, v in extra.items()}

    def one(threads, kind_):
        if model == "spike_slab":
            st = {k: np.ascontiguousarray(v[:m_s]).copy() for k, v in inp.state_copy().items()}
            t0 = time.perf_counter()
            O.cpp_e_step(lb, ip, data, std_beta, st["var_gamma"], st["var_mu"], st["eta"], st["q"],
                         st["eta_diff"], vec["u_logs"], vec["sqrt_half_var_tau"], vec["mu_mult"], ld.dq_scale,
                         threads, ld.low_memory, kind=kind_)
        elif model == "mixture":
            vg = np.full((m_s, width), pi0, dtype=T)
            vm = np.zeros((m_s, width), dtype=T)
            eta, q, ed = (np.zeros(m_s, dtype=T) for _ in range(3))
            t0 = time.perf_counter()
            O.cpp_e_step_mixture(lb, ip, data, std_beta, vg, vm, eta, q, ed, vec["log_null_pi"], vec["u_logs"],
                                 vec["sqrt_half_var_tau"], vec["mu_mult"], ld.dq_scale, threads, ld.low_memory, kind=kind_)
        else:
            vg = np.full((m_s, width), pi0, dtype=T, order="F")
            vm, eta, q, ed = (np.zeros((m_s, width), dtype=T, order="F") for _ in range(4))
            t0 = time.perf_counter()
            O.cpp_e_step_grid(lb, ip, data, std_beta, vg, vm, eta, q, ed, vec["u_logs"], vec["half_var_tau"],
                              vec["mu_mult"], ld.dq_scale, np.arange(width, dtype=np.int32), threads, ld.low_memory,
                              kind=kind_)
        return time.perf_counter() - t0

    def timed(fn, share):
        fn()                                           # warm-up
        ts, t_used = [], 0.0
        while t_used < budget_s * share and len(ts) < 15:
            dt = fn()
            ts.append(dt)
            t_used += dt
        return float(np.median(ts))

    res = {"threads1": m_s / timed(lambda: one(1, kind), 0.25)}
    mt = cores if kind == "reference" else 1
    res["all_cores"] = m_s / timed(lambda: one(mt, kind), 0.2)
    variants = {
        "1_single_thread": res["threads1"],
        "2_openmp_all_threads_racy": res["all_cores"],
    }
    if kind == "reference" and O.have_reference("reference_v3"):
        variants["4_openmp_all_threads_racy_march_x86_64_v3"] = m_s / timed(lambda: one(mt, "reference_v3"), 0.15)
        variants["4_single_thread_march_x86_64_v3"] = m_s / timed(lambda: one(1, "reference_v3"), 0.15)
    if model == "spike_slab" and kind == "reference":
        variants["3_block_parallel_exact"] = _block_parallel_exact(ld, inp, "reference", cores, budget_s * 0.15)
        if O.have_reference("reference_v3"):
            variants["3_block_parallel_exact_march_x86_64_v3"] = _block_parallel_exact(ld, inp, "reference_v3", cores,
                                                                                       budget_s * 0.1)
    exact = {k: v for k, v in variants.items() if "racy" not in k}
    best = max(exact, key=exact.get)
    return {
        "value": res["all_cores"], "unit": "SNP-updates/s", "cores": mt,
        "best_exact": {"variant": best, "value": exact[best], "threads": 1 if "single" in best else cores},
        "host": host,
        "kind": "reference" if kind == "reference" else "port",
        "sample": f"first {nb} LD blocks ({m_s} SNPs, {nnz_s} LD entries) of the same workload, model={model}"
                  + (f" width={width}" if model != "spike_slab" else "")
                  + f", state re-initialised per call, median; OpenMP threads={mt} (racy, as the reference)"
                  + "; variants 3 = every block of the WHOLE workload, one threads=1 call per block, native OpenMP loop "
                    f"over blocks on {cores} threads",
        "single_thread_value": res["threads1"],
        "variants": variants,
    }


def _block_parallel_exact(ld, inp, kind, workers, budget_s):
    """SNP-updates/s of the WHOLE workload with one exact (threads=1) reference call per LD block, blocks handed to
    `workers` OpenMP threads longest first (native loop inside oracle/_ref: ref_shim.cpp `ref_e_step_blocks`)."""
    from oracle import oracle as O

    def sweep():
        st = inp.state_copy()
        t0 = time.perf_counter()
        O.e_step_block_parallel(ld.block_start, ld.ld_left_bound, ld.ld_indptr, ld.ld_data, inp.std_beta,
                                st["var_gamma"], st["var_mu"], st["eta"], st["q"], st["eta_diff"], inp.u_logs,
                                inp.sqrt_half_var_tau, inp.mu_mult, ld.dq_scale, workers, ld.low_memory, kind=kind)
        return time.perf_counter() - t0

    sweep()
    ts, used = [], 0.0
    while used < budget_s and len(ts) < 10:
        ts.append(sweep())
        used += ts[-1]
    return ld.m / float(np.median(ts))


# ---- workload ---------------------------------------------------------------------------------------------
def build_workload(args, sizes_all, mine, seed, low_memory, ld_dtype, data=True):
    """LD + inputs of the blocks `mine` of the workload (`sizes_all`, seed): every random draw is made for the
    WHOLE workload (block LD parameters, effects, noise, hyper-parameters M pi / h2), so a block holds
    the same numbers whichever rank it lands on and however many ranks share the workload.
    `data=False` ("longrange" LD only): the LD skeleton -- index arrays and block parameters, `ld_data = None`; the
    entries are generated on the device when the plan is created (`LDPlan.synthetic`), bit-identical to the host's."""
    from viprs_amd.utils import synthetic as syn
    kind = getattr(args, "ld_kind", "ar1")
    data = bool(data) or kind != "longrange" or getattr(args, "host_ld", False)
    rng = np.random.default_rng(seed + 1)
    rho_all = rng.uniform(0.3, 0.8, len(sizes_all))
    params_all = syn.longrange_params(sizes_all, seed) if kind == "longrange" else None
    if mine is None:
        ld = syn.make_ld(sizes_all, low_memory=low_memory, ld_dtype=ld_dtype, seed=seed, rho=rho_all, kind=kind,
                         params=params_all, data=data)
        ss = syn.make_sumstats(ld, seed=seed)
        return ld, ss, syn.make_inputs(ss), ld.m
    starts = np.concatenate([[0], np.cumsum(sizes_all)]).astype(np.int64)
    m_all = int(starts[-1])
    skeleton = syn.SyntheticLD(np.empty(m_all, np.int32), None, None, starts, rho_all, low_memory, kind=kind,
                               params=params_all)
    ss_all = syn.make_sumstats(skeleton, seed=seed)
    inp_all = syn.make_inputs(ss_all)
    idx = np.concatenate([np.arange(starts[b], starts[b + 1]) for b in mine]) if len(mine) else np.zeros(0, np.int64)
    ld = syn.make_ld(sizes_all[mine], low_memory=low_memory, ld_dtype=ld_dtype, seed=seed, rho=rho_all[mine], kind=kind,
                     params=[params_all[b] for b in mine] if params_all is not None else None, data=data)
    ss = syn.SyntheticSumstats(ss_all.std_beta[idx], ss_all.n_per_snp[idx], ss_all.beta_true[idx], ss_all.n)
    take = lambda a: np.ascontiguousarray(a[idx])
    inp = syn.EStepInputs(**{k: take(getattr(inp_all, k)) for k in
                             ("std_beta", "var_gamma", "var_mu", "eta", "q", "eta_diff", "u_logs", "sqrt_half_var_tau",
                              "mu_mult")},
                          pi=inp_all.pi, sigma_epsilon=inp_all.sigma_epsilon, tau_beta=inp_all.tau_beta)
    return ld, ss, inp, m_all


class Sweep:
    """Device-resident plan + state of one workload (share) and the timed step.  `plan`: an existing plan of the same
    LD to put another model's state on (the LD is uploaded once)."""

    def __init__(self, args, ld, ss, inp, device, model, width, low_memory, plan=None, precision="float32"):
        from viprs_amd.plan import DeviceState, LDPlan
        from viprs_amd.utils import synthetic as syn
        self.ld = ld
        self.own_plan = plan is None
        if plan is not None:
            self.plan = plan
        elif ld.ld_data is None:                      # skeleton: the LD entries are generated on the device
            self.plan = LDPlan.synthetic(ld, device=device, math_mode=args.math)
        else:
            self.plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, low_memory, device=device, math_mode=args.math)
        # (ranks sharing a device in a dry run: no placement probe -- its sweeps are not under the device lock)
        self.state = DeviceState(self.plan, precision, model, width, placement="off" if Sweep.device_lock else None)
        self.model, self.width = model, width
        self.state_itemsize = np.dtype(precision).itemsize
        self.active = None
        self.host_extra = None
        self.pi0 = inp.pi
        if model == "spike_slab":
            for name in ("std_beta", "u_logs", "sqrt_half_var_tau", "mu_mult"):
                self.state.upload(name, getattr(inp, name).astype(precision, copy=False))
        else:
            extra = syn.make_mixture_inputs(ss, width) if model == "mixture" else syn.make_grid_inputs(ss, width)
            self.pi0 = extra.pop("pi")
            self.host_extra = extra
            self.state.upload("std_beta", inp.std_beta)
            for name, arr in extra.items():
                self.state.upload(name, arr)
            if model == "grid":
                self.active = np.arange(width, dtype=np.int32)

    # Dry runs of the multi-rank logic with several ranks on ONE device (VIPRS_BENCH_COMM=file): the sweep kernels size
    # their grids to the whole device and their team workgroups wait for each other, so kernels of different processes
    # must not share the device -- the ranks take turns through a file lock (set by main()).  Never on a real run.
    device_lock = None

    def step(self):
        if Sweep.device_lock is None:
            self.state.reset(self.pi0)
            self.state.e_step(self.ld.dq_scale, self.active, sync=False)
            return
        import fcntl
        with open(Sweep.device_lock, "w") as f:
            fcntl.flock(f, fcntl.LOCK_EX)
            try:
                self.state.reset(self.pi0)
                self.state.e_step(self.ld.dq_scale, self.active, sync=True)
            finally:
                fcntl.flock(f, fcntl.LOCK_UN)

    def run(self, steps, warmup, barrier):
        """W untimed steps, barrier, exactly K timed steps, device idle; returns this rank's seconds."""
        for _ in range(warmup):
            self.step()
        barrier()
        self.plan.timing_reset()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        self.state.synchronize()
        barrier()
        return time.perf_counter() - t0

    def algorithmic_bytes(self):
        """LD element size x entries streamed (the upper-triangular form reads its entries twice) +
        per-SNP index / input / state bytes of the model (spike-and-slab: 68 B)."""
        ld, w = self.ld, self.width
        nnz = ld.nnz * (2 if ld.low_memory else 1)
        per_snp = {"spike_slab": STATE_BYTES_PER_SNP, "mixture": 12 + 4 + 4 * (3 * w + 1) + 8 * (2 * w + 3),
                   "grid": 12 + 4 + 36 * w}[self.model]
        if self.model == "spike_slab" and self.state_itemsize != 4:          # 12 index bytes + 14 state / input words
            per_snp = 12 + 14 * self.state_itemsize
        return ld.itemsize * nnz + per_snp * ld.m

    def close(self):
        self.state.close()
        if self.own_plan:
            self.plan.close()


OUTPUTS = ("var_gamma", "var_mu", "eta", "q", "eta_diff")      # what the E-step hands back to its caller
DUMP_BUDGET_BYTES = 64 << 20
DUMP_SAMPLE_SEED = 20240917


def dump_outputs(directory, arrays, budget=DUMP_BUDGET_BYTES, suffix=""):
    """Writes `arrays` (name -> float32 / float64 array with one row per SNP) as DIR/<name><suffix>.npy.  Over `budget` bytes
    in all, every array keeps the same rows: a fixed, seeded sample in SNP order, whose row numbers are written as
    DIR/sample_rows<suffix>.npy (float64).  Returns the names written."""
    os.makedirs(directory, exist_ok=True)
    m = len(next(iter(arrays.values())))
    for name, a in arrays.items():
        if a.dtype not in (np.float32, np.float64) or len(a) != m:
            raise ValueError(f"dump_outputs: {name} is {a.dtype} with {len(a)} rows, expected float32 / float64 with {m}")
    row_bytes = sum(a.nbytes // max(1, m) for a in arrays.values())
    if row_bytes * m > budget:
        n = max(1, int(budget // (row_bytes + 8)))                          # (+ 8: the row number itself)
        rows = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(m, size=n, replace=False))
        arrays = {k: np.ascontiguousarray(a[rows]) for k, a in arrays.items()}
        arrays["sample_rows"] = rows.astype(np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(directory, f"{name}{suffix}.npy"), np.ascontiguousarray(a))
    return sorted(arrays)


def pct(v, q):
    return float(np.percentile(v, q)) if len(v) else None


# ---- time model of one sweep on one GPU -----------------------------------------------------------------------
# What a sweep cannot beat, from three measured machine constants: the HBM stream, the serial chain of the
# largest block, and the chip's total chain work spread over the chains in flight.
STREAM_GBS = 6300.0                                 # what a float4 copy reaches on MI355X (MI355X_MICROARCH.md)
CHAIN_NS = {                                        # ns per serial SNP step of ONE chain, per-phase work included
    ("spike_slab", "exact"): 135.0, ("spike_slab", "fast"): 95.0,
    ("mixture", "exact"): 275.0, ("mixture", "fast"): 220.0,          # K = 4 (lane-parallel softmax chain; tools/chain_ns_models.py)
    ("grid", "exact"): 430.0, ("grid", "fast"): 420.0,                # 32 models per step
    ("spike_slab_f64", "exact"): 300.0,                                # estep_tile.h: 237 ns + 4 us per panel
}
CHAINS_IN_FLIGHT = {"spike_slab": 512, "mixture": 512, "grid": 256, "spike_slab_f64": 256}


def sweep_time_model(sizes, algo_bytes, model, math_mode, f64=False):
    """max(bytes / 6.3 TB/s, largest block's chain, total chain work / chains in flight) in ms, and which term it is."""
    key = "spike_slab_f64" if f64 else model
    ns = CHAIN_NS.get((key, math_mode), CHAIN_NS[(key, "exact")])
    sizes = np.asarray(sizes, dtype=np.float64)
    terms = {"hbm_stream": algo_bytes / (STREAM_GBS * 1e9) * 1e3,
             "largest_block_chain": float(sizes.max()) * ns * 1e-6 if sizes.size else 0.0,
             "chain_throughput": float(sizes.sum()) * ns * 1e-6 / CHAINS_IN_FLIGHT[key]}
    bound = max(terms, key=terms.get)
    return terms[bound], bound, ns, terms


def pmc_traffic(key):
    """(HBM bytes per sweep from profiles/pmc_traffic.json, note).  The figure is a constant of the kernel it was
    collected on (separate rocprofv3 --pmc passes, profiles/summarize.py), not measured in this run: it is quoted only
    while the sources of that kernel family hash to what they were then -- otherwise None and the note says why."""
    prof = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        e = json.load(open(prof)).get(key)
    except Exception:
        return None, "profiles/pmc_traffic.json unreadable"
    if not isinstance(e, dict):
        return None, f"no PMC traffic recorded for {key}"
    from viprs_amd.utils import kernel_id
    now = kernel_id.source_hash(e.get("family") or kernel_id.family_of(key))
    if e.get("src_hash") != now:
        return None, (f"stale: collected on {e.get('family')} kernel sources {e.get('src_hash')} ({e.get('collected')}), the "
                      f"library now builds from {now} -- re-run tools/profile.sh")
    return int(e["hbm_bytes_per_sweep"]), ("profiles/pmc_traffic.json: (2 FETCH_SIZE + WRITE_SIZE) x 1024 from separate rocprofv3 "
                                           f"--pmc passes of this command ({e.get('collected')}, kernel sources {now}: a constant "
                                           "of the kernel, not measured in this run)")


HOST_IN_BRACKET_MS = 0.1


def clean_kernel_times(k, k_host):
    """Per-sweep kernel times (HIP events) without the sweeps whose event bracket provably holds host time: the library stamps
    the host clock where it records the dominant kernel's start event and behind the end event's record (`timing_history(2)`:
    normally 0.007 ms).  A sweep submitted into an EMPTY stream has its start event reached at once, so a slow launch call --
    the HIP runtime's takes 1.3-1.4 ms about once per few thousand launches, then 0.3 ms on the next (EXPERIMENTS.md 6.10) --
    is counted as kernel time: 2.1 ms beside 0.69.  Such sweeps (host time inside the bracket > 0.1 ms) are left out of the mean,
    listed and counted; the raw mean is reported beside it."""
    k = list(k)
    if not k_host or len(k_host) != len(k):
        return k, []
    bad = [i for i, h in enumerate(k_host) if h > HOST_IN_BRACKET_MS]
    good = [x for i, x in enumerate(k) if i not in bad]
    return (good or k), bad


def measure_secondary(name, sw, steps, barrier, math_mode="exact", traffic_key=None):
    """One secondary configuration on one GPU: K timed steps, kernel time from the library's HIP events; with the
    time model of the sweep (what bounds it and how close the kernel is: `frac_of_model`) and the PMC traffic."""
    # (0.1 s of untimed sweeps first, as the primary workload gets 0.3 s: a freshly built plan's first sweeps run 2-5 % slower)
    t_pre = time.perf_counter()
    while time.perf_counter() - t_pre < SECONDARY_PREWARM_S:
        sw.step()
    sw.state.synchronize()
    el = sw.run(steps, 3, barrier)
    k = sw.plan.timing_history(which=1)
    k_all = sw.plan.timing_history(which=0)
    k_host = sw.plan.timing_history(which=2)      # host time inside each sweep's event bracket (the launch call)
    by = sw.algorithmic_bytes()
    f64 = sw.state_itemsize != 4
    t_model, bound, ns, terms = sweep_time_model(np.diff(sw.ld.block_start), by, sw.model, math_mode, f64)
    # `kernel_ms_avg`: mean of the timed sweeps whose event bracket holds no host time (`clean_kernel_times`: per-sweep
    # evidence, not a threshold on the kernel time itself); `kernel_ms_avg_raw` is the plain mean, every sweep's kernel time
    # and host time inside the bracket are in the line.
    k_good, k_bad = clean_kernel_times(k, k_host)
    k_med = float(np.median(k))
    k_avg = float(np.mean(k_good))
    out = {"name": name, "value": sw.ld.m * steps / el, "unit": "SNP-updates/s", "ms_per_step": el / steps * 1e3,
           "kernel_ms_avg": k_avg, "kernel_ms_p50": k_med, "kernel_ms_max": float(np.max(k)),
           "kernel_ms_all": [round(float(x), 4) for x in k], "outlier_sweeps": int(sum(x > 1.5 * k_med for x in k)),
           "kernel_ms_avg_raw": float(np.mean(k)), "host_ms_inside_the_bracket_all": [round(float(x), 4) for x in k_host],
           "sweeps_with_host_time_inside_the_bracket": k_bad,
           "all_kernels_ms_avg": float(np.mean(k_all)) if k_all else None,
           "roofline_frac": by / (k_avg * 1e-3) / 1e9 / HBM_PEAK_GBS,
           "algorithmic_bytes_per_launch": int(by), "steps": steps, "prewarm_s": SECONDARY_PREWARM_S, "math_mode": math_mode,
           "math_mode_effective": sw.plan.effective_math_mode(),      # what the kernels really ran in (fast: not every model has it)
           "time_model_ms": t_model, "time_model_bound": bound, "time_model_terms_ms": terms,
           "chain_ns_per_snp_model": ns, "frac_of_model": t_model / float(np.mean(k_all) if k_all else k_avg)}
    tr, tr_note = pmc_traffic(traffic_key) if traffic_key else (None, None)
    out["traffic"] = tr
    out["traffic_source"] = tr_note
    out["traffic_over_algorithmic"] = (tr / by) if tr else None
    if sw.model == "grid":
        out["snp_x_model_updates_per_s"] = out["value"] * sw.width
    return out


def chain_ns_per_snp(args, device, math_mode, low_memory=False, size=6000, steps=10):
    """Measured ns per serial chain step: one isolated LD block of `size` SNPs (nothing else on the chip), sweep time / size."""
    from viprs_amd.utils import synthetic as syn

    class A:
        math = math_mode
    ld, ss, inp = syn.make_problem(sizes=[size], low_memory=low_memory, seed=3)
    sw = Sweep(A, ld, ss, inp, device, "spike_slab", 1, low_memory)
    sw.run(steps, 3, lambda: None)
    k = sw.plan.timing_history(which=1)
    sw.close()
    return float(np.median(k)) * 1e6 / size


def measure_fit_iteration(kind, ld, ss, device, iters=12, warm=3, math_mode="exact"):
    """One EM iteration of VIPRS / VIPRSMix(K=4) / VIPRSGrid(32 models, batched) on the workload's LD: what
    VIPRS.fit() does per iteration (VIPRS.py:979-1019: e_step, m_step, ELBO + stopping rules).
    `ms_per_iteration` = wall time of `iters` free-running iterations of fit() from the standard start (after `warm`
    iterations), / iters; `split_ms` = the same iteration taken apart with a device synchronisation between the phases
    (which the free-running loop does not have): prep + sweep enqueue-to-idle, the sweep kernel alone (HIP events), the
    device reduction of the partial sums + its read-back, the host's M-step / ELBO / stopping rules."""
    from viprs_amd.data import ArrayDataLoader, LDArrays, SumstatsArrays
    from viprs_amd.model import VIPRS, VIPRSMix
    form = (ld.ld_left_bound, ld.ld_indptr, ld.ld_data)
    lm = bool(ld.low_memory)
    gdl = ArrayDataLoader({1: LDArrays(upper=form, dq_scale=ld.dq_scale) if lm else LDArrays(symmetric=form, dq_scale=ld.dq_scale)},
                          {1: SumstatsArrays(ss.std_beta, ss.n_per_snp)}, n=float(ss.n))
    stamps = []
    cb = lambda i: stamps.append(time.perf_counter())
    # integer LD stays integer on the device (dequantize_on_the_fly, VIPRS.py:156-165: the published stores are int8)
    dq_fly = bool(np.issubdtype(ld.ld_data.dtype, np.integer))
    out = {"name": f"fit_iteration {kind}" + (f", {ld.ld_data.dtype.name} LD" if dq_fly else "") + (", math_mode=fast" if math_mode == "fast" else ""),
           "unit": "ms per EM iteration", "iterations": iters, "warmup_iterations": warm,
           "math_mode": math_mode, "snps": int(ld.m), "low_memory": lm, "ld_dtype": ld.ld_data.dtype.name}
    if kind.startswith("VIPRSGrid"):
        from viprs_amd.model.gridsearch.HyperparameterGrid import HyperparameterGrid
        from viprs_amd.model.gridsearch.VIPRSGrid import VIPRSGrid
        grid = HyperparameterGrid(n_snps=gdl.m)
        grid.generate_pi_grid(steps=8)
        grid.generate_sigma_epsilon_grid(steps=4)
        model = VIPRSGrid(gdl, grid, low_memory=lm, device=device, math_mode=math_mode, dequantize_on_the_fly=dq_fly)
        model.fit(max_iter=warm + iters, min_iter=warm + iters + 1, batched=True, on_iteration=cb)
        plan = next(iter(model._plans.values()))
        out["models"] = int(model.n_models)
    else:
        # a FIXED start (the reference draws pi and h2 at random when none is given, VIPRS.py:260-292: run-to-run
        # different trajectories): pi = 0.01, sigma_epsilon = 0.8, the start of the sweep benchmark
        if kind.startswith("VIPRSMix"):
            model = VIPRSMix(gdl, K=4, low_memory=lm, device=device, math_mode=math_mode, dequantize_on_the_fly=dq_fly)
            theta = {"pis": np.full(4, 0.01 / 4), "sigma_epsilon": 0.8}
        else:
            model = VIPRS(gdl, low_memory=lm, device=device, math_mode=math_mode, dequantize_on_the_fly=dq_fly)
            theta = {"pi": 0.01, "sigma_epsilon": 0.8}
        out["theta_0"] = {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in theta.items()}
        model.fit(max_iter=warm + iters, min_iter=warm + iters + 1, theta_0=theta, on_iteration=cb)
        plan = next(iter(model._plans.values()))
    out["math_mode_effective"] = plan.effective_math_mode()
    out["iterations_run"] = len(stamps)
    out["message"] = str(getattr(getattr(model, "optim_result", None), "message", ""))[:80]
    if len(stamps) < warm + 3:
        # (a fit that stops early -- negative MSE, ELBO undefined: the reference's own stopping rules -- is reported, not
        #  an error of the measurement)
        out["ms_per_iteration"] = None
        return out
    d = np.diff(np.array(stamps))[warm - 1:]                               # iterations warm+1 .. the last one run
    out["ms_per_iteration"] = float(np.median(d)) * 1e3                    # (median: the host loop is Python, a GC pause is not the iteration)
    out["ms_per_iteration_mean"] = float(np.mean(d)) * 1e3
    out["ms_per_iteration_all"] = [round(float(x) * 1e3, 4) for x in d]
    k = plan.timing_history(which=0)
    out["sweep_kernels_ms_avg"] = float(np.mean(k[-iters:])) if k else None
    out["skipped_snps_last_sweep"] = int(plan.last_skipped())
    # (VIPRS.py:1025-1044: a negative MSE restarts the fit with sigma_epsilon fixed; the synthetic workload does that once)
    out["sigma_epsilon_fixed_by_restart"] = bool("sigma_epsilon" in getattr(model, "fix_params", {}))
    if not kind.startswith("VIPRSGrid"):
        # the same iteration, phase by phase (continuing the same trajectory)
        sync = lambda: _lib_sync(device)
        ph = np.zeros(4)
        n2 = max(5, iters // 2)
        plan.timing_reset()
        for _ in range(n2):
            t0 = time.perf_counter()
            model.e_step()
            sync()
            t1 = time.perf_counter()
            model._reduce()
            t2 = time.perf_counter()
            model.m_step()
            model.update_theta_history()
            t3 = time.perf_counter()
            ph += (t1 - t0, 0.0, t2 - t1, t3 - t2)
        kk = plan.timing_history(which=0)
        sweep = float(np.mean(kk)) if kk else 0.0
        ph = ph / n2 * 1e3
        out["split_ms"] = {"prep_launch_sync": max(0.0, ph[0] - sweep), "sweep_kernels": sweep, "sums_reduce_readback": ph[2],
                           "host_mstep_elbo_rules": ph[3], "sum_with_syncs": float(ph[0] + ph[2] + ph[3])}
    else:
        # the batched grid iteration, phase by phase (all models active; the hyper-parameters keep moving as in the fit)
        import copy
        em, states, all_sums = model._lockstep
        em = copy.deepcopy(em)
        sync = lambda: _lib_sync(device)
        a = np.arange(model.n_models, dtype=np.int32)
        ph = np.zeros(5)
        n2 = max(5, iters // 2)
        plan.timing_reset()
        for it in range(n2):
            t0 = time.perf_counter()
            rows = em.prep_rows(a)
            for st in states.values():
                st.prep_columns(rows)
            sync()
            t1 = time.perf_counter()
            for st in states.values():
                st.e_step(model.dequantize_scale, active_model_idx=a, sync=False)
            sync()
            t2 = time.perf_counter()
            s_ = all_sums(a)
            t3 = time.perf_counter()
            em.update(a, s_, 10_000 + it)
            t4 = time.perf_counter()
            ph += (t1 - t0, t2 - t1, 0.0, t3 - t2, t4 - t3)
        kk = plan.timing_history(which=0)
        sweep = float(np.mean(kk)) if kk else 0.0
        ph = ph / n2 * 1e3
        out["split_ms"] = {"prep_columns_launch_sync": ph[0], "sweep_launch_sync": ph[1], "sweep_kernels": sweep,
                           "sums_columns_reduce_readback": ph[3], "host_mstep_elbo_rules": ph[4],
                           "sum_with_syncs": float(ph[0] + ph[1] + ph[3] + ph[4])}
        out["ms_per_iteration_max_over_median"] = float(np.max(d) / np.median(d)) if len(d) else None
    try:
        model.close()
    except Exception:
        pass
    return out


def _lib_sync(device):
    from viprs_amd import _lib
    _lib.check(_lib.lib.viprs_device_synchronize(device))


# ---- the reference's DEFAULT mode: one model per chromosome (bin/viprs_fit:232-238, :1079-1086) ---------------------
CHROM_MB = (249, 243, 198, 191, 181, 171, 159, 146, 141, 136, 135, 134, 115, 107, 103, 90, 81, 78, 59, 63, 48, 51)   # GRCh37 autosomes


def split_into_chromosomes(ld, ss):
    """The workload's LD blocks as 22 'chromosomes': contiguous runs of blocks whose SNP counts follow the autosomes'
    lengths (chr1 8.6 % ... chr21 1.7 %).  Returns an ArrayDataLoader over views of the workload's host arrays."""
    from viprs_amd.data import ArrayDataLoader, LDArrays, SumstatsArrays
    starts = np.asarray(ld.block_start, dtype=np.int64)
    cum = np.cumsum(CHROM_MB) / float(np.sum(CHROM_MB)) * ld.m
    cut = [0] + [int(np.argmin(np.abs(starts - c))) for c in cum[:-1]] + [len(starts) - 1]
    for i in range(1, len(cut)):                              # every chromosome at least one block
        cut[i] = max(cut[i], cut[i - 1] + 1)
    cut[-1] = len(starts) - 1
    lds, sss, sizes = {}, {}, {}
    for c in range(22):
        a, b = int(starts[cut[c]]), int(starts[cut[c + 1]])
        o = int(ld.ld_indptr[a])
        form = (np.ascontiguousarray(ld.ld_left_bound[a:b] - a).astype(np.int32), np.ascontiguousarray(ld.ld_indptr[a:b + 1] - o),
                ld.ld_data[o:int(ld.ld_indptr[b])])
        lds[c + 1] = LDArrays(upper=form, dq_scale=ld.dq_scale) if ld.low_memory else LDArrays(symmetric=form, dq_scale=ld.dq_scale)
        sss[c + 1] = SumstatsArrays(ss.std_beta[a:b], ss.n_per_snp[a:b])
        sizes[c + 1] = np.diff(starts[cut[c]:cut[c + 1] + 1])
    return ArrayDataLoader(lds, sss), sizes


def measure_per_chromosome(ld, ss, device, iters=12, warm=3, math_mode="exact", mixture_k=0):
    """22 independent per-chromosome models (what `viprs_fit` runs unless --genomewide): ONE lock-step batch on one plan
    (`VIPRSPerChromosome`: per-group hyper-parameters and sums, one sweep per EM round) against the same 22 models fitted
    one after the other by `VIPRS` (one plan, one sweep, one reduction per chromosome per iteration).  ms per EM ROUND =
    one iteration of every chromosome's model; a fixed start (pi = 0.01, sigma_epsilon = 0.8), stopping rules held off
    (`min_iter`) so that every round updates all 22 models."""
    from viprs_amd.model import VIPRS, VIPRSMix, VIPRSMixPerChromosome, VIPRSPerChromosome
    gdl, sizes = split_into_chromosomes(ld, ss)
    lm = bool(ld.low_memory)
    theta = {"pi": 0.01, "sigma_epsilon": 0.8}
    batch_cls, one_cls, kw, what = VIPRSPerChromosome, VIPRS, {}, "models"
    if mixture_k:               # (`mixture_k` = K: VIPRSMix per chromosome, `VIPRSMixPerChromosome` against K-component fits in turn)
        theta = {"pis": 0.01 * np.array([0.4, 0.3, 0.2, 0.1])[:mixture_k] if mixture_k <= 4 else np.full(mixture_k, 0.01 / mixture_k),
                 "sigma_epsilon": 0.8}
        batch_cls, one_cls, kw, what = VIPRSMixPerChromosome, VIPRSMix, {"K": mixture_k}, f"VIPRSMix(K={mixture_k}) models"
    n_it = warm + iters
    out = {"name": f"22 per-chromosome {what} (the reference's default mode, bin/viprs_fit:232-238): lock-step batch vs one fit after the other",
           "unit": "ms per EM round (one iteration of all 22 models)", "iterations": iters, "warmup_iterations": warm,
           "math_mode": math_mode, "snps": int(ld.m), "low_memory": lm, "chromosomes": 22,
           "snps_per_chromosome": [int(np.sum(sizes[c])) for c in sorted(sizes)],
           "largest_block_per_chromosome": [int(np.max(sizes[c])) for c in sorted(sizes)]}
    stamps = []
    model = batch_cls(gdl, low_memory=lm, device=device, math_mode=math_mode, **kw)
    model.fit(max_iter=n_it, min_iter=n_it + 1, theta_0=dict(theta), on_iteration=lambda i: stamps.append(time.perf_counter()))
    d = np.diff(np.array(stamps))[warm - 1:]
    plan = model._plans["*"]
    k = plan.timing_history(which=0)
    out["batched"] = {"ms_per_round": float(np.median(d)) * 1e3 if len(d) else None, "ms_per_round_mean": float(np.mean(d)) * 1e3 if len(d) else None,
                      "ms_per_round_all": [round(float(x) * 1e3, 4) for x in d], "rounds_run": len(stamps),
                      "sweep_kernels_ms_avg": float(np.mean(k[-iters:])) if k else None,
                      "models_still_iterating_at_the_end": int(sum(not r.success and "Maximum" in str(r.message) for r in model.optim_results.values()))}
    elbo_b = {c: list(model.history[c]["ELBO"]) for c in model.groups}
    del model
    # the same 22 fits, one after the other (each on its own plan and state: what 22 VIPRS objects cost)
    per_chrom, sweep_k, same = [], [], True
    for c, sub in gdl.split_by_chromosome().items():
        st = []
        one = one_cls(sub, low_memory=lm, device=device, math_mode=math_mode, **kw)
        one.fit(max_iter=n_it, min_iter=n_it + 1, theta_0=dict(theta), on_iteration=lambda i: st.append(time.perf_counter()))
        dd = np.diff(np.array(st))[warm - 1:]
        per_chrom.append(float(np.median(dd)) * 1e3 if len(dd) else float("nan"))
        kk = next(iter(one._plans.values())).timing_history(which=0)
        sweep_k.append(float(np.mean(kk[-iters:])) if kk else float("nan"))
        same = same and (one.history["ELBO"] == elbo_b[c])
        del one
    out["sequential"] = {"ms_per_round": float(np.sum(per_chrom)), "ms_per_iteration_per_chromosome": [round(x, 4) for x in per_chrom],
                         "sweep_kernel_ms_per_chromosome": [round(x, 4) for x in sweep_k], "sweep_kernels_ms_sum": float(np.sum(sweep_k))}
    out["elbo_trajectories_identical"] = bool(same)          # the batch computes, bit for bit, what the 22 separate fits compute
    if out["batched"]["ms_per_round"]:
        out["speedup_batched_over_sequential"] = out["sequential"]["ms_per_round"] / out["batched"]["ms_per_round"]
    return out


def measure_small_config(args, cfg, device, barrier, steps, cpu_seconds):
    """BASELINE configs[0] / configs[1] (cfg1: one 500-SNP block, "reference Cython CPU e_step (1 thread)"; cfg2: chr22-like,
    19k SNPs / 40 blocks, "1 x MI355X vs OpenMP CPU") on the device -- resident sweep, time model (both are bound by the
    serial chain of their largest block, not by HBM) -- with the CPU baseline of the SAME workload beside it, and the
    PCIe-inclusive one-shot host-buffer call (`cpp_e_step`, never `value`)."""
    sizes = config_sizes(cfg, args.seed)
    ld, ss, inp, _ = build_workload(args, sizes, None, args.seed, True, np.dtype("float32"), data=True)
    sw = Sweep(args, ld, ss, inp, device, "spike_slab", 1, True)
    what = {"cfg1": "configs[0]: single LD block, 500 SNPs", "cfg2": "configs[1]: chr22-like, ~19k SNPs / 40 LD blocks"}[cfg]
    out = measure_secondary(f"{what}, spike-and-slab, upper-triangular fp32 LD (low_memory=True)", sw, steps, barrier, args.math)
    out["config"] = cfg
    out["largest_block"] = int(np.max(sizes))
    sw.close()
    from viprs_amd.vi import e_step_hip as H
    st = inp.state_copy()
    call = lambda: H.cpp_e_step(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, inp.std_beta, st["var_gamma"], st["var_mu"], st["eta"], st["q"],
                                st["eta_diff"], inp.u_logs, inp.sqrt_half_var_tau, inp.mu_mult, ld.dq_scale, 1, True)
    for _ in range(3):
        call()
    ts = []
    for _ in range(20):
        for k, v in inp.state_copy().items():
            st[k][...] = v
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    out["one_shot_host_call"] = {"ms_per_call": float(np.median(ts)) * 1e3, "value": ld.m / float(np.median(ts)), "unit": "SNP-updates/s",
                                 "note": "cpp_e_step drop-in on HOST buffers: 9 vectors up, sweep, 5 vectors down per call (LD resident "
                                         "after the first call): the PCIe-inclusive rate, never `value`"}
    if cpu_seconds > 0:
        cb = cpu_baseline(ld, inp, cpu_seconds, "spike_slab", 1, None, None, args.cpu_threads)
        # configs[0] is worded for ONE thread, configs[1] for the OpenMP path
        cb["headline"] = ({"value": cb["single_thread_value"], "cores": 1, "variant": "1_single_thread"} if cfg == "cfg1" else
                          {"value": cb["value"], "cores": cb["cores"], "variant": "2_openmp_all_threads_racy"})
        out["cpu_baseline"] = cb
        out["gpu_over_cpu"] = {"resident_sweep_over_headline": out["value"] / cb["headline"]["value"],
                               "resident_sweep_over_best_exact": out["value"] / cb["best_exact"]["value"],
                               "one_shot_call_over_headline": out["one_shot_host_call"]["value"] / cb["headline"]["value"]}
    return out


def per_rank(comm, rank, world, x):
    """One scalar per rank -> the vector of all ranks' values, on every rank."""
    v = np.zeros(world)
    v[rank] = float(x)
    return comm.allreduce_sum(v)


def launch_ranks(n, argv):
    """`bench.py --gpus N` without a launcher: start N rank processes of this script (one per GPU) and relay rank 0's
    JSON line.  This parent never imports the HIP library or touches a device (children are fresh interpreters, not
    an exec of a process that holds a GPU context).  Returns the exit status: 0 only if every rank exited 0 and
    rank 0 printed exactly one line."""
    import secrets
    import socket
    import subprocess
    import threading
    with socket.socket() as s:                              # a free port names this launch (nothing listens on it:
        s.bind(("127.0.0.1", 0))                            # the RCCL id travels through files keyed by it)
        port = s.getsockname()[1]
    env = dict(os.environ, WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               VIPRS_RUN_ID=os.environ.get("VIPRS_RUN_ID") or secrets.token_hex(6), HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs, outs = [], [[] for _ in range(n)]

    def pump(r, stream):
        for line in stream:
            if line.startswith("{") and r == 0:
                outs[r].append(line)
            else:                                           # everything else (warnings, tracebacks) goes to stderr
                sys.stderr.write(f"[rank {r}] {line}")

    threads = []
    for r in range(n):
        p = subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv),
                             env=dict(env, RANK=str(r), LOCAL_RANK=str(r), GROUP_RANK="0"),
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, bufsize=1)
        procs.append(p)
        t = threading.Thread(target=pump, args=(r, p.stdout), daemon=True)
        t.start()
        threads.append(t)
    status = 0
    live = set(range(n))
    deadline = time.time() + float(os.environ.get("VIPRS_BENCH_LAUNCH_TIMEOUT", "3600"))
    try:
        while live:
            for r in sorted(live):
                rc = procs[r].poll()
                if rc is None:
                    continue
                live.discard(r)
                if rc != 0 and status == 0:
                    status = rc if rc > 0 else 1
                    sys.stderr.write(f"bench.py: rank {r} exited with status {rc}; stopping the other ranks\n")
                    for q in live:                          # exactly the processes started above
                        procs[q].terminate()
            if live and time.time() > deadline and status == 0:
                status = 124
                sys.stderr.write(f"bench.py: ranks {sorted(live)} still running at the launch timeout; stopping them\n")
                for q in live:
                    procs[q].terminate()
            time.sleep(0.05)
    finally:
        for p in procs:                                     # (interrupted parent: never leave rank processes behind)
            if p.poll() is None:
                p.kill()
    for t in threads:
        t.join(timeout=10)
    if status == 0 and len(outs[0]) != 1:
        sys.stderr.write(f"bench.py: rank 0 printed {len(outs[0])} JSON lines, expected 1\n")
        status = 1
    if status == 0:
        sys.stdout.write(outs[0][0])
        sys.stdout.flush()
    return status


def main():
    args = parse_args()
    n_gpus = args.gpus
    if n_gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if "WORLD_SIZE" not in os.environ and n_gpus > 1:
        # no launcher: be the launcher (before anything loads the HIP library in this process)
        raise SystemExit(launch_ranks(n_gpus, sys.argv[1:]))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != n_gpus:
        # never a line whose n_gpus is not the number of ranks that ran
        raise SystemExit(f"bench.py: --gpus {n_gpus} but WORLD_SIZE={world}: refusing to print a mislabelled line")

    from viprs_amd import _lib
    from viprs_amd.parallel import LocalComm, RcclComm, rank_time_model

    ndev = _lib.device_count()
    if ndev < 1:
        raise SystemExit("bench.py needs a HIP device (the E-step has no CPU fallback)")
    dry = os.environ.get("VIPRS_BENCH_COMM") == "file"     # dry run of the multi-rank logic (ranks may share a device)
    if world > ndev and not dry:
        raise SystemExit(f"bench.py: --gpus {n_gpus} but only {ndev} HIP device(s) visible: one rank per GPU, refusing to "
                         "oversubscribe (VIPRS_BENCH_COMM=file runs the multi-rank logic on fewer devices, labelled as such)")
    device = local_rank % ndev
    shared_device = dry and world > ndev
    if shared_device:
        Sweep.device_lock = os.path.join(os.environ.get("TMPDIR", "/tmp"),
                                         f"viprs_bench_device{device}_{os.environ.get('MASTER_PORT', '0')}.lock")
    comm_kind = "rccl" if world > 1 else "none"
    if world > 1 and os.environ.get("VIPRS_BENCH_COMM") == "file":
        comm_kind = "file transport (VIPRS_BENCH_COMM=file)" + (
            f"; DRY RUN: {world} ranks on {ndev} device(s), sweeps of ranks sharing a device serialised by a file lock -- "
            "times are not multi-GPU times" if shared_device else "")
        from viprs_amd.parallel import FileComm        # dry runs of the multi-rank logic on a box RCCL cannot span
        comm = FileComm(rank, world)
    elif world > 1:
        # RCCL over xGMI through the C ABI (no PyTorch).  Should the communicator not come up on this node, the run
        # still completes over the file transport -- with the barriers' file-system latency inside the timed region,
        # which the JSON line then says (`comm`).
        from viprs_amd.parallel import FileComm
        side = FileComm(rank, world)
        try:
            comm, err = RcclComm(rank, world, device), ""
        except Exception as e:                          # noqa: BLE001 -- any failure leads to the same fallback
            comm, err = None, f"{type(e).__name__}: {e}"
        n_ok = int(round(float(side.allreduce_sum(np.array([1.0 if comm is not None else 0.0]))[0])))
        if n_ok != world:
            if comm is not None:
                comm.close()
            comm = side
            comm_kind = f"file transport (RCCL communicator came up on {n_ok} of {world} ranks; rank {rank}: {err or 'ok'})"
        else:
            side.close()                                # RCCL is up on every rank: the side channel is done
    else:
        comm = LocalComm()
    # the number of ranks the transport itself reports (RCCL: ncclCommCount through viprs_comm_rank)
    comm_ranks = comm.size() if hasattr(comm, "size") else comm.world_size
    if comm_ranks != n_gpus:
        raise SystemExit(f"bench.py: the communicator spans {comm_ranks} ranks, --gpus says {n_gpus}")

    def barrier():
        # every rank: device idle (hipDeviceSynchronize), then all ranks arrived (RCCL collective + stream sync)
        _lib.check(_lib.lib.viprs_device_synchronize(device))
        comm.barrier()

    ld_dtype = np.dtype(args.ld_dtype)
    sizes_all = config_sizes(args.config, args.seed)
    width = args.width or {"spike_slab": 1, "mixture": 4, "grid": 32}[args.model]
    if args.precision != "float32" and args.model != "spike_slab":
        raise SystemExit("--precision float64 is measured for the spike-and-slab model only")

    # ---- primary measurement -----------------------------------------------------------------------------
    t_start = time.perf_counter()
    strong = world > 1 and args.scaling == "strong"
    # LD entries: on the device for every rank of a multi-GPU run; the N = 1 headline workload on the host (the CPU
    # baseline and the fit() secondaries run on the host arrays) unless neither is asked for (plain and profiling runs)
    on_host = world == 1 and (args.host_ld or (args.full and (args.cpu_seconds > 0 or not args.no_secondary)))
    if strong:
        parts = shard_blocks_lpt(sizes_all, world)
        mine = parts[rank]
        ld, ss, inp, m_total = build_workload(args, sizes_all, mine, args.seed, args.low_memory, ld_dtype, data=on_host)
        total_snps = float(m_total)
    else:
        seed = args.seed + 1000 * rank                 # weak: every rank its own genome-scale workload
        ld, ss, inp, _ = build_workload(args, sizes_all, None, seed, args.low_memory, ld_dtype, data=on_host)
        total_snps = float(comm.allreduce_sum(np.array([float(ld.m)]))[0])
    t_built = time.perf_counter()
    sw = Sweep(args, ld, ss, inp, device, args.model, width, args.low_memory, precision=args.precision)
    t_resident = time.perf_counter()
    if args.prewarm_seconds > 0:                          # steady-state clocks before the W warm-up steps (untimed)
        t_pw = time.perf_counter()
        while time.perf_counter() - t_pw < args.prewarm_seconds:
            for _ in range(10):
                sw.step()
            sw.state.synchronize()
    my_elapsed = sw.run(args.steps, args.warmup, barrier)
    if args.dump_outputs:                                 # (before anything else sweeps on this state)
        dump_outputs(args.dump_outputs, {k: sw.state.download(k) for k in OUTPUTS}, DUMP_BUDGET_BYTES // world,
                     f"_rank{rank}" if world > 1 else "")
    elapsed = float(comm.allreduce_max(np.array([my_elapsed]))[0])
    skipped = sw.plan.last_skipped()
    sw_math_effective = sw.plan.effective_math_mode() if hasattr(sw.plan, "effective_math_mode") else None
    k_ms = sw.plan.timing_history(which=1)
    sweep_ms = sw.plan.timing_history(which=0)
    es = ld_dtype.itemsize
    algo_bytes = sw.algorithmic_bytes()                                   # this rank's share
    k_host_ms = sw.plan.timing_history(which=2)
    k_good_ms, k_bad_idx = clean_kernel_times(k_ms, k_host_ms)
    k_avg_ms = float(np.mean(k_good_ms)) if k_ms else float("nan")
    # per-rank kernel time and bytes -> node-level achieved bandwidth = all ranks' bytes / slowest rank's kernel time
    bytes_ranks = per_rank(comm, rank, world, algo_bytes)
    k_ranks = per_rank(comm, rank, world, k_avg_ms)
    model_ranks = per_rank(comm, rank, world, rank_time_model(np.diff(ld.block_start), es) * 1e3)
    snps_ranks = per_rank(comm, rank, world, ld.m)
    blocks_ranks = per_rank(comm, rank, world, len(ld.block_start) - 1)
    largest_ranks = per_rank(comm, rank, world, int(np.max(np.diff(ld.block_start))) if ld.m else 0)
    elapsed_ranks = per_rank(comm, rank, world, my_elapsed)
    k_max_ms = float(np.max(k_ranks))
    achieved = float(bytes_ranks.sum()) / (k_max_ms * 1e-3) / 1e9
    model_ms = float(np.max(model_ranks))

    chain_ns = None
    if args.full and world == 1 and args.model == "spike_slab" and args.precision == "float32" and not args.no_secondary:
        chain_ns = chain_ns_per_snp(args, device, args.math, args.low_memory)     # isolated 6 000-SNP block

    # ---- secondary measurements (--full) ---------------------------------------------------------------------
    secondary = []
    weak = None
    if args.full and not args.no_secondary and args.model == "spike_slab" and args.precision == "float32":
        half = max(5, args.steps // 2)
        if world == 1 and args.low_memory and args.ld_dtype == "float32" and args.config != "cfg1":
            # `value` is the reference's DEFAULT LD form (low_memory=True, VIPRS.py:75: the upper-triangular store, swept over
            # its mirror image on the device); the secondaries: the same workload in the symmetric form, configs[3] / configs[4]
            # in both forms, the published int8 store format, float64 state, math_mode=fast, the EM iteration around the sweep
            cfgk = args.config
            UP = "upper-triangular fp32 LD (low_memory=True, the reference's default form)"
            SY = "symmetric fp32 LD (low_memory=False)"
            ld_s, ss_s, inp_s, _ = build_workload(args, sizes_all, None, args.seed, False, np.dtype("float32"), data=False)
            sw_s = Sweep(args, ld_s, ss_s, inp_s, device, "spike_slab", 1, False)
            secondary.append(measure_secondary(SY + ", spike-and-slab", sw_s, half, barrier, args.math, f"{cfgk}_float32_sym"))
            for model2, w2, nm in (("mixture", 4, "configs[3]: sparse mixture prior K=4"),
                                   ("grid", 32, "configs[4]: grid of 32 (sigma_eps x pi) models batched per SNP")):
                # on the LD plans that are already resident: the primary (upper-triangular) one, then the symmetric one
                sw2 = Sweep(args, ld, ss, inp, device, model2, w2, True, plan=sw.plan)
                secondary.append(measure_secondary(f"{nm}, {UP}", sw2, half, barrier, args.math, f"{cfgk}_float32_upper_{model2}{w2}"))
                sw2.close()
                sw2 = Sweep(args, ld_s, ss_s, inp_s, device, model2, w2, False, plan=sw_s.plan)
                secondary.append(measure_secondary(f"{nm}, {SY}", sw2, half, barrier, args.math, f"{cfgk}_float32_sym_{model2}{w2}"))
                sw2.close()
            if args.math == "exact":
                # math_mode = fast (v_exp_f32 / v_rcp_f32 sigmoid; deviations of the size a one-ulp change of the inputs
                # causes, tests/test_gpu_fast_math.py) on the same plans and inputs: the chain step is what changes
                # (on the plans' own state objects: where the allocator puts a state's arrays moves the sweep by up to 8 % --
                #  EXPERIMENTS.md round 5 -- and the first state of a plan is what a fit uses)
                for nm, sw0, lm0 in ((UP, sw, True), (SY, sw_s, False)):
                    sw0.plan.set_math_mode("fast")
                    secondary.append(measure_secondary(f"math_mode=fast: {nm}, spike-and-slab", sw0, half, barrier, "fast"))
                    sw0.plan.set_math_mode("exact")
                    secondary[-1]["chain_ns_per_snp"] = chain_ns_per_snp(args, device, "fast", lm0)
            sw_s.close()
            del ld_s, sw_s
            # int8 (dq_scale = 1/127): the format of the reference's published LD stores (docs/download_ld.md:6-10)
            nm8 = "upper-triangular int8 LD (low_memory=True + the published store format), spike-and-slab"
            ld_u, ss_u, inp_u, _ = build_workload(args, sizes_all, None, args.seed, True, np.dtype("int8"), data=False)
            sw_u = Sweep(args, ld_u, ss_u, inp_u, device, "spike_slab", 1, True)
            secondary.append(measure_secondary(nm8, sw_u, half, barrier, args.math, f"{cfgk}_int8_upper"))
            # float_precision='float64' (VIPRS.py:72) on the same plan: the panel-walking kernels of estep_tile.h
            sw_d = Sweep(args, ld_u, ss_u, inp_u, device, "spike_slab", 1, True, plan=sw_u.plan, precision="float64")
            secondary.append(measure_secondary("float64 state (float_precision='float64'), upper-triangular int8 LD, spike-and-slab",
                                               sw_d, half, barrier, "exact", f"{cfgk}_int8_upper_f64"))
            secondary[-1]["dtype"] = "f64"
            sw_d.close()
            if args.math == "exact":
                sw_u.plan.set_math_mode("fast")
                secondary.append(measure_secondary("math_mode=fast: " + nm8, sw_u, half, barrier, "fast"))
                sw_u.plan.set_math_mode("exact")
            sw_u.close()
            del ld_u, sw_u
            # the EM iteration around the sweep (VIPRS.py:979-1019): what a user of fit() pays per iteration (default LD form)
            if args.config in ("cfg3", "cfg2"):
                for kind in ("VIPRS", "VIPRSMix(K=4)", "VIPRSGrid(32 models, batched)"):
                    secondary.append(measure_fit_iteration(kind, ld, ss, device, math_mode=args.math))
            if args.config == "cfg3" and args.math == "exact":
                # the published store format (int8, upper-triangular) end to end, exact and math_mode="fast" (inside north_star's
                # 1e-5 where the problem is well conditioned; tests/test_gpu_fast_math.py): fast shortens the chain step, the
                # floor of this format's sweep
                import copy
                ld8 = copy.copy(ld)
                ld8.ld_data = np.rint(ld.ld_data * np.float32(127.0)).astype(np.int8)      # = make_ld(..., ld_dtype=int8), tests/test_synth_device.py
                ld8.dq_scale = 1.0 / 127.0
                for mm in ("exact", "fast"):
                    for kind in ("VIPRS", "VIPRSMix(K=4)", "VIPRSGrid(32 models, batched)"):
                        secondary.append(measure_fit_iteration(kind, ld8, ss, device, math_mode=mm))
                del ld8
            if args.config == "cfg3":
                # the reference's default operating mode: one model per chromosome -- 22 of them in one lock-step batch
                secondary.append(measure_per_chromosome(ld, ss, device, math_mode=args.math))
                secondary.append(measure_per_chromosome(ld, ss, device, math_mode=args.math, mixture_k=4, iters=8))
                # BASELINE configs[0] and configs[1], each with the CPU baseline of its own workload
                for cfg_small, cpu_s in (("cfg1", 2.0), ("cfg2", 6.0)):
                    secondary.append(measure_small_config(args, cfg_small, device, barrier, max(10, args.steps),
                                                          cpu_s if args.cpu_seconds > 0 else 0.0))
        if world > 1:
            # the other scaling figure beside `value`, same run, same ranks
            sw.close()
            if strong:      # weak: every rank sweeps a whole genome-scale workload of its own
                ld_w, ss_w, inp_w, _ = build_workload(args, sizes_all, None, args.seed + 1000 * rank, args.low_memory, ld_dtype,
                                                      data=False)
            else:           # strong: the blocks of ONE workload sharded over the ranks
                ld_w, ss_w, inp_w, m_one = build_workload(args, sizes_all, shard_blocks_lpt(sizes_all, world)[rank], args.seed,
                                                          args.low_memory, ld_dtype, data=False)
            sw_w = Sweep(args, ld_w, ss_w, inp_w, device, args.model, width, args.low_memory)
            my_w = sw_w.run(half, 3, barrier)
            el_w = float(comm.allreduce_max(np.array([my_w]))[0])
            tot_w = float(comm.allreduce_sum(np.array([float(ld_w.m)]))[0])
            kw_ranks = per_rank(comm, rank, world, float(np.mean(sw_w.plan.timing_history(which=1))))
            lb_ranks = per_rank(comm, rank, world, int(np.max(np.diff(ld_w.block_start))) if ld_w.m else 0)
            other = {"value": tot_w * half / el_w, "unit": "SNP-updates/s", "ms_per_step": el_w / half * 1e3,
                     "steps": half, "kernel_ms_avg_per_rank": [float(x) for x in kw_ranks]}
            if strong:
                other.update(metric=f"SNP-updates/sec/E-step, {world} INDEPENDENT 1.1M-SNP / 1700-block workloads, one per GPU "
                                    f"({world} x the work of `value`'s configuration; not BASELINE's metric)",
                             snps_per_gpu=int(ld_w.m), snps_total=int(tot_w),
                             note="every rank sweeps its own genome-scale workload: per-GPU work fixed, no data-path collective")
            else:
                other.update(metric="SNP-updates/sec/E-step (1M SNPs, ~1700 LD blocks), ONE workload block-sharded over the ranks "
                                    "(BASELINE configs[2])",
                             snps_total=int(m_one), largest_block_per_rank=[int(x) for x in lb_ranks],
                             note="the blocks of ONE 1.1 M-SNP workload sharded over the ranks (chain-aware LPT, no data-path "
                                  "collective); see strong_scaling_ceiling")
            weak = other
            sw_w.close()

    if rank == 0:
        traffic, traffic_src = None, None
        if world == 1:
            key = f"{args.config}_{args.ld_dtype}_{'upper' if args.low_memory else 'sym'}"
            if args.model != "spike_slab":
                key += f"_{args.model}{width}"
            if args.precision != "float32":
                key += "_f64"
            if args.math != "exact":
                key += "_fast"
            traffic, traffic_src = pmc_traffic(key)
        ld_name = {"ar1": "AR(1) block LD", "longrange": "long-range non-Toeplitz block LD (every entry matters)"}[args.ld_kind]
        out = {
            "metric": "SNP-updates/sec/E-step (1M SNPs, ~1700 LD blocks)" if (n_gpus == 1 or strong) else
                      f"SNP-updates/sec/E-step, {n_gpus} independent (1M SNPs, ~1700 LD blocks) workloads, one per GPU",
            "value": total_snps * args.steps / elapsed,
            "unit": "SNP-updates/s",
            "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            # the series over N: ONE workload block-sharded over the ranks ("strong", BASELINE configs[2]) unless --scaling weak
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "f32" if args.precision == "float32" else "f64",
            "data": "synthetic",
            "config": {
                "workload": {"cfg1": "configs[0]: single LD block, 500 SNPs",
                             "cfg2": "configs[1]: chr22-like, ~19k SNPs / 40 LD blocks",
                             "cfg3": "configs[2]: genome-wide, ~1.1M SNPs / 1700 LD blocks",
                             "cfg3max": "configs[2] with one 6 000-SNP block (BASELINE's clip limit)"}[args.config]
                            + {"spike_slab": ", spike-and-slab", "mixture": f", sparse mixture prior K={width} (configs[3])",
                               "grid": f", grid of {width} (sigma_eps x pi) models batched per SNP (configs[4])"}[args.model]
                            + ", " + ld_name
                            + (f", ONE workload block-sharded over {n_gpus} GPUs" if strong else
                               (f", {n_gpus} INDEPENDENT workloads, one per GPU ({n_gpus} x the work of BASELINE's configuration)"
                                if n_gpus > 1 else "")),
                "prior": args.model, "prior_width": width,
                "snp_x_grid_point_updates_per_s": total_snps * width * args.steps / elapsed if args.model == "grid" else None,
                "snps_total": int(total_snps), "snps_rank0": int(ld.m), "ld_blocks_rank0": int(len(ld.block_start) - 1),
                "ld_entries_rank0": int(ld.ld_indptr[-1]), "ld_dtype": args.ld_dtype, "ld_kind": args.ld_kind,
                "largest_block": int(np.max(sizes_all)),
                "ld_form": "upper-triangular (low_memory=True)" if ld.low_memory else "symmetric (low_memory=False)",
                "primary": "`value` is the " + ("upper-triangular LD form -- what VIPRS() runs by default (low_memory=True, VIPRS.py:75); "
                                                "the symmetric form is the FIRST entry of `secondary`" if ld.low_memory else
                                                "symmetric LD form (--symmetric); the reference's default is low_memory=True"),
                "math_mode": args.math, "math_mode_effective": sw_math_effective, "skipped_snps_last_sweep_rank0": int(skipped),
                "comm": comm_kind, "rccl_ranks": int(comm_ranks) if comm_kind == "rccl" else None,
                "ranks": int(comm_ranks),
                "parallelism": (f"ld-blocks x{n_gpus} (strong: chain-aware LPT, no data-path collective; RCCL barrier / max only)"
                                if strong else f"one workload per GPU x{n_gpus}") if n_gpus > 1 else "single GPU",
                "step": "device state re-init + one E-step sweep over all blocks",
                "prewarm_s": args.prewarm_seconds,        # untimed sweeps before the W warm-up steps (steady-state clocks)
                "full": bool(args.full),                  # secondaries, chain-step probe and CPU baseline were measured
                # where the state's per-SNP arrays were put: best of n allocations by a probe sweep (viprs_amd/plan.py)
                "state_placement": getattr(sw.state, "placement", None),
                "time_model_ms": model_ms,
                "chain_ns_per_snp": chain_ns if world == 1 else None,
                "secondary": secondary or None,
            },
            "roofline": {
                "bound": "hbm",
                "kernel": ("estep_grid_mfma_kernel (one workgroup per LD block, LD read once for all models)"
                           + ("; upper-triangular form: the second pass runs inside it, over the mirrored blocks" if ld.low_memory else "")) if args.model == "grid" else
                          ("estep_tile_f64_kernel (float64 state: one workgroup per LD block, two block-size classes on two "
                           "streams" + (" + tile_f64_second_pass_exact_kernel" if ld.low_memory else "") + ")")
                          if args.precision == "float64" else
                          ("estep_sweep_kernel (ONE launch per sweep: team workgroups for the large LD blocks, small-block workers "
                           "behind them" + ("; upper-triangular form: the dense blocks hold the mirrored upper triangle and the second "
                                            "pass runs inside the sweep as strip updates into per-row sums" if ld.low_memory else "") + ")"),
                "achieved": achieved, "peak": HBM_PEAK_GBS * n_gpus, "unit": "GB/s", "frac": achieved / (HBM_PEAK_GBS * n_gpus),
                "traffic": traffic, "traffic_source": traffic_src, "algorithmic_bytes_per_launch": int(bytes_ranks.sum()),
                "kernel_ms_avg": k_max_ms, "kernel_ms_p10": pct(k_ms, 10), "kernel_ms_p50": pct(k_ms, 50),
                "kernel_ms_p90": pct(k_ms, 90), "kernel_ms_max": float(np.max(k_ms)) if k_ms else None,
                "sweep_ms_avg": float(np.mean(sweep_ms)) if sweep_ms else None,
                "kernel_ms_avg_raw": float(np.mean(k_ms)) if k_ms else None, "kernel_ms_all": [round(float(x), 4) for x in k_ms],
                "host_ms_inside_the_bracket_all": [round(float(x), 4) for x in k_host_ms],
                "sweeps_with_host_time_inside_the_bracket": k_bad_idx,
                "note": "achieved = algorithmic bytes of all ranks / slowest rank's mean kernel time (HIP events on the "
                        "kernels' own streams; a sweep whose event bracket holds > 0.1 ms of HOST time -- stamped by the library, "
                        "`host_ms_inside_the_bracket_all` -- is left out of the mean and listed); percentiles are rank 0's "
                        "per-sweep kernel times",
            },
        }
        # what `value` is, versioned: rounds 1-4 quoted the symmetric form and weak scaling; since round 5 the reference's default
        # LD form, strong scaling and the best-of-n state placement (`symmetric_ld_form` / `weak_scaling` keep the old figures)
        out["metric_definition"] = {"version": 2, "since": "round 5",
                                    "ld_form": "upper-triangular (low_memory=True)" if ld.low_memory else "symmetric (low_memory=False)",
                                    "scaling": args.scaling, "state_placement": "probe (best of n allocations)" if getattr(sw.state, "placement", None) else "first allocation",
                                    "version_1": "rounds 1-4: symmetric LD form, weak scaling for N > 1, first allocation"}
        # which LD form `value` is, at the top level too (the reference's default is low_memory=True, VIPRS.py:75)
        out["default_ld_form"] = {"ld_form": "upper-triangular (low_memory=True, the reference's default)",
                                  "is_value": bool(ld.low_memory),
                                  "note": "`value` IS this form" if ld.low_memory else "`value` is the symmetric form (--symmetric)"}
        if ld.low_memory and secondary and str(secondary[0].get("name", "")).startswith("symmetric fp32"):
            d0 = secondary[0]
            out["symmetric_ld_form"] = {"value": d0["value"], "unit": d0["unit"], "ms_per_step": d0["ms_per_step"],
                                        "kernel_ms_avg": d0["kernel_ms_avg"], "roofline_frac": d0["roofline_frac"],
                                        "note": "the same workload with low_memory=False; details: config.secondary[0]"}
        if n_gpus > 1:
            # self-diagnosing multi-GPU line: what every rank held and how long its kernel took, next to the model
            out["per_rank"] = {
                "snps": [int(x) for x in snps_ranks], "ld_blocks": [int(x) for x in blocks_ranks],
                "largest_block": [int(x) for x in largest_ranks],
                "algorithmic_bytes": [int(x) for x in bytes_ranks],
                "kernel_ms_avg": [float(x) for x in k_ranks], "time_model_ms": [float(x) for x in model_ranks],
                "wall_ms_per_step": [float(x) / args.steps * 1e3 for x in elapsed_ranks],
            }
            # what bounds the strong figure: no rank finishes before the serial Gauss-Seidel chain of its largest LD block
            # (e_step.hpp:387-431 is sequential within a block), whatever N; one GPU needs `one_gpu_model_ms` for everything
            from viprs_amd.parallel import CHAIN_STEP_S
            one_gpu_ms = rank_time_model(sizes_all, es) * 1e3
            floor_ms = float(np.max(sizes_all)) * CHAIN_STEP_S * 1e3
            out["strong_scaling_ceiling"] = {
                "largest_block_snps": int(np.max(sizes_all)), "chain_ns_per_snp_model": CHAIN_STEP_S * 1e9,
                "largest_block_chain_ms": floor_ms, "one_gpu_model_ms": one_gpu_ms,
                "max_speedup_over_one_gpu": one_gpu_ms / floor_ms,
                "note": "ONE 1.1M-SNP workload is ~0.7 ms of work for one GPU; sharded over N GPUs no rank can finish before the "
                        "serial chain of its largest LD block, so the strong figure saturates at max_speedup_over_one_gpu for any "
                        "N >= 2 (per_rank.kernel_ms_avg ~ largest_block_chain_ms on the rank holding that block = at the physical "
                        "limit, not a scheduling defect).  `weak_scaling` is the figure that grows with N.",
            }
            # (also under `config`, next to the workload it qualifies)
            out["config"]["strong_scaling_ceiling"] = out["strong_scaling_ceiling"]
            out["config"]["per_rank_projection"] = {
                "time_model_ms": [float(x) for x in model_ranks], "slowest_rank_time_model_ms": model_ms,
                "projected_value": total_snps / (model_ms * 1e-3),
                "note": "every rank's sweep time model (max of its HBM stream, its largest block's chain and its chain throughput); "
                        "no multi-GPU hardware curve exists for this build: the per-rank kernel times are what was measured"}
            out["startup_s_rank0"] = {"workload_built": t_built - t_start, "ld_resident": t_resident - t_built,
                                      "ld_entries": "generated on the device" if ld.ld_data is None else "built on the host, uploaded"}
        if weak is not None:
            out["weak_scaling" if strong else "strong_scaling"] = weak
        if args.full and n_gpus == 1 and args.cpu_seconds > 0 and args.precision == "float32":
            out["cpu_baseline"] = cpu_baseline(ld, inp, args.cpu_seconds, args.model, width, sw.host_extra, sw.pi0,
                                               args.cpu_threads)
        print(json.dumps(out), flush=True)

    comm.barrier()
    if world > 1:
        comm.close()


if __name__ == "__main__":
    main()
