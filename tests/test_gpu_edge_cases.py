"""GPU: edge cases of the drop-in boundary and full-size properties (BASELINE.json sizes)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H
from viprs_amd.utils import synthetic as syn

pytestmark = pytest.mark.gpu


def test_empty_chromosome(gpu):
    from viprs_amd.vi import e_step_hip as S
    z = lambda: np.zeros(0, np.float32)
    S.cpp_e_step(np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.float32), z(), z(), z(), z(), z(), z(),
                 z(), z(), z(), 1.0, 1, False)


@pytest.mark.parametrize("low_memory", [False, True])
def test_singleton_blocks_and_int32_indptr(gpu, low_memory):
    ld, ss, inp = syn.make_problem(sizes=[1] * 70 + [3, 1, 2], low_memory=low_memory, seed=5, indptr_dtype=np.int32)
    st0 = inp.state_copy()
    ref = H.run_oracle(ld, inp, st0, sweeps=2)
    got = H.run_hip(ld, inp, st0, sweeps=2)
    H.assert_state_close(got, ref)


@pytest.mark.parametrize("ld_dtype", [np.float32, np.int8])
@pytest.mark.parametrize("low_memory", [False, True])
def test_team_blocks_bit_exact(gpu, ld_dtype, low_memory):
    """Blocks large enough for the multi-CU team kernels (>= 1280 and >= 2304 SNPs)."""
    ld, ss, inp = syn.make_problem(sizes=[2500, 1300, 1290, 4100], low_memory=low_memory, ld_dtype=ld_dtype, seed=9)
    st0 = inp.state_copy()
    ref = H.run_oracle(ld, inp, st0, sweeps=2)
    got = H.run_hip(ld, inp, st0, sweeps=2)
    H.assert_state_close(got, ref)
    H.assert_state_equal(got, ref)     # bit-for-bit in both LD forms


def test_fast_math_mode_within_tolerance(gpu):
    from viprs_amd.vi import e_step_hip as S
    ld, ss, inp = syn.make_problem(sizes=[700, 300], low_memory=False, seed=12)
    st0 = inp.state_copy()
    ref = H.run_oracle(ld, inp, st0, sweeps=1)
    S.set_default_math_mode("fast")
    try:
        got = H.run_hip(ld, inp, st0, sweeps=1)
    finally:
        S.set_default_math_mode("exact")
    # the hardware-transcendental sigmoid may flip the skip branch for SNPs whose |eta_diff| sits within
    # rounding of the threshold; everything else stays inside the 1e-5 relative tolerance
    H.assert_state_close(got, ref, rtol=1e-5, max_flips=3)


def test_float64_state_and_exotic_ld_dtypes(gpu):
    for ld_dtype, T in ((np.float32, np.float64), (np.float64, np.float64)):
        ld, ss, inp = syn.make_problem(sizes=[90, 140], low_memory=False, ld_dtype=ld_dtype, seed=3, float_precision=T)
        st0 = inp.state_copy()
        ref = H.run_oracle(ld, inp, st0, sweeps=2)
        got = H.run_hip(ld, inp, st0, sweeps=2)
        H.assert_state_close(got, ref, rtol=1e-11)
    # fp32 state on LD element types the panel kernels do not specialise (row-by-row kernels): still bit for bit
    for ld_dtype in (np.int32, np.int64, np.float64):
        for low_memory in (False, True):
            ld, ss, inp = syn.make_problem(sizes=[90, 700, 140], low_memory=low_memory, ld_dtype=ld_dtype, seed=3, kind="longrange")
            st0 = inp.state_copy()
            H.assert_state_equal(H.run_hip(ld, inp, st0, sweeps=2), H.run_oracle(ld, inp, st0, sweeps=2))


def test_low_memory_mismatch_and_threads_are_handled(gpu):
    from viprs_amd.plan import LDPlan
    ld, ss, inp = syn.make_problem(sizes=[64], low_memory=False, seed=2)
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, False)
    st = inp.state_copy()
    with pytest.raises(ValueError, match="low_memory"):
        plan.e_step(inp.std_beta, st["var_gamma"], st["var_mu"], st["eta"], st["q"], st["eta_diff"], inp.u_logs,
                    inp.sqrt_half_var_tau, inp.mu_mult, 1.0, threads=1, low_memory=True)
    a, b = inp.state_copy(), inp.state_copy()
    for st, thr in ((a, 1), (b, 8)):     # `threads` is accepted and ignored: always the serial semantics
        plan.e_step(inp.std_beta, st["var_gamma"], st["var_mu"], st["eta"], st["q"], st["eta_diff"], inp.u_logs,
                    inp.sqrt_half_var_tau, inp.mu_mult, 1.0, threads=thr)
    H.assert_state_equal(a, b)
    plan.close()


@pytest.mark.parametrize("kind", ["longrange", "sample", "ar1"])
def test_cfg2_full_size_against_oracle(gpu, kind):
    """BASELINE configs[1]: chr22-like, ~19k SNPs / 40 LD blocks, symmetric and upper forms, three sweeps, `==`.
    On LD whose far field matters (long-range non-Toeplitz blocks; sample correlations of simulated genotypes) -- the
    oracle first proves that cutting every entry more than 128 columns off the diagonal changes the result; the AR(1)
    case (blind beyond ~128 columns, the data of rounds 1-2) stays as the third parameter."""
    for low_memory in (False, True):
        ld, ss, inp = syn.make_problem("cfg2", low_memory=low_memory, kind=kind)
        st0 = inp.state_copy()
        ref = H.run_oracle(ld, inp, st0, sweeps=3)
        if kind != "ar1":
            cut = H.run_oracle(H.cut_far_field(ld, 128), inp, st0, sweeps=1)
            one = H.run_oracle(ld, inp, st0, sweeps=1)
            assert int((cut["q"] != one["q"]).sum()) > ld.m // 2, "far field does not matter for this input"
        got = H.run_hip(ld, inp, st0, sweeps=3)
        H.assert_state_close(got, ref)
        H.assert_state_equal(got, ref)     # bit-for-bit in both LD forms


def test_cfg3_full_size_properties(gpu):
    """BASELINE configs[2] (1.1 M SNPs, 1 700 blocks): size-independent properties of one sweep from
    q = eta = 0 -- q == (R - I) eta per block (closed form), run-to-run bit reproducibility, and the
    oracle on a sample of blocks (largest, smallest, a few in between)."""
    from viprs_amd.plan import DeviceState, LDPlan
    ld, ss, inp = syn.make_problem("cfg3", low_memory=False)
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, False)
    state = DeviceState(plan)
    for n in ("std_beta", "u_logs", "sqrt_half_var_tau", "mu_mult"):
        state.upload(n, getattr(inp, n))
    outs = []
    for _ in range(2):
        state.reset(inp.pi)
        state.e_step(ld.dq_scale)
        outs.append({k: state.download(k) for k in H.STATE})
    H.assert_state_equal(outs[0], outs[1])                       # race-free by construction
    got = outs[0]
    assert plan.last_skipped() == int((got["eta_diff"] == 0).sum())
    sizes = np.diff(ld.block_start)
    order = np.argsort(sizes)
    sample = list(order[:3]) + list(order[-3:]) + list(order[len(order) // 2 - 2: len(order) // 2 + 2])
    for bi in sample:
        s, e = int(ld.block_start[bi]), int(ld.block_start[bi + 1])
        b = e - s
        off = int(ld.ld_indptr[s])
        R = ld.ld_data[off:off + b * b].reshape(b, b).astype(np.float64)
        q = (R - np.eye(b)) @ got["eta"][s:e].astype(np.float64)
        np.testing.assert_allclose(got["q"][s:e], q, rtol=5e-4, atol=5e-6)
        # the same block alone through the oracle: bit-identical
        sub = syn.SyntheticLD(np.zeros(b, np.int32), np.arange(0, b * b + 1, b, dtype=np.int64),
                              ld.ld_data[off:off + b * b], np.array([0, b]), ld.rho[bi:bi + 1], False, 1.0)
        st = {k: v[s:e].copy() for k, v in inp.state_copy().items()}
        O.cpp_e_step(sub.ld_left_bound, sub.ld_indptr, sub.ld_data, inp.std_beta[s:e].copy(), st["var_gamma"],
                     st["var_mu"], st["eta"], st["q"], st["eta_diff"], inp.u_logs[s:e].copy(),
                     inp.sqrt_half_var_tau[s:e].copy(), inp.mu_mult[s:e].copy(), 1.0, 1, False)
        for k in H.STATE:
            assert np.array_equal(got[k][s:e], st[k]), (k, int(bi), b)
    plan.close()


def test_device_prep_and_sums_match_host_formulas(gpu):
    """viprs_state_prep / viprs_state_sums (device-resident EM iteration) against the NumPy statements
    of VIPRS.py:400-418, :896, :426-471, :497-581 used by the host path."""
    from viprs_amd.plan import DeviceState, LDPlan
    ld, ss, inp = syn.make_problem(sizes=[300, 1400, 77], low_memory=False, seed=4)
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, False)
    st = DeviceState(plan)
    st.upload("std_beta", inp.std_beta)
    st.set_n_per_snp(ss.n_per_snp)
    pi, sig, tau, lam = np.float32(0.013), np.float32(0.77), 123.4, np.float32(0.01)
    logit = float(np.log(pi) - np.log(1.0 - pi))
    st.reset(float(pi))
    st.prep(logit, float(np.log(tau)), sig, tau, 1.0 + lam)
    var_tau = ss.n_per_snp * (1.0 + lam) / sig + tau
    np.testing.assert_array_equal(st.download("mu_mult"), (ss.n_per_snp / (var_tau * sig)).astype(np.float32))
    np.testing.assert_allclose(st.download("u_logs"),
                               (np.log(pi) - np.log(1.0 - pi) + 0.5 * (np.log(tau) - np.log(var_tau))).astype(np.float32),
                               rtol=1.2e-7)
    np.testing.assert_array_equal(st.download("sqrt_half_var_tau"), np.sqrt(0.5 * var_tau).astype(np.float32))
    st.e_step(ld.dq_scale)
    v = st.sums(1.0 + lam)
    g, mu, eta, q, ed = (st.download(k).astype(np.float64) for k in ("var_gamma", "var_mu", "eta", "q", "eta_diff"))
    zeta = g * (mu ** 2 + 1.0 / var_tau)
    gc, ng = np.clip(g, 1e-15, 1 - 1e-15), np.clip(1 - g, 1e-15, 1 - 1e-15)
    want = [g.sum(), zeta.sum(), ((1.0 + lam) * zeta + (q.astype(np.float32) * eta.astype(np.float32))).sum(),
            (inp.std_beta.astype(np.float64) * eta).sum(), (eta ** 2).sum(), (gc * np.log(gc)).sum(),
            (ng * np.log(ng)).sum(), gc.sum(), ng.sum(), (gc * np.log(var_tau)).sum(), np.abs(ed).max()]
    np.testing.assert_allclose(v, want, rtol=1e-12, atol=1e-300)
    v2 = st.sums(1.0 + lam)
    assert np.array_equal(v, v2)                                  # fixed-order reduction: reproducible
    plan.close()


def test_device_resident_fit_equals_host_mirrored_fit(gpu):
    from viprs_amd.data import ArrayDataLoader
    from viprs_amd.model import VIPRS
    gdl = ArrayDataLoader.synthetic({21: [210, 330], 22: [1300, 64]}, seed=77)
    runs = []
    for resident in (True, False):
        m = VIPRS(gdl, low_memory=True, device_resident=resident)
        m.fit(max_iter=40, theta_0={"pi": 0.01, "sigma_epsilon": 0.8})
        runs.append(m)
    a, b = runs
    assert a.optim_result.nit == b.optim_result.nit and a.optim_result.message == b.optim_result.message
    np.testing.assert_allclose(a.history["ELBO"], b.history["ELBO"], rtol=1e-7, atol=0.02)
    for c in a.chromosomes:
        np.testing.assert_allclose(a.pip[c], b.pip[c], rtol=1e-3, atol=1e-6)
        np.testing.assert_allclose(a.post_mean_beta[c], b.post_mean_beta[c], rtol=1e-3, atol=1e-7)
    # the resident run above keeps both chromosomes in ONE device plan; one plan per chromosome must agree
    assert a._merged and set(a._dstate) == {"*"}
    u = VIPRS(gdl, low_memory=True, device_resident=True, merge_chromosomes=False)
    u.fit(max_iter=40, theta_0={"pi": 0.01, "sigma_epsilon": 0.8})
    assert not u._merged and u.optim_result.nit == a.optim_result.nit
    np.testing.assert_allclose(a.history["ELBO"], u.history["ELBO"], rtol=1e-9, atol=1e-4)
    for c in a.chromosomes:
        np.testing.assert_allclose(a.pip[c], u.pip[c], rtol=1e-4, atol=1e-7)
        np.testing.assert_allclose(a.q[c], u.q[c], rtol=1e-4, atol=1e-7)


def test_team_handoffs_are_reproducible_under_repetition(gpu):
    """Stress the multi-CU hand-offs: many back-to-back sweeps over team-sized blocks of different
    sizes (different phase counts, so the teams drift against each other), every result bit-identical
    to the first and to the oracle."""
    from viprs_amd.plan import DeviceState, LDPlan
    sizes = [4100, 2400, 2310, 1900, 1500, 1300, 1281, 3000] + [90] * 40
    ld, ss, inp = syn.make_problem(sizes=sizes, low_memory=False, seed=19)
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, False)
    state = DeviceState(plan)
    for n in ("std_beta", "u_logs", "sqrt_half_var_tau", "mu_mult"):
        state.upload(n, getattr(inp, n))
    first = None
    for it in range(25):
        state.reset(inp.pi)
        state.e_step(ld.dq_scale, sync=False)
        state.e_step(ld.dq_scale, sync=False)          # second sweep from the first one's state
        out = {k: state.download(k) for k in H.STATE}
        if first is None:
            first = out
            ref = H.run_oracle(ld, inp, inp.state_copy(), sweeps=2)
            H.assert_state_equal(out, ref)
        else:
            H.assert_state_equal(out, first)
    plan.close()


def test_one_shot_call_rate_is_reported(gpu, capsys):
    """PCIe-inclusive rate of the reference-style call (9 vectors up, 5 down per call); printed for
    DESIGN.md, asserted only loosely."""
    import time
    from viprs_amd.vi import e_step_hip as S
    ld, ss, inp = syn.make_problem("cfg2", low_memory=False)
    st = inp.state_copy()
    args = lambda: (ld.ld_left_bound, ld.ld_indptr, ld.ld_data, inp.std_beta, st["var_gamma"], st["var_mu"], st["eta"],
                    st["q"], st["eta_diff"], inp.u_logs, inp.sqrt_half_var_tau, inp.mu_mult, ld.dq_scale, 1, False)
    S.cpp_e_step(*args())
    t0 = time.perf_counter()
    for _ in range(20):
        S.cpp_e_step(*args())
    dt = (time.perf_counter() - t0) / 20
    with capsys.disabled():
        print(f"[one-shot cpp_e_step, cfg2 {ld.m} SNPs] {dt * 1e3:.3f} ms per call = {ld.m / dt / 1e6:.1f} M SNP-updates/s")
    assert dt < 1.0


def _block_sample(ld, n_small=2, n_large=2, n_mid=2):
    sizes = np.diff(ld.block_start)
    order = np.argsort(sizes)
    mid = len(order) // 2
    return list(order[:n_small]) + list(order[-n_large:]) + list(order[mid - n_mid // 2: mid + (n_mid + 1) // 2])


def _sub_block(ld, bi):
    s, e = int(ld.block_start[bi]), int(ld.block_start[bi + 1])
    b = e - s
    off = int(ld.ld_indptr[s])
    sub = syn.SyntheticLD(np.zeros(b, np.int32), np.arange(0, b * b + 1, b, dtype=np.int64),
                          ld.ld_data[off:off + b * b], np.array([0, b]), ld.rho[bi:bi + 1], False, 1.0)
    return s, e, b, off, sub


def test_cfg3_mixture_full_size_properties(gpu):
    """BASELINE configs[3] (genome-wide, K = 4 sparse mixture): run-to-run bit reproducibility,
    q == (R - I) eta per block, and the oracle on a sample of blocks (bit-identical)."""
    from viprs_amd.plan import DeviceState, LDPlan
    K = 4
    ld, ss, inp = syn.make_problem("cfg3", low_memory=False)
    x = syn.make_mixture_inputs(ss, K)
    pi0 = x.pop("pi")
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, False)
    state = DeviceState(plan, "float32", "mixture", K)
    state.upload("std_beta", inp.std_beta)
    for n, a in x.items():
        state.upload(n, a)
    outs = []
    for _ in range(2):
        state.reset(pi0)
        state.e_step(ld.dq_scale)
        outs.append({k: state.download(k) for k in H.STATE})
    H.assert_state_equal(outs[0], outs[1])
    got = outs[0]
    assert np.all(np.isfinite(got["var_mu"])) and np.all(got["var_gamma"] >= 0)
    assert np.all(got["var_gamma"].sum(axis=1) <= 1.0 + 1e-6)
    for bi in _block_sample(ld):
        s, e, b, off, sub = _sub_block(ld, bi)
        R = ld.ld_data[off:off + b * b].reshape(b, b).astype(np.float64)
        np.testing.assert_allclose(got["q"][s:e], (R - np.eye(b)) @ got["eta"][s:e].astype(np.float64),
                                   rtol=5e-4, atol=5e-6)
        vg = np.full((b, K), pi0, dtype=np.float32)
        vm = np.zeros((b, K), dtype=np.float32)
        eta, q, ed = (np.zeros(b, dtype=np.float32) for _ in range(3))
        O.cpp_e_step_mixture(sub.ld_left_bound, sub.ld_indptr, sub.ld_data, inp.std_beta[s:e].copy(), vg, vm, eta, q,
                             ed, x["log_null_pi"][s:e].copy(), x["u_logs"][s:e].copy(),
                             x["sqrt_half_var_tau"][s:e].copy(), x["mu_mult"][s:e].copy(), 1.0, 1, False)
        ref = dict(var_gamma=vg, var_mu=vm, eta=eta, q=q, eta_diff=ed)
        for k in H.STATE:
            assert np.array_equal(got[k][s:e], ref[k]), (k, int(bi), b)
    plan.close()


def test_cfg3_grid_full_size_properties(gpu):
    """BASELINE configs[4] (genome-wide, 32 grid models batched on the matrix cores): run-to-run bit
    reproducibility, untouched inactive columns, q == (R - I) eta per block and model, the item
    schedule on the same inputs (bit-identical) and the oracle on a sample of blocks (bit-identical)."""
    import os
    from viprs_amd.plan import DeviceState, LDPlan
    G = 32
    ld, ss, inp = syn.make_problem("cfg3", low_memory=False)
    x = syn.make_grid_inputs(ss, G)
    pi0 = x.pop("pi")
    active = np.array([g for g in range(G) if g not in (3, 17)], dtype=np.int32)      # 30 of 32 models
    results = {}
    for mode in ("1", "0"):
        os.environ["VIPRS_GRID_MFMA"] = mode
        try:
            plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, False)
        finally:
            os.environ.pop("VIPRS_GRID_MFMA", None)
        state = DeviceState(plan, "float32", "grid", G)
        state.upload("std_beta", inp.std_beta)
        for n, a in x.items():
            state.upload(n, a)
        outs = []
        for _ in range(2 if mode == "1" else 1):
            state.reset(pi0)
            state.e_step(ld.dq_scale, active)
            outs.append({k: state.download(k) for k in H.STATE})
        if mode == "1":
            H.assert_state_equal(outs[0], outs[1])
        results[mode] = outs[0]
        plan.close()
    got = results["1"]
    H.assert_state_equal(got, results["0"])
    for g in (3, 17):
        assert np.all(got["eta"][:, g] == 0) and np.all(got["q"][:, g] == 0) and np.all(got["var_gamma"][:, g] == np.float32(pi0))
    for bi in _block_sample(ld, 2, 1, 2):
        s, e, b, off, sub = _sub_block(ld, bi)
        R = ld.ld_data[off:off + b * b].reshape(b, b).astype(np.float64)
        for g in (0, 31):
            np.testing.assert_allclose(got["q"][s:e, g], (R - np.eye(b)) @ got["eta"][s:e, g].astype(np.float64),
                                       rtol=5e-4, atol=5e-6)
        mk = lambda v: np.asfortranarray(v)
        vg = mk(np.full((b, G), pi0, dtype=np.float32))
        vm, eta, q, ed = (mk(np.zeros((b, G), dtype=np.float32)) for _ in range(4))
        O.cpp_e_step_grid(sub.ld_left_bound, sub.ld_indptr, sub.ld_data, inp.std_beta[s:e].copy(), vg, vm, eta, q, ed,
                          mk(x["u_logs"][s:e]), mk(x["half_var_tau"][s:e]), mk(x["mu_mult"][s:e]), 1.0, active, 1, False)
        ref = dict(var_gamma=vg, var_mu=vm, eta=eta, q=q, eta_diff=ed)
        for k in H.STATE:
            assert np.array_equal(got[k][s:e], ref[k]), (k, int(bi), b)


def test_device_resident_mixture_fit_equals_host_mirrored_fit(gpu):
    """VIPRSMix: the whole EM iteration on the device (prep_mixture / sums_mixture kernels, chromosomes merged
    into one plan) against the host-mirrored iteration."""
    from viprs_amd.data import ArrayDataLoader
    from viprs_amd.model import VIPRSMix
    gdl = ArrayDataLoader.synthetic({21: [210, 330], 22: [1300, 64]}, seed=78)
    runs = []
    for resident in (True, False):
        m = VIPRSMix(gdl, K=4, low_memory=True, device_resident=resident)
        m.fit(max_iter=12, min_iter=12, theta_0={"pis": np.array([0.008, 0.006, 0.004, 0.002]), "sigma_epsilon": 0.8})
        runs.append(m)
    a, b = runs
    assert a._resident and a._merged and not b._resident
    # (device sums are float64; the host path follows the reference's float32 row-order sums: the
    #  trajectories agree to ~1e-6 per iteration, compared here over the first 12 iterations)
    assert len(a.history["ELBO"]) == len(b.history["ELBO"]) >= 12
    np.testing.assert_allclose(a.history["ELBO"], b.history["ELBO"], rtol=2e-6, atol=0.05)
    np.testing.assert_allclose(np.asarray(a.pi, dtype=np.float64), np.asarray(b.pi, dtype=np.float64), rtol=2e-3)
    np.testing.assert_allclose(np.asarray(a.tau_beta), np.asarray(b.tau_beta), rtol=2e-3)
    np.testing.assert_allclose(float(a.sigma_epsilon), float(b.sigma_epsilon), rtol=1e-5)
    for c in a.chromosomes:
        np.testing.assert_allclose(a.pip[c], b.pip[c], rtol=5e-3, atol=2e-6)
        np.testing.assert_allclose(a.post_mean_beta[c], b.post_mean_beta[c], rtol=5e-3, atol=2e-7)


def test_device_resident_entry_points_reject_misuse(gpu):
    """Error behaviour of the device-resident EM entry points: wrong model kind, missing set-up calls,
    bad column indices, `end` without `begin` -- every misuse is a Python exception, never a crash."""
    from viprs_amd._lib import ViprsHipError
    bad = (ValueError, ViprsHipError)          # VIPRS_EINVAL -> ValueError, everything else -> ViprsHipError
    from viprs_amd.plan import DeviceState, LDPlan
    ld, ss, inp = syn.make_problem(sizes=[100, 70], low_memory=False, seed=3)
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, False)
    ss_state = DeviceState(plan)
    mix = DeviceState(plan, "float32", "mixture", 4)
    grid = DeviceState(plan, "float32", "grid", 6)
    with pytest.raises(bad):
        ss_state.prep_mixture(np.zeros(1), np.zeros(1), np.ones(1), -0.1, 0.8, 1.0)      # not a mixture state
    with pytest.raises(bad):
        mix.prep_mixture(np.zeros(4), np.zeros(4), np.ones(4), -0.1, 0.8, 1.0)           # n_per_snp not set
    with pytest.raises(bad):
        mix.sums_mixture_end()                                                           # nothing in flight
    mix.set_n_per_snp(ss.n_per_snp)
    mix.prep_mixture(np.zeros(4), np.zeros(4), np.ones(4), -0.1, 0.8, 1.0)
    with pytest.raises(bad):
        mix.sums_mixture_begin(1.0)                                                      # log_var_tau not set
    with pytest.raises(bad):
        ss_state.sums_end()                                                              # nothing in flight
    with pytest.raises(bad):
        grid.prep_columns(np.array([[0, 0.0, 0.0, 0.8, 1.0, 1.0]]))                      # n_per_snp not set
    grid.set_n_per_snp(ss.n_per_snp)
    with pytest.raises(bad):
        grid.prep_columns(np.array([[6, 0.0, 0.0, 0.8, 1.0, 1.0]]))                      # column out of range
    with pytest.raises(bad):
        grid.sums_columns_begin([0, 1], 1.0)                                             # prep not called
    grid.prep_columns(np.array([[g, -4.0, 9.0, 0.8, 8000.0, 1.0] for g in range(6)]))
    grid.sums_columns_begin([5, 0], 1.0)
    out = grid.sums_columns_end()
    assert out.shape == (2, 11) and np.all(np.isfinite(out))
    with pytest.raises(bad):
        grid.sums_columns_end()                                                          # already collected
    with pytest.raises(ValueError):
        ss_state.set_snp_weights(np.ones(3))                                             # wrong length
    plan.close()


def test_dense_block_beyond_the_lds_limit(gpu):
    """A dense block whose q does not fit the panel kernels' LDS (> ~13 000 SNPs) is scheduled like a
    windowed component instead of failing: same bits as the oracle."""
    ld, ss, inp = syn.make_problem(sizes=[30500, 70], low_memory=True, ld_dtype=np.int8, seed=17)
    st0 = inp.state_copy()
    H.assert_state_equal(H.run_hip(ld, inp, st0, sweeps=1), H.run_oracle(ld, inp, st0, sweeps=1))


@pytest.mark.parametrize("low_memory", [False, True])
def test_dense_block_at_the_lds_limit(gpu, low_memory):
    """The largest block the panel kernels take (13 184 SNPs: q -- and, in the upper-triangular form, the second-pass
    sums -- of the whole block in LDS next to the tiles, 160 KB, one workgroup per CU) and the first size beyond it
    (windowed-component schedule): same bits as the oracle on far-field-sensitive LD."""
    for size in (13184, 13248):
        ld, ss, inp = syn.make_problem(sizes=[size, 130], low_memory=low_memory, ld_dtype=np.int8, seed=19, kind="longrange")
        st0 = inp.state_copy()
        H.assert_state_equal(H.run_hip(ld, inp, st0, sweeps=1), H.run_oracle(ld, inp, st0, sweeps=1))


def test_in_place_edit_of_ld_data_is_noticed_by_the_drop_in_call(gpu):
    """e_step_cpp.pyx:91-122 reads the caller's memory on every call.  The drop-in keeps the LD resident on the device,
    keyed by buffer identity: an in-place edit must not silently run on the stale device copy (content fingerprint,
    viprs_amd/vi/e_step_hip.py::plan_for)."""
    ld, ss, inp = syn.make_problem(sizes=[700, 90], seed=5, kind="longrange")
    st0 = inp.state_copy()
    H.assert_state_equal(H.run_hip(ld, inp, st0), H.run_oracle(ld, inp, st0))
    off = ld.ld_data.copy()
    d = off.reshape(-1)
    mask = np.ones(d.shape[0], bool)
    # halve every off-diagonal entry in place (same buffers, same identity)
    for bi in range(len(ld.block_start) - 1):
        s, e = int(ld.block_start[bi]), int(ld.block_start[bi + 1])
        o, b = int(ld.ld_indptr[s]), e - s
        mask[o:o + b * b:b + 1] = False
    ld.ld_data[mask] *= np.float32(0.5)
    ref = H.run_oracle(ld, inp, st0)
    got = H.run_hip(ld, inp, st0)
    H.assert_state_equal(got, ref)
    ld.ld_data[...] = off
    H.assert_state_equal(H.run_hip(ld, inp, st0), H.run_oracle(ld, inp, st0))


@pytest.mark.parametrize("team0, size", [("1", 12900), ("7", 6100), ("5", 3000)])
def test_forced_team_sizes_and_the_lds_budget_path(gpu, monkeypatch, team0, size):
    """VIPRS_TEAM0 forces team sizes the planner never picks (5, 7), and with VIPRS_TEAM0=1 an int8
    upper-triangular block of 12 900 SNPs does not fit one workgroup's 160 KB (q + second-pass sums + the off-diagonal
    tile integer LD stages in LDS): the launcher grows the team until it fits (launch_panel.inc).  Same bits as the
    oracle in every case."""
    from viprs_amd.vi import e_step_hip as S
    monkeypatch.setenv("VIPRS_TEAM0", team0)
    S.clear_plan_cache()
    try:
        ld, ss, inp = syn.make_problem(sizes=[size, 130, 64], low_memory=True, ld_dtype=np.int8, seed=23, kind="longrange")
        st0 = inp.state_copy()
        H.assert_state_equal(H.run_hip(ld, inp, st0, sweeps=2), H.run_oracle(ld, inp, st0, sweeps=2))
    finally:
        S.clear_plan_cache()


def _assert_equal_with_nonfinite(got, ref):
    """Finite entries and infinities bit for bit, NaNs in the same places (a NaN's payload / sign is not part of the contract:
    x86 and gfx950 generate different default NaNs)."""
    for k in H.STATE:
        a, b = got[k], ref[k]
        assert np.array_equal(np.isnan(a), np.isnan(b)), f"{k}: NaN in different places ({int(np.isnan(a).sum())} vs {int(np.isnan(b).sum())})"
        ok = ~np.isnan(b)
        assert np.array_equal(a[ok], b[ok]), f"{k}: {int((a[ok] != b[ok]).sum())} non-NaN entries differ"


@pytest.mark.parametrize("precision", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
@pytest.mark.parametrize("sweeps", [1, 2])
def test_nonfinite_inputs_propagate_as_in_the_reference(gpu, low_memory, precision, sweeps):
    """The reference has no input checks (`noexcept nogil`): a NaN in the summary statistics poisons its LD block (q of the
    whole window becomes NaN: fma(R, NaN, q)), u_logs = -inf (pi = 0) gives gamma = exp(-inf) / (1 + exp(-inf)) = 0, an
    overflowing effect runs through inf.  The device follows it entry for entry -- team blocks, single workgroups, both LD
    forms, float32 and float64 states -- and leaves the other blocks untouched."""
    ld, ss, inp = syn.make_problem(sizes=[1700, 300, 130, 64, 700], low_memory=low_memory, seed=29, kind="longrange",
                                   float_precision=precision)
    s = ld.block_start
    inp.std_beta[s[0] + 1000] = np.nan                      # the team block, late in the block
    inp.u_logs[s[1] + 5: s[1] + 9] = -np.inf                # pi = 0 for four SNPs of block 1
    inp.std_beta[s[3] + 10] = 1e30 if precision == np.float32 else 1e300      # overflow in block 3
    inp.mu_mult[s[4] + 3] = np.inf                          # inf times a finite residual in block 4
    if sweeps == 1:
        # the LAST SNP of block 2: its eta_diff is NaN, but in the upper-triangular form no row's second-pass dot covers a
        # column <= the row itself (e_step.hpp:331-337 starts at j + 1), so q of that SNP stays finite after one sweep -- a
        # device pass that multiplies the stored zeros on / left of the diagonal by eta_diff would make it NaN
        inp.std_beta[s[3] - 1] = np.nan
    st0 = inp.state_copy()
    with np.errstate(all="ignore"):
        ref = H.run_oracle(ld, inp, st0, sweeps=sweeps)
    got = H.run_hip(ld, inp, st0, sweeps=sweeps)
    _assert_equal_with_nonfinite(got, ref)
    assert np.isnan(ref["q"][s[0]:s[1]]).all()                 # the poisoned block
    if sweeps == 1:
        assert np.isnan(ref["eta_diff"][s[3] - 1]) and np.isnan(ref["q"][s[2]:s[3] - 1]).all()
        assert np.isfinite(ref["q"][s[3] - 1]) == bool(low_memory)
    else:
        assert np.isfinite(ref["q"][s[2]:s[3]]).all()          # an untouched block
    # (gamma = 0 there: d = -eta_old = 0 takes the skip branch, e_step.hpp:410-413 -- eta_diff 0, var_gamma keeps its start)
    assert (ref["eta_diff"][s[1] + 5: s[1] + 9] == 0).all() and (ref["var_gamma"][s[1] + 5: s[1] + 9] == precision(inp.pi)).all()


@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
@pytest.mark.parametrize("model", ["mixture4", "mixture10", "grid_mfma", "grid_items"])
def test_nonfinite_inputs_mixture_and_grid(gpu, model, low_memory, monkeypatch):
    """The same for the sparse mixture (lane-parallel chain K = 4, wide chain K = 10: a -inf logit is a component with
    pi_k = 0, a NaN poisons the block through the softmax) and for the grid (batched matrix-core kernel and per-(block, model)
    items): NaNs in the same places, everything else bit for bit."""
    from tests.test_gpu_models import _run_grid, _run_mix
    from tests.test_oracle_vs_ref import _grid_inputs, _mixture_inputs
    from viprs_amd.vi import e_step_hip as S
    ld, ss, inp = syn.make_problem(sizes=[1700, 300, 130, 64], low_memory=low_memory, seed=37, kind="longrange")
    s = ld.block_start
    inp.std_beta[s[0] + 900] = np.nan
    inp.std_beta[s[3] + 10] = 1e30
    with np.errstate(all="ignore"):
        if model.startswith("mixture"):
            K = int(model[7:])
            mix, st0 = _mixture_inputs(ld, ss, K)
            mix["u_logs"][s[1] + 5: s[1] + 9, 0] = -np.inf          # component 0 switched off for four SNPs
            mix["u_logs"][s[1] + 20, :] = -np.inf                  # every component off: all the mass on the null
            ref = _run_mix(O, ld, inp, mix, st0, 2)
            got = _run_mix(S, ld, inp, mix, st0, 2)
        else:
            monkeypatch.setenv("VIPRS_GRID_MFMA", "1" if model == "grid_mfma" else "0")
            S.clear_plan_cache()
            g, st0 = _grid_inputs(ld, ss, 12)
            g["u_logs"][s[1] + 5: s[1] + 9, 3] = -np.inf
            active = np.array([11, 0, 3, 8], dtype=np.int32)
            ref = _run_grid(O, ld, inp, g, st0, active)
            got = _run_grid(S, ld, inp, g, st0, active)
            S.clear_plan_cache()
    _assert_equal_with_nonfinite(got, ref)
    assert np.isnan(ref["q"][s[0]:s[1]]).any() and np.isfinite(ref["q"][s[2]:s[3]]).all()


def test_kernel_time_does_not_depend_on_the_queue_depth(gpu):
    """The HIP events that time a sweep bracket the kernel launch itself (`SweepTiming::launcher_start`, adjacent to
    hipLaunchKernel): a sweep submitted into an EMPTY stream -- where the start event is reached at once and anything the
    host does before the launch would count as kernel time -- reports the same kernel time as sweeps submitted back to back.
    (Round 5's driver run showed a 1.9 ms 'sweep' among ten of 0.38: host time inside the bracket; profiles/r06_stall.md.)"""
    from viprs_amd.plan import DeviceState, LDPlan
    ld = syn.make_ld(syn.block_sizes("cfg2"), low_memory=True, kind="longrange")
    inp = syn.make_inputs(syn.make_sumstats(ld))
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, True)
    st = DeviceState(plan, "float32", "spike_slab")
    for k in ("std_beta", "u_logs", "sqrt_half_var_tau", "mu_mult"):
        st.upload(k, getattr(inp, k))
    for _ in range(30):
        st.reset(inp.pi); st.e_step(ld.dq_scale, sync=False)
    st.synchronize()
    plan.timing_reset()
    for _ in range(40):
        st.reset(inp.pi); st.e_step(ld.dq_scale, sync=False)
    st.synchronize()
    full = np.median(plan.timing_history(which=1)[5:])
    empty = []
    for _ in range(40):
        st.reset(inp.pi)
        st.synchronize()
        st.e_step(ld.dq_scale, sync=True)
        empty.append(plan.last_kernel_ms(1))
    assert abs(np.median(empty) / full - 1.0) < 0.05, (full, np.median(empty))
    # which = 2: the HOST time the library spent between recording the start event and recording the end event of each sweep
    # (the launch call) -- a sweep whose kernel time is off while this is large was not slow on the device
    host = np.array(plan.timing_history(which=2))[-40:]                       # (the 40 sweeps into an empty stream)
    assert host.shape == (40,) and (host >= 0).all() and np.median(host) < 0.1, host
    slow = np.array(empty) > 1.5 * np.median(empty)
    assert (host[slow] > 0.1).all(), (np.array(empty)[slow], host[slow])      # every outlier is explained by its host stamp
    plan.close()


def test_timing_record_follows_the_route_of_each_sweep(gpu):
    """The timing record of a sweep holds what THAT sweep bracketed.  One dense block beside one windowed component, fp32
    spike-and-slab: the dense bracket lies inside the whole sweep's; a sweep over the windowed component only brackets no
    dense kernel and reports 0 for which = 1 and which = 2 (not the stamps an earlier sweep left in the ring slot); a mixture
    sweep has one bracket, which stands for both.  The state is `==` the oracle's after the same sweeps over the same blocks."""
    from tests.test_band import _inputs, dense_beside_banded
    from tests.test_oracle_vs_ref import _mixture_inputs
    from viprs_amd import _lib as L
    from viprs_amd.plan import DeviceState, LDPlan
    ld = dense_beside_banded([90], 300, 20, False)
    ss, inp = _inputs(ld.m, seed=21)
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, False)
    assert (plan.info(L.INFO_N_DENSE), plan.info(L.INFO_N_RAGGED)) == (1, 1)
    st = DeviceState(plan, "float32", "spike_slab")
    for k in ("std_beta", "u_logs", "sqrt_half_var_tau", "mu_mult") + H.STATE:
        st.upload(k, getattr(inp, k))
    plan.timing_reset()
    st.e_step(ld.dq_scale)
    whole, dense, host = (plan.timing_history(which=w) for w in (0, 1, 2))
    assert len(whole) == len(dense) == len(host) == 1
    assert whole[0] >= dense[0] > 0 and host[0] >= 0, (whole, dense, host)
    starts, _ = plan.blocks()
    plan.timing_reset()
    plan.set_active_blocks(starts[:-1] >= 90)             # the windowed component only
    st.e_step(ld.dq_scale)
    assert plan.timing_history(which=1) == [0.0] and plan.timing_history(which=2) == [0.0]
    assert plan.timing_history(which=0)[0] > 0
    plan.set_active_blocks(None)
    st.e_step(ld.dq_scale)
    for w in (0, 1, 2):
        t = np.array(plan.timing_history(which=w))
        assert t.shape == (2,) and np.isfinite(t).all() and (t >= 0).all(), (w, t)
    # the oracle: LD blocks are independent, so the dense block keeps its state through the second sweep
    ref1 = H.run_oracle(ld, inp, inp.state_copy(), sweeps=1)
    ref2 = H.run_oracle(ld, inp, ref1, sweeps=1)
    for k in H.STATE:
        ref2[k][:90] = ref1[k][:90]
    H.assert_state_equal({k: st.download(k) for k in H.STATE}, H.run_oracle(ld, inp, ref2, sweeps=1))
    # mixture: only one bracket exists on that route
    mix, st0 = _mixture_inputs(ld, ss, 4)
    sm = DeviceState(plan, "float32", "mixture", 4)
    sm.upload("std_beta", inp.std_beta)
    for k, v in (("log_null_pi", mix["log_null_pi"]), ("u_logs", mix["u_logs"]), ("sqrt_half_var_tau", mix["shvt"]),
                 ("mu_mult", mix["mu_mult"])) + tuple(st0.items()):
        sm.upload(k, v)
    plan.timing_reset()
    sm.e_step(ld.dq_scale)
    assert plan.timing_history(which=0) == plan.timing_history(which=1) and plan.timing_history(which=0)[0] > 0
    plan.close()


def test_state_destroyed_after_its_plan(gpu):
    """Finalizers of a garbage collector run in any order: a `DeviceState` may be destroyed AFTER its `LDPlan` (the plan's
    weak set of states is already cleared then).  `viprs_state_destroy` must not read the plan (it used to take the device
    index from it: freed memory, `hipSetDevice(garbage)`, and "invalid device ordinal" left behind as the thread's last error
    -- which the next plan creation reported as its own kernel launch failing: a once-in-three-runs failure of the suite)."""
    import ctypes
    from viprs_amd import _lib as L
    from viprs_amd.plan import DeviceState, LDPlan
    ld, ss, inp = syn.make_problem(sizes=[200, 90], low_memory=True, seed=5)
    for _ in range(20):
        plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, True)
        st = DeviceState(plan, "float32", "spike_slab")
        h_state, st._h = st._h, ctypes.c_void_p()          # detach: the plan's close() will not find the state
        plan._states.discard(st)
        plan.close()
        junk = [np.full(4096, -1, dtype=np.int64) for _ in range(8)]      # (let the allocator reuse the plan's memory)
        L.check(L.lib.viprs_state_destroy(h_state))
        del junk
        again = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, True)  # raised ViprsHipError: invalid device ordinal
        again.close()
