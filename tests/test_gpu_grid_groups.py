"""Grid states with SNP groups on the device (viprs_state_prep_grid_groups / _sums_grid_groups_* /
_set_group_columns) and the lock-step per-chromosome grid fit `VIPRSGridPerChromosome` on the GPU."""
import os

import numpy as np
import pytest

from tests.test_grid_per_chromosome import (FIXTURES, MAX_ITER, assert_same_fit, check_against_reference, fit, load,
                                            one_chromosome_loader)

# chromosomes of mixed blocks: a team-sized block (> kGridResMaxCols = 1 536 SNPs) and 64-column edge cases
SIZES = {1: [700, 64, 1700], 2: [300, 63], 3: [64, 65, 900, 128], 4: [200, 64]}
FIELDS = ("var_gamma", "var_mu", "eta", "q", "eta_diff")


def _ld(c, low_memory, ld_dtype):
    from viprs_amd.utils import synthetic as syn
    return syn.make_ld(SIZES[c], low_memory=low_memory, ld_dtype=ld_dtype, seed=40 + c, kind="longrange")


def _pair_params(rng, chroms, G):
    rows = []
    for gi, _ in enumerate(chroms):
        for g in range(G):
            pi, sig, tau, lam = rng.uniform(0.002, 0.05), rng.uniform(0.6, 0.95), rng.uniform(200, 3000), rng.choice([0.0, 0.3])
            rows.append([gi, g, np.log(pi) - np.log(1 - pi), np.log(tau), sig, tau, 1.0 + lam])
    return np.array(rows)


def _initial(rng, m, G):
    gam = rng.uniform(0.001, 0.3, (m, G)).astype(np.float32)
    mu = (0.01 * rng.standard_normal((m, G))).astype(np.float32)
    return dict(var_gamma=np.asfortranarray(gam), var_mu=np.asfortranarray(mu), eta=np.asfortranarray(gam * mu),
                q=np.asfortranarray((0.01 * rng.standard_normal((m, G))).astype(np.float32)),
                eta_diff=np.zeros((m, G), np.float32, order="F"))


@pytest.mark.gpu
@pytest.mark.parametrize("G", [6, 40])
@pytest.mark.parametrize("mfma", ["0", "1"])
@pytest.mark.parametrize("low_memory", [True, False])
@pytest.mark.parametrize("ld_dtype", ["float32", "int8", "int16"])
def test_grid_groups_equal_a_plan_per_chromosome(gpu, monkeypatch, mfma, low_memory, ld_dtype, G):
    """prep_grid_groups + two sweeps under a pair mask + sums_grid_groups on the merged plan == a one-chromosome grid state
    swept with that chromosome's active list (panel path: VIPRS_GRID_MFMA=0, matrix-core path: =1; G = 40: two launches of
    32 columns on the matrix cores); pairs outside the mask, a chromosome whose blocks left the sweep and a chromosome whose
    blocks stay in the sweep with every mask bit off keep every bit."""
    from viprs_amd.data import merge_ld_arrays
    from viprs_amd.plan import DeviceState, LDPlan
    from viprs_amd.utils import synthetic as syn
    monkeypatch.setenv("VIPRS_GRID_MFMA", mfma)
    chroms = sorted(SIZES)
    lds = {c: _ld(c, low_memory, np.dtype(ld_dtype)) for c in chroms}
    sss = {c: syn.make_sumstats(_ld(c, low_memory, np.float32), n=5e4 * c, seed=30 + c) for c in chroms}
    shapes = {c: lds[c].m for c in chroms}
    lb, ip, data, seg = merge_ld_arrays(chroms, shapes, {c: lds[c].ld_left_bound for c in chroms},
                                        {c: lds[c].ld_indptr for c in chroms}, {c: lds[c].ld_data for c in chroms})
    dq = 1.0 if ld_dtype == "float32" else 1.0 / np.iinfo(ld_dtype).max
    rng = np.random.default_rng(7)
    plan = LDPlan(lb, ip, data, low_memory)
    st = DeviceState(plan, "float32", "grid", G)
    st.upload("std_beta", np.concatenate([sss[c].std_beta for c in chroms]))
    st.set_n_per_snp(np.concatenate([sss[c].n_per_snp for c in chroms]))
    gs = np.array([0] + [seg[c][1] for c in chroms], dtype=np.int64)
    st.set_groups(gs)
    with pytest.raises(ValueError, match="cuts through"):           # (a refused list leaves the groups as they were)
        st.set_groups(np.array([0, 100, gs[-1]], dtype=np.int64))
    init = _initial(rng, plan.m, G)
    for k, v in init.items():
        st.upload(k, v)
    rows = _pair_params(rng, chroms, G)
    st.prep_grid_groups(rows)
    # chromosome 1: columns 0, 2, 3, 5 (+ 33, 35, 39) on; chromosome 2: 1, 4 (+ 34); chromosome 3: all on, but its blocks
    # leave the sweep; chromosome 4: every bit off, its blocks stay (the kernels skip them)
    mask = np.zeros((len(chroms), G), np.uint8)
    mask[0, [g for g in (0, 2, 3, 5, 33, 35, 39) if g < G]] = 1
    mask[1, [g for g in (1, 4, 34) if g < G]] = 1
    mask[2, :] = 1
    st.set_group_columns(mask)
    active = np.array([g for g in range(G) if g not in (3, 36)], dtype=np.int32)     # columns 3 and 36 are not active
    starts, _ = plan.blocks()
    block_group = np.searchsorted(gs, starts[:-1], side="right") - 1
    plan.set_active_blocks(block_group != 2)
    st.e_step(dq, active_model_idx=active)
    st.e_step(dq, active_model_idx=active)
    plan.set_active_blocks(None)
    pairs = [(gi, g) for gi in range(len(chroms)) for g in range(G)]
    st.sums_grid_groups_begin([p[0] for p in pairs], [p[1] for p in pairs], rows[:, 6])
    sums = st.sums_grid_groups_end()
    got = {k: st.download(k) for k in FIELDS + ("u_logs", "half_var_tau", "mu_mult")}
    for gi, c in enumerate(chroms):
        a, b = seg[c]
        on = [g for g in active if mask[gi, g]] if c != 3 else []
        p1 = LDPlan(lds[c].ld_left_bound, lds[c].ld_indptr, lds[c].ld_data, low_memory)
        s1 = DeviceState(p1, "float32", "grid", G)
        s1.upload("std_beta", sss[c].std_beta)
        s1.set_n_per_snp(sss[c].n_per_snp)
        for k, v in init.items():
            s1.upload(k, np.asfortranarray(v[a:b]))
        r = rows[rows[:, 0] == gi]
        s1.prep_columns(np.column_stack([r[:, 1], r[:, 2:]]))
        if on:
            s1.e_step(dq, active_model_idx=np.array(on, dtype=np.int32))
            s1.e_step(dq, active_model_idx=np.array(on, dtype=np.int32))
        s1.sums_columns_begin(np.arange(G), r[:, 6])
        ref_sums = s1.sums_columns_end()
        for k in got:
            assert np.array_equal(got[k][a:b], s1.download(k)), (c, k)
        for g in range(G):
            if g not in on:                                      # outside the mask: byte-identical to before the sweeps
                for k in FIELDS:
                    assert got[k][a:b, g].tobytes() == init[k][a:b, g].tobytes(), (c, g, k)
        assert np.array_equal(sums[gi * G:(gi + 1) * G], ref_sums), c
        p1.close()


@pytest.mark.gpu
def test_grid_mask_refusals(gpu):
    """Paths without a mask refuse a grid state under one: ragged (banded) blocks and float64 states."""
    from viprs_amd.plan import DeviceState, LDPlan
    from viprs_amd.utils import synthetic as syn
    ld = syn.make_ld([200, 150], low_memory=False)
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, False)
    st = DeviceState(plan, "float64", "grid", 3)
    st.set_n_per_snp(np.full(plan.m, 1e5))
    st.set_groups(np.array([0, 200, 350], dtype=np.int64))
    st.set_group_columns(np.ones((2, 3), np.uint8))
    with pytest.raises(NotImplementedError, match="float64"):
        st.e_step(1.0)
    st.set_group_columns(None)
    st.e_step(1.0)                                               # no mask: the float64 grid sweep as before
    # a banded block: windows narrower than the block (the ragged kind)
    m = 300
    lb = np.maximum(np.arange(m) - 20, 0).astype(np.int32)
    right = np.minimum(np.arange(m) + 21, m)
    ip = np.concatenate([[0], np.cumsum(right - lb)]).astype(np.int64)
    data = np.concatenate([0.5 ** np.abs(np.arange(lb[j], right[j]) - j) for j in range(m)]).astype(np.float32)
    rplan = LDPlan(lb, ip, data, False)
    rs = DeviceState(rplan, "float32", "grid", 2)
    rs.set_n_per_snp(np.full(m, 1e5))
    rs.set_groups(np.array([0, m], dtype=np.int64))
    rs.set_group_columns(np.ones((1, 2), np.uint8))
    with pytest.raises(NotImplementedError, match="ragged"):
        rs.e_step(1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_lockstep_fit_hip_matches_reference_and_sequential_grids(gpu, name):
    """The lock-step fit on the device: the reference's per-chromosome fits at the common tolerances, and `==` (ELBOs, nit,
    messages, every (m_c, G) array) to one VIPRSGrid(batched=True) fit per chromosome, run one after the other."""
    from viprs_amd.model import VIPRSGrid
    fx, gdl = load(name)
    model = fit(fx, gdl)
    check_against_reference(model, fx)
    assert len({r.nit for rs in model.optim_results.values() for r in rs}) > 1
    for c in model.groups:
        seq = VIPRSGrid(one_chromosome_loader(gdl, c), model.grids[c], low_memory=bool(fx["low_memory"]))
        seq.fit(batched=True, max_iter=MAX_ITER)
        assert_same_fit(model, seq, c, model.n_models)


@pytest.mark.gpu
@pytest.mark.parametrize("criterion", ["ELBO", "pseudo_validation", "bma"])
def test_selection_and_bma_hip_equal_sequential_grids(gpu, criterion):
    from viprs_amd.model import (VIPRSGrid, bayesian_model_average, bayesian_model_average_per_chromosome,
                                 select_best_model, select_best_model_per_chromosome)
    fx, gdl = load("fitchr_grid_3chr_upper")
    model = fit(fx, gdl)
    vb = {c: fx[f"validation_std_beta_{c}"] for c in model.groups}
    refs = {}
    for c in model.groups:
        seq = VIPRSGrid(one_chromosome_loader(gdl, c), model.grids[c], low_memory=True).fit(batched=True, max_iter=MAX_ITER)
        refs[c] = bayesian_model_average(seq) if criterion == "bma" else select_best_model(seq, {c: vb[c]}, criterion=criterion)
    out = bayesian_model_average_per_chromosome(model) if criterion == "bma" else \
        select_best_model_per_chromosome(model, vb, criterion=criterion)
    for c, ref in refs.items():
        for name in ("pip", "post_mean_beta", "post_var_beta", "var_gamma", "var_mu", "var_tau", "q"):
            assert np.array_equal(getattr(out, name)[c], getattr(ref, name)[c]), (c, name)
        for name in ("pi", "tau_beta", "sigma_epsilon", "_sigma_g"):
            assert np.float64(getattr(out, name)[c]) == np.float64(getattr(ref, name)), (c, name)


@pytest.mark.gpu
def test_lockstep_fit_refuses_ragged_ld(gpu):
    from viprs_amd.data import ArrayDataLoader, LDArrays, SumstatsArrays
    from viprs_amd.model import HyperparameterGrid, VIPRSGridPerChromosome
    m = 300
    lb = np.maximum(np.arange(m) - 20, 0).astype(np.int32)
    right = np.minimum(np.arange(m) + 21, m)
    ip = np.concatenate([[0], np.cumsum(right - lb)]).astype(np.int64)
    data = np.concatenate([0.5 ** np.abs(np.arange(lb[j], right[j]) - j) for j in range(m)]).astype(np.float32)
    rng = np.random.default_rng(3)
    gdl = ArrayDataLoader({21: LDArrays(symmetric=(lb, ip, data))},
                          {21: SumstatsArrays((0.01 * rng.standard_normal(m)).astype(np.float32), np.full(m, 1e5))})
    with pytest.raises(NotImplementedError, match="dense"):
        VIPRSGridPerChromosome(gdl, HyperparameterGrid(sigma_epsilon_steps=2, pi_steps=2, n_snps=m), low_memory=False)
