"""The pathwise grid search per chromosome on the device: `viprs_state_commit_groups` (SNP groups of a spike-and-slab state
into columns of a grid state) and `VIPRSGridPathwisePerChromosome`, `==` the serial pathwise fits of each chromosome."""
import ctypes

import numpy as np
import pytest

from tests.test_grid_pathwise_per_chromosome import (FIXTURES, assert_same_as_sequential, check_against_fixture,
                                                     check_restart, fit, load, restart_case, sequential)

FIELDS = ("var_gamma", "var_mu", "eta", "q", "eta_diff")
SIZES = {1: [300, 64], 2: [130], 3: [64, 65, 200], 4: [90]}


def _plan_and_groups():
    from viprs_amd.data import merge_ld_arrays
    from viprs_amd.plan import LDPlan
    from viprs_amd.utils import synthetic as syn
    chroms = sorted(SIZES)
    lds = {c: syn.make_ld(SIZES[c], low_memory=True, seed=50 + c) for c in chroms}
    shapes = {c: lds[c].m for c in chroms}
    lb, ip, data, seg = merge_ld_arrays(chroms, shapes, {c: lds[c].ld_left_bound for c in chroms},
                                        {c: lds[c].ld_indptr for c in chroms}, {c: lds[c].ld_data for c in chroms})
    return LDPlan(lb, ip, data, True), np.array([0] + [seg[c][1] for c in chroms], dtype=np.int64)


# ---- the ABI ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_commit_groups_copies_exactly_the_pairs(gpu, dtype):
    from viprs_amd import _lib as L
    from viprs_amd.plan import DeviceState
    plan, gs = _plan_and_groups()
    m, G, T = plan.m, 5, np.dtype(dtype)
    rng = np.random.default_rng(11)
    src = DeviceState(plan, dtype, "spike_slab", placement="off")
    src.set_groups(gs)
    vals = {f: rng.standard_normal(m).astype(T) for f in FIELDS}
    for f, v in vals.items():
        src.upload(f, v)
    dst = DeviceState(plan, dtype, "grid", G, placement="off")
    sentinel = np.full((m, G), -7.25, dtype=T, order="F")
    for f in FIELDS:
        dst.upload(f, sentinel)
    # first and last group, an odd-sized group at an unaligned offset, one group into two columns
    groups, cols = np.array([0, 3, 2, 1, 2]), np.array([4, 0, 1, 2, 3])
    dst.commit_groups(src, groups, cols)
    for f in FIELDS:
        got = dst.download(f)
        want = sentinel.copy()
        for g, col in zip(groups, cols):
            want[gs[g]:gs[g + 1], col] = vals[f][gs[g]:gs[g + 1]]
        assert got.dtype == T and np.array_equal(got, want), f
    assert np.array_equal(src.download("var_gamma"), vals["var_gamma"])
    # refusals: an error, nothing launched, dst as it was
    before = {f: dst.download(f) for f in FIELDS}
    other_plan, _ = _plan_and_groups()
    other = DeviceState(other_plan, dtype, "spike_slab", placement="off")
    other.set_groups(gs)
    wrong_dtype = DeviceState(plan, "float64" if dtype == "float32" else "float32", "spike_slab", placement="off")
    wrong_dtype.set_groups(gs)
    no_groups = DeviceState(plan, dtype, "spike_slab", placement="off")
    grid_src = DeviceState(plan, dtype, "grid", G, placement="off")
    grid_src.set_groups(gs)
    pair = np.array([[0, 0]], dtype=np.int32)
    ptr = pair.ctypes.data_as(ctypes.c_void_p)
    lib = L.lib
    cases = [(lib.viprs_state_commit_groups, (None, src._h, 1, ptr)), (lib.viprs_state_commit_groups, (dst._h, None, 1, ptr)),
             (lib.viprs_state_commit_groups, (dst._h, src._h, 1, None)), (lib.viprs_state_commit_groups, (dst._h, src._h, -1, ptr))]
    for fn, args in cases:
        assert fn(*args) == L.EINVAL
    for s, msg in ((other, "different plans"), (wrong_dtype, "dtypes"), (no_groups, "set_groups"), (grid_src, "spike-and-slab")):
        with pytest.raises(ValueError, match=msg):
            dst.commit_groups(s, [0], [0])
    with pytest.raises(ValueError, match="not a grid state"):
        src.commit_groups(src, [0], [0])
    with pytest.raises(ValueError, match="group index"):
        dst.commit_groups(src, [len(gs) - 1], [0])
    with pytest.raises(ValueError, match="column index"):
        dst.commit_groups(src, [0], [G])
    with pytest.raises(ValueError, match="column index"):
        dst.commit_groups(src, [1, 0], [0, -1])
    for f in FIELDS:
        assert np.array_equal(dst.download(f), before[f]), f


# ---- the fit --------------------------------------------------------------------------------------------------------------
def _count_sweeps(monkeypatch):
    from viprs_amd.plan import DeviceState
    calls = []
    orig = DeviceState.e_step

    def counting(self, *a, **k):
        calls.append(self.model)
        return orig(self, *a, **k)

    monkeypatch.setattr(DeviceState, "e_step", counting)
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_pathwise_fit_hip_matches_reference_and_sequential_fits(gpu, monkeypatch, name):
    fx, gdl = load(name)
    rounds = []
    sweeps = _count_sweeps(monkeypatch)
    model = fit(fx, gdl, e_step="hip", on_iteration=rounds.append)
    assert list(model._plans) == ["*"]
    assert len(sweeps) == len(rounds) and rounds == list(range(1, len(rounds) + 1))      # one sweep per EM round
    assert len(rounds) == max(len(h["ELBO"]) - 1 for h in model.history.values())
    monkeypatch.undo()
    check_against_fixture(model, fx)
    assert_same_as_sequential(model, sequential(model, gdl, fx, e_step="hip"))


@pytest.mark.gpu
def test_pathwise_fit_hip_mixed_banded_and_block_ld(gpu):
    """A chromosome of banded (ragged) LD beside chromosomes of dense blocks: the spike-and-slab kernels take every LD kind."""
    from viprs_amd.data import ArrayDataLoader, LDArrays, SumstatsArrays
    from viprs_amd import _lib as L
    from viprs_amd.model import HyperparameterGrid, VIPRSGridPathwisePerChromosome
    fx, gdl = load(FIXTURES[0])
    m = 300
    lb = np.maximum(np.arange(m) - 20, 0).astype(np.int32)
    right = np.minimum(np.arange(m) + 21, m)
    ip = np.concatenate([[0], np.cumsum(right - lb)]).astype(np.int64)
    data = np.concatenate([0.5 ** np.abs(np.arange(lb[j], right[j]) - j) for j in range(m)]).astype(np.float32)
    rng = np.random.default_rng(3)
    ld = dict(gdl.ld)
    ld[19] = LDArrays(symmetric=(lb, ip, data))
    ss = dict(gdl.sumstats_table)
    ss[19] = SumstatsArrays((0.01 * rng.standard_normal(m)).astype(np.float32), np.full(m, 1e5))
    mixed = ArrayDataLoader(ld, ss)
    model = VIPRSGridPathwisePerChromosome(mixed, HyperparameterGrid(sigma_epsilon_steps=2, pi_steps=2, n_snps=mixed.m),
                                           low_memory=False)
    assert model._plans["*"].info(L.INFO_N_RAGGED) > 0
    model.fit(max_iter=60)
    fx_like = dict(low_memory=False, float_precision="float32", dequantize_on_the_fly=False)
    assert_same_as_sequential(model, sequential(model, mixed, fx_like, e_step="hip", max_iter=60))


@pytest.mark.gpu
@pytest.mark.parametrize("criterion", ["ELBO", "pseudo_validation", "bma"])
def test_selection_and_bma_hip_equal_sequential_fits(gpu, criterion):
    from viprs_amd.model import (bayesian_model_average, bayesian_model_average_per_chromosome, select_best_model,
                                 select_best_model_per_chromosome)
    fx, gdl = load(FIXTURES[1])
    model = fit(fx, gdl, e_step="hip")
    seq = sequential(model, gdl, fx, e_step="hip")
    vb = {c: fx[f"validation_std_beta_{c}"] for c in model.groups}
    if criterion == "bma":
        refs = {c: bayesian_model_average(s) for c, s in seq.items()}
        out = bayesian_model_average_per_chromosome(model)
    else:
        refs = {c: select_best_model(s, {c: vb[c]}, criterion=criterion) for c, s in seq.items()}
        out = select_best_model_per_chromosome(model, vb, criterion=criterion)
    for c, ref in refs.items():
        for name in ("pip", "post_mean_beta", "post_var_beta", "var_gamma", "var_mu", "var_tau", "q"):
            assert np.array_equal(getattr(out, name)[c], getattr(ref, name)[c]), (c, name)
        for name in ("pi", "tau_beta", "sigma_epsilon", "_sigma_g"):
            assert np.float64(getattr(out, name)[c]) == np.float64(getattr(ref, name)), (c, name)


@pytest.mark.gpu
def test_negative_mse_restarts_only_that_chromosome_hip(gpu):
    fx, gdl, bad, grid = restart_case()
    theta = {"sigma_epsilon": 0.8}
    model = fit(fx, gdl, e_step="hip", grid=grid, max_iter=40, theta_0=theta)
    check_restart(model, sequential(model, gdl, fx, e_step="hip", max_iter=40, theta_0=theta), bad)
