"""GPU: the panel sweep's LD load sites that carry a cache policy (panel_loads.h `kCached` / `kStream`, the per-site
choice in estep_panel.h `PanelLdPolicy`), bit for bit against the oracle -- and streamed loads of LD that a kernel wrote
on the same stream just before the sweep.

The blocks: 1601 = 25 panels + a last panel of one row, a medium-class team of 4 (wide strips, team tile staging at the
default policy); 321 = five panels + a one-row panel in the queue role (a strip that straddles the chain in the upper
form -- strip_update<MIXED> -- and a FULL = false strip); 130, a queue block with a partial last panel; 64, exactly one
panel (no off-diagonal tile)."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H
from tests.test_gpu_models import _run_mix
from tests.test_oracle_vs_ref import _mixture_inputs
from viprs_amd.utils import synthetic as syn

pytestmark = pytest.mark.gpu
SIZES = [1601, 321, 130, 64]
FRESH_SIZES = [321, 130, 64]
SWEEPS = 3
INPUTS = ("std_beta", "u_logs", "sqrt_half_var_tau", "mu_mult")


@functools.lru_cache(maxsize=None)
def _problem(low_memory, ld_dtype):
    return syn.make_problem(sizes=SIZES, low_memory=low_memory, ld_dtype=ld_dtype, seed=67, kind="longrange")


@pytest.mark.parametrize("model", ["spike_slab", "mix4"])
@pytest.mark.parametrize("ld_dtype", [np.float32, np.int16], ids=["f32", "i16"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_every_policy_site_matches_the_oracle_after_every_sweep(gpu, low_memory, ld_dtype, model):
    from viprs_amd.vi import e_step_hip as S
    ld, ss, inp = _problem(low_memory, ld_dtype)
    S.clear_plan_cache()
    try:
        if model == "spike_slab":
            got = ref = inp.state_copy()
            for sweep in range(SWEEPS):
                got, ref = H.run_hip(ld, inp, got, sweeps=1), H.run_oracle(ld, inp, ref, sweeps=1)
                H.assert_state_equal(got, ref)
        else:
            mix, st0 = _mixture_inputs(ld, ss, 4)
            got = ref = st0
            for sweep in range(SWEEPS):
                got, ref = _run_mix(S, ld, inp, mix, got, 1), _run_mix(O, ld, inp, mix, ref, 1)
                H.assert_state_equal(got, ref)
        assert np.count_nonzero(ref["eta_diff"]) > 0.5 * ref["eta_diff"].size      # (the sweeps did something)
    finally:
        S.clear_plan_cache()


def _sweep_state(plan, inp, dq_scale, sweeps=1):
    from viprs_amd.plan import DeviceState
    st = DeviceState(plan, "float32", "spike_slab", 1)
    try:
        for name in INPUTS:
            st.upload(name, getattr(inp, name))
        st.reset(inp.pi)
        for _ in range(sweeps):
            st.e_step(dq_scale, None, sync=True)
        return {k: st.download(k) for k in H.STATE}
    finally:
        st.close()


@pytest.mark.parametrize("ld_dtype", [np.float32, np.int16], ids=["f32", "i16"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_sweep_straight_after_device_generated_ld(gpu, low_memory, ld_dtype):
    """`LDPlan.synthetic` writes the LD entries with a kernel; the first sweep follows on the same stream."""
    from viprs_amd.plan import LDPlan
    ld = syn.make_ld(FRESH_SIZES, low_memory=low_memory, ld_dtype=ld_dtype, seed=68, kind="longrange")
    inp = syn.make_inputs(syn.make_sumstats(ld, seed=68))
    plan = LDPlan.synthetic(syn.make_ld(FRESH_SIZES, low_memory=low_memory, ld_dtype=ld_dtype, seed=68, kind="longrange",
                                        data=False))
    try:
        got = _sweep_state(plan, inp, ld.dq_scale)
    finally:
        plan.close()
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, low_memory)
    try:
        ref = _sweep_state(plan, inp, ld.dq_scale)
    finally:
        plan.close()
    H.assert_state_equal(got, ref)
    H.assert_state_equal(got, H.run_oracle(ld, inp, inp.state_copy(), sweeps=1))


@pytest.mark.parametrize("ld_dtype", [np.float32, np.int16], ids=["f32", "i16"])
def test_sweep_straight_after_the_blocks_are_mirrored_again(gpu, ld_dtype):
    """One upper-form plan: a float64 sweep leaves its blocks in the packed form (zeros on and left of the diagonal); the
    fp32 sweep that follows at once has them mirrored again on the plan's stream immediately before the panel kernel."""
    from viprs_amd.plan import LDPlan
    ld, ss, inp = syn.make_problem(sizes=FRESH_SIZES, low_memory=True, ld_dtype=ld_dtype, seed=69, kind="longrange")
    _, _, inp64 = syn.make_problem(sizes=FRESH_SIZES, low_memory=True, ld_dtype=ld_dtype, seed=69, kind="longrange",
                                   float_precision=np.float64)

    def sweep(plan, i):
        st = i.state_copy()
        plan.e_step(i.std_beta, st["var_gamma"], st["var_mu"], st["eta"], st["q"], st["eta_diff"], i.u_logs,
                    i.sqrt_half_var_tau, i.mu_mult, ld.dq_scale)
        return st

    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, True)
    try:
        sweep(plan, inp)                      # mirrored
        got64 = sweep(plan, inp64)            # packed
        got = sweep(plan, inp)                # mirrored again, swept at once
    finally:
        plan.close()
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, True)
    try:
        ref = sweep(plan, inp)
    finally:
        plan.close()
    H.assert_state_equal(got, ref)
    H.assert_state_equal(got, H.run_oracle(ld, inp, inp.state_copy(), sweeps=1))
    H.assert_state_equal(got64, H.run_oracle(ld, inp64, inp64.state_copy(), sweeps=1))
