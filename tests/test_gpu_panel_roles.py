"""GPU: every role of the panel sweep kernel (estep_panel.h) in one small plan, for every exact-math instantiation,
bit for bit against the oracle.

The blocks: 2370 = 37 panels + a last panel of 2 rows, a large-class team block (>= 2304); 1601 = 25 panels + a last
panel of 1 row, a medium-class team block (>= 1600); 130, a queue block with a partial last panel; 64, exactly one panel
(no off-diagonal tile); 1, a single row.  Two sweeps: the second runs on the first's q, with the launch generation of the
hand-off tags advanced and the queue heads reset by the kernel's last workgroup."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H
from tests.test_gpu_models import _run_grid, _run_mix
from tests.test_oracle_vs_ref import _grid_inputs, _mixture_inputs
from viprs_amd.utils import synthetic as syn

pytestmark = pytest.mark.gpu
SIZES = [2370, 1601, 130, 64, 1]
SWEEPS = 2
# spike-and-slab | grid columns (per-(block, model) panel items) | the three run_panel variants of the K <= 8 mixture
# chain (K < 4, K == 4, K > 4) | MixtureWideModel<15> | MixtureWideModel<31>
MODELS = ["spike_slab", "grid", "mix3", "mix4", "mix6", "mix12", "mix20"]


@functools.lru_cache(maxsize=None)
def _problem(low_memory, ld_dtype):
    return syn.make_problem(sizes=SIZES, low_memory=low_memory, ld_dtype=ld_dtype, seed=53, kind="longrange")


def _spike_slab(ld, inp):
    """Through a plan of its own: the skip count of the last sweep is read from it."""
    from viprs_amd.plan import LDPlan
    st0 = inp.state_copy()
    ref = H.run_oracle(ld, inp, st0, sweeps=SWEEPS)
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory)
    try:
        got = {k: v.copy() for k, v in st0.items()}
        for _ in range(SWEEPS):
            plan.e_step(inp.std_beta, got["var_gamma"], got["var_mu"], got["eta"], got["q"], got["eta_diff"], inp.u_logs,
                        inp.sqrt_half_var_tau, inp.mu_mult, ld.dq_scale)
        skipped = plan.last_skipped()
    finally:
        plan.close()
    H.assert_state_equal(got, ref)
    assert skipped == int((got["eta_diff"] == 0).sum())


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("ld_dtype", [np.float32, np.int8, np.int16], ids=["f32", "i8", "i16"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_every_role_of_the_panel_kernel_matches_the_oracle(gpu, low_memory, ld_dtype, model, monkeypatch):
    from viprs_amd.vi import e_step_hip as S
    ld, ss, inp = _problem(low_memory, ld_dtype)
    narrow = low_memory and ld_dtype != np.float32
    if narrow:
        monkeypatch.setenv("VIPRS_TEAM0", "8")      # teams of 8: the large class takes the narrow team strips
    monkeypatch.setenv("VIPRS_GRID_MFMA", "0")      # grid columns as panel items, not the batched matrix-core kernel
    S.clear_plan_cache()
    try:
        if model == "spike_slab":
            _spike_slab(ld, inp)
        elif model == "grid":
            g, st0 = _grid_inputs(ld, ss, 5)
            active = np.array([4, 0, 2], dtype=np.int32)
            H.assert_state_equal(_run_grid(S, ld, inp, g, st0, active, sweeps=SWEEPS),
                                 _run_grid(O, ld, inp, g, st0, active, sweeps=SWEEPS))
        else:
            mix, st0 = _mixture_inputs(ld, ss, int(model[3:]))
            H.assert_state_equal(_run_mix(S, ld, inp, mix, st0, SWEEPS), _run_mix(O, ld, inp, mix, st0, SWEEPS))
    finally:
        S.clear_plan_cache()
