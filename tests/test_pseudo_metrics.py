"""viprs_amd/eval/pseudo_metrics.py on the CPU: the LD product is injected (`dot_fn=` = the host reference of
tests/ld_dot_reference.py), the expected values are worked out directly in NumPy float64 from dense matrices."""
import os

import numpy as np
import pytest

from tests import ld_dot_reference as R
from viprs_amd.utils import synthetic as syn

HERE = os.path.dirname(os.path.abspath(__file__))


def _panel(sizes, low_memory, ld_dtype, seed):
    ld = syn.make_ld(sizes, low_memory=low_memory, ld_dtype=ld_dtype, kind="longrange", seed=seed)
    dense = np.zeros((ld.m, ld.m))
    for bi in range(len(sizes)):
        s, e = int(ld.block_start[bi]), int(ld.block_start[bi + 1])
        dense[s:e, s:e] = syn.dense_block(ld, bi)
    np.fill_diagonal(dense, 1.0)
    return (ld.ld_left_bound, ld.ld_indptr, ld.ld_data, low_memory, ld.dq_scale), dense


@pytest.mark.parametrize("low_memory, ld_dtype", [(False, np.float32), (True, np.float32), (True, np.int8)])
@pytest.mark.parametrize("n_models", [None, 5])
def test_metrics_against_dense_numpy(low_memory, ld_dtype, n_models):
    from viprs_amd.eval import pseudo_pearson_r, pseudo_r2
    rng = np.random.default_rng(3)
    panels = {1: _panel([40, 17], low_memory, ld_dtype, 1), 2: _panel([33], low_memory, ld_dtype, 2)}
    ld = {c: p[0] for c, p in panels.items()}
    beta = {c: 0.05 * rng.standard_normal((p[1].shape[0],) if n_models is None else (p[1].shape[0], n_models))
            for c, p in panels.items()}
    r = {c: 0.05 * rng.standard_normal(p[1].shape[0]) for c, p in panels.items()}
    rb = sum(beta[c].T @ r[c] for c in panels)
    bsb = sum(np.sum(beta[c] * (panels[c][1] @ beta[c]), axis=0) for c in panels)
    got = pseudo_pearson_r(ld, r, beta, dot_fn=R.dot_fn(None))
    np.testing.assert_allclose(got, rb / np.sqrt(bsb), rtol=1e-12)
    np.testing.assert_allclose(pseudo_r2(ld, r, beta, dot_fn=R.dot_fn(None)), rb ** 2 / bsb, rtol=1e-12)
    assert np.shape(got) == (() if n_models is None else (n_models,))
    # one chromosome handed over bare, and an object with .dot
    one = pseudo_r2(ld[2], r[2], beta[2], dot_fn=R.dot_fn(None))
    np.testing.assert_allclose(one, (beta[2].T @ r[2]) ** 2 / np.sum(beta[2] * (panels[2][1] @ beta[2]), axis=0), rtol=1e-12)

    class Dense:
        def __init__(self, M):
            self.M = M

        def dot(self, B):
            return self.M @ B
    np.testing.assert_allclose(pseudo_r2({c: Dense(p[1]) for c, p in panels.items()}, r, beta), rb ** 2 / bsb, rtol=1e-12)


def test_zero_column_gives_nan_and_streamlined_form():
    from viprs_amd.eval import _streamlined_pseudo_r2, pseudo_r2
    rng = np.random.default_rng(4)
    ld, dense = _panel([25, 30], True, np.float32, 5)
    beta = 0.1 * rng.standard_normal((55, 3))
    beta[:, 1] = 0.0
    r = 0.1 * rng.standard_normal(55)
    got = pseudo_r2(ld, r, beta, dot_fn=R.dot_fn(None))
    assert np.isnan(got[1]) and np.all(np.isfinite(got[[0, 2]]))
    want = (beta.T @ r) ** 2 / np.sum(beta * (dense @ beta), axis=0)
    np.testing.assert_allclose(got[[0, 2]], want[[0, 2]], rtol=1e-12)
    np.testing.assert_allclose(_streamlined_pseudo_r2(r, beta, dense @ beta)[[0, 2]], want[[0, 2]], rtol=1e-12)
    assert np.isnan(_streamlined_pseudo_r2(r, beta, dense @ beta)[1])
    with pytest.raises(ValueError):
        pseudo_r2(ld, r[:-1], beta, dot_fn=R.dot_fn(None))
    # a chromosome of the effects without validation betas or LD is an error, not a silently smaller score
    with pytest.raises(ValueError):
        pseudo_r2({1: ld, 2: ld}, {1: r}, {1: beta, 2: beta}, dot_fn=R.dot_fn(None))
    with pytest.raises(ValueError):
        pseudo_r2({1: ld}, {1: r, 2: r}, {1: beta, 2: beta}, dot_fn=R.dot_fn(None))


def test_pseudo_validate_without_a_panel_is_unchanged():
    """`validation_ld=None`: the same bits as the expression `VIPRS.pseudo_validate` has always evaluated."""
    from oracle import oracle as O
    from tests.test_fit import loader_from_fixture
    from viprs_amd.model import HyperparameterGrid, VIPRSGrid
    fx = np.load(os.path.join(HERE, "golden", "fitgrid_independent.npz"))
    gdl = loader_from_fixture(fx)
    grid = HyperparameterGrid(sigma_epsilon_steps=2, pi_steps=3, n_snps=gdl.m, h2_est=0.2, h2_se=0.1)
    m = VIPRSGrid(gdl, grid, low_memory=True, e_step_fn=O.cpp_e_step).fit(pathwise=True, max_iter=30)
    vb = {22: fx["validation_std_beta_22"]}
    b, r = np.asarray(m.post_mean_beta[22]), np.asarray(vb[22])
    rb = np.sum((b.T * r).T, axis=0)
    want = rb ** 2 / np.sum(b * (m.q[22] + m.post_mean_beta[22]), axis=0)
    assert np.array_equal(m.pseudo_validate(vb), want)
    assert np.array_equal(m.pseudo_validate(vb, validation_ld=None), want)
    # the host reference stands in for a panel object: same LD as the fit -> the same scores up to rounding
    up = syn.make_ld(fx["sizes_22"], low_memory=True, rho=fx["rho_22"])
    from viprs_amd.eval import pseudo_r2
    ext = pseudo_r2({22: (up.ld_left_bound, up.ld_indptr, up.ld_data, True, 1.0)}, vb, {22: b}, dot_fn=R.dot_fn(None))
    np.testing.assert_allclose(ext, want, rtol=2e-4)
