"""CPU: the model layer of `Lassosum` through the `sweep_fn` hook (`enet_sweep_host`) on two chromosomes, 3 lambda x
s = (0.5, 1.0): layout and `grid_table`, the closed form of s = 1, the warm-started path against cold starts, a diverged
column, `select_best` by validation R^2 and `predict()`."""
import copy

import numpy as np
import pytest

from tests import enet_replay as ER
from tests.test_clump_model import _merged, _validation_loader
from viprs_amd.model import Lassosum
from viprs_amd.stats import enet as EN

f32 = np.float32
N_LAM = len(ER.MODEL_LAMBDAS)


def _std_beta(gdl):
    return np.concatenate([np.asarray(gdl.sumstats_table[c].get_snp_pseudo_corr(), dtype=f32) for c in sorted(gdl.shapes)])


def test_layout_grid_table_and_closed_form():
    model = ER.model_fit()
    gdl = model.gdl
    assert model.n_models == 6 and {c: b.shape for c, b in model.post_mean_beta.items()} == {1: (194, 6), 2: (201, 6)}
    assert all(b.dtype == f32 for b in model.post_mean_beta.values())
    t = model.grid_table
    assert list(t.columns) == ["s", "lambda", "n_sweeps", "converged", "diverged", "n_nonzero", "objective"]
    assert t["s"].tolist() == [0.5] * 3 + [1.0] * 3 and t["lambda"].tolist() == list(ER.MODEL_LAMBDAS) * 2
    assert t["converged"].all() and not t["diverged"].any()
    assert all(2 < n < 200 for n in t["n_sweeps"][:3]) and t["n_sweeps"][3:].tolist() == [0, 0, 0]
    B = np.concatenate([model.post_mean_beta[c] for c in (1, 2)])
    assert t["n_nonzero"].tolist() == np.count_nonzero(B, axis=0).tolist()
    # a sparser model at a larger penalty; the path thins out but is neither empty nor full
    nz = np.array(t["n_nonzero"]).reshape(2, 3)
    assert np.all(np.diff(nz, axis=1) > 0) and 0 < nz.min() and nz.max() < gdl.m
    # s = 1: soft(std_beta, lambda)
    b = _std_beta(gdl)
    for k, lam in enumerate(ER.MODEL_LAMBDAS):
        a = np.abs(b) - f32(lam)
        want = np.where(a > 0, np.copysign(a, b), f32(0)).astype(f32)
        assert np.array_equal(B[:, N_LAM + k], want), lam
    # the objective of the table is the objective of the effects
    lb, ip, data, _ = _merged(gdl, np.int8)
    R = ER.dense_matrix(lb, ip, data, True, 1.0 / 127.0)
    for i, row in t.iterrows():
        x = B[:, i].astype(np.float64)
        s = 1.0 - float(f32(1.0 - row["s"]))
        want = x @ (((1 - s) * R + s * np.eye(gdl.m)) @ x) - 2 * x @ b.astype(np.float64) + 2 * float(f32(row["lambda"])) * np.abs(x).sum()
        assert np.isclose(row["objective"], want, rtol=1e-4, atol=1e-7), i


def test_warm_started_path_reaches_the_cold_start_fixed_points():
    """Every column of the path and the same (s, lambda) swept from eta = q = 0 on its own: both within the KKT bound
    (4 x the violation measured at a fixed point of the replay, tests/enet_replay.py), so -- the objective is strongly
    convex with modulus s -- no further apart than 2 sqrt(m) bound / s."""
    model = ER.model_fit()
    gdl = model.gdl
    lb, ip, data, _ = _merged(gdl, np.int8)
    m, b, s = gdl.m, _std_beta(gdl), 0.5
    R = ER.dense_matrix(lb, ip, data, True, 1.0 / 127.0)
    B = np.concatenate([model.post_mean_beta[c] for c in (1, 2)])
    mult = np.full(m, f32(1.0 - s))
    for k, lam in enumerate(ER.MODEL_LAMBDAS):
        pen = np.full(m, f32(lam))
        eta, q = np.zeros(m, dtype=f32), np.zeros(m, dtype=f32)
        for n in range(1, 401):
            ed, _, _ = ER.replay_sweep(lb, ip, data, True, b, mult, pen, eta, q, 1.0 / 127.0)
            if np.abs(ed).max() <= ER.MODEL_TOL:
                break
        assert n < 400
        v_cold = ER.kkt_violation(R, b, eta, s, float(pen[0]))
        v_path = ER.kkt_violation(R, b, B[:, k], s, float(pen[0]))
        print(f"lambda = {lam}: cold start {n} sweeps, KKT violation {v_cold:.2e}; path column {v_path:.2e}; "
              f"max |difference| {np.abs(eta - B[:, k]).max():.2e}")
        assert v_cold < ER.KKT_BOUND_ANY and v_path < ER.KKT_BOUND_ANY
        assert np.linalg.norm(eta.astype(np.float64) - B[:, k]) <= 2 * np.sqrt(m) * ER.KKT_BOUND_ANY / s
        # warm starts pay: fewer sweeps than the cold start from the second lambda on
        if k > 0:
            assert model.grid_table["n_sweeps"][k] <= n


def test_diverged_column():
    """A column whose eta stops being finite at the second lambda: reported, zero from there on, out of the sweeps."""
    calls = []

    def sweep_fn(lb, ip, data, low_memory, std_beta, mult, penalty, eta, q, dq_scale):
        lam = float(penalty[0])
        calls.append((float(mult[0]), lam))
        out = EN.enet_sweep_host(lb, ip, data, low_memory, std_beta, mult, penalty, eta, q, dq_scale)
        if mult[0] == f32(0.8) and lam == float(f32(ER.MODEL_LAMBDAS[1])):
            eta[3] = np.inf
        return out

    model = Lassosum(ER.model_gdl(), s=(0.2, 0.5), lambdas=ER.MODEL_LAMBDAS, tol=1e-4, dequantize_on_the_fly=True,
                     sweep_fn=sweep_fn).fit()
    t = model.grid_table
    assert t["diverged"].tolist() == [False, True, True, False, False, False]
    assert t["converged"].tolist() == [True, False, False, True, True, True]
    assert t["n_sweeps"][1] == 1 and t["n_sweeps"][2] == 0 and t["n_nonzero"][1:3].tolist() == [0, 0]
    B = np.concatenate([model.post_mean_beta[c] for c in (1, 2)])
    assert np.all(np.isfinite(B)) and not B[:, 1:3].any() and B[:, 0].any() and B[:, 3:].any(axis=0).all()
    lam1, lam2 = (float(f32(l)) for l in ER.MODEL_LAMBDAS[1:])
    assert (float(f32(0.8)), lam1) in calls and (float(f32(0.8)), lam2) not in calls and (0.5, lam2) in calls
    # the other column is what it is without the diverged one beside it
    alone = Lassosum(ER.model_gdl(), s=(0.5,), lambdas=ER.MODEL_LAMBDAS, tol=1e-4, dequantize_on_the_fly=True,
                     sweep_fn=EN.enet_sweep_host).fit()
    assert np.array_equal(np.concatenate([alone.post_mean_beta[c] for c in (1, 2)]), B[:, 3:])


def test_select_best_by_validation_and_predict():
    model = copy.deepcopy(ER.model_fit())
    gdl = model.gdl
    grid = {c: b.copy() for c, b in model.post_mean_beta.items()}
    val = _validation_loader(gdl, model, planted=1)
    prs = model.predict(test_gdl=val)
    assert prs.shape == (150, 6) and np.all(np.isfinite(prs))
    assert model.select_best(validation_gdl=val) is model
    r = np.asarray(model.validation_result["Validation_R2"])
    assert r.shape == (6,) and model.best_model_idx == int(np.argmax(r)) == 1 and r[1] > 0.99
    assert all(np.array_equal(model.post_mean_beta[c], grid[c][:, 1]) for c in grid) and model.n_models == 1
    assert model.predict(test_gdl=val).shape == (150,)
    assert list(model.to_table().columns) == ["CHR", "IDX", "BETA"]


def test_refusals():
    gdl = ER.model_gdl()

    class TwoRanks:
        world_size, rank = 2, 0
    with pytest.raises(NotImplementedError, match="world_size"):
        Lassosum(gdl, sweep_fn=EN.enet_sweep_host, comm=TwoRanks())
    for kw in (dict(s=[0.0]), dict(s=[1.5]), dict(lambdas=[]), dict(lambdas=[-1.0]), dict(float_precision="float64"),
               dict(penalty_factor=np.ones(3)), dict(max_sweeps=0)):
        with pytest.raises(ValueError):
            Lassosum(gdl, sweep_fn=EN.enet_sweep_host, **kw)
    model = Lassosum(gdl, sweep_fn=EN.enet_sweep_host)
    assert model.n_models == 80 and model.lambdas.shape == (20,) and model.post_mean_beta is None
    from viprs_amd import _lib
    if _lib.device_count() < 1:
        with pytest.raises(RuntimeError, match="HIP device"):
            Lassosum(gdl)
