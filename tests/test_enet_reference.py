"""CPU: the elastic-net sweep's host definition (`viprs_amd.stats.enet`) against the C replay (tests/enet_replay.c, libm
`fmaf`), its closed forms, the fixed points of the sweep and their KKT violation against the dense blocks, the sums."""
import ctypes
import ctypes.util
import functools

import numpy as np
import pytest

from tests import enet_replay as ER
from viprs_amd.stats import enet as EN
from viprs_amd.utils import synthetic as syn

f32 = np.float32


def soft(x, pen):
    a = np.abs(x) - pen
    return np.where(a > 0, np.copysign(a, x), f32(0.0)).astype(f32)


def test_fma32_is_libm_fmaf():
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rng = np.random.default_rng(3)
    n = 20000
    a = rng.standard_normal(n).astype(f32)
    b = rng.standard_normal(n).astype(f32)
    c = (rng.standard_normal(n) * 10.0 ** rng.integers(-8, 3, n)).astype(f32)
    # a float64 sum that lands exactly halfway between two float32 values while the true value lies above it -- what two
    # roundings get wrong: (1 + x)(1 - x + x^2) = 1 + x^3, so a b = 2^-24 (1 + x^3) and c + a b = 1 + 2^-24 + 2^-24 x^3
    x = 2.0 ** -rng.integers(10, 12, 4000)
    scale = 2.0 ** rng.integers(-20, 20, 4000) * np.where(rng.random(4000) < 0.5, -1.0, 1.0)
    a[:4000] = (scale * 2.0 ** -24 * (1.0 + x)).astype(f32)
    b[:4000] = (1.0 - x + x * x).astype(f32)
    c[:4000] = scale.astype(f32)
    a[-3:], b[-3:], c[-3:] = [np.inf, 1e30, 0.0], [1.0, 1e30, 5.0], [1.0, 1.0, -0.0]
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=f32)
    got = EN.fma32(a, b, c)
    with np.errstate(over="ignore"):
        naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)
    assert got.dtype == f32 and np.array_equal(got, want, equal_nan=True)
    assert (naive[:4000] != want[:4000]).all()                     # the cases do separate one rounding from two


@pytest.mark.parametrize("sweep", [EN.enet_sweep_host, ER.replay_sweep], ids=["host", "replay"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_closed_forms(sweep, low_memory):
    ld, ss, inp = syn.make_problem(sizes=[130, 64, 1], low_memory=low_memory, seed=5, kind="longrange")
    m = ld.m
    rng = np.random.default_rng(2)
    pen = np.abs(0.004 * rng.standard_normal(m)).astype(f32)
    # c = 0: one sweep from eta = 0 gives soft(std_beta, pen) whatever the LD and whatever q
    eta, q = np.zeros(m, dtype=f32), (0.01 * rng.standard_normal(m)).astype(f32)
    ed, mu, gam = sweep(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, low_memory, inp.std_beta, np.zeros(m, dtype=f32), pen, eta,
                        q, ld.dq_scale)
    want = soft(inp.std_beta, pen)
    assert np.array_equal(eta, want) and np.array_equal(ed, want) and np.array_equal(mu, inp.std_beta)
    assert np.array_equal(gam, (want != 0).astype(f32)) and 0 < np.count_nonzero(want) < m
    # LD with zero off-diagonals: q stays 0, the result is the same for any c, sweep after sweep
    if low_memory:
        lb, ip, data = np.minimum(np.arange(1, m + 1), m - 1).astype(np.int32), np.zeros(m + 1, dtype=np.int64), np.zeros(0, dtype=f32)
    else:
        lb, ip, data = np.arange(m, dtype=np.int32), np.arange(m + 1, dtype=np.int64), np.ones(m, dtype=f32)
    for c in (0.0, 0.3, 1.0):
        eta, q = np.zeros(m, dtype=f32), np.zeros(m, dtype=f32)
        for _ in range(2):
            sweep(lb, ip, data, low_memory, inp.std_beta, np.full(m, c, dtype=f32), pen, eta, q, 1.0)
        assert np.array_equal(eta, want) and not q.any(), c


@pytest.mark.parametrize("ld_dtype", [np.float32, np.int8, np.int16], ids=["f32", "i8", "i16"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_host_sweep_equals_the_replay(low_memory, ld_dtype):
    ld, ss, inp = syn.make_problem(sizes=[130, 64, 1], low_memory=low_memory, ld_dtype=ld_dtype, seed=5, kind="longrange")
    m = ld.m
    rng = np.random.default_rng(1)
    for G in (None, 3):
        shape = (m,) if G is None else (m, G)
        mk = lambda a: np.asfortranarray(np.broadcast_to(a, (m, G or 1)).reshape(shape).astype(f32))
        mult = mk(np.array([0.8, 0.5, 0.1][:G or 1], dtype=f32))
        pen = mk(np.array([0.002, 0.005, 0.003][:G or 1], dtype=f32))
        e1, q1 = (np.asfortranarray((0.01 * rng.standard_normal(shape)).astype(f32)) for _ in range(2))
        e2, q2 = e1.copy(order="F"), q1.copy(order="F")
        for _ in range(3):
            a = ER.replay_sweep(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, low_memory, inp.std_beta, mult, pen, e1, q1, ld.dq_scale)
            b = EN.enet_sweep_host(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, low_memory, inp.std_beta, mult, pen, e2, q2, ld.dq_scale)
        assert np.array_equal(e1, e2) and np.array_equal(q1, q2)
        assert all(x.shape == shape and np.array_equal(x, y) for x, y in zip(a, b))
        assert 0.1 < np.count_nonzero(e1) / e1.size < 0.95
        # the sums: the ordered float64 reduction is within rounding of the plain one, and exact where it must be
        sums = EN.enet_sums_host(inp.std_beta, pen, e1, q1, a[0])
        E, Q, D, P = (np.asarray(x, dtype=np.float64).reshape(m, -1) for x in (e1, q1, a[0], pen))
        b64 = inp.std_beta.astype(np.float64)[:, None]
        plain = np.stack([np.abs(D).max(0), (b64 * E).sum(0), (Q * E).sum(0), (E * E).sum(0), (P * np.abs(E)).sum(0),
                          (E != 0).sum(0)], axis=1)
        assert sums.shape == plain.shape and np.array_equal(sums[:, [0, 5]], plain[:, [0, 5]])
        assert np.allclose(sums, plain, rtol=1e-13, atol=1e-18)
        s = 1.0 - mult.reshape(m, -1)[0].astype(np.float64)
        assert np.allclose(EN.enet_objective(sums, s), (1 - s) * (plain[:, 2] + plain[:, 3]) + s * plain[:, 3] - 2 * plain[:, 1]
                           + 2 * plain[:, 4], rtol=1e-12)


def test_sums_order_over_many_workgroups():
    """A row of more SNPs than 256 workgroups hold: grid rows take 256 workgroups, the others up to 1024."""
    rng = np.random.default_rng(9)
    m = 256 * 300 + 17
    v = [rng.standard_normal(m).astype(f32) for _ in range(5)]
    one = EN.enet_sums_host(v[0], np.abs(v[1]), v[2], v[3], v[4])
    as_grid = EN.enet_sums_host(v[0], np.abs(v[1]), v[2], v[3], v[4], grid=True)
    assert one.shape == as_grid.shape == (1, 6) and np.allclose(one, as_grid, rtol=1e-12)
    assert np.array_equal(one[:, [0, 5]], as_grid[:, [0, 5]]) and not np.array_equal(one, as_grid)
    nan = v[4].copy()
    nan[5] = np.nan
    assert EN.enet_sums_host(v[0], np.abs(v[1]), v[2], v[3], nan)[0, 0] == np.abs(np.delete(v[4], 5)).max()
    assert np.array_equal(EN.enet_sums_host(v[0][:0], v[1][:0], v[2][:0], v[3][:0], v[4][:0]), np.zeros((1, 6)))


def test_lambda_path():
    lam = EN.lambda_path()
    assert lam.shape == (20,) and np.isclose(lam[0], 0.1) and np.isclose(lam[-1], 0.001) and np.all(np.diff(lam) < 0)
    assert np.allclose(lam[1:] / lam[:-1], lam[1] / lam[0])
    assert np.allclose(EN.lambda_path(0.01, 1.0, 3), [1.0, 0.1, 0.01])
    with pytest.raises(ValueError):
        EN.lambda_path(0.0, 1.0, 3)


@functools.lru_cache(maxsize=None)
def _big():
    ld, ss, inp = syn.make_problem(sizes=[1601, 130, 64, 1], seed=53, kind="longrange")
    return ld, inp.std_beta, ER.dense_matrix(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, False)


@pytest.mark.parametrize("s, lam", [(0.9, 0.005), (0.9, 0.012)])
def test_fixed_point_and_its_kkt_violation(s, lam):
    """Measured with the replay (EXPERIMENTS.md, "Lassosum"): fixed points after 136 and 104 sweeps, KKT violation 2.14e-6
    and 1.33e-6; the bound is 4 x the measurement of the case (tests/enet_replay.py)."""
    ld, std_beta, R = _big()
    m = ld.m
    mult, pen = np.full(m, f32(1.0 - s)), np.full(m, f32(lam))
    eta, q, n = ER.to_fixed_point(ER.replay_sweep, ld, std_beta, mult, pen, max_sweeps=400)
    viol = ER.kkt_violation(R, std_beta, eta, 1.0 - float(mult[0]), float(pen[0]))
    print(f"(s, lambda) = ({s}, {lam}): fixed point after {n} sweeps, KKT violation {viol:.3e}, "
          f"{np.count_nonzero(eta) / m:.3f} of eta non-zero")
    assert n <= 400 and 0 < np.count_nonzero(eta) < m
    assert viol < ER.KKT_BOUND[(s, lam)]


def test_host_sweep_equals_the_replay_on_the_large_block():
    ld, std_beta, _ = _big()
    m = ld.m
    mult, pen = np.full(m, f32(0.1)), np.full(m, f32(0.005))
    state = [(np.zeros(m, dtype=f32), np.zeros(m, dtype=f32)) for _ in range(2)]
    for _ in range(2):
        out = [fn(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, False, std_beta, mult, pen, e, q, 1.0)
               for fn, (e, q) in zip((ER.replay_sweep, EN.enet_sweep_host), state)]
    assert all(np.array_equal(x, y) for x, y in zip(out[0], out[1]))
    assert np.array_equal(state[0][0], state[1][0]) and np.array_equal(state[0][1], state[1][1])
