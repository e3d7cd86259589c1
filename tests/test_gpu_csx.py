"""GPU: PRS-CSx (abi_csx.hip) against the host definition `viprs_amd.stats.csx` -- one population `==`
`viprs_state_cs_update`; several populations against `csx_update_host` fed the variates the device used (delta and the
closed-form rows `==`, the sampler's rows within one float32 ulp, the attempt counts `==`); the cap never reached over 2^22
draws; the floor, NaN, the moments of 2^20 draws; the sums `==` a host replay of THE ORDER; unlisted columns; determinism;
the chain across P streams `==` the C sweep replay fed the device's logs; `PRSCSx.fit()` against the host backend; the refusals."""
import numpy as np
import pytest

from tests import gibbs_replay as GR
from tests.test_gpu_cs import CS_OUT, INPUTS, SEED, SWEPT, VAR, _bits, _diag_plan, _junk_state, _open_state
from tests.test_gpu_gibbs import E2E_CHROMS, SIZES, _problem
from viprs_amd.stats import cs as CS
from viprs_amd.stats import csx as CX

pytestmark = pytest.mark.gpu
f32 = np.float32


def _row_of(m, P, overlap, rng):
    """P populations of m SNPs each: 'full' -- one SNP set (populations 1.. in a permuted order); 'partial' -- population k
    shifted by k * ceil(m / 3) union rows; 'none' -- disjoint."""
    step = {"full": 0, "partial": -(-m // 3), "none": m}[overlap]
    mu = m + (P - 1) * step
    row_of = np.full((P, mu), -1, dtype=np.int64)
    for k in range(P):
        row_of[k, k * step:k * step + m] = np.arange(m) if k == 0 else rng.permutation(m)
    return row_of


class _Coupled:
    """P junk states on P diagonal plans (P streams) and their coupling."""

    def __init__(self, m, P, overlap, G, seed, row_of=None, junk=None):
        from viprs_amd.plan import DeviceCoupling
        rng = np.random.default_rng(seed)
        self.row_of = _row_of(m, P, overlap, rng) if row_of is None else row_of
        self.junk = [_junk_state(m, G, seed + 10 * k) for k in range(P)] if junk is None else junk
        self.plans, self.states, self.coupling = [], [], None
        try:
            for j in self.junk:
                self.plans.append(_diag_plan(j["n"].shape[0]))
                self.states.append(_open_state(self.plans[-1], j))
            self.coupling = DeviceCoupling(self.states, self.row_of)
        except Exception:
            self.close()
            raise
        mu = self.row_of.shape[1]
        self.psi0 = np.asfortranarray(rng.uniform(1e-3, 1.0, (mu, G)).astype(f32))
        self.delta0 = np.asfortranarray(rng.uniform(0.1, 5.0, (mu, G)).astype(f32))
        self.coupling.upload("psi", self.psi0)
        self.coupling.upload("delta", self.delta0)

    def close(self):
        if self.coupling is not None:
            self.coupling.close()
        for st in self.states:
            st.close()
        for p in self.plans:
            p.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def device(self):
        out = dict(psi=self.coupling.download("psi"), delta=self.coupling.download("delta"),
                   attempts=self.coupling.download("attempts"), members=[])
        for st in self.states:
            d = {k: st.cs_download(k) for k in CS_OUT + VAR}
            d.update({k: st.download(k) for k in INPUTS + ("eta",)})
            out["members"].append(d)
        return out

    def union_variates(self, dev):
        """(ub, z1, z2, e) over the union, from the planes of the first population carrying each SNP."""
        mu, G = self.psi0.shape
        out = [np.zeros((mu, G), dtype=f32, order="F") for _ in VAR]
        for k in reversed(range(len(self.states))):
            u = np.flatnonzero(self.row_of[k] >= 0)
            for o, name in zip(out, VAR):
                o[u] = dev["members"][k][name][self.row_of[k, u]]
        return out

    def host(self, params, psi_max, variates, draw_index, prepare_only=False):
        psi, delta = self.psi0.copy(order="F"), self.delta0.copy(order="F")
        members = [tuple(j[k].copy(order="F") for k in CS_OUT + INPUTS) for j in self.junk]
        attempts, capped = CX.csx_update_host(self.row_of, [j["n"] for j in self.junk], [j["eta"] for j in self.junk], psi, delta,
                                              members, params, psi_max, variates, SEED, draw_index, prepare_only)
        return dict(psi=psi, delta=delta, attempts=attempts, capped=capped, members=members)


def _params(cols, P, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([np.asarray(cols, dtype=np.float64)[:, None], 10.0 ** rng.uniform(-4, 0, (len(cols), 1)),
                           rng.uniform(0.5, 1.5, (len(cols), P))], axis=1)


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes(order="A") == b.tobytes(order="A")


def _ulp_apart(a, b):
    return np.abs(_bits(a).astype(np.int64) - _bits(b).astype(np.int64))


def _assert_against_host(c, dev, want, cols, psi_max=1.0):
    K = (c.row_of >= 0).sum(axis=0)
    one, many = np.flatnonzero(K == 1), np.flatnonzero(K >= 2)
    cols = list(cols)
    assert np.array_equal(_bits(dev["delta"]), _bits(want["delta"]))
    assert np.array_equal(_bits(dev["psi"][one]), _bits(want["psi"][one]))
    apart = _ulp_apart(dev["psi"][many], want["psi"][many])
    print(f"K >= 2: {many.shape[0] * len(cols)} draws, {int((apart != 0).sum())} one float32 ulp apart, largest distance "
          f"{int(apart.max()) if apart.size else 0} ulp; mean attempts "
          f"{float(dev['attempts'][many][:, cols].mean()) if many.size else 0:.3f}, longest {int(dev['attempts'].max())}")
    assert apart.size == 0 or apart.max() <= 1                       # no draw differs by more (a flipped accept would)
    assert np.array_equal(dev["attempts"], want["attempts"]) and want["capped"] == 0
    assert not dev["attempts"][one].any()
    undrawn = dev["attempts"][many][:, cols] == 0                    # two carrying populations, nothing drawn: B == 0, the floor
    assert np.all(dev["psi"][many][:, cols][undrawn] == f32(2.0 ** -40)) and (many.size == 0 or not undrawn.all())
    assert np.all(dev["psi"][:, cols] >= f32(2.0 ** -40)) and np.all(dev["psi"][:, cols] <= f32(psi_max))
    return one, many


@pytest.mark.parametrize("m", [1, 255, 256, 257, 2370])
@pytest.mark.parametrize("width", [1, 3], ids=["width1", "grid3"])
def test_one_population_equals_cs_update(gpu, m, width):
    """The identity map: every cs buffer and every field `==` `viprs_state_cs_update` on a state of its own."""
    cols = [0] if width == 1 else [2, 0]
    j = _junk_state(m, width, 300 + m)
    par = _params(cols, 1, m)
    plan = _diag_plan(m)
    try:
        ref = _open_state(plan, j)
        ref.cs_update(par[:, [0, 2, 1]], 0.9, seed=SEED, draw_index=3)
        want = {k: ref.cs_download(k) for k in CS_OUT + VAR}
        want.update({k: ref.download(k) for k in INPUTS + ("eta",)})
        ref.close()
    finally:
        plan.close()
    with _Coupled(m, 1, "full", width, 300 + m, junk=[j]) as c:
        c.coupling.upload("psi", j["psi"])
        c.coupling.upload("delta", j["delta"])
        c.coupling.update(par, 0.9, seed=SEED, draw_index=3)
        dev = c.device()
        ms, capped = c.coupling.last()
    for k in CS_OUT + VAR + INPUTS + ("eta",):
        assert np.array_equal(_bits(dev["members"][0][k]), _bits(want[k])), k
    assert np.array_equal(_bits(dev["psi"]), _bits(want["psi"])) and np.array_equal(_bits(dev["delta"]), _bits(want["delta"]))
    assert not dev["attempts"].any() and capped == 0 and ms > 0


@pytest.mark.parametrize("m", [1, 255, 256, 257, 2370])
@pytest.mark.parametrize("width", [1, 3], ids=["width1", "grid3"])
@pytest.mark.parametrize("P,overlap", [(2, "full"), (2, "partial"), (2, "none"), (3, "partial"), (4, "partial"), (4, "full")])
def test_update_against_the_host(gpu, m, width, P, overlap):
    cols = [0] if width == 1 else [2, 0]
    par = _params(cols, P, 7 * m + P)
    with _Coupled(m, P, overlap, width, 1000 + m + P) as c:
        c.coupling.update(par, 0.8, seed=SEED, draw_index=2 ** 33 + 5)
        dev = c.device()
        _, capped = c.coupling.last()
    assert capped == 0
    want = c.host(par, 0.8, c.union_variates(dev), 2 ** 33 + 5)
    ub = CS.cs_variates_host(SEED, 2 ** 33 + 5, c.row_of.shape[1], cols)[0]
    for a, g in enumerate(cols):
        assert np.array_equal(c.union_variates(dev)[0][:, g], ub[:, a])          # the variates of union SNP u, wherever it lands
    one, many = _assert_against_host(c, dev, want, cols, 0.8)
    if m > 1:                                                        # (one SNP: 'partial' has nothing to share)
        assert (many.size > 0) == (overlap != "none") and (overlap == "full") == (one.size == 0)
    for k, (st, j) in enumerate(zip(dev["members"], c.junk)):
        u = np.flatnonzero(c.row_of[k] >= 0)
        r = c.row_of[k, u]
        for a, g in enumerate(cols):
            p = dev["psi"][u, g].astype(np.float64)                  # the existing formulas on the DEVICE's psi32
            assert np.array_equal(_bits(st["psi"][r, g]), _bits(dev["psi"][u, g]))
            assert np.array_equal(_bits(st["delta"][r, g]), _bits(dev["delta"][u, g]))
            assert np.array_equal(_bits(st["mu_mult"][r, g]), _bits((p / (1.0 + p)).astype(f32)))
            assert np.array_equal(_bits(st["half_var_tau"][r, g]), _bits((j["n"][r] * (1.0 + 1.0 / p) / (2.0 * par[a, 2 + k])).astype(f32)))
            assert np.all(st["u_logs"][r, g] == 32.0)
        assert np.array_equal(_bits(st["eta"]), _bits(j["eta"]))
        if width == 3:                                               # column 1: junk that survives, in every state ...
            for name in CS_OUT + VAR + INPUTS:
                assert np.array_equal(_bits(st[name][:, 1]), _bits(j[name][:, 1])), name
    if width == 3:                                                   # ... and in the handle
        assert np.array_equal(_bits(dev["psi"][:, 1]), _bits(c.psi0[:, 1])) and np.array_equal(_bits(dev["delta"][:, 1]), _bits(c.delta0[:, 1]))
        assert not dev["attempts"][:, 1].any()


def test_update_where_the_walk_wraps(gpu):
    """32 columns of 70 001 union SNPs, two populations: more elements than the 8192 workgroups of 256 threads of one pass."""
    m, G = 70001, 32
    assert m * G > 8192 * 256
    cols = list(np.random.default_rng(9).permutation(G))
    par = _params(cols, 2, 3)
    with _Coupled(m, 2, "full", G, 77) as c:
        c.coupling.update(par, 0.75, seed=SEED, draw_index=3)
        dev = c.device()
        _, capped = c.coupling.last()
    want = c.host(par, 0.75, c.union_variates(dev), 3)
    _assert_against_host(c, dev, want, cols, 0.75)
    assert capped == 0 and dev["psi"].max() == f32(0.75) and (dev["psi"] < 0.75).any()
    u = np.arange(m)
    for st, k in zip(dev["members"], range(2)):
        assert np.array_equal(_bits(st["psi"][c.row_of[k, u]]), _bits(dev["psi"]))


def test_the_cap_is_never_reached_over_2_22_draws(gpu):
    """2^19 union SNPs x 8 columns, two populations, B spanning omega = sqrt(lam B) from about 1e-8 to 1e4."""
    m, G = 2 ** 19, 8
    rng = np.random.default_rng(21)
    B = 10.0 ** rng.uniform(-16, 8, (m, G))
    junk = []
    for k in range(2):
        j = _junk_state(m, G, 40 + k)
        j["n"] = np.full(m, 1e4)
        j["eta"] = np.asfortranarray(np.sqrt(B / 2e4).astype(f32))    # n eta^2 / sigma2 = B / 2 in each population
        junk.append(j)
    par = np.concatenate([np.arange(G, dtype=np.float64)[:, None], np.full((G, 1), 0.5), np.ones((G, 2))], axis=1)
    with _Coupled(m, 2, "full", G, 5, row_of=np.stack([np.arange(m), np.arange(m)]), junk=junk) as c:
        c.coupling.update(par, 1e30, seed=SEED, draw_index=11)
        ms, capped = c.coupling.last()
        att = c.coupling.download("attempts")
        psi, delta = c.coupling.download("psi"), c.coupling.download("delta")
    omega = np.sqrt(2.0 * delta.astype(np.float64) * B)
    print(f"2^22 draws in {ms:.3f} ms: n_capped {capped}, mean attempts {att.mean():.4f}, longest {att.max()}, omega "
          f"{omega.min():.2e} .. {omega.max():.2e}")
    assert capped == 0 and att.min() >= 1 and att.max() < CX.MAX_ATTEMPTS
    assert omega.min() < 1e-7 and omega.max() > 1e4 and np.all(np.isfinite(psi)) and np.all(psi > 0)


def test_the_floor_and_nan(gpu):
    m, G = 600, 2
    junk = [_junk_state(m, G, 60 + k) for k in range(2)]
    for j in junk:
        j["eta"][:100, 0] = 0.0                                      # B == 0 in both: the conditional is improper
        j["eta"][100:200, 0] = [0.0, -0.0] * 50
    junk[1]["eta"][100:200, 0] = 0.01                                # zero in one population only: a proper draw
    junk[0]["eta"][200:210, 0] = np.nan
    par = _params([0], 2, 8)
    with _Coupled(m, 2, "full", G, 6, row_of=np.stack([np.arange(m), np.arange(m)]), junk=junk) as c:
        c.coupling.update(par, 1.0, seed=SEED, draw_index=1)
        dev = c.device()
        _, capped = c.coupling.last()
    assert np.all(dev["psi"][:100, 0] == f32(2.0 ** -40)) and not dev["attempts"][:100, 0].any()
    assert np.all(dev["attempts"][100:200, 0] >= 1) and np.all(np.isfinite(dev["psi"][100:200, 0]))
    assert capped == 10 and np.all(dev["attempts"][200:210, 0] == CX.MAX_ATTEMPTS) and np.isnan(dev["psi"][200:210, 0]).all()
    for st in dev["members"]:
        assert np.isnan(st["psi"][200:210, 0]).all() and np.isnan(st["mu_mult"][200:210, 0]).all()
        assert np.all(np.isfinite(st["delta"][:, 0])) and np.all(st["mu_mult"][:100, 0] == f32(2.0 ** -40 / (1 + 2.0 ** -40)))
    want = c.host(par, 1.0, c.union_variates(dev), 1)
    assert want["capped"] == 10 and np.array_equal(dev["attempts"], want["attempts"])
    ok = np.setdiff1d(np.arange(m), np.arange(200, 210))
    assert _ulp_apart(dev["psi"][ok, 0], want["psi"][ok, 0]).max() <= 1


def test_moments_of_2_20_draws_at_index_zero(gpu):
    """Two populations, constant variates kept in the buffers (z2 = 0, e = 0.75, psi_old = 0.5, phi = 1: lam = 1) and a constant
    B = 1: 2^20 draws of GIG(0, 1, 1).  The sample means of X and 1 / X within 5 standard errors of the quadrature."""
    m = 2 ** 20
    junk = []
    for k in range(2):
        j = _junk_state(m, 1, 80 + k)
        j["n"] = np.full(m, 1e4)
        j["eta"] = np.full((m, 1), np.sqrt(0.5 / 1e4), dtype=f32, order="F")
        j["z2"][...], j["e"][...] = 0.0, 0.75
        junk.append(j)
    par = np.array([[0.0, 1.0, 1.0, 1.0]])
    with _Coupled(m, 2, "full", 1, 9, row_of=np.stack([np.arange(m), np.arange(m)]), junk=junk) as c:
        c.coupling.upload("psi", np.full((m, 1), 0.5, dtype=f32, order="F"))
        c.coupling.update(par, 1e30, seed=SEED, draw_index=4, keep_variates=True)
        x = c.coupling.download("psi")[:, 0].astype(np.float64)
        delta = c.coupling.download("delta")[:, 0]
        att = c.coupling.download("attempts")[:, 0]
        _, capped = c.coupling.last()
    assert np.all(delta == f32(0.5)) and capped == 0
    b = 2.0 * 1e4 * float(f32(np.sqrt(0.5 / 1e4))) ** 2              # B as the kernel forms it from the float32 eta
    m1, v1, i1, iv = CX.gig_moments(0.0, 1.0, b)
    z_x, z_inv = (x.mean() - m1) / np.sqrt(v1 / m), ((1.0 / x).mean() - i1) / np.sqrt(iv / m)
    print(f"GIG(0, 1, {b:.6f}): E X {x.mean():.6f} vs {m1:.6f} ({z_x:+.2f} se), E 1/X {(1 / x).mean():.6f} vs {i1:.6f} "
          f"({z_inv:+.2f} se); rejection share {1 - 1 / att.mean():.4f}, longest run {att.max()}")
    assert abs(z_x) < 5 and abs(z_inv) < 5
    assert 0.10 < 1 - 1 / att.mean() < 0.20                          # (0.177 on the host at p = 0, omega = 1)


def test_prepare_only_and_keep_variates(gpu):
    m, G, P = 2370, 3, 2
    par = _params([2, 0], P, 12)
    with _Coupled(m, P, "partial", G, 31) as c:
        c.coupling.update(par, prepare_only=True)
        dev = c.device()
        want = c.host(par, 1.0, None, 0, prepare_only=True)
        assert np.array_equal(_bits(dev["psi"]), _bits(c.psi0)) and np.array_equal(_bits(dev["delta"]), _bits(c.delta0))
        for st, j, w in zip(dev["members"], c.junk, want["members"]):
            for name in VAR:                                         # nothing is drawn
                assert np.array_equal(_bits(st[name]), _bits(j[name])), name
            for name, a in zip(CS_OUT + INPUTS, w):
                assert np.array_equal(_bits(st[name]), _bits(a)), name
        # KEEP_VARIATES: the uploaded junk of the first carrying population is what the update uses, and it stays
        c.coupling.update(par, seed=SEED, draw_index=1, keep_variates=True)
        dev = c.device()
        for st, j in zip(dev["members"], c.junk):
            for name in VAR:
                assert np.array_equal(_bits(st[name]), _bits(j[name])), name
        _assert_against_host(c, dev, c.host(par, 1.0, c.union_variates(dev), 1), [2, 0])


@pytest.mark.parametrize("m", [2370, 70001], ids=["one_pass", "two_passes"])
@pytest.mark.parametrize("width", [1, 3], ids=["width1", "grid3"])
def test_sums_equal_the_host_replay_of_the_order(gpu, m, width):
    cols = None if width == 1 else [2, 0]
    with _Coupled(m, 2, "partial", width, 55 + m) as c:
        got, again, one = c.coupling.sums(cols), c.coupling.sums(cols), c.coupling.sums([0])
        c.coupling.update(_params([0], 2, 1), seed=SEED, draw_index=0)
        after = c.coupling.sums(cols)
        dev = c.device()
        member_sums = [st.cs_sums(cols) for st in c.states]
    want = CX.csx_sums_host(c.psi0, c.delta0, cols)
    assert got.shape == (1 if width == 1 else 2, 2) and np.array_equal(got, want) and np.array_equal(got, again)
    assert np.array_equal(one[0], got[-1]) and np.all(got > 0)
    assert np.array_equal(after, CX.csx_sums_host(dev["psi"], dev["delta"], cols)) and not np.array_equal(after, got)
    # the unchanged cs_sums of each member state on what the update scattered
    for k, (st, j) in enumerate(zip(dev["members"], c.junk)):
        assert np.array_equal(member_sums[k], CS.cs_sums_host(j["n"], j["eta"], st["psi"], st["delta"], cols))


def test_determinism(gpu):
    par = _params([2, 0], 3, 5)
    runs = []
    for _ in range(2):
        with _Coupled(2370, 3, "partial", 3, 91) as c:
            c.coupling.update(par, seed=SEED, draw_index=6)
            runs.append(c.device())
    with _Coupled(2370, 3, "partial", 3, 91) as c:
        c.coupling.update(par[::-1], seed=SEED, draw_index=6)        # the columns listed in another order
        runs.append(c.device())
    with _Coupled(2370, 3, "partial", 3, 91) as c:
        c.coupling.update(par, seed=SEED + 1, draw_index=6)
        other = c.device()
    for b in runs[1:]:
        for name in ("psi", "delta", "attempts"):
            assert _same_bytes(runs[0][name], b[name]), name
        for x, y in zip(runs[0]["members"], b["members"]):
            assert all(np.array_equal(_bits(x[k]), _bits(y[k])) for k in x)
    assert not np.array_equal(runs[0]["psi"][:, 0], other["psi"][:, 0])


S2 = [[[0.9, 7.0, 1.1], [1.05, 7.0, 0.8], [0.7, 7.0, 1.0], [1.2, 7.0, 0.95]],        # population, iteration, column; column 1 is
      [[1.1, 7.0, 0.9], [0.95, 7.0, 1.2], [1.3, 7.0, 0.85], [0.8, 7.0, 1.05]]]       # the one nobody lists
PHI = [[1.0, 7.0, 1e-2], [0.3, 7.0, 1e-2], [0.05, 7.0, 1e-2], [0.02, 7.0, 1e-2]]
LISTED = [2, 0]


@pytest.mark.parametrize("ld_dtype", [np.float32, np.int8], ids=["f32", "i8"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_the_chain_across_streams(gpu, low_memory, ld_dtype):
    """Two populations on two plans (two streams), partial overlap, four iterations of (two sweeps, sums, coupled update) with
    nothing synchronised between a sweep and the update that reads its eta, nor between the update and the next sweeps:
    every field `==` the C sweep replay fed the logged Gibbs draws and the logged device (psi, delta)."""
    from viprs_amd.plan import DeviceCoupling, DeviceState, LDPlan
    ld, std_beta, n = _problem(low_memory, ld_dtype, tuple(SIZES))
    m, G = ld.m, 3
    rng = np.random.default_rng(17)
    betas = [std_beta, (std_beta + 0.01 * rng.standard_normal(m)).astype(f32)]
    ns = [n.astype(np.float64) * np.linspace(0.6, 1.4, m), 0.2 * n.astype(np.float64) * np.linspace(1.3, 0.7, m)]
    shift = m // 4
    row_of = np.full((2, m + shift), -1, dtype=np.int64)
    row_of[0, :m] = np.arange(m)
    row_of[1, shift:] = np.arange(m)
    rows = lambda i: np.array([[g, PHI[i][g], S2[0][i][g], S2[1][i][g]] for g in LISTED])
    start = np.array([[g, 1.0, 1.0, 1.0] for g in LISTED])
    active = np.array(LISTED, dtype=np.int32)
    plans, states, coupling = [], [], None
    draws, coupled, sums = [], [], []
    try:
        for b, nk in zip(betas, ns):
            plans.append(LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory))
            st = DeviceState(plans[-1], "float32", model="grid", width=G, placement="off")
            st.upload("std_beta", b)
            st.set_n_per_snp(nk)
            states.append(st)
        coupling = DeviceCoupling(states, row_of)
        coupling.update(start, prepare_only=True, sync=False)
        for i in range(4):
            for k, st in enumerate(states):
                st.gibbs_sweep(ld.dq_scale, active_model_idx=active, seed=SEED + k, draw_index=i, sync=False)
            coupling.update(rows(i), seed=SEED, draw_index=i, sync=False)
            draws.append([(st.gibbs_download("unif"), st.gibbs_download("noise")) for st in reversed(states)][::-1])
            coupled.append((coupling.download("psi"), coupling.download("delta")))
            sums.append((coupling.sums(LISTED), [st.cs_sums(LISTED) for st in states]))
        got = [{k: st.download(k) for k in SWEPT + INPUTS} for st in states]
        for g, st in zip(got, states):
            g.update({k: st.cs_download(k) for k in CS_OUT})
        assert coupling.last()[1] == 0
    finally:
        if coupling is not None:
            coupling.close()
        for st in states:
            st.close()
        for p in plans:
            p.close()
    z = lambda mk: np.zeros((mk, G), dtype=f32, order="F")
    h = [{k: z(m) for k in SWEPT + INPUTS + CS_OUT} for _ in range(2)]
    for x in h:
        x["psi"][...] = 1                                            # the cs buffers of a fresh state
    psi, delta = np.ones((m + shift, G), dtype=f32, order="F"), z(m + shift)
    scatter = lambda par: CX.csx_update_host(row_of, ns, [x["eta"] for x in h], psi, delta,
                                             [tuple(x[k] for k in CS_OUT + INPUTS) for x in h], par, prepare_only=True)
    scatter(start)
    for i in range(4):
        for k in range(2):
            unif, noise = draws[i][k]
            for g in LISTED:
                eta, q = h[k]["eta"][:, g].copy(), h[k]["q"][:, g].copy()
                _, mu, gam = GR.replay_sweep(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory, betas[k], h[k]["mu_mult"][:, g],
                                             h[k]["half_var_tau"][:, g], h[k]["u_logs"][:, g], unif[:, g].copy(), noise[:, g].copy(),
                                             eta, q, ld.dq_scale)
                for name, v in zip(SWEPT, (eta, q, mu, gam)):
                    h[k][name][:, g] = v
        psi[:, LISTED], delta[:, LISTED] = coupled[i][0][:, LISTED], coupled[i][1][:, LISTED]
        scatter(rows(i))
        assert np.array_equal(sums[i][0], CX.csx_sums_host(psi, delta, LISTED))
        for k in range(2):
            assert np.array_equal(sums[i][1][k], CS.cs_sums_host(ns[k], h[k]["eta"], h[k]["psi"], h[k]["delta"], LISTED))
    for k in range(2):
        for name in SWEPT + CS_OUT + INPUTS:
            assert np.array_equal(_bits(got[k][name]), _bits(h[k][name])), (k, name, int((_bits(got[k][name]) != _bits(h[k][name])).sum()))
        assert np.all(got[k]["eta"][:, LISTED] != 0) and not got[k]["eta"][:, 1].any()
    assert len(np.unique(psi[:, LISTED])) > m // 2                   # the scales moved


def _tables(gdl):
    gdl.snp_table = {c: {"SNP": np.array([f"rs{c}_{j}" for j in range(m)])} for c, m in gdl.shapes.items()}
    return gdl


def test_prscsx_fit_equals_the_host_fit(gpu):
    """Short chains, 3 columns (fixed, auto, fixed), two populations of 1 995 SNPs: the device fit against the same fit on the host
    backend (the C sweep replay as `sweep_fn`), fed the Gibbs draws and the (psi, delta) the device used."""
    from viprs_amd.model import PRSCSx
    from viprs_amd.data import SumstatsArrays

    def gdls():
        a, b = _tables(GR.model_gdl(E2E_CHROMS)), _tables(GR.model_gdl(E2E_CHROMS, n=1e4))
        rng = np.random.default_rng(3)
        for c, s in b.sumstats_table.items():
            v = np.asarray(s.get_snp_pseudo_corr(), dtype=np.float64)
            b.sumstats_table[c] = SumstatsArrays((v + 0.01 * rng.standard_normal(v.shape[0])).astype(f32), s.n_per_snp)
        return {"EUR": a, "EAS": b}
    kw = dict(phi=(1e-2, None, 1.0), n_iter=14, n_burnin=4, thin=2, seed=11, dequantize_on_the_fly=True)
    dev = PRSCSx(gdls(), keep_draws_log=True, **kw).fit()
    assert len(dev.coupled_log) == 14 and all(len(v) == 14 for v in dev.draws_log.values()) and dev.n_capped_total == 0
    host = PRSCSx(gdls(), sweep_fn=GR.replay_sweep,
                  draws_fn={name: (lambda seed, i, hvt, cols, log=log: log[i]) for name, log in dev.draws_log.items()},
                  coupled_fn=lambda i, cols: dev.coupled_log[i], **kw).fit()
    for name in dev.populations:
        for c in host.post_mean_beta[name]:
            assert np.array_equal(dev.post_mean_beta[name][c], host.post_mean_beta[name][c]), (name, c)
            assert dev.post_mean_beta[name][c].shape[1] == 3 and dev.post_mean_beta[name][c].any(axis=0).all()
        assert np.array_equal(dev.sigma2_history[name], host.sigma2_history[name])
    assert dev.grid_table.equals(host.grid_table) and not dev.grid_table["diverged"].any()
    assert np.array_equal(dev.phi_history, host.phi_history) and len(np.unique(dev.phi_history[:, 1])) == 14
    assert np.array_equal(dev.meta_beta(), host.meta_beta())


CREATE_REFUSALS = ["float64", "spike_slab", "mixture", "masked_grid", "comm", "no_n_per_snp", "widths", "state_twice",
                   "row_uncarried", "row_out_of_range", "row_negative", "row_twice", "wide"]
UPDATE_REFUSALS = ["column_out_of_range", "column_twice", "sigma2_zero", "sigma2_nan", "phi_negative", "phi_inf",
                   "psi_max_small", "psi_max_inf", "unknown_flag", "null_params"]


@pytest.mark.parametrize("case", CREATE_REFUSALS)
def test_create_refusals(gpu, case):
    """Each is a ValueError (VIPRS_EINVAL) and leaves no handle.  (States on different devices need two devices: not run.)"""
    from viprs_amd.plan import DeviceCoupling, DeviceState
    m = 300
    plans, states, comm = [_diag_plan(m), _diag_plan(m)], [], None
    try:
        kind = {"float64": dict(float_precision="float64", model="grid", width=2), "spike_slab": {},
                "mixture": dict(model="mixture", width=2), "widths": dict(model="grid", width=3),
                "wide": dict(model="grid", width=2 ** 16)}.get(case, dict(model="grid", width=2))
        if case == "wide":
            plans = [_diag_plan(1), _diag_plan(1)]
            m = 1
        states.append(DeviceState(plans[0], placement="off", **(dict(model="grid", width=2 ** 16) if case == "wide" else
                                                                 dict(model="grid", width=2))))
        states.append(DeviceState(plans[1], placement="off", **kind))
        if case == "masked_grid":
            states[1].set_groups([0, 130, m])
            states[1].set_group_columns(np.array([[1, 0], [1, 1]], dtype=np.uint8))
        if case == "comm":
            from viprs_amd.parallel import RcclComm
            comm = RcclComm(rank=0, world_size=1, device=0)
            states[1].set_comm(comm)
        states[0].set_n_per_snp(np.full(m, 5e4))
        if case != "no_n_per_snp":
            states[1].set_n_per_snp(np.full(m, 5e4))
        row_of = np.stack([np.arange(m), np.arange(m)]).astype(np.int64)
        if case == "row_uncarried":
            row_of = np.concatenate([row_of, [[-1], [-1]]], axis=1)
        if case == "row_out_of_range":
            row_of[1, 7] = m
        if case == "row_negative":
            row_of[1, 7] = -2
        if case == "row_twice":
            row_of[1, 7] = row_of[1, 8]
        use = [states[0], states[0]] if case == "state_twice" else states
        with pytest.raises(ValueError, match="PRS-CS"):
            DeviceCoupling(use, row_of)
        if case != "wide":
            good = DeviceCoupling([states[0]], row_of[:1, :m])       # the states are still usable
            good.close()
    finally:
        for st in states:
            st.close()
        if comm is not None:
            comm.close()
        for p in plans:
            p.close()


@pytest.mark.parametrize("case", UPDATE_REFUSALS)
def test_update_refusals_launch_nothing(gpu, case):
    from viprs_amd import _lib as L
    from viprs_amd.plan import _ptr
    good = np.array([[0, 0.5, 1.0, 1.0], [1, 0.5, 1.0, 1.0]])
    bad = {"column_out_of_range": [[0, 0.5, 1.0, 1.0], [2, 0.5, 1.0, 1.0]], "column_twice": [[1, 0.5, 1.0, 1.0], [1, 0.5, 1.0, 1.0]],
           "sigma2_zero": [[0, 0.5, 1.0, 0.0]], "sigma2_nan": [[0, 0.5, np.nan, 1.0]], "phi_negative": [[0, -0.5, 1.0, 1.0]],
           "phi_inf": [[0, np.inf, 1.0, 1.0]]}
    params = np.array(bad.get(case, good), dtype=np.float64)
    psi_max = {"psi_max_small": 2.0 ** -40, "psi_max_inf": np.inf}.get(case, 1.0)
    with _Coupled(300, 2, "partial", 2, 3) as c:
        before = c.device()
        with pytest.raises(ValueError, match="PRS-CSx"):
            if case == "unknown_flag":
                L.check(L.lib.viprs_csx_update(c.coupling._h, 2, _ptr(params), 1.0, 1, 2, 4, 1))
            elif case == "null_params":
                L.check(L.lib.viprs_csx_update(c.coupling._h, 2, None, 1.0, 1, 2, 0, 1))
            else:
                c.coupling.update(params, psi_max, seed=1, draw_index=2)
        out = np.full((2, 2), -7.0)
        if case in ("column_out_of_range", "column_twice"):
            cols = np.array(params[:, 0], dtype=np.int32)
            assert L.lib.viprs_csx_sums(c.coupling._h, 2, _ptr(cols), _ptr(out)) == L.EINVAL and "PRS-CSx" in L.last_error()
        assert L.lib.viprs_csx_sums(c.coupling._h, 1, None, _ptr(out)) == L.EINVAL                 # NULL lists every column
        assert L.lib.viprs_csx_sums(c.coupling._h, 2, None, None) == L.EINVAL
        assert L.lib.viprs_csx_download(c.coupling._h, 3, _ptr(out)) == L.EINVAL
        assert L.lib.viprs_csx_upload(c.coupling._h, 0, None) == L.EINVAL
        assert np.all(out == -7.0)
        with pytest.raises(ValueError, match="no timed PRS-CSx update"):
            c.coupling.last()
        after = c.device()
        for name in ("psi", "delta", "attempts"):
            assert _same_bytes(before[name], after[name]), name
        for x, y in zip(before["members"], after["members"]):
            assert all(np.array_equal(_bits(x[k]), _bits(y[k])) for k in x)


def test_an_empty_union(gpu):
    from viprs_amd.plan import DeviceCoupling, DeviceState, LDPlan
    empty = LDPlan(np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.float32), False)
    try:
        st = DeviceState(empty, "float32", model="grid", width=2, placement="off")
        c = DeviceCoupling([st], np.zeros((1, 0), dtype=np.int64))
        c.update(np.array([[0, 1.0, 1.0]]), prepare_only=True)
        c.update(np.array([[1, 1.0, 1.0]]))
        assert not c.sums().any() and c.download("psi").shape == (0, 2)
        c.close()
        st.close()
    finally:
        empty.close()
