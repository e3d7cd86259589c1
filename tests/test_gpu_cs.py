"""GPU: PRS-CS (abi_cs.hip, viprs_state_cs_sums) against the host definition `viprs_amd.stats.cs` -- the uniforms `==` the
host's Philox and the other variates within measured bounds, the update `==` `cs_update_host` fed the variates the device
used, the sums `==` a host replay of THE ORDER, the chain (Gibbs sweep, sums, update) `==` the C sweep replay plus
`cs_update_host`, determinism, `PRSCS.fit()` against the same fit on the host, the refusals."""
import numpy as np
import pytest

from tests import gibbs_replay as GR
from tests.test_band import _inputs as band_inputs, banded_ld
from tests.test_gpu_gibbs import E2E_CHROMS, SIZES, Z_TOL, _problem
from viprs_amd.stats import cs as CS

pytestmark = pytest.mark.gpu
SEED = 0x2545F4914F6CDD1D
VAR = ("ub", "z1", "z2", "e")
CS_OUT = ("psi", "delta")
INPUTS = ("mu_mult", "half_var_tau", "u_logs")
SWEPT = ("eta", "q", "var_mu", "var_gamma")

# The largest |z2_dev - z2_host| and |e_dev - e_host| over the 2^20 draws of test_variates_against_the_host (host: the float64
# formula rounded to float32; device: ocml's logf, sinpif in float32), measured on an MI355X (EXPERIMENTS.md 6.29).  The
# bounds of the test are four times that, the rule of tests/test_gpu_gibbs.py: the functions are a few ulp each and the
# product compounds them; |z2| <= 5.9 and e <= 16.7 (an ulp of 1.9e-6), a wrong formula is off by O(1).  Neither bound may
# exceed 1e-5.
Z2_MEASURED = 4.768e-7
E_MEASURED = 9.537e-7
Z2_TOL, E_TOL = 4 * Z2_MEASURED, 4 * E_MEASURED
assert Z2_TOL <= 1e-5 and E_TOL <= 1e-5


def _diag_plan(m):
    """`m` SNPs that see only themselves: the cs kernels never read LD."""
    from viprs_amd.plan import LDPlan
    return LDPlan(np.arange(m, dtype=np.int32), np.arange(m + 1, dtype=np.int64), np.ones(m, dtype=np.float32), False)


def _eta(m, G, rng):
    """Both signs, exact zeros (of both signs), denormals, a few large values."""
    eta = (0.02 * rng.standard_normal((m, G))).astype(np.float32)
    kind = rng.integers(0, 8, (m, G))
    eta[kind == 0] = 0.0
    eta[kind == 1] = np.float32(1e-41) * np.sign(eta[kind == 1])
    eta[kind == 2] = -0.0
    return np.asfortranarray(eta)


def _junk_state(m, G, seed):
    rng = np.random.default_rng(seed)
    f = lambda lo, hi: np.asfortranarray(rng.uniform(lo, hi, (m, G)).astype(np.float32))
    n = rng.uniform(2e4, 9e4, m)
    return dict(n=n, eta=_eta(m, G, rng), psi=f(1e-3, 1.0), delta=f(0.1, 5.0), ub=f(0, 1), z1=f(-1, 1), z2=f(-1, 1), e=f(0, 2),
                mu_mult=f(0, 1), half_var_tau=f(1, 9), u_logs=f(-3, 3))


def _open_state(plan, j):
    from viprs_amd.plan import DeviceState
    G = j["eta"].shape[1]
    st = DeviceState(plan, "float32", model="grid", width=G, placement="off")
    st.set_n_per_snp(j["n"])
    st.upload("eta", j["eta"])
    for k in INPUTS:
        st.upload(k, j[k])
    for k in CS_OUT + VAR:
        st.cs_upload(k, j[k])
    return st


def _bits(a):
    return np.asarray(a).view(np.uint32)


def test_variates_against_the_host(gpu):
    """2^20 SNPs, one column."""
    from viprs_amd.plan import DeviceState
    m, di = 2 ** 20, 2 ** 40 + 5
    plan = _diag_plan(m)
    try:
        st = DeviceState(plan, "float32", model="grid", width=1, placement="off")
        st.cs_variates(SEED, di)
        v_ms, u_ms = plan.last_cs_ms()
        assert v_ms > 0 and u_ms == 0
        dev = {k: st.cs_download(k)[:, 0] for k in VAR}
        assert np.all(st.cs_download("psi") == 1) and not st.cs_download("delta").any()
        st.close()
    finally:
        plan.close()
    ub, z1, z2, e = (a[:, 0] for a in CS.cs_variates_host(SEED, di, m, [0]))
    assert np.array_equal(dev["ub"], ub)
    k = dev["ub"].astype(np.float64) * 2.0 ** 24
    assert np.all((dev["ub"] > 0) & (dev["ub"] < 1)) and np.array_equal(k, np.round(k)) and np.all(k.astype(np.int64) % 2 == 1)
    err = {n: float(np.abs(dev[n].astype(np.float64) - h.astype(np.float64)).max()) for n, h in (("z1", z1), ("z2", z2), ("e", e))}
    print("max |dev - host| over 2^20 draws: " + ", ".join(f"{n} {v:.3e}" for n, v in err.items())
          + f" (bounds {Z_TOL:.3e}, {Z2_TOL:.3e}, {E_TOL:.3e})")
    assert err["z1"] <= Z_TOL and err["z2"] <= Z2_TOL and err["e"] <= E_TOL
    assert np.all(dev["e"] > 0) and np.all(dev["z1"] != 0) and np.all(dev["z2"] != 0)
    # the stream is not the Gibbs stream of the same (seed, draw_index, j, g)
    from viprs_amd.stats import gibbs as GB
    assert not np.array_equal(dev["ub"], GB.gibbs_normals_host(SEED, di, m, [0])[0][:, 0])
    g15 = 0.5 * dev["z2"].astype(np.float64) ** 2 + dev["e"]
    assert abs(g15.mean() - 1.5) < 5 * np.sqrt(1.5 / m) and abs(g15.var() - 1.5) < 5 * np.sqrt(13.5 / m)


def _update_case(m, G, cols, seed, psi_max=1.0):
    """One update of `cols` on junk: the device's outputs and variates, and the host's outputs from those variates."""
    j = _junk_state(m, G, seed)
    rng = np.random.default_rng(seed + 1)
    params = np.stack([np.asarray(cols, dtype=np.float64), rng.uniform(0.5, 1.5, len(cols)), 10.0 ** rng.uniform(-4, 0, len(cols))],
                      axis=1)
    plan = _diag_plan(m)
    try:
        st = _open_state(plan, j)
        st.cs_update(params, psi_max, seed=SEED, draw_index=3)
        dev = {k: st.cs_download(k) for k in CS_OUT + VAR}
        dev.update({k: st.download(k) for k in INPUTS + ("eta",)})
        st.close()
    finally:
        plan.close()
    want = {k: j[k].copy(order="F") for k in CS_OUT + INPUTS}
    CS.cs_update_host(j["n"], j["eta"], want["psi"], want["delta"], want["mu_mult"], want["half_var_tau"], want["u_logs"], params,
                      psi_max, tuple(dev[k] for k in VAR))
    return j, dev, want


@pytest.mark.parametrize("m", [1, 255, 256, 257, 2370])
@pytest.mark.parametrize("width", [1, 3], ids=["width1", "grid3"])
def test_update_equals_the_host(gpu, m, width):
    cols = [0] if width == 1 else [2, 0]
    j, dev, want = _update_case(m, width, cols, seed=100 + m)
    ub = CS.cs_variates_host(SEED, 3, m, cols)[0]
    for a, g in enumerate(cols):
        assert np.array_equal(dev["ub"][:, g], ub[:, a])
    for k in CS_OUT + INPUTS:
        assert np.array_equal(_bits(dev[k]), _bits(want[k])), (k, int((_bits(dev[k]) != _bits(want[k])).sum()))
    assert np.all(dev["psi"][:, cols] >= np.float32(2.0 ** -40)) and np.all(dev["psi"][:, cols] <= 1.0)
    assert np.all(dev["u_logs"][:, cols] == 32.0) and np.array_equal(_bits(dev["eta"]), _bits(j["eta"]))
    if m >= 255:                                       # the three kinds of eta all occur, and both branches of the draw
        e = j["eta"][:, cols]
        assert (e == 0).any() and ((e != 0) & (np.abs(e) < 1e-38)).any() and (e > 0).any() and (e < 0).any()
    if width == 3:                                     # column 1: junk that survives, buffers and fields alike
        for k in CS_OUT + VAR + INPUTS:
            assert np.array_equal(_bits(dev[k][:, 1]), _bits(j[k][:, 1])), k


def test_update_where_the_walk_wraps(gpu):
    """32 columns of 70 001 SNPs: more elements than the 8192 workgroups of 256 threads of one pass."""
    m, G = 70001, 32
    assert m * G > 8192 * 256
    cols = list(np.random.default_rng(9).permutation(G))
    j, dev, want = _update_case(m, G, cols, seed=7, psi_max=0.75)
    for k in CS_OUT + INPUTS:
        assert np.array_equal(_bits(dev[k]), _bits(want[k])), k
    assert dev["psi"].max() == np.float32(0.75) and (dev["psi"] < 0.75).any()
    ub = CS.cs_variates_host(SEED, 3, m, [5, 31])[0]
    assert np.array_equal(dev["ub"][:, 5], ub[:, 0]) and np.array_equal(dev["ub"][:, 31], ub[:, 1])


def test_prepare_only_and_keep_variates(gpu):
    m, G = 2370, 3
    j = _junk_state(m, G, 31)
    params = np.array([[2, 0.8, 0.3], [0, 1.7, 1e-3]])
    plan = _diag_plan(m)
    try:
        st = _open_state(plan, j)
        st.cs_update(params, prepare_only=True)
        got = {k: st.cs_download(k) for k in CS_OUT + VAR}
        for k in CS_OUT + VAR:                                             # nothing but the three fields changes
            assert np.array_equal(_bits(got[k]), _bits(j[k])), k
        want = {k: j[k].copy(order="F") for k in CS_OUT + INPUTS}
        CS.cs_update_host(j["n"], j["eta"], want["psi"], want["delta"], want["mu_mult"], want["half_var_tau"], want["u_logs"],
                          params, prepare_only=True)
        for k in INPUTS:
            assert np.array_equal(_bits(st.download(k)), _bits(want[k])), k
        # KEEP_VARIATES: the uploaded junk variates are what the update uses, and they stay
        st.cs_update(params, seed=SEED, draw_index=1, keep_variates=True)
        for k in VAR:
            assert np.array_equal(_bits(st.cs_download(k)), _bits(j[k])), k
        CS.cs_update_host(j["n"], j["eta"], want["psi"], want["delta"], want["mu_mult"], want["half_var_tau"], want["u_logs"],
                          params, 1.0, tuple(j[k] for k in VAR))
        for k in CS_OUT:
            assert np.array_equal(_bits(st.cs_download(k)), _bits(want[k])), k
        for k in INPUTS:
            assert np.array_equal(_bits(st.download(k)), _bits(want[k])), k
        st.close()
    finally:
        plan.close()


@pytest.mark.parametrize("m", [2370, 70001], ids=["one_pass", "two_passes"])
@pytest.mark.parametrize("width", [1, 3], ids=["width1", "grid3"])
def test_sums_equal_the_host_replay_of_the_order(gpu, m, width):
    cols = None if width == 1 else [2, 0]
    j = _junk_state(m, width, 55 + m)
    plan = _diag_plan(m)
    try:
        st = _open_state(plan, j)
        got = st.cs_sums(cols)
        again = st.cs_sums(cols)
        one = st.cs_sums([0])
        st.close()
    finally:
        plan.close()
    want = CS.cs_sums_host(j["n"], j["eta"], j["psi"], j["delta"], cols)
    assert got.shape == (1 if width == 1 else 2, 4) and np.array_equal(got, want) and np.array_equal(got, again)
    assert np.array_equal(one[0], got[-1]) and np.all(got > 0)


def _chain(ld, std_beta, n_per_snp, G, cols, s2, phi, seed=SEED, junk=None, order=None):
    """len(s2) iterations of (Gibbs sweep, sums, update) from the PRS-CS start; the device's fields, buffers, sums, and the
    draws and variates it used."""
    from viprs_amd.plan import DeviceState, LDPlan
    m = ld.m
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory)
    try:
        st = DeviceState(plan, "float32", model="grid", width=G, placement="off")
        st.upload("std_beta", std_beta)
        st.set_n_per_snp(n_per_snp)
        if junk is not None:
            for k in SWEPT + INPUTS:
                st.upload(k, junk[k])
            for k in CS_OUT:
                st.cs_upload(k, junk[k])
        listed = list(cols if order is None else order)
        rows = lambda i: np.array([[g, s2[i][g], phi[i][g]] for g in listed])
        st.cs_update(np.array([[g, 1.0, 1.0] for g in listed]), prepare_only=True)
        draws, variates, sums = [], [], []
        for i in range(len(s2)):
            st.gibbs_sweep(ld.dq_scale, active_model_idx=np.array(listed, dtype=np.int32), seed=seed, draw_index=i)
            draws.append((st.gibbs_download("unif"), st.gibbs_download("noise")))
            sums.append((st.enet_sums(cols), st.cs_sums(cols)))
            st.cs_update(rows(i), seed=seed, draw_index=i)
            variates.append(tuple(st.cs_download(k) for k in VAR))
        out = {k: st.download(k) for k in SWEPT + INPUTS}
        out.update({k: st.cs_download(k) for k in CS_OUT})
        st.close()
        return out, draws, variates, sums
    finally:
        plan.close()


def _chain_host(ld, std_beta, n_per_snp, G, cols, s2, phi, draws, variates, junk=None):
    m = ld.m
    z = lambda: np.zeros((m, G), dtype=np.float32, order="F")
    h = {k: z() for k in SWEPT + INPUTS + CS_OUT}
    h["psi"][...] = 1
    if junk is not None:
        for k in SWEPT + INPUTS + CS_OUT:
            h[k][...] = junk[k]
    upd = lambda params, v, prep: CS.cs_update_host(n_per_snp, h["eta"], h["psi"], h["delta"], h["mu_mult"], h["half_var_tau"],
                                                    h["u_logs"], params, 1.0, v, prep)
    upd(np.array([[g, 1.0, 1.0] for g in cols]), None, True)
    sums = []
    for i in range(len(s2)):
        unif, noise = draws[i]
        for g in cols:
            eta, q = h["eta"][:, g].copy(), h["q"][:, g].copy()
            _, mu, gam = GR.replay_sweep(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, ld.low_memory, std_beta, h["mu_mult"][:, g],
                                         h["half_var_tau"][:, g], h["u_logs"][:, g], unif[:, g].copy(), noise[:, g].copy(), eta, q,
                                         ld.dq_scale)
            for k, v in zip(SWEPT, (eta, q, mu, gam)):
                h[k][:, g] = v
        sums.append(CS.cs_sums_host(n_per_snp, h["eta"], h["psi"], h["delta"], cols))
        upd(np.array([[g, s2[i][g], phi[i][g]] for g in cols]), variates[i], False)
    return h, sums


S2 = [[0.9, 7.0, 1.1], [1.05, 7.0, 0.8], [0.7, 7.0, 1.0], [1.2, 7.0, 0.95]]        # per iteration and column; column 1 is
PHI = [[1.0, 7.0, 1e-2], [0.3, 7.0, 1e-2], [0.05, 7.0, 1e-2], [0.02, 7.0, 1e-2]]   # the one nobody lists
LISTED = [2, 0]


def _assert_chain(ld, std_beta, n_per_snp, junk=None):
    got, draws, variates, sums = _chain(ld, std_beta, n_per_snp, 3, LISTED, S2, PHI, junk=junk)
    want, want_sums = _chain_host(ld, std_beta, n_per_snp, 3, LISTED, S2, PHI, draws, variates, junk=junk)
    for g in LISTED:
        assert np.all(got["var_gamma"][:, g] == 1) and np.all(got["eta"][:, g] != 0)
    for k in SWEPT + CS_OUT + INPUTS:
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (k, int((_bits(got[k]) != _bits(want[k])).sum()))
    for (_, c), w in zip(sums, want_sums):
        assert np.array_equal(c, w)
    assert len(np.unique(got["psi"][:, LISTED])) > ld.m // 2          # the scales moved
    return got


@pytest.mark.parametrize("ld_dtype", [np.float32, np.int8], ids=["f32", "i8"])
@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_the_chain(gpu, low_memory, ld_dtype):
    """The SIZES of tests/test_gpu_gibbs.py (every role of the panel sweep), 3 columns with junk in the unlisted one."""
    ld, std_beta, n = _problem(low_memory, ld_dtype, tuple(SIZES))
    junk = _junk_state(ld.m, 3, 77)
    rng = np.random.default_rng(5)
    for k in SWEPT:
        junk[k] = np.asfortranarray(np.where(np.arange(3) == 1, 0.01 * rng.standard_normal((ld.m, 3)), 0).astype(np.float32))
    junk["psi"][:, LISTED] = 1
    junk["delta"][:, LISTED] = 0
    got = _assert_chain(ld, std_beta, n.astype(np.float64) * np.linspace(0.6, 1.4, ld.m), junk=junk)
    for k in SWEPT + INPUTS + CS_OUT:
        assert np.array_equal(_bits(got[k][:, 1]), _bits(junk[k][:, 1])), k


def test_the_chain_on_windowed_ld(gpu):
    ld = banded_ld(900, 40, 40, True, np.int8, seed=8)
    ss, _ = band_inputs(900, seed=4)
    _assert_chain(ld, ss.std_beta, np.asarray(ss.n_per_snp, dtype=np.float64) * np.linspace(0.5, 1.5, 900))


def test_determinism(gpu):
    """Two runs: the same bits.  A column alone, or listed in another order: the same column.  Another seed: another chain."""
    ld, std_beta, n = _problem(True, np.float32, (1601, 130, 64, 1))
    n = n.astype(np.float64)
    a, da, va, sa = _chain(ld, std_beta, n, 3, LISTED, S2[:3], PHI[:3])
    b, db, vb, sb = _chain(ld, std_beta, n, 3, LISTED, S2[:3], PHI[:3])
    c, _, _, sc = _chain(ld, std_beta, n, 3, LISTED, S2[:3], PHI[:3], order=[0, 2])
    d, _, _, sd = _chain(ld, std_beta, n, 3, [0], S2[:3], PHI[:3])
    for k in SWEPT + CS_OUT + INPUTS:
        assert np.array_equal(_bits(a[k]), _bits(b[k])) and np.array_equal(_bits(a[k]), _bits(c[k])), k
        assert np.array_equal(_bits(a[k][:, 0]), _bits(d[k][:, 0])), k
    for x, y in zip(va, vb):
        assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(x, y))
    for (ea, ca), (eb, cb), (ec, cc), (ed, cd) in zip(sa, sb, sc, sd):
        assert np.array_equal(ca, cb) and np.array_equal(ca, cc) and np.array_equal(ca[1], cd[0])
    e, _, _, _ = _chain(ld, std_beta, n, 3, LISTED, S2[:3], PHI[:3], seed=SEED + 1)
    assert not np.array_equal(a["psi"][:, 0], e["psi"][:, 0]) and not np.array_equal(a["eta"][:, 2], e["eta"][:, 2])


def test_prscs_fit_equals_the_host_fit(gpu):
    """Short chains, 3 columns (fixed, auto, fixed), 1 995 SNPs: the device fit against the same fit on the host backend (the C
    sweep replay as `sweep_fn`), fed the draws and the variates the device used."""
    from viprs_amd.model import PRSCS
    kw = dict(phi=(1e-2, None, 1.0), n_iter=14, n_burnin=4, thin=2, seed=11, dequantize_on_the_fly=True)
    dev = PRSCS(GR.model_gdl(E2E_CHROMS), keep_draws_log=True, **kw).fit()
    assert len(dev.draws_log) == 14 and len(dev.variates_log) == 14
    host = PRSCS(GR.model_gdl(E2E_CHROMS), sweep_fn=GR.replay_sweep, draws_fn=lambda seed, i, hvt, cols: dev.draws_log[i],
                 variates_fn=lambda seed, i, m, cols: dev.variates_log[i], **kw).fit()
    for c in host.post_mean_beta:
        assert np.array_equal(dev.post_mean_beta[c], host.post_mean_beta[c]), c
        assert dev.post_mean_beta[c].shape[1] == 3 and dev.post_mean_beta[c].any(axis=0).all()
    assert dev.grid_table.equals(host.grid_table) and not dev.grid_table["diverged"].any()
    assert np.array_equal(dev.phi_history, host.phi_history) and np.array_equal(dev.sigma2_history, host.sigma2_history)
    assert np.all(dev.phi_history[:, 0] == 1e-2) and len(np.unique(dev.phi_history[:, 1])) == 14


REFUSALS = ["float64", "spike_slab", "mixture", "masked_grid", "comm", "no_n_per_snp", "column_out_of_range", "column_twice",
            "sigma2_zero", "sigma2_nan", "phi_negative", "phi_inf", "psi_max_small", "psi_max_inf", "keep_variates_first",
            "unknown_flag"]


@pytest.mark.parametrize("case", REFUSALS)
def test_refusals_launch_nothing(gpu, case):
    """Each refusal is a ValueError (VIPRS_EINVAL) before any launch: no cs kernel is timed, the fields, the cs buffers and
    the output of the sums keep their bits."""
    from viprs_amd import _lib as L
    from viprs_amd.plan import DeviceState, _ptr
    m = 300
    plan = _diag_plan(m)
    comm = None
    try:
        kind = {"float64": dict(float_precision="float64", model="grid", width=2), "spike_slab": {},
                "mixture": dict(model="mixture", width=3)}.get(case, dict(model="grid", width=2))
        st = DeviceState(plan, placement="off", **kind)
        state_level = case in ("float64", "spike_slab", "mixture", "masked_grid", "comm")
        if case == "masked_grid":
            st.set_groups([0, 130, m])
            st.set_group_columns(np.array([[1, 0], [1, 1]], dtype=np.uint8))
        if case == "comm":
            from viprs_amd.parallel import RcclComm
            comm = RcclComm(rank=0, world_size=1, device=0)
            st.set_comm(comm)
        if case != "no_n_per_snp":
            st.set_n_per_snp(np.full(m, 5e4))
        rng = np.random.default_rng(5)
        names = ["std_beta", "u_logs", "half_var_tau", "mu_mult", "eta", "q", "var_mu", "var_gamma"]
        before = {}
        for k in names:
            a = rng.standard_normal(st._shape(k)).astype(st.dtype)
            before[k] = np.asfortranarray(a) if st.model == "grid" and a.ndim == 2 else a
            st.upload(k, before[k])
        cs_before = None
        if not state_level and case != "keep_variates_first":
            cs_before = {k: np.asfortranarray(rng.uniform(0.1, 1, (m, 2)).astype(np.float32)) for k in CS_OUT + VAR}
            for k, a in cs_before.items():
                st.cs_upload(k, a)
        good = np.array([[0, 1.0, 0.5], [1, 1.0, 0.5]])
        bad = {"column_out_of_range": [[0, 1.0, 0.5], [2, 1.0, 0.5]], "column_twice": [[1, 1.0, 0.5], [1, 1.0, 0.5]],
               "sigma2_zero": [[0, 0.0, 0.5]], "sigma2_nan": [[0, np.nan, 0.5]], "phi_negative": [[0, 1.0, -0.5]],
               "phi_inf": [[0, 1.0, np.inf]]}
        params = np.array(bad.get(case, good), dtype=np.float64)
        psi_max = {"psi_max_small": 2.0 ** -40, "psi_max_inf": np.inf}.get(case, 1.0)
        out = np.full((2, 4), -7.0)
        with pytest.raises(ValueError, match="PRS-CS"):
            if case == "unknown_flag":
                L.check(L.lib.viprs_state_cs_update(st._h, 2, _ptr(params), 1.0, 1, 2, 4, 1))
            else:
                st.cs_update(params, psi_max, seed=1, draw_index=2, keep_variates=case == "keep_variates_first")
        if state_level or case == "no_n_per_snp":
            assert L.lib.viprs_state_cs_sums(st._h, 2, None, _ptr(out)) == L.EINVAL and "PRS-CS" in L.last_error()
        if state_level:
            with pytest.raises(ValueError, match="PRS-CS"):
                st.cs_variates(1, 2)
            with pytest.raises(ValueError, match="PRS-CS"):
                st.cs_download("psi")
        if case in ("column_out_of_range", "column_twice"):
            cols = np.array(params[:, 0], dtype=np.int32)
            assert L.lib.viprs_state_cs_sums(st._h, 2, _ptr(cols), _ptr(out)) == L.EINVAL and "PRS-CS" in L.last_error()
            with pytest.raises(ValueError, match="PRS-CS"):
                st.cs_variates(1, 2, cols)
        assert np.all(out == -7.0)
        assert L.lib.viprs_plan_last_cs_ms(plan.handle, None, None) == L.EINVAL
        with pytest.raises(ValueError, match="no timed PRS-CS call"):
            plan.last_cs_ms()
        for k in names:
            u = f"u{st.dtype.itemsize}"
            assert np.array_equal(st.download(k).view(u), before[k].view(u)), k
        if cs_before is not None:
            for k, a in cs_before.items():
                assert np.array_equal(_bits(st.cs_download(k)), _bits(a)), k
        st.close()
    finally:
        if comm is not None:
            comm.close()
        plan.close()


def test_null_pointers_and_an_empty_plan(gpu):
    from viprs_amd import _lib as L
    from viprs_amd.plan import DeviceState, LDPlan, _ptr
    plan = _diag_plan(10)
    try:
        st = DeviceState(plan, "float32", model="grid", width=1, placement="off")
        st.set_n_per_snp(np.full(10, 1e4))
        assert L.lib.viprs_state_cs_update(st._h, 1, None, 1.0, 0, 0, 0, 1) == L.EINVAL
        assert L.lib.viprs_state_cs_sums(st._h, 1, None, None) == L.EINVAL
        assert L.lib.viprs_state_cs_upload(st._h, L.CS_PSI, None) == L.EINVAL
        assert L.lib.viprs_state_cs_download(st._h, L.CS_PSI, None) == L.EINVAL
        buf = np.zeros(10, dtype=np.float32)
        assert L.lib.viprs_state_cs_download(st._h, 6, _ptr(buf)) == L.EINVAL
        st.close()
    finally:
        plan.close()
    empty = LDPlan(np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.float32), False)
    try:
        st = DeviceState(empty, "float32", model="grid", width=2, placement="off")
        st.cs_variates(1, 2)
        st.cs_update(np.array([[0, 1.0, 1.0]]), prepare_only=True)
        st.cs_update(np.array([[1, 1.0, 1.0]]), keep_variates=True)
        assert not st.cs_sums().any() and st.cs_download("psi").shape == (0, 2)
        st.close()
    finally:
        empty.close()
