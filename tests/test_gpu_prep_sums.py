"""GPU: every prep / sums entry point of `DeviceState` against the host reference of tests/em_reference.py.

The state arrays are UPLOADED (no sweep runs here), so the values are the test's: var_gamma with exact 0, exact 1 and values
inside the clip margins, signed eta / q / std_beta whose products cancel, n_per_snp over two orders of magnitude, the largest
|eta_diff| at a negative entry at the first or the last SNP of a row.

What is asserted, and why nothing here is a tuned tolerance:

* `mu_mult`, `sqrt_half_var_tau` / `half_var_tau`, `log_null_pi` and every stored output outside the listed rows: `==`
  (+, *, / and sqrt are correctly rounded on both sides; the library is built without contraction).
* `u_logs`: the device `log` is the only inexact operation.  float32 states: one float32 ulp (`rtol=1.2e-7`, as
  tests/test_gpu_edge_cases.py).  float64 states: `em_reference.u_logs_bound`, derived there from `LOG_ULPS`.  ROCm documents no
  accuracy figure for its device library's float64 `log` on this installation, so `LOG_ULPS` is twice the MEASURED
  largest difference between the device's log and `np.log` over the inputs of these tests: `test_device_log_accuracy`
  measured 1 ulp (EXPERIMENTS.md).
* each sum against the exactly rounded sum of its float64 terms:  |got - exact| <= eps64 (D + C) fsum(|terms|), D the number of
  additions on the longest path of the row's reduction (the contract of include/viprs_hip.h, `em_reference.reduction_depth`),
  C the rounded operations in one term.  The worst case of floating-point summation: a correct kernel cannot exceed it, one
  dropped, doubled or misplaced term does by many orders of magnitude.
* max |eta_diff|: `==`.  A sums call repeated: identical bits.  A row of a batch: identical bits to the row requested alone.
"""
import numpy as np
import pytest

from tests import em_reference as R

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64"]
STATE = ("var_gamma", "var_mu", "eta", "q", "eta_diff")


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def block_ld(group_lengths, block=96, ld_dtype=np.float32):
    """Block-diagonal LD (symmetric form, identity blocks: nothing here sweeps) whose blocks never straddle a group boundary.
    Returns (left_bound, indptr, data, group_start)."""
    sizes = []
    for n in group_lengths:
        sizes += [block] * (n // block) + ([n % block] if n % block else [])
    sizes = np.asarray(sizes, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    m = int(starts[-1])
    row_start = np.repeat(starts[:-1], sizes)
    row_len = np.repeat(sizes, sizes)
    indptr = np.concatenate([[0], np.cumsum(row_len)]).astype(np.int64)
    data = np.zeros(int(indptr[-1]), dtype=ld_dtype)
    one = np.iinfo(ld_dtype).max if np.issubdtype(np.dtype(ld_dtype), np.integer) else 1
    data[indptr[:-1] + (np.arange(m) - row_start)] = one
    gs = np.concatenate([[0], np.cumsum(group_lengths)]).astype(np.int64)
    return row_start.astype(np.int32), indptr, data, gs


def make_plan(group_lengths, **kw):
    from viprs_amd.plan import LDPlan
    lb, ip, data, gs = block_ld(group_lengths, **kw)
    return LDPlan(lb, ip, data, False), gs


def special_gamma(rng, shape, T):
    """Ordinary values with exact 0, exact 1, a value below the lower clip margin and one above the upper one mixed in."""
    near_one = 1.0 - 2.0 ** -24 if T == np.float32 else 1.0 - 1e-16
    g = rng.uniform(1e-4, 0.6, shape)
    pick = rng.integers(0, 12, shape)
    for code, v in ((0, 0.0), (1, 1.0), (2, 1e-20), (3, near_one)):
        g[pick == code] = v
    g = g.astype(T)
    assert (g == 0).any() or g.size < 12
    return g


def make_state(rng, m, T, rows, peak, width=None, mixture=False):
    """The five state arrays + std_beta + n_per_snp.  `rows`: the (start, end) SNP ranges whose extreme |eta_diff| sits at
    their first (`peak="first"`) or last SNP, negative.  `width`: columns of a grid state / components of a mixture."""
    T = np.dtype(T).type
    wide = (m,) if width is None else (m, width)
    vec = (m,) if (width is None or mixture) else (m, width)
    g = special_gamma(rng, wide, T)
    if mixture:                                      # rows that leave no room for the null component, and ordinary ones
        g = (g / np.maximum(1.0, 1.1 * g.sum(axis=1, keepdims=True) * rng.uniform(0.5, 1.5, (m, 1)))).astype(T)
        g[rng.integers(0, 9, m) == 0] = 0
        one_hot = rng.integers(0, 9, m) == 1
        g[one_hot] = 0
        g[one_hot, rng.integers(0, width, int(one_hot.sum()))] = 1
        g[rng.integers(0, 9, wide) == 2] = 1e-20
    mu = (0.05 * rng.standard_normal(wide)).astype(T)
    if mixture:                                      # kv rows 1 and 5 (gamma vs clipped gamma times mu^2 + 1 / var_tau) differ only
        mu[g == 0] = T(30.0)                         # where gamma is clipped: a large second moment there tells them apart
    eta = (0.05 * rng.standard_normal(vec)).astype(T)
    eta[eta == 0] = T(0.01)
    q = (0.05 * rng.standard_normal(vec)).astype(T)
    # std_beta * eta = +c, -c, +c, ... up to rounding: sum [3] cancels to far below sum |terms|
    sign = np.where(np.arange(m) % 2 == 0, 1.0, -1.0)
    eta_for_beta = eta if eta.ndim == 1 else eta[:, 0]
    beta = (sign * 1e-3 / eta_for_beta.astype(np.float64)).astype(T)
    ed = (1e-3 * rng.standard_normal(vec)).astype(T)
    for a, b in rows:
        if b > a:
            at = a if peak == "first" else b - 1
            ed[at] = -T(0.5 + 0.001 * (a % 7))
    n = 10.0 ** rng.uniform(3.0, 5.0, m)
    return dict(var_gamma=g, var_mu=mu, eta=eta, q=q, eta_diff=ed, std_beta=beta, n=n)


def upload_state(st, s, order="C"):
    for k in STATE:
        st.upload(k, np.asarray(s[k], order=order))
    st.upload("std_beta", s["std_beta"])
    st.set_n_per_snp(s["n"])


def hyper(rng, n, K=None):
    """n sets of (pi, sigma_eps, tau_beta, lambda) with distinct values; K: mixtures (pi and tau_beta are K-vectors)."""
    out = []
    for _ in range(n):
        sig, lam = float(rng.uniform(0.5, 1.0)), float(rng.uniform(0.0, 0.05))
        if K is None:
            out.append((float(rng.uniform(0.001, 0.2)), sig, float(10.0 ** rng.uniform(1.5, 4.5)), lam))
        else:
            out.append((rng.uniform(0.001, 0.1, K), sig, 10.0 ** rng.uniform(1.5, 4.5, K), lam))
    return out


def logit(p):
    return np.log(p) - np.log(1.0 - p)


def sentinel(rng, st, names):
    """Recognisable values in the prep outputs: what a prep does not list must keep these bits."""
    out = {}
    for k in names:
        shape = st._shape(k)
        a = rng.uniform(-7.0, 7.0, shape).astype(st.dtype)
        out[k] = np.asarray(a, order="F" if (st.model == "grid" and len(shape) == 2) else "C")
        st.upload(k, out[k])
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- assertions -------------------------------------------------------------------------------------------------------------
def check_prep(got, ref, T, scalars, what):
    """got / ref: dicts with mu_mult, u_logs, shvt (+ log_null_pi); scalars: (logit_pi, log_tau_beta) as in `ref`."""
    for k in ("mu_mult", "shvt") + (("log_null_pi",) if "log_null_pi" in ref else ()):
        assert np.array_equal(got[k], ref[k]), (what, k)
    if np.dtype(T) == np.float32:
        np.testing.assert_allclose(got["u_logs"], ref["u_logs"], rtol=1.2e-7, err_msg=str(what))
    else:
        bound = R.u_logs_bound(scalars[0], scalars[1], ref["var_tau"])
        err = np.abs(got["u_logs"].astype(np.float64) - ref["u_logs"])
        print(f"[u_logs {what}] max err / bound = {float(np.max(err / bound)) if err.size else 0.0:.3f}")
        assert np.all(err <= bound), (what, float(np.max(err / bound)))


def check_sums(got, exact, scale, ops, length, kind, what):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == exact.shape, (what, got.shape, exact.shape)
    bound = R.sums_bound(scale[:-1], ops, length, kind)
    err = np.abs(got[:-1] - exact[:-1])
    nan = np.isnan(exact[:-1])
    assert np.array_equal(np.isnan(got[:-1]), nan), (what, got, exact)
    ok = nan | (err <= bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    print(f"[sums {what} len={length}] max err / bound = {np.nanmax(ratio) if ratio.size else 0.0:.4f} (sum {int(np.nanargmax(ratio))})")
    assert ok.all(), (what, length, np.nonzero(~ok)[0], got[:-1][~ok], exact[:-1][~ok], bound[~ok])
    assert got[-1] == exact[-1], (what, "max |eta_diff|", got[-1], exact[-1])


def cancels(exact, scale, k, length):
    if length >= 64:
        assert abs(exact[k]) < 1e-2 * scale[k], (exact[k], scale[k])


# ---- the device log --------------------------------------------------------------------------------------------------------
def test_device_log_accuracy(gpu):
    """Measures the device's float64 `log` through a prep that leaves it bare (n (1 + 0) / 1 + 0 = n, 0 + 0.5 (0 - log n) is
    exact), against `np.log`, over the values the sums take logs of: var_gamma and 1 - var_gamma of the generator clipped as
    the ELBO clips them, var_tau of the tests' hyper-parameters, and 40 000 values log-uniform in [1e-15, 1e7].
    Measured on an MI355X (ROCm 7.2): at most 1.00 ulp of the result, 1 519 of the 140 000 values differ; `em_reference.LOG_ULPS`
    is twice that."""
    from viprs_amd.plan import DeviceState
    rng = np.random.default_rng(1)
    g = special_gamma(rng, (20_000,), np.float32).astype(np.float64)
    g64 = special_gamma(rng, (20_000,), np.float64).astype(np.float64)
    x = np.concatenate([np.clip(g, R.RES, 1 - R.RES), np.clip(1 - g, R.RES, 1 - R.RES), np.clip(g64, R.RES, 1 - R.RES),
                        np.clip(1 - g64, R.RES, 1 - R.RES), 10.0 ** rng.uniform(3, 5, 20_000) * 1.03 / 0.7 + 300.0,
                        10.0 ** rng.uniform(-15, 7, 40_000)])
    plan, _ = make_plan([x.shape[0]], block=64, ld_dtype=np.int8)
    st = DeviceState(plan, "float64")
    st.set_n_per_snp(x)
    st.prep(0.0, 0.0, 1.0, 0.0, 1.0)
    dev = -2.0 * st.download("u_logs")
    ref = np.log(x)
    ulps = np.abs(dev - ref) / np.spacing(np.abs(ref))
    ulps[ref == 0] = np.abs(dev[ref == 0]) / np.spacing(1.0)
    print(f"[device log] max |device - np.log| = {ulps.max():.2f} ulp; differing: {int((dev != ref).sum())} of {x.size}")
    assert np.all(np.abs(dev - ref) <= R.LOG_ULPS * R.EPS64 * np.abs(ref))
    plan.close()


# ---- spike-and-slab, the whole plan: prep / sums / sums_begin, _end, with and without SNP weights ---------------------------
@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("m", [1, 255, 256, 257, 1803])
def test_spike_slab_plan(gpu, T, m):
    from viprs_amd.plan import DeviceState
    rng = np.random.default_rng(100 + m)
    plan, _ = make_plan([m])
    st = DeviceState(plan, T)
    (pi, sig, tau, lam), = hyper(rng, 1)
    for peak in ("first", "last"):
        s = make_state(rng, m, T, [(0, m)], peak)
        upload_state(st, s)
        st.set_snp_weights(None)
        st.prep(logit(pi), np.log(tau), sig, tau, 1.0 + lam)
        ref = R.prep(s["n"], logit(pi), np.log(tau), sig, tau, 1.0 + lam, T)
        got = {"mu_mult": st.download("mu_mult"), "u_logs": st.download("u_logs"), "shvt": st.download("sqrt_half_var_tau")}
        check_prep(got, ref, T, (logit(pi), np.log(tau)), ("prep", m))
        args = (s["var_gamma"], s["var_mu"], s["eta"], s["q"], s["eta_diff"], s["std_beta"], ref["var_tau"], 1.0 + lam)
        exact, scale = R.sums(*args)
        cancels(exact, scale, 3, m)
        assert exact[10] == 0.5 and s["eta_diff"][0 if peak == "first" else m - 1] == -0.5
        v = st.sums(1.0 + lam)
        check_sums(v, exact, scale, R.sums_ops(weighted=False), m, "spike_slab", "sums")
        st.sums_begin(1.0 + lam)
        assert same_bits(st.sums_end(), v) and same_bits(st.sums(1.0 + lam), v)
        w = 1.0 / rng.integers(1, 2000, m).astype(np.float64)
        st.set_snp_weights(w)
        exact_w, scale_w = R.sums(*args, weight=w)
        vw = st.sums(1.0 + lam)
        check_sums(vw, exact_w, scale_w, R.sums_ops(weighted=True), m, "spike_slab", "sums, weighted")
        assert same_bits(vw[1:], v[1:])
        st.sums_begin(1.0 + lam)
        assert same_bits(st.sums_end(), vw)
    plan.close()


# ---- SNP groups -------------------------------------------------------------------------------------------------------------
# lengths 1, 255, 256, 257, an EMPTY group between two others, groups that start off multiples of 4 and of 256
GROUPS = [1, 255, 0, 256, 257, 1031, 3]


def _rows(gs):
    return [(int(gs[g]), int(gs[g + 1])) for g in range(len(gs) - 1)]


@pytest.mark.parametrize("T", DTYPES)
def test_spike_slab_groups(gpu, T):
    from viprs_amd.plan import DeviceState
    rng = np.random.default_rng(7)
    plan, gs = make_plan(GROUPS)
    rows, G, m = _rows(gs), len(GROUPS), plan.m
    assert any(a % 4 for a, _ in rows) and any(a % 256 for a, _ in rows)
    st = DeviceState(plan, T)
    st.set_groups(gs)
    s = make_state(rng, m, T, rows, "last")
    upload_state(st, s)
    st.set_snp_weights(np.full(m, 0.25))                      # a group's [0] is the plain sum: weights must not reach it
    first, second = hyper(rng, G), hyper(rng, G)
    prow = lambda g, h: [g, logit(h[0]), np.log(h[2]), h[1], h[2], 1.0 + h[3]]
    st.prep_groups(np.array([prow(g, first[g]) for g in range(G)]))
    keep = {k: st.download(k) for k in ("mu_mult", "u_logs", "sqrt_half_var_tau")}
    listed = [5, 1, 2, 3]                                     # a subset in permuted order, the empty group among them
    st.prep_groups(np.array([prow(g, second[g]) for g in listed]))
    got = {k: st.download(k) for k in keep}
    now = [second[g] if g in listed else first[g] for g in range(G)]
    var_tau = np.empty(m)
    for g, (a, b) in enumerate(rows):
        h = now[g]
        ref = R.prep(s["n"][a:b], logit(h[0]), np.log(h[2]), h[1], h[2], 1.0 + h[3], T)
        var_tau[a:b] = ref["var_tau"]
        if g in listed:
            check_prep({"mu_mult": got["mu_mult"][a:b], "u_logs": got["u_logs"][a:b], "shvt": got["sqrt_half_var_tau"][a:b]},
                       ref, T, (logit(h[0]), np.log(h[2])), ("prep_groups", g))
        else:
            assert all(same_bits(got[k][a:b], keep[k][a:b]) for k in keep), g
    opl = [1.0 + h[3] for h in now]
    for peak in ("last", "first"):
        if peak == "first":
            s["eta_diff"] = make_state(np.random.default_rng(8), m, T, rows, "first")["eta_diff"]
            st.upload("eta_diff", s["eta_diff"])
        st.sums_groups_begin(np.arange(G), opl)
        allv = st.sums_groups_end()
        for g, (a, b) in enumerate(rows):
            exact, scale = R.sums(*(s[k][a:b] for k in STATE), s["std_beta"][a:b], var_tau[a:b], opl[g])
            cancels(exact, scale, 3, b - a)
            check_sums(allv[g], exact, scale, R.sums_ops(weighted=False), b - a, "spike_slab", ("sums_groups", g))
        assert not allv[2].any()                              # the sums of no terms
        st.sums_groups_begin(np.arange(G), opl)
        assert same_bits(st.sums_groups_end(), allv)
        order = [4, 2, 6, 0]
        st.sums_groups_begin(order, [opl[g] for g in order])
        assert same_bits(st.sums_groups_end(), allv[order])
        for g in (1, 2, 5):
            st.sums_groups_begin([g], [opl[g]])
            assert same_bits(st.sums_groups_end(), allv[[g]])
    plan.close()


# ---- grid states: columns ---------------------------------------------------------------------------------------------------
def _grid_outputs(st):
    return {k: st.download(k) for k in ("mu_mult", "u_logs", "half_var_tau")}


def _check_grid_prep(got, ref, T, h, sl, c, what):
    check_prep({"mu_mult": got["mu_mult"][sl, c], "u_logs": got["u_logs"][sl, c], "shvt": got["half_var_tau"][sl, c]},
               ref, T, (logit(h[0]), np.log(h[2])), what)


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("m", [1, 257, 1803])
def test_grid_columns(gpu, T, m):
    from viprs_amd.plan import DeviceState
    rng = np.random.default_rng(200 + m)
    G = 4
    plan, _ = make_plan([m])
    st = DeviceState(plan, T, "grid", G)
    s = make_state(rng, m, T, [(0, m)], "first", width=G)
    s["eta_diff"][m - 1, 1::2] = -0.75                        # odd columns: the extreme at the LAST SNP
    upload_state(st, s, order="F")
    hs = hyper(rng, G + 2)
    keep = sentinel(rng, st, ("mu_mult", "u_logs", "half_var_tau"))
    pcol = lambda c, h: [c, logit(h[0]), np.log(h[2]), h[1], h[2], 1.0 + h[3]]
    # prep_column writes column 1 only
    st.prep_column(*pcol(1, hs[1]))
    got = _grid_outputs(st)
    vt = {1: R.prep(s["n"], *pcol(1, hs[1])[1:], T, grid=True)}
    _check_grid_prep(got, vt[1], T, hs[1], slice(None), 1, ("prep_column", 1))
    assert all(same_bits(got[k][:, c], keep[k][:, c]) for k in keep for c in (0, 2, 3))
    # prep_columns writes 3 and 0 (in that order); 1 keeps its prep, 2 the sentinel
    st.prep_columns(np.array([pcol(3, hs[3]), pcol(0, hs[0])]))
    got2 = _grid_outputs(st)
    for c in (3, 0):
        vt[c] = R.prep(s["n"], *pcol(c, hs[c])[1:], T, grid=True)
        _check_grid_prep(got2, vt[c], T, hs[c], slice(None), c, ("prep_columns", c))
    assert all(same_bits(got2[k][:, 1], got[k][:, 1]) and same_bits(got2[k][:, 2], keep[k][:, 2]) for k in keep)
    opl = {c: 1.0 + hs[c][3] for c in range(G)}
    for weights in (None, 1.0 / rng.integers(1, 500, m).astype(np.float64)):
        st.set_snp_weights(weights)
        want = {}
        for c in (0, 1, 3):
            exact, scale = R.sums(*(s[k][:, c] for k in STATE), s["std_beta"], vt[c]["var_tau"], opl[c], weight=weights)
            want[c] = (exact, scale)
            assert exact[10] == (0.75 if c % 2 else 0.5)
            v = st.sums_column(c, opl[c])
            check_sums(v, exact, scale, R.sums_ops(weights is not None), m, "grid", ("sums_column", c))
            assert same_bits(st.sums_column(c, opl[c]), v)
            want[c] += (v,)
        order = [3, 0, 1]
        st.sums_columns_begin(order, [opl[c] for c in order])
        batch = st.sums_columns_end()
        for i, c in enumerate(order):
            check_sums(batch[i], want[c][0], want[c][1], R.sums_ops(weights is not None), m, "grid", ("sums_columns", c))
            assert same_bits(batch[i], want[c][2])            # a row of the batch == the column requested alone
        st.sums_columns_begin(order, [opl[c] for c in order])
        assert same_bits(st.sums_columns_end(), batch)
    # a column prepared again with other scalars: its sums follow (var_tau is formed from the LAST prep's scalars)
    st.prep_column(*pcol(1, hs[4]))
    ref = R.prep(s["n"], *pcol(1, hs[4])[1:], T, grid=True)
    exact, scale = R.sums(*(s[k][:, 1] for k in STATE), s["std_beta"], ref["var_tau"], 1.0 + hs[4][3], weight=weights)
    check_sums(st.sums_column(1, 1.0 + hs[4][3]), exact, scale, R.sums_ops(True), m, "grid", "sums_column after a new prep")
    plan.close()


# ---- grid states: (group, column) pairs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", DTYPES)
def test_grid_groups(gpu, T):
    from viprs_amd.plan import DeviceState
    rng = np.random.default_rng(9)
    G = 3
    plan, gs = make_plan(GROUPS)
    rows, NG, m = _rows(gs), len(GROUPS), plan.m
    st = DeviceState(plan, T, "grid", G)
    st.set_groups(gs)
    s = make_state(rng, m, T, rows, "first", width=G)
    for a, b in rows:
        if b > a:
            s["eta_diff"][b - 1, 1] = -0.75                   # column 1: the extreme at the LAST SNP of every group
    upload_state(st, s, order="F")
    st.set_snp_weights(np.full(m, 0.25))                      # a pair's [0] is the plain sum over the group
    pairs = [(g, c) for g in range(NG) for c in range(G)]
    first = dict(zip(pairs, hyper(rng, len(pairs))))
    second = dict(zip(pairs, hyper(rng, len(pairs))))
    prow = lambda p, h: [p[0], p[1], logit(h[0]), np.log(h[2]), h[1], h[2], 1.0 + h[3]]
    st.prep_grid_groups(np.array([prow(p, first[p]) for p in pairs]))
    keep = _grid_outputs(st)
    listed = [(5, 2), (1, 0), (2, 1), (3, 2), (5, 0), (4, 1)]
    st.prep_grid_groups(np.array([prow(p, second[p]) for p in listed]))
    got = _grid_outputs(st)
    now = {p: (second[p] if p in listed else first[p]) for p in pairs}
    var_tau = np.empty((m, G))
    for (g, c) in pairs:
        a, b = rows[g]
        h = now[(g, c)]
        ref = R.prep(s["n"][a:b], *prow((g, c), h)[2:], T, grid=True)
        var_tau[a:b, c] = ref["var_tau"]
        if (g, c) in listed:
            _check_grid_prep(got, ref, T, h, slice(a, b), c, ("prep_grid_groups", g, c))
        else:
            assert all(same_bits(got[k][a:b, c], keep[k][a:b, c]) for k in keep), (g, c)
    opl = {p: 1.0 + now[p][3] for p in pairs}
    sel = [pairs[i] for i in rng.permutation(len(pairs))]
    st.sums_grid_groups_begin([p[0] for p in sel], [p[1] for p in sel], [opl[p] for p in sel])
    batch = st.sums_grid_groups_end()
    for i, (g, c) in enumerate(sel):
        a, b = rows[g]
        exact, scale = R.sums(*(s[k][a:b, c] for k in STATE), s["std_beta"][a:b], var_tau[a:b, c], opl[(g, c)])
        if c == 0:                                            # (std_beta is shared by the columns: it pairs with column 0's eta)
            cancels(exact, scale, 3, b - a)
        check_sums(batch[i], exact, scale, R.sums_ops(weighted=False), b - a, "grid", ("sums_grid_groups", g, c))
        if g == 2:
            assert not batch[i].any()
    st.sums_grid_groups_begin([p[0] for p in sel], [p[1] for p in sel], [opl[p] for p in sel])
    assert same_bits(st.sums_grid_groups_end(), batch)
    for i in (0, 5, 11, 20):
        g, c = sel[i]
        st.sums_grid_groups_begin([g], [c], [opl[(g, c)]])
        assert same_bits(st.sums_grid_groups_end(), batch[[i]])
    plan.close()


# ---- mixtures ---------------------------------------------------------------------------------------------------------------
def _mix_args(h):
    pi, sig, tau, lam = h
    return logit(pi), np.log(tau), tau, float(np.log(1.0 - pi.sum())), sig, 1.0 + lam


def _mix_outputs(st):
    return {"mu_mult": st.download("mu_mult"), "u_logs": st.download("u_logs"), "shvt": st.download("sqrt_half_var_tau"),
            "log_null_pi": st.download("log_null_pi")}


def _check_mix_prep(got, ref, T, h, sl, what):
    lp, lt = _mix_args(h)[:2]
    check_prep({k: v[sl] for k, v in got.items()}, ref, T, (lp[None, :], lt[None, :]), what)


def _stale_log_var_tau(rng, m, K):
    """What the reference's ELBO uses: the log of the INITIAL var_tau -- values that are not log(var_tau) of any prep here."""
    return np.log(10.0 ** rng.uniform(2.0, 6.0, (m, K)))


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("K", [1, 3, 4, 8])
def test_mixture_plan(gpu, T, K):
    from viprs_amd.plan import DeviceState
    for m in (257, 1) if K != 3 else (1803, 255, 256):
        rng = np.random.default_rng(300 + 10 * K + m)
        plan, _ = make_plan([m])
        st = DeviceState(plan, T, "mixture", K)
        h, = hyper(rng, 1, K)
        lv0 = _stale_log_var_tau(rng, m, K)
        st.set_log_var_tau(lv0)
        for peak in ("first", "last"):
            s = make_state(rng, m, T, [(0, m)], peak, width=K, mixture=True)
            upload_state(st, s)
            st.prep_mixture(*_mix_args(h))
            ref = R.prep_mixture(s["n"], *_mix_args(h), T)
            _check_mix_prep(_mix_outputs(st), ref, T, h, slice(None), ("prep_mixture", K, m))
            exact, scale = R.mixture_sums(*(s[k] for k in STATE), s["std_beta"], ref["var_tau"], lv0, 1.0 + h[3])
            cancels(exact, scale, 2, m)
            assert exact.shape == (7 + 6 * K,) and exact[-1] == 0.5
            st.sums_mixture_begin(1.0 + h[3])
            v = st.sums_mixture_end()
            check_sums(v, exact, scale, R.mixture_sums_ops(K), m, "mixture", ("sums_mixture", K))
            st.sums_mixture_begin(1.0 + h[3])
            assert same_bits(st.sums_mixture_end(), v)
        plan.close()


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("K", [1, 3, 4, 8])
def test_mixture_groups(gpu, T, K):
    from viprs_amd.plan import DeviceState
    rng = np.random.default_rng(400 + K)
    plan, gs = make_plan(GROUPS)
    rows, G, m = _rows(gs), len(GROUPS), plan.m
    st = DeviceState(plan, T, "mixture", K)
    st.set_groups(gs)
    s = make_state(rng, m, T, rows, "last" if K % 2 else "first", width=K, mixture=True)
    upload_state(st, s)
    lv0 = _stale_log_var_tau(rng, m, K)
    st.set_log_var_tau(lv0)
    first, second = hyper(rng, G, K), hyper(rng, G, K)

    def prow(g, h):
        lp, lt, tau, lnp, sig, opl = _mix_args(h)
        return np.concatenate([[g, lnp, sig, opl], lp, lt, tau])
    st.prep_mixture_groups(np.array([prow(g, first[g]) for g in range(G)]))
    keep = _mix_outputs(st)
    listed = [6, 3, 2, 1]
    st.prep_mixture_groups(np.array([prow(g, second[g]) for g in listed]))
    got = _mix_outputs(st)
    now = [second[g] if g in listed else first[g] for g in range(G)]
    var_tau = np.empty((m, K))
    for g, (a, b) in enumerate(rows):
        ref = R.prep_mixture(s["n"][a:b], *_mix_args(now[g]), T)
        var_tau[a:b] = ref["var_tau"]
        if g in listed:
            _check_mix_prep(got, ref, T, now[g], slice(a, b), ("prep_mixture_groups", K, g))
        else:
            assert all(same_bits(got[k][a:b], keep[k][a:b]) for k in keep), g
    opl = [1.0 + h[3] for h in now]
    st.sums_mixture_groups_begin(np.arange(G), opl)
    allv = st.sums_mixture_groups_end()
    assert allv.shape == (G, 7 + 6 * K)
    for g, (a, b) in enumerate(rows):
        exact, scale = R.mixture_sums(*(s[k][a:b] for k in STATE), s["std_beta"][a:b], var_tau[a:b], lv0[a:b], opl[g])
        check_sums(allv[g], exact, scale, R.mixture_sums_ops(K), b - a, "mixture", ("sums_mixture_groups", K, g))
    assert not allv[2].any()
    st.sums_mixture_groups_begin(np.arange(G), opl)
    assert same_bits(st.sums_mixture_groups_end(), allv)
    order = [5, 2, 0, 4]
    st.sums_mixture_groups_begin(order, [opl[g] for g in order])
    assert same_bits(st.sums_mixture_groups_end(), allv[order])
    for g in (1, 3):
        st.sums_mixture_groups_begin([g], [opl[g]])
        assert same_bits(st.sums_mixture_groups_end(), allv[[g]])
    plan.close()


# ---- the capped regime of the reduction: rows longer than cap * 256 SNPs ----------------------------------------------------
FULL = 1024 * 256                                             # spike-and-slab / mixture rows: 1 024 workgroups at most
FULL_GRID = 256 * 256                                         # grid rows: 256


@pytest.mark.parametrize("T", DTYPES)
def test_long_rows_spike_slab(gpu, T):
    """Groups of cap * 256 - 1 and cap * 256 + 1 SNPs (the strided loop starts at the second), the whole plan = 2 cap * 256 SNPs
    (two full passes; the final kernel walks 16 partials per lane)."""
    from viprs_amd.plan import DeviceState
    rng = np.random.default_rng(11)
    plan, gs = make_plan([FULL - 1, FULL + 1], block=64, ld_dtype=np.int8)
    rows, m = _rows(gs), plan.m
    st = DeviceState(plan, T, placement="off")
    s = make_state(rng, m, T, rows, "last")
    upload_state(st, s)
    (pi, sig, tau, lam), (pi2, sig2, tau2, lam2) = hyper(rng, 2)
    st.prep(logit(pi), np.log(tau), sig, tau, 1.0 + lam)
    ref = R.prep(s["n"], logit(pi), np.log(tau), sig, tau, 1.0 + lam, T)
    check_prep({"mu_mult": st.download("mu_mult"), "u_logs": st.download("u_logs"), "shvt": st.download("sqrt_half_var_tau")},
               ref, T, (logit(pi), np.log(tau)), "prep, long")
    w = np.repeat(1.0 / np.diff(gs), np.diff(gs))
    st.set_snp_weights(w)
    exact, scale = R.sums(*(s[k] for k in STATE), s["std_beta"], ref["var_tau"], 1.0 + lam, weight=w)
    cancels(exact, scale, 3, m)
    v = st.sums(1.0 + lam)
    check_sums(v, exact, scale, R.sums_ops(True), m, "spike_slab", "sums, long")
    assert same_bits(st.sums(1.0 + lam), v)
    st.set_groups(gs)
    st.prep_groups(np.array([[1, logit(pi2), np.log(tau2), sig2, tau2, 1.0 + lam2]]))
    a, b = rows[1]
    ref2 = R.prep(s["n"][a:b], logit(pi2), np.log(tau2), sig2, tau2, 1.0 + lam2, T)
    check_prep({"mu_mult": st.download("mu_mult")[a:b], "u_logs": st.download("u_logs")[a:b],
                "shvt": st.download("sqrt_half_var_tau")[a:b]}, ref2, T, (logit(pi2), np.log(tau2)), "prep_groups, long")
    var_tau = np.concatenate([ref["var_tau"][:a], ref2["var_tau"]])
    opl = [1.0 + lam, 1.0 + lam2]
    st.sums_groups_begin([1, 0], opl[::-1])
    gv = st.sums_groups_end()
    for i, g in enumerate((1, 0)):
        a, b = rows[g]
        exact, scale = R.sums(*(s[k][a:b] for k in STATE), s["std_beta"][a:b], var_tau[a:b], opl[g])
        check_sums(gv[i], exact, scale, R.sums_ops(False), b - a, "spike_slab", ("sums_groups, long", g))
    st.sums_groups_begin([1, 0], opl[::-1])
    assert same_bits(st.sums_groups_end(), gv)
    plan.close()


@pytest.mark.parametrize("T,K", [("float32", 3), ("float64", 8)])
def test_long_rows_mixture(gpu, T, K):
    from viprs_amd.plan import DeviceState
    rng = np.random.default_rng(12)
    plan, gs = make_plan([FULL + 1, FULL - 1], block=64, ld_dtype=np.int8)
    rows, m = _rows(gs), plan.m
    st = DeviceState(plan, T, "mixture", K, placement="off")
    s = make_state(rng, m, T, rows, "first", width=K, mixture=True)
    upload_state(st, s)
    lv0 = _stale_log_var_tau(rng, m, K)
    st.set_log_var_tau(lv0)
    h, h1 = hyper(rng, 2, K)
    st.prep_mixture(*_mix_args(h))
    ref = R.prep_mixture(s["n"], *_mix_args(h), T)
    _check_mix_prep(_mix_outputs(st), ref, T, h, slice(None), ("prep_mixture, long", K))
    exact, scale = R.mixture_sums(*(s[k] for k in STATE), s["std_beta"], ref["var_tau"], lv0, 1.0 + h[3])
    st.sums_mixture_begin(1.0 + h[3])
    v = st.sums_mixture_end()
    check_sums(v, exact, scale, R.mixture_sums_ops(K), m, "mixture", ("sums_mixture, long", K))
    st.set_groups(gs)
    lp, lt, tau, lnp, sig, opl1 = _mix_args(h1)
    st.prep_mixture_groups(np.array([np.concatenate([[1, lnp, sig, opl1], lp, lt, tau])]))
    a, b = rows[1]
    ref1 = R.prep_mixture(s["n"][a:b], *_mix_args(h1), T)
    _check_mix_prep(_mix_outputs(st), ref1, T, h1, slice(a, b), ("prep_mixture_groups, long", K))
    var_tau = np.concatenate([ref["var_tau"][:a], ref1["var_tau"]])
    opl = [1.0 + h[3], opl1]
    st.sums_mixture_groups_begin([0, 1], opl)
    gv = st.sums_mixture_groups_end()
    for g, (a, b) in enumerate(rows):
        exact, scale = R.mixture_sums(*(s[k][a:b] for k in STATE), s["std_beta"][a:b], var_tau[a:b], lv0[a:b], opl[g])
        check_sums(gv[g], exact, scale, R.mixture_sums_ops(K), b - a, "mixture", ("sums_mixture_groups, long", K, g))
    st.sums_mixture_groups_begin([0, 1], opl)
    assert same_bits(st.sums_mixture_groups_end(), gv)
    plan.close()


@pytest.mark.parametrize("T", DTYPES)
def test_long_rows_grid(gpu, T):
    from viprs_amd.plan import DeviceState
    rng = np.random.default_rng(13)
    G = 2
    plan, gs = make_plan([FULL_GRID - 1, FULL_GRID + 1], block=64, ld_dtype=np.int8)
    rows, m = _rows(gs), plan.m
    st = DeviceState(plan, T, "grid", G)
    s = make_state(rng, m, T, rows, "last", width=G)
    upload_state(st, s, order="F")
    hs = hyper(rng, 4)
    pcol = lambda c, h: [c, logit(h[0]), np.log(h[2]), h[1], h[2], 1.0 + h[3]]
    st.prep_columns(np.array([pcol(c, hs[c]) for c in range(G)]))
    got = _grid_outputs(st)
    for c in range(G):
        ref = R.prep(s["n"], *pcol(c, hs[c])[1:], T, grid=True)
        _check_grid_prep(got, ref, T, hs[c], slice(None), c, ("prep_columns, long", c))
        exact, scale = R.sums(*(s[k][:, c] for k in STATE), s["std_beta"], ref["var_tau"], 1.0 + hs[c][3])
        check_sums(st.sums_column(c, 1.0 + hs[c][3]), exact, scale, R.sums_ops(False), m, "grid", ("sums_column, long", c))
    st.set_groups(gs)
    pairs = [(1, 0), (0, 1), (1, 1), (0, 0)]
    prm = {p: hs[(2 * p[0] + p[1] + 1) % 4] for p in pairs}
    st.prep_grid_groups(np.array([[g, c] + pcol(c, prm[(g, c)])[1:] for g, c in pairs]))
    got = _grid_outputs(st)
    st.sums_grid_groups_begin([p[0] for p in pairs], [p[1] for p in pairs], [1.0 + prm[p][3] for p in pairs])
    gv = st.sums_grid_groups_end()
    for i, (g, c) in enumerate(pairs):
        a, b = rows[g]
        ref = R.prep(s["n"][a:b], *pcol(c, prm[(g, c)])[1:], T, grid=True)
        _check_grid_prep(got, ref, T, prm[(g, c)], slice(a, b), c, ("prep_grid_groups, long", g, c))
        exact, scale = R.sums(*(s[k][a:b, c] for k in STATE), s["std_beta"][a:b], ref["var_tau"], 1.0 + prm[(g, c)][3])
        check_sums(gv[i], exact, scale, R.sums_ops(False), b - a, "grid", ("sums_grid_groups, long", g, c))
    plan.close()


# ---- a diverged state -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", DTYPES)
def test_nan_in_the_state(gpu, T):
    """Documented behaviour, not a demand.  The device's maximum uses `fmax`, which drops NaNs; `np.max(np.abs(.))` does not:
    with a NaN in eta_diff alone, the device returns the largest |eta_diff| of the OTHER SNPs (asserted here as what it does
    today) and every sum is as without it.  That is harmless: eta_diff is NaN only where the sweep wrote NaN into eta as well
    (eta_diff is the change of eta), and then sums [1..4] (spike-and-slab; [0..3] of a mixture) are NaN exactly where the
    reference's are -- asserted below -- so the ELBO is NaN and the fit stops on its non-finite-objective check
    (`VIPRS._after_e_step`, "Objective (ELBO) is undefined", evaluated before the max |eta_diff| rule; the same order in
    `_lockstep.LockstepEM`)."""
    from viprs_amd.plan import DeviceState
    rng = np.random.default_rng(21)
    m, K = 700, 3
    plan, _ = make_plan([m])
    st = DeviceState(plan, T)
    (pi, sig, tau, lam), = hyper(rng, 1)
    s = make_state(rng, m, T, [(0, m)], "last")
    s["eta_diff"][333] = np.nan
    upload_state(st, s)
    st.prep(logit(pi), np.log(tau), sig, tau, 1.0 + lam)
    vt = R.prep(s["n"], logit(pi), np.log(tau), sig, tau, 1.0 + lam, T)["var_tau"]
    exact, scale = R.sums(*(s[k] for k in STATE), s["std_beta"], vt, 1.0 + lam)
    assert np.isnan(exact[10]) and not np.isnan(exact[:10]).any()
    exact[10] = 0.5                                           # what the device returns today: the NaN is dropped
    check_sums(st.sums(1.0 + lam), exact, scale, R.sums_ops(False), m, "spike_slab", "NaN in eta_diff")
    s["eta"][333] = s["var_mu"][333] = np.nan                # the diverged SNP as a sweep leaves it
    st.upload("eta", s["eta"])
    st.upload("var_mu", s["var_mu"])
    exact, scale = R.sums(*(s[k] for k in STATE), s["std_beta"], vt, 1.0 + lam)
    assert np.isnan(exact[1:5]).all()
    exact[10] = 0.5
    v = st.sums(1.0 + lam)
    check_sums(v, exact, scale, R.sums_ops(False), m, "spike_slab", "NaN in eta")
    assert np.isnan(v[1:5]).all() and not np.isnan(v[5:]).any()
    # the same for a mixture
    stm = DeviceState(plan, T, "mixture", K)
    h, = hyper(rng, 1, K)
    s = make_state(rng, m, T, [(0, m)], "first", width=K, mixture=True)
    s["eta_diff"][333] = s["eta"][333] = s["var_mu"][333, 1] = np.nan
    upload_state(stm, s)
    lv0 = _stale_log_var_tau(rng, m, K)
    stm.set_log_var_tau(lv0)
    stm.prep_mixture(*_mix_args(h))
    vt = R.prep_mixture(s["n"], *_mix_args(h), T)["var_tau"]
    exact, scale = R.mixture_sums(*(s[k] for k in STATE), s["std_beta"], vt, lv0, 1.0 + h[3])
    assert np.isnan(exact[:4]).all() and np.isnan(exact[-1])
    exact[-1] = 0.5
    stm.sums_mixture_begin(1.0 + h[3])
    check_sums(stm.sums_mixture_end(), exact, scale, R.mixture_sums_ops(K), m, "mixture", "NaN in eta, mixture")
    plan.close()
