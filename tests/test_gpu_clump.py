"""Greedy LD clumping on the device (`viprs_plan_clump`, include/viprs_hip.h) against the host implementation
`viprs_amd.stats.clump.clump_host` with `==`: every storage of both LD forms, every LD dtype, 1 / 5 / 32 columns, with and
without members; independence / determinism; the refusals; a clump between two sweeps; and the model layer
(`ClumpThreshold`, the .bed pipeline).  The host references are computed once per case and never modified."""
import ctypes
import functools

import numpy as np
import pytest

from tests.test_clump_reference import chisq_draw
from tests.test_gpu_ld_dot import _banded_windows, _float64_sweep, _sweep_state
from viprs_amd.stats.clump import clump_host, clump_order
from viprs_amd.utils import synthetic as syn

pytestmark = pytest.mark.gpu

# dense block sizes straddling one 16-byte load (4 / 8 / 16 elements), one pass of the 256-thread workgroup over a row
# (256 x V = 1024 / 2048 / 4096 elements) and the 64-column padding of the dense squares
DENSE_SIZES = (1, 63, 64, 65, 255, 257, 1023, 1025, 2047, 2049, 2305, 4095, 4097)
SMALL_SIZES = (500, 65, 257)
R2_5 = (0.05, 0.1, 0.2, 0.5, 0.8)
R2_32 = tuple(float(x) for x in np.round(np.linspace(0.02, 0.64, 32), 4))
LD_DTYPES = {"int8": np.int8, "int16": np.int16, "fp32": np.float32, "int32": np.int32, "int64": np.int64, "fp64": np.float64}
CASES = [(k, l) for k in ("dense", "small", "banded") for l in ("int8", "fp32")] + \
        [(k, l) for k in ("small", "banded") for l in ("int16", "int32", "int64", "fp64")]


def _arrays(kind, ld_name, low_memory):
    ld_dtype = LD_DTYPES[ld_name]
    if kind == "banded":
        lb, ip = _banded_windows(2500, 90, 140, low_memory, seed=14, jitter=60)
        u = np.random.default_rng(15).uniform(-1.0, 1.0, int(ip[-1])) ** 3         # (most entries small, a few near +-1)
        if np.issubdtype(ld_dtype, np.floating):
            return lb, ip, u.astype(ld_dtype), 1.0
        qmax = min(float(np.iinfo(ld_dtype).max), 2.0 ** 30 if ld_dtype == np.int32 else 2.0 ** 52)
        return lb, ip, np.round(u * qmax).astype(ld_dtype), 1.0 / qmax
    sizes = DENSE_SIZES if kind == "dense" else SMALL_SIZES
    ld = syn.make_ld(sizes, low_memory=low_memory, ld_dtype=ld_dtype, kind="longrange", seed=5, rho_range=(0.6, 0.95))
    dq = ld.dq_scale
    if ld_dtype == np.int32:
        dq = 2.0 ** -30                             # (make_ld caps the quantisation of the wide integers)
    elif ld_dtype == np.int64:
        dq = 2.0 ** -52
    return ld.ld_left_bound, ld.ld_indptr, ld.ld_data, dq


@functools.lru_cache(maxsize=None)
def case(kind, ld_name, low_memory):
    """The arrays, the order (chi^2 >= 1), the members (chi^2 >= 0.3) and the host results for 5 columns with and without
    members -- and, on the small and the banded shape, for 32 columns.  The conditions that keep the comparison from
    passing vacuously are asserted here, on the host results."""
    lb, ip, data, dq = _arrays(kind, ld_name, low_memory)
    m = lb.shape[0]
    chisq = chisq_draw(m, 7)
    order, member = clump_order(chisq, 1.0), chisq >= 0.3
    ref = {(5, True): clump_host(lb, ip, data, low_memory, order, R2_5, member, dq),
           (5, False): clump_host(lb, ip, data, low_memory, order, R2_5, None, dq)}
    if kind != "dense":
        ref[(32, True)] = clump_host(lb, ip, data, low_memory, order, R2_32, member, dq)
    own = np.arange(m)[:, None]
    for (n_cols, with_member), r in ref.items():
        claimed = ((r >= 0) & (r != own)).sum(axis=0)
        members = int(member.sum()) if with_member else m
        for g, r2 in enumerate(R2_5 if n_cols == 5 else R2_32):
            if r2 <= 0.2:
                assert claimed[g] >= 0.1 * members, (kind, ld_name, low_memory, r2, int(claimed[g]), members)
        if n_cols == 5:
            assert np.all((r[:, 1:] != r[:, :-1]).sum(axis=0) >= 5), "adjacent columns differ in at least 5 SNPs"
        else:                                       # (32 thresholds 0.02 apart: neighbours may agree, the range does not)
            assert len({r[:, g].tobytes() for g in range(n_cols)}) >= 8, "at least 8 different columns among the 32"
    assert np.any(clump_host(lb, ip, data, low_memory, order[::-1], R2_5[2], member, dq) != ref[(5, True)][:, 2]), \
        "reversing the order changes the result"
    for a in (lb, ip, data, order, member, *ref.values()):
        a.setflags(write=False)
    return lb, ip, data, dq, order, member, ref


def _first_difference(got, want):
    bad = np.argwhere(got != want)
    if not bad.size:
        return ""
    j, g = (int(v) for v in bad[0])
    return f"{bad.shape[0]} values differ, first at SNP {j} column {g}: got {int(got[j, g])}, want {int(want[j, g])}"


@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
@pytest.mark.parametrize("kind, ld_name", CASES)
def test_device_equals_the_host_reference(gpu, kind, ld_name, low_memory):
    from viprs_amd import _lib as L
    from viprs_amd.plan import LDPlan
    lb, ip, data, dq, order, member, ref = case(kind, ld_name, low_memory)
    m = lb.shape[0]
    plan = LDPlan(lb, ip, data, low_memory)

    def check(storage):
        for (n_cols, with_member), want in ref.items():
            r2 = R2_5 if n_cols == 5 else R2_32
            got = plan.clump(order, r2, member=member if with_member else None, dq_scale=dq)
            assert got.shape == (m, n_cols) and got.dtype == np.int32 and got.flags.f_contiguous
            diff = _first_difference(got, want)
            assert not diff, f"{kind} {ld_name} upper={low_memory} {storage} n_cols={n_cols} member={with_member}: {diff}"
        # one column: a scalar threshold gives (m,), the same column as inside the 5-column call; a second call the same
        one = plan.clump(order, R2_5[1], member=member, dq_scale=dq)
        assert one.shape == (m,) and np.array_equal(one, ref[(5, True)][:, 1]), f"{storage}: a column alone"
        assert np.array_equal(plan.clump(order, R2_5[1], member=member, dq_scale=dq), one), "a repeated call changed the result"
    try:
        check("as created")
        assert plan.last_clump_ms() > 0.0
        if low_memory:
            # the dense blocks in the float64 sweeps' storage (zero lower triangle): entries left of the diagonal are read
            # from the column above it
            dense = plan.info(L.INFO_N_DENSE) > 0
            assert not dense or plan.info(L.INFO_UPPER_MIRRORED) == 1
            _float64_sweep(plan)
            assert not dense or plan.info(L.INFO_UPPER_MIRRORED) == 0
            check("zero lower triangle")
            assert not dense or plan.info(L.INFO_UPPER_MIRRORED) == 0, "the call converted the storage"
    finally:
        plan.close()


@pytest.mark.parametrize("low_memory", [False, True], ids=["sym", "upper"])
def test_edges_and_independence(gpu, low_memory):
    from viprs_amd.plan import LDPlan
    lb, ip, data, dq, order, member, ref = case("small", "int8", low_memory)
    m = lb.shape[0]
    plan = LDPlan(lb, ip, data, low_memory)
    try:
        ring = plan.timing_history()
        # an empty order claims nothing
        assert np.all(plan.clump(np.zeros(0, np.int32), R2_5, dq_scale=dq) == -1)
        # r2 = 0: every entry passes -- the first SNP of a block's piece of the order takes the whole block (its members)
        zero = plan.clump(order, 0.0, member=member, dq_scale=dq)
        assert np.array_equal(zero, clump_host(lb, ip, data, low_memory, order, 0.0, member, dq))
        starts = np.concatenate([[0], np.cumsum(SMALL_SIZES)])
        for s, e in zip(starts[:-1], starts[1:]):
            first = next(int(j) for j in order if s <= j < e)
            assert np.all(zero[s:e][member[s:e]] == first) and np.all(zero[s:e][~member[s:e]] == -1)
        # r2 above every entry: every SNP of the order is its own index SNP, nobody else is claimed
        above = plan.clump(order, 4.0, member=member, dq_scale=dq)
        want = np.full(m, -1, dtype=np.int32)
        want[order] = order
        assert np.array_equal(above, want)
        # the natural order (LD pruning) and the reverse order
        for o in (np.arange(m), np.arange(m)[::-1]):
            assert np.array_equal(plan.clump(o, R2_5, dq_scale=dq), clump_host(lb, ip, data, low_memory, o, R2_5, None, dq))
        # a column does not depend on the other columns, nor on their number
        full = plan.clump(order, R2_32, member=member, dq_scale=dq)
        assert np.array_equal(full, ref[(32, True)])
        for g in (0, 13, 31):
            other = list(R2_32[::-1])
            other[g] = R2_32[g]
            assert np.array_equal(plan.clump(order, other, member=member, dq_scale=dq)[:, g], full[:, g]), g
            assert np.array_equal(plan.clump(order, R2_32[g:g + 1], member=member, dq_scale=dq)[:, 0], full[:, g]), g
        # the active-block filter of the sweeps does not reach the call; the sweeps' timing ring never sees it
        plan.set_active_blocks(np.arange(plan.n_blocks) % 2 == 0)
        assert np.array_equal(plan.clump(order, R2_32, member=member, dq_scale=dq), full)
        plan.set_active_blocks(None)
        assert plan.timing_history() == ring
    finally:
        plan.close()


def test_argument_checks_with_a_plan(gpu):
    from viprs_amd import _lib as L
    from viprs_amd.plan import LDPlan
    ld = syn.make_ld([65, 30], low_memory=True, kind="longrange", ld_dtype=np.int8, seed=8)
    plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, True)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    try:
        out = np.full((ld.m, 33), 7, dtype=np.int32, order="F")
        order = np.arange(10, dtype=np.int32)
        member = np.ones(ld.m, dtype=np.uint8)
        member[50] = 0
        r2 = np.full(33, 0.1)
        ms = ctypes.c_double(-1.0)
        assert L.lib.viprs_plan_last_clump_ms(plan.handle, ctypes.byref(ms)) == L.EINVAL and ms.value == -1.0
        repeated = np.array([3, 4, 3], dtype=np.int32)
        outside = np.array([3, ld.m], dtype=np.int32)
        negative = np.array([-1], dtype=np.int32)
        not_member = np.array([3, 50], dtype=np.int32)
        for args, word in (((10, vp(order), None, 33, vp(r2), 1.0, vp(out)), "n_cols"),
                           ((10, vp(order), None, 0, vp(r2), 1.0, vp(out)), "n_cols"),
                           ((3, vp(repeated), None, 2, vp(r2), 1.0, vp(out)), "repeated"),
                           ((2, vp(outside), None, 2, vp(r2), 1.0, vp(out)), "out of range"),
                           ((1, vp(negative), None, 2, vp(r2), 1.0, vp(out)), "out of range"),
                           ((2, vp(not_member), vp(member), 2, vp(r2), 1.0, vp(out)), "member"),
                           ((10, None, None, 2, vp(r2), 1.0, vp(out)), "order"),
                           ((10, vp(order), None, 2, None, 1.0, vp(out)), "r2"),
                           ((10, vp(order), None, 2, vp(r2), 0.0, vp(out)), "dq_scale"),
                           ((10, vp(order), None, 2, vp(np.array([0.1, -1.0])), 1.0, vp(out)), "thresholds"),
                           ((10, vp(order), None, 2, vp(r2), 1.0, None), "null")):
            assert L.lib.viprs_plan_clump(plan.handle, *args) == L.EINVAL, word
            assert word in L.last_error(), (word, L.last_error())
        assert np.all(out == 7)
        for kw in (dict(order=[3, 4, 3]), dict(order=[3, 50], member=member), dict(order=[ld.m]), dict(order=[3], r2=[0.1] * 33),
                   dict(order=[3], member=np.ones(ld.m + 1))):
            with pytest.raises(ValueError):
                plan.clump(np.asarray(kw["order"]), kw.get("r2", 0.1), member=kw.get("member"))
        # the same SNP as a member is fine
        assert plan.clump(np.array([3, 50]), 0.1, dq_scale=ld.dq_scale)[50] in (3, 50)
    finally:
        plan.close()
    empty = LDPlan(np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.int8), True)
    try:
        assert empty.clump(np.zeros(0, np.int32), (0.1, 0.2)).shape == (0, 2)
        assert L.lib.viprs_plan_clump(empty.handle, 0, None, None, 2, vp(r2), 1.0, vp(out)) == L.OK and np.all(out == 7)
    finally:
        empty.close()


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_clump_between_sweeps_leaves_the_sweeps_alone(gpu, T):
    """Upper form: the fp32 sweeps and the float64 sweeps keep the dense blocks in different storages; a clump between two
    sweeps reads whichever is there and must not disturb what the second sweep computes."""
    from viprs_amd.plan import LDPlan
    ld, ss, inp = syn.make_problem(sizes=[500, 130, 1700], low_memory=True, seed=3, kind="longrange", float_precision=T)
    order = clump_order(chisq_draw(ld.m, 7), 1.0)
    want = clump_host(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, True, order, R2_5, None, ld.dq_scale)
    out = []
    for with_clump in (False, True):
        plan = LDPlan(ld.ld_left_bound, ld.ld_indptr, ld.ld_data, True)
        try:
            st = _sweep_state(plan, inp, T)
            st.e_step(ld.dq_scale)
            if with_clump:
                assert np.array_equal(plan.clump(order, R2_5, dq_scale=ld.dq_scale), want)
            st.e_step(ld.dq_scale)
            out.append({k: st.download(k) for k in ("var_gamma", "var_mu", "eta", "q", "eta_diff")})
        finally:
            plan.close()
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k


def test_model_layer(gpu):
    """`ClumpThreshold(gdl).fit()` on the device is the hook path on the host; `stats.clump.clump` on the device is its
    host path."""
    from viprs_amd.data import ArrayDataLoader
    from viprs_amd.model import ClumpThreshold
    from viprs_amd.stats import clump as C
    gdl = ArrayDataLoader.synthetic({1: [300, 130], 2: [257], 3: [65, 90]}, ld_dtype=np.int8, n=5e4, kind="longrange", h2=0.5)
    for kw in (dict(dequantize_on_the_fly=True), dict(low_memory=False), dict(float_precision="float64")):
        dev = ClumpThreshold(gdl, **kw).fit()
        host = ClumpThreshold(gdl, clump_fn=C.clump_host, **kw).fit()
        assert dev.n_models == 36 and dev.grid_table.equals(host.grid_table)
        n = dev.grid_table["n_snps"].to_numpy()
        assert 0 < n.min() < n.max() <= gdl.m
        for c in gdl.shapes:
            assert np.array_equal(dev.index_of[c], host.index_of[c]), (kw, c)
            assert dev.post_mean_beta[c].dtype == host.post_mean_beta[c].dtype
            assert np.array_equal(dev.post_mean_beta[c], host.post_mean_beta[c])
        # pseudo-validation through the plan's product against the host's float64 product
        vb = {c: np.asarray(gdl.sumstats_table[c].get_snp_pseudo_corr(), dtype=np.float64) for c in gdl.shapes}
        np.testing.assert_allclose(dev.pseudo_validate(vb), host.pseudo_validate(vb), rtol=1e-4)
    got = C.clump(gdl, r2=(0.1, 0.5), p1=0.05, p2=0.5, dequantize_on_the_fly=True)
    want = C.clump(gdl, r2=(0.1, 0.5), p1=0.05, p2=0.5, dequantize_on_the_fly=True, clump_fn=C.clump_host)
    for c in gdl.shapes:
        assert got[c].shape == (gdl.shapes[c], 2) and np.array_equal(got[c], want[c])
        assert np.any((want[c] >= 0) & (want[c] != np.arange(gdl.shapes[c])[:, None]))


def test_from_a_bed_to_clumped_scores(gpu, tmp_path):
    """The .bed pipeline: perform_gwas -> compute_ld -> ClumpThreshold.fit -> predict."""
    from tests import genotype_gwas_reference as R
    from viprs_amd.data import ArrayDataLoader
    from viprs_amd.io.plink_bed import write_bed
    from viprs_amd.model import ClumpThreshold
    rng = np.random.default_rng(25)
    m, n = 300, 600
    beta = rng.standard_normal(m) * (rng.random(m) < 0.1)
    codes = R.random_codes(rng, m, n, 0.02)
    g = np.array([2.0, 0.0, 1.0, 0.0])[codes].T @ beta
    y = g + rng.standard_normal(n) * np.sqrt(g.var())
    prefix = str(tmp_path / "cohort")
    write_bed(prefix, codes, None, y)
    gdl = ArrayDataLoader({}, {}, genotype={22: prefix})
    try:
        gdl.perform_gwas()
        gdl.compute_ld(("windowed", 50))
        model = ClumpThreshold(gdl).fit()
        prs = model.predict()
        assert prs.shape == (n, model.n_models) and model.n_models == 36 and np.all(np.isfinite(prs))
        n_snps = model.grid_table["n_snps"].to_numpy()
        assert n_snps.max() > 0 and np.all(np.ptp(prs[:, n_snps > 0], axis=0) > 0)
        model.select_best(validation_gdl=gdl)
        assert model.predict().shape == (n,) and np.corrcoef(model.predict(), y)[0, 1] > 0.3
    finally:
        gdl.close_genotypes()
