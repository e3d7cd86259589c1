"""CPU: the path from a data loader's LD matrix objects to host arrays and from there to device plans, as every entry
point walks it -- `VIPRS`, `LDPredInf`, `stats.ldsc.ld_scores`, `stats.spectrum.ld_spectrum` and `_pseudo_r2_external`.

The LD matrices record every ``load(return_symmetric, dtype)``; `viprs_amd.plan.LDPlan` / `DeviceState` are replaced by
fakes that record which constructor was used with what, into the same log.  What is expected stands in the tables below
as literals.  Two chromosomes, LD blocks of [1, 5, 33, 70] and [3, 66] SNPs: a single-SNP block, a small one and one past
64 SNPs each.
"""
import numpy as np
import pytest

from viprs_amd import _lib, plan as plan_mod
from viprs_amd.data import ArrayDataLoader, LDArrays, SumstatsArrays
from viprs_amd.utils import synthetic as syn

SIZES = {1: [1, 5, 33, 70], 2: [3, 66]}
M = {1: 109, 2: 69}
NNZ = {"upper": {1: 2953, 2: 2148}, "symmetric": {1: 6015, 2: 4365}}      # sum b (b - 1) / 2, sum b^2


class RecordingLD(LDArrays):
    """`LDArrays` that logs ``("load", chromosome, return_symmetric, dtype name)``."""

    def __init__(self, log, chrom, **kw):
        super().__init__(**kw)
        self.log, self.chrom = log, chrom

    def load(self, return_symmetric=False, dtype=None):
        self.log.append(("load", self.chrom, bool(return_symmetric), None if dtype is None else np.dtype(dtype).name))
        return super().load(return_symmetric, dtype)


class RecordingRowStore(RecordingLD):
    """An upper-only store that hands out row ranges (the surface of `ZarrLDMatrix` that the multi-rank deal uses)."""

    def indptr(self):
        return self._forms[False][1]

    def load_rows(self, start, stop, dtype=None):
        self.log.append(("load_rows", self.chrom, int(start), int(stop)))
        lb, ip, data = self._forms[False]
        a, e = int(ip[start]), int(ip[stop])
        return lb[start:stop], ip[start:stop + 1] - ip[start], data[a:e] if dtype is None else data[a:e].astype(dtype)


def _no_device_fn(*a, **k):
    raise AssertionError("the constructor path calls neither the E-step nor the solver")


def _loader(log, forms="both", stored="int8", cls=RecordingLD, sample_size=None, **kw):
    """`stored`: one dtype name, or ``{chromosome: name}``."""
    ld, ss = {}, {}
    for c, sizes in SIZES.items():
        dt = np.dtype(stored[c] if isinstance(stored, dict) else stored)
        sym = syn.make_ld(sizes, low_memory=False, ld_dtype=dt, seed=40 + c)
        up = syn.make_ld(sizes, low_memory=True, ld_dtype=dt, seed=40 + c)
        ld[c] = cls(log, c, symmetric=(sym.ld_left_bound, sym.ld_indptr, sym.ld_data) if forms == "both" else None,
                    upper=(up.ld_left_bound, up.ld_indptr, up.ld_data), stored_dtype=dt, dq_scale=sym.dq_scale,
                    sample_size=sample_size)
        s = syn.make_sumstats(sym, seed=40 + c, **kw)
        ss[c] = SumstatsArrays(s.std_beta, s.n_per_snp)
    return ArrayDataLoader(ld, ss)


@pytest.fixture
def log(monkeypatch):
    """The shared event log, with the fakes installed on `viprs_amd.plan` (after `viprs_amd` was imported: the code under
    test has to look the classes up when it is called)."""
    events = []

    class FakePlan:
        def __init__(self, lb, ip, data, low_memory, device=0, math_mode="exact"):
            plan_mod._check_index_arrays(lb, ip)                        # (what the real constructor refuses)
            self._init("LDPlan", int(lb.shape[0]), ip, data, low_memory)

        @classmethod
        def from_upper(cls, ip, data, diag_value=None, device=0, math_mode="exact"):
            assert isinstance(ip, np.ndarray) and ip.dtype in (np.int32, np.int64) and ip.flags.c_contiguous
            self = cls.__new__(cls)
            self._init("from_upper", int(ip.shape[0]) - 1, ip, data, False)
            return self

        def _init(self, ctor, m, ip, data, low_memory):
            assert isinstance(data, np.ndarray) and data.ndim == 1 and data.flags.c_contiguous
            assert int(ip[-1]) == data.shape[0]
            self.m, self.low_memory, self.ld_dtype, self.closed = m, bool(low_memory), data.dtype, False
            self.indptr, self.data = ip, data
            events.append(("plan", ctor, bool(low_memory), data.dtype.name, int(data.shape[0]), m))

        def close(self):
            self.closed = True
            events.append(("close", self.m))

        def blocks(self):
            return np.array([0, self.m], dtype=np.int64), np.zeros(1, np.int32)

        def extremal_eigenvalues(self, dq_scale=1.0, rtol=None, maxiter=None, float_precision="float32"):
            events.append(("extremal_eigenvalues", float(dq_scale), float_precision))
            return plan_mod.SpectrumInfo([0.25], [3.0], [0.0], [0.0], [7], [0])

        def ld_scores(self, weights=None, correction=None, dq_scale=1.0, float_precision="float32"):
            events.append(("ld_scores", float(dq_scale), float_precision))
            return np.ones(self.m)

        def dot(self, B, dq_scale=1.0, include_diagonal=True):
            events.append(("dot", self.m, float(dq_scale)))
            return np.asarray(B)

    class FakeState:
        def __init__(self, plan, float_precision="float32", model="spike_slab", width=1, placement=None):
            self.plan = plan
            events.append(("state", plan.m))

        def upload(self, name, arr):
            assert arr.shape[0] == self.plan.m
            events.append(("upload", name, self.plan.m))

        def set_n_per_snp(self, n):
            assert np.asarray(n).shape[0] == self.plan.m
            events.append(("set_n_per_snp", self.plan.m))

        def set_snp_weights(self, w):
            assert np.asarray(w).shape[0] == self.plan.m
            events.append(("set_snp_weights", self.plan.m))

    monkeypatch.setattr(plan_mod, "LDPlan", FakePlan)
    monkeypatch.setattr(plan_mod, "DeviceState", FakeState)
    monkeypatch.setattr(_lib, "device_count", lambda: 1)
    return events


def _of(log, *kinds):
    return [e for e in log if e[0] in kinds]


# ---- VIPRS: the table --------------------------------------------------------------------------------------------------
# low_memory, expand_ld_on_device, forms | return_symmetric of the load calls of ONE chromosome, plan constructor, the
# plan's low_memory, the form of the arrays that reach it, `_expanded`   (None: the constructor raises ValueError)
FORM_ROWS = [
    (True, None, "both", ([False], "LDPlan", True, "upper", False)),
    (True, None, "upper", ([False], "LDPlan", True, "upper", False)),
    (True, True, "both", ([False], "LDPlan", True, "upper", False)),
    (True, True, "upper", ([False], "LDPlan", True, "upper", False)),
    (True, False, "both", ([False], "LDPlan", True, "upper", False)),
    (True, False, "upper", ([False], "LDPlan", True, "upper", False)),
    (False, None, "both", ([True], "LDPlan", False, "symmetric", False)),
    (False, None, "upper", ([True, False], "from_upper", False, "upper", True)),     # asks, is refused, loads the store
    (False, True, "both", ([False], "from_upper", False, "upper", True)),
    (False, True, "upper", ([False], "from_upper", False, "upper", True)),
    (False, False, "both", ([True], "LDPlan", False, "symmetric", False)),
    (False, False, "upper", None),
]
# stored dtype, dequantize_on_the_fly given | dtype asked of load(), dequantize_on_the_fly kept, dequantize_scale,
# dtype of ld_data[c]
DTYPE_ROWS = [
    ("int8", True, ("int8", True, 1.0 / 127, "int8")),
    ("int8", False, ("float32", False, 1.0, "float32")),
    ("float32", True, ("float32", False, 1.0, "float32")),
]


def _ids(rows):
    return ["-".join(str(x) for x in r[:-1]) for r in rows]


@pytest.mark.parametrize("merge", [True, False], ids=["merged", "per-chromosome"])
@pytest.mark.parametrize("dtype_row", DTYPE_ROWS, ids=_ids(DTYPE_ROWS))
@pytest.mark.parametrize("form_row", FORM_ROWS, ids=_ids(FORM_ROWS))
def test_viprs_constructor_loads_and_plans(log, form_row, dtype_row, merge):
    from viprs_amd.model import VIPRS
    low_memory, expand, forms, want = form_row
    stored, deq, (load_dtype, deq_kept, scale, data_dtype) = dtype_row
    gdl = _loader(log, forms, stored)
    kw = dict(low_memory=low_memory, expand_ld_on_device=expand, dequantize_on_the_fly=deq, merge_chromosomes=merge)
    if want is None:
        with pytest.raises(ValueError, match="return_symmetric=True was not provided"):
            VIPRS(gdl, **kw)
        assert _of(log, "load") == [("load", 1, True, load_dtype)] and not _of(log, "plan")
        return
    loads, ctor, plan_low_memory, form, expanded = want
    v = VIPRS(gdl, **kw)
    assert _of(log, "load") == [("load", c, rs, load_dtype) for c in (1, 2) for rs in loads]
    if merge:
        plans = [("plan", ctor, plan_low_memory, data_dtype, NNZ[form][1] + NNZ[form][2], M[1] + M[2])]
    else:
        plans = [("plan", ctor, plan_low_memory, data_dtype, NNZ[form][c], M[c]) for c in (1, 2)]
    assert _of(log, "plan") == plans
    assert v._merged is merge and sorted(v._plans) == (["*"] if merge else [1, 2])
    assert v._expanded is expanded
    assert v.dequantize_on_the_fly is deq_kept
    assert v.dequantize_scale == scale
    for c in (1, 2):
        assert v.ld_data[c].dtype == np.dtype(data_dtype) and v.ld_data[c].shape[0] == NNZ[form][c]
        assert v.ld_left_bound[c].dtype == np.int32 and v.ld_indptr[c].shape[0] == M[c] + 1


def test_viprs_order_of_device_work(log):
    """All host loads come before the first plan; plans and states in sorted chromosome order; per-chromosome layout:
    `set_n_per_snp` after all plans exist; merged layout: upload, set_n_per_snp, set_snp_weights."""
    from viprs_amd.model import VIPRS
    VIPRS(_loader(log), merge_chromosomes=False)
    assert [e[0] for e in log[:2]] == ["load", "load"]
    assert log[2:] == [("plan", "LDPlan", True, "float32", 2953, 109), ("state", 109), ("upload", "std_beta", 109),
                       ("plan", "LDPlan", True, "float32", 2148, 69), ("state", 69), ("upload", "std_beta", 69),
                       ("set_n_per_snp", 109), ("set_n_per_snp", 69)]
    del log[:]
    VIPRS(_loader(log), merge_chromosomes=True)
    assert [e[0] for e in log[:2]] == ["load", "load"]
    assert log[2:] == [("plan", "LDPlan", True, "float32", 5101, 178), ("state", 178), ("upload", "std_beta", 178),
                       ("set_n_per_snp", 178), ("set_snp_weights", 178)]


def test_viprs_lambda_min_policy(log):
    """None: 0; a number: itself; 'infer': the LAST chromosome's value, a NotImplementedError re-raised with the
    chromosome and the remedy."""
    from viprs_amd.model import VIPRS
    gdl = _loader(log)
    gdl.ld[1]._lambda_min, gdl.ld[2]._lambda_min = 0.125, 0.5
    kw = dict(e_step_fn=_no_device_fn)
    assert VIPRS(gdl, **kw).lambda_min == 0.0
    assert VIPRS(gdl, lambda_min=0.03, **kw).lambda_min == 0.03
    assert VIPRS(gdl, lambda_min="infer", **kw).lambda_min == 0.5
    gdl.ld[2].set_extremal(-0.1, 30.0)                       # (extremes without a chosen formula: get_lambda_min refuses)
    with pytest.raises(NotImplementedError, match=r"lambda_min='infer', chromosome 2: .*Remedy: VIPRS\(\.\.\., lambda_min="):
        VIPRS(gdl, lambda_min="infer", **kw)
    with pytest.raises(RuntimeError, match="lambda_min='compute' needs a HIP device"):
        VIPRS(gdl, lambda_min="compute", **kw)


def test_viprs_e_step_fn_mirrors_the_upper_store_on_the_host(log):
    from viprs_amd.model import VIPRS
    v = VIPRS(_loader(log, "upper"), low_memory=False, e_step_fn=_no_device_fn)
    assert v._expanded is False and not v._merged and not v._resident and not v._plans and not _of(log, "plan")
    assert [v.ld_data[c].shape[0] for c in (1, 2)] == [NNZ["symmetric"][1], NNZ["symmetric"][2]]


# ---- the seven models on one merged plan -------------------------------------------------------------------------------
# class name, the hook that puts it on the host path, further arguments, the error without a HIP device (literal: copied from
# the constructors before they shared `MergedPlanModel._load`), `_ld` kept beside a plan, has `_n_per_snp`
def _hooks():
    from viprs_amd.stats import clump, enet, gibbs, susie
    return dict(clump=clump.clump_host, enet=enet.enet_sweep_host, gibbs=gibbs.gibbs_sweep_host, susie=susie.susie_host)


MERGED_MODELS = [
    ("ClumpThreshold", dict(clump_fn="clump"), {},
     "ClumpThreshold needs a HIP device (viprs_amd.stats.clump.clump runs on the host)", False, False),
    ("LDPredInf", dict(solve_fn=_no_device_fn), dict(h2=0.3),
     "LDPredInf needs a HIP device: the solve has no CPU fallback", False, False),
    ("Lassosum", dict(sweep_fn="enet"), {},
     "Lassosum needs a HIP device (viprs_amd.stats.enet.enet_sweep_host is the sweep on the host: pass it as sweep_fn)",
     False, False),
    ("LDpred2", dict(sweep_fn="gibbs"), dict(h2_init=0.3),
     "LDpred2 needs a HIP device (viprs_amd.stats.gibbs.gibbs_sweep_host is the sweep on the host: pass it as sweep_fn)",
     False, True),
    ("PRSCS", dict(sweep_fn="gibbs"), {},
     "PRSCS needs a HIP device (viprs_amd.stats.gibbs.gibbs_sweep_host is the sweep on the host: pass it as sweep_fn)",
     False, True),
    ("SBayesR", dict(backend="host"), dict(h2_init=0.3),
     "SBayesR needs a HIP device (backend='host' runs viprs_amd.stats.bayesr on the CPU)", False, True),
    ("SuSiE", dict(fit_fn="susie"), {},
     "SuSiE needs a HIP device: pass fit_fn=viprs_amd.stats.susie.susie_host for a host fit", True, False),
]
MERGED_CHROMS = {1: [130, 64], 2: [200, 1]}                 # the loader of the model tests: 194 + 201 = 395 SNPs
MERGED_NNZ = {True: 8385 + 2016 + 19900 + 0, False: 130 ** 2 + 64 ** 2 + 200 ** 2 + 1}     # by `low_memory`


def _merged_model(name, low_memory=True, hook=None, gdl=None, **kw):
    import viprs_amd.model as models
    if gdl is None:
        gdl = ArrayDataLoader.synthetic(MERGED_CHROMS, ld_dtype=np.int8, n=5e4, kind="longrange", h2=0.5)
    hook = {k: _hooks().get(v, v) if isinstance(v, str) else v for k, v in (hook or {}).items()}     # ("host" stays "host")
    return getattr(models, name)(gdl, low_memory=low_memory, dequantize_on_the_fly=True, **hook, **kw)


# ---- the mixed loader: chromosome 1 stored in float32, chromosome 2 in int8, dequantize_on_the_fly=True ----------------
def test_mixed_stored_dtypes(log):
    """`VIPRS` and the seven models on a merged plan (`LDPredInf` with ``h2=0.3`` and `solve_fn` among them) thread
    `dequantize_on_the_fly` through the chromosomes in sorted order: the float-stored first chromosome turns it off for the
    int8 one after it.  `ld_scores` decides per matrix."""
    from viprs_amd.model import VIPRS
    from viprs_amd.stats.ldsc import ld_scores, ld_scores_host
    mixed = {1: "float32", 2: "int8"}
    for make in [lambda g: VIPRS(g, dequantize_on_the_fly=True, e_step_fn=_no_device_fn)] + [
            lambda g, r=r: _merged_model(r[0], hook=r[1], gdl=g, **r[2]) for r in MERGED_MODELS]:
        del log[:]
        model = make(_loader(log, stored=mixed))
        assert log == [("load", 1, False, "float32"), ("load", 2, False, "float32")]
        assert model.dequantize_on_the_fly is False and model.dequantize_scale == 1.0
    del log[:]
    seen = []

    def score_fn(lb, ip, data, upper, A, corr, dq):
        seen.append((data.dtype.name, upper, dq))
        return ld_scores_host(lb, ip, data, upper, A, corr, dq)

    ld_scores(_loader(log, stored=mixed), corrected=False, dequantize_on_the_fly=True, score_fn=score_fn)
    assert log == [("load", 1, False, "float32"), ("load", 2, False, "int8")]
    assert seen == [("float32", True, 1.0), ("int8", True, 1.0 / 127)]


# ---- LDPredInf ---------------------------------------------------------------------------------------------------------
# low_memory, forms, stored, dequantize_on_the_fly | loads of one chromosome, dtype asked, plan
LDPRED_ROWS = [
    (True, "both", "int8", True, ([False], "int8", ("plan", "LDPlan", True, "int8", 5101, 178))),
    (True, "upper", "int8", False, ([False], "float32", ("plan", "LDPlan", True, "float32", 5101, 178))),
    (False, "both", "float32", True, ([True], "float32", ("plan", "LDPlan", False, "float32", 10380, 178))),
    (False, "upper", "int8", True, None),                    # never expands: the matrix's ValueError
]


@pytest.mark.parametrize("row", LDPRED_ROWS, ids=_ids(LDPRED_ROWS))
@pytest.mark.parametrize("host", [True, False], ids=["solve_fn", "device"])
def test_ldpredinf_constructor_loads_and_plans(log, row, host):
    from viprs_amd.model.LDPredInf import LDPredInf
    low_memory, forms, stored, deq, want = row
    kw = dict(h2=0.3, low_memory=low_memory, dequantize_on_the_fly=deq, solve_fn=_no_device_fn if host else None)
    if want is None:
        with pytest.raises(ValueError, match="return_symmetric=True was not provided"):
            LDPredInf(_loader(log, forms, stored), **kw)
        assert log == [("load", 1, True, "int8")]
        return
    loads, load_dtype, plan = want
    model = LDPredInf(_loader(log, forms, stored), **kw)
    assert _of(log, "load") == [("load", c, rs, load_dtype) for c in (1, 2) for rs in loads]
    assert _of(log, "plan") == ([] if host else [plan])
    assert model.dequantize_on_the_fly is (deq and stored == "int8")
    assert model.dequantize_scale == (1.0 / 127 if deq and stored == "int8" else 1.0)
    if host:
        lb, ip, data = model._ld
        assert (lb.dtype, data.dtype.name, data.shape[0], lb.shape[0]) == (np.int32,) + plan[3:]


# ---- the seven models on one merged plan: the constructors --------------------------------------------------------------
@pytest.mark.parametrize("low_memory", [True, False], ids=["upper", "symmetric"])
@pytest.mark.parametrize("row", MERGED_MODELS, ids=[r[0] for r in MERGED_MODELS])
def test_merged_plan_models_load_once_and_open_one_plan(log, monkeypatch, row, low_memory):
    """Each of the seven constructors, on its host path and on a recorded plan: one plan over the merged arrays of both
    chromosomes in the form `low_memory` implies; `_ld`, `device`, `_seg`, `std_beta` (`SuSiE`: `z`) and `_n_per_snp`; and
    without a HIP device its own RuntimeError before any plan."""
    name, hook, kw, no_device, keeps_ld, has_n = row
    host = _merged_model(name, low_memory, hook, **kw)
    assert not _of(log, "plan") and host._plan is None and not hasattr(host, "device")
    lb, ip, data = host._ld
    assert (lb.dtype, lb.shape, ip.shape, data.dtype, data.shape) == (np.int32, (395,), (396,), np.int8, (MERGED_NNZ[low_memory],))
    dev = _merged_model(name, low_memory, **kw)
    assert _of(log, "plan") == [("plan", "LDPlan", low_memory, "int8", MERGED_NNZ[low_memory], 395)]
    assert dev.device == 0 and dev._plan.m == 395 and dev._plan.low_memory is low_memory
    assert np.array_equal(dev._plan.indptr, ip) and np.array_equal(dev._plan.data, data)      # (the merged arrays)
    if keeps_ld:
        assert dev._ld[1] is dev._plan.indptr and dev._ld[2] is dev._plan.data
    else:
        assert getattr(dev, "_ld", None) is None
    for model in (host, dev):
        assert model._seg == {1: (0, 194), 2: (194, 395)} and model.shapes == {1: 194, 2: 201} and model.m == 395
        assert model.low_memory is low_memory and model.dequantize_on_the_fly is True and model.dequantize_scale == 1.0 / 127
        assert model.float_precision == "float32" and model._T == np.float32
        per_snp = model.z if name == "SuSiE" else model.std_beta
        assert hasattr(model, "std_beta") is (name != "SuSiE") and hasattr(model, "_sqrt_n") is (name == "SuSiE")
        assert {c: (a.shape, a.dtype) for c, a in per_snp.items()} == {
            c: ((n,), np.dtype(np.float64 if name == "SuSiE" else np.float32)) for c, n in ((1, 194), (2, 201))}
        assert hasattr(model, "_n_per_snp") is has_n
        if has_n:
            assert model._n_per_snp.shape == (395,) and model._n_per_snp.dtype == np.float64
    for c in (1, 2):
        assert np.array_equal(host.z[c] if name == "SuSiE" else host.std_beta[c], dev.z[c] if name == "SuSiE" else dev.std_beta[c])
    del log[:]
    monkeypatch.setattr(_lib, "device_count", lambda: 0)
    with pytest.raises(RuntimeError) as e:
        _merged_model(name, low_memory, **kw)
    assert str(e.value) == no_device and not _of(log, "plan")


def test_split_and_concat_are_inverses():
    model = _merged_model("ClumpThreshold", True, dict(clump_fn="clump"))
    rng = np.random.default_rng(0)
    d = {1: rng.normal(size=194), 2: rng.normal(size=201)}
    D = {1: rng.normal(size=(194, 3)).astype(np.float32), 2: rng.normal(size=(201, 3)).astype(np.float32)}
    for per_chromosome in (d, D):
        whole = model._concat(per_chromosome)
        assert whole.shape[0] == 395 and whole.dtype == per_chromosome[1].dtype
        back = model._split(whole)
        assert list(back) == [1, 2] and all(np.array_equal(back[c], per_chromosome[c]) for c in (1, 2))
        assert not any(np.shares_memory(back[c], whole) for c in (1, 2))


# ---- ld_scores ---------------------------------------------------------------------------------------------------------
# low_memory, forms | loads of one chromosome, the form the scores are computed in (upper: True)
SCORE_ROWS = [
    (True, "both", ([False], True)),
    (False, "both", ([True], False)),
    (False, "upper", ([True, False], True)),                 # an upper-only store is scored in the upper form
]


@pytest.mark.parametrize("row", SCORE_ROWS, ids=_ids(SCORE_ROWS))
@pytest.mark.parametrize("host", [True, False], ids=["score_fn", "device"])
def test_ld_scores_loads_and_plans(log, row, host):
    from viprs_amd.stats.ldsc import ld_scores, ld_scores_host
    low_memory, forms, (loads, upper) = row
    seen = []

    def score_fn(lb, ip, data, up, A, corr, dq):
        seen.append((lb.dtype, data.dtype.name, data.shape[0], up, dq))
        return ld_scores_host(lb, ip, data, up, A, corr, dq)

    out = ld_scores(_loader(log, forms), corrected=False, low_memory=low_memory, dequantize_on_the_fly=True,
                    score_fn=score_fn if host else None)
    form = "upper" if upper else "symmetric"
    assert _of(log, "load") == [("load", c, rs, "int8") for c in (1, 2) for rs in loads]
    assert sorted(out) == [1, 2] and [out[c].shape for c in (1, 2)] == [(109,), (69,)]
    if host:
        assert seen == [(np.int32, "int8", NNZ[form][c], upper, 1.0 / 127) for c in (1, 2)] and not _of(log, "plan")
    else:                                                    # one plan per matrix, closed before the next is loaded
        assert log == [e for c in (1, 2) for e in
                       [("load", c, rs, "int8") for rs in loads]
                       + [("plan", "LDPlan", upper, "int8", NNZ[form][c], M[c]), ("ld_scores", 1.0 / 127, "float32"),
                          ("close", M[c])]]


# ---- ld_spectrum -------------------------------------------------------------------------------------------------------
# low_memory, forms, stored, dequantize_on_the_fly | loads of one chromosome, dtype asked, constructor, plan low_memory,
# form, dq_scale
SPECTRUM_ROWS = [
    (True, "both", "int8", True, ([False], "int8", "LDPlan", True, "upper", 1.0 / 127)),
    (False, "both", "int8", False, ([True], "float32", "LDPlan", False, "symmetric", 1.0)),
    (False, "upper", "int8", True, ([True, False], "int8", "from_upper", False, "upper", 1.0 / 127)),   # mirrored on the device
    (False, "upper", "float32", True, ([True, False], "float32", "from_upper", False, "upper", 1.0)),
]


@pytest.mark.parametrize("row", SPECTRUM_ROWS, ids=_ids(SPECTRUM_ROWS))
def test_ld_spectrum_loads_and_plans(log, row):
    from viprs_amd.stats.spectrum import ld_spectrum
    low_memory, forms, stored, deq, (loads, load_dtype, ctor, plan_low_memory, form, dq) = row
    out = ld_spectrum(_loader(log, forms, stored), low_memory=low_memory, dequantize_on_the_fly=deq)
    assert log == [e for c in (1, 2) for e in
                   [("load", c, rs, load_dtype) for rs in loads]
                   + [("plan", ctor, plan_low_memory, load_dtype, NNZ[form][c], M[c]),
                      ("extremal_eigenvalues", dq, "float32"), ("close", M[c])]]
    assert {c: (s["min"], s["max"]) for c, s in out.items()} == {1: (0.25, 3.0), 2: (0.25, 3.0)}


# ---- _pseudo_r2_external -----------------------------------------------------------------------------------------------
def test_pseudo_r2_external_closes_its_own_plans_only(log):
    from viprs_amd.model.VIPRS import _pseudo_r2_external
    up = syn.make_ld(SIZES[1], low_memory=True, ld_dtype=np.int8, seed=41)
    handed_in = plan_mod.LDPlan(np.arange(1, 70, dtype=np.int32), np.zeros(70, np.int64), np.zeros(0, np.float32), True)
    del log[:]
    rng = np.random.default_rng(3)
    beta = {1: rng.normal(size=109), 2: rng.normal(size=69)}
    r2 = _pseudo_r2_external({1: (up.ld_left_bound.astype(np.int64), up.ld_indptr, up.ld_data, 1), 2: handed_in},
                             {c: b + 0.1 for c, b in beta.items()}, beta)
    assert np.isfinite(r2)
    assert log == [("plan", "LDPlan", True, "int8", 2953, 109), ("dot", 109, 1.0 / 127), ("dot", 69, 1.0), ("close", 109)]
    assert not handed_in.closed
    with pytest.raises(ValueError, match="validation_ld has no LD for chromosome 2"):
        _pseudo_r2_external({1: handed_in}, beta, beta)


# ---- the two-rank deal, without processes ------------------------------------------------------------------------------
class _TwoRanks:
    world_size, device_side = 2, False

    def __init__(self, rank):
        self.rank = rank


@pytest.mark.parametrize("cls", [RecordingLD, RecordingRowStore], ids=["arrays", "row-store"])
def test_two_rank_deal(cls):
    from viprs_amd.model import VIPRS
    logs, models = [[], []], []
    for r in range(2):
        gdl = _loader(logs[r], "upper", "int8", cls=cls)
        models.append(VIPRS(gdl, comm=_TwoRanks(r), dequantize_on_the_fly=True, e_step_fn=_no_device_fn))
    a, b = models
    for c in (1, 2):
        starts = np.concatenate([[0], np.cumsum(SIZES[c])])
        for v in (a, b):
            np.testing.assert_array_equal(v._block_owner[c][0], starts)
        np.testing.assert_array_equal(a._block_owner[c][1], b._block_owner[c][1])
        mine = [list(v._shard[c].blocks) for v in (a, b)]
        assert sorted(mine[0] + mine[1]) == list(range(len(SIZES[c]))) and not set(mine[0]) & set(mine[1])
        for r, v in enumerate((a, b)):
            assert mine[r] == [i for i, o in enumerate(v._block_owner[c][1]) if o == r]
            want = [("load_rows", c, int(starts[i]), int(starts[i + 1])) for i in mine[r]]
            if cls is RecordingRowStore:                     # only the index was read, then the rows of this rank's blocks
                assert [e for e in logs[r] if e[1] == c] == want
            else:
                assert [e for e in logs[r] if e[1] == c] == [("load", c, False, "int8")]
            if mine[r]:
                assert v.shapes[c] == sum(SIZES[c][i] for i in mine[r]) == v.std_beta[c].shape[0] == v.n_per_snp[c].shape[0]
                assert v.ld_data[c].dtype == np.int8
                assert v.ld_data[c].shape[0] == sum(SIZES[c][i] * (SIZES[c][i] - 1) // 2 for i in mine[r])
            else:
                assert c not in v.shapes and c not in v.ld_data
    assert a._all_shapes == b._all_shapes == M
    # the element size of the deal is the first chromosome's load dtype; both ranks hold something
    assert all(v.chromosomes for v in (a, b))


def test_rank_without_blocks_builds_the_empty_merged_plan(log):
    """More ranks than LD blocks: the last rank holds nothing and still opens one (empty) plan, whose `data` has the stored
    dtype when dequantising on the fly, else the model's."""
    from viprs_amd.model import VIPRS

    class Comm:
        world_size, device_side, rank = 7, False, 6

    for deq, dtype in ((True, "int8"), (False, "float32")):
        del log[:]
        v = VIPRS(_loader(log, "both", "int8"), comm=Comm(), dequantize_on_the_fly=deq)
        assert v.chromosomes == [] and v._merged and v._seg == {}
        assert _of(log, "plan") == [("plan", "LDPlan", True, dtype, 0, 0)]
        assert log[-4:] == [("state", 0), ("upload", "std_beta", 0), ("set_n_per_snp", 0), ("set_snp_weights", 0)]


# ---- one LD-score estimate behind the three entry points ---------------------------------------------------------------
def test_the_three_ldsc_estimates_agree():
    from viprs_amd.model import VIPRS
    from viprs_amd.model.LDPredInf import LDPredInf
    from viprs_amd.stats.ldsc import chisq_statistic, ld_correction, ld_scores_host, ldsc_estimate, simple_ldsc
    gdl = _loader([], "both", "float32", sample_size=400, n=2e4, h2=0.5, pi=0.3)
    chisq, scores, n = [], [], []
    for c in (1, 2):
        lop = gdl.ld[c].load(return_symmetric=False, dtype="float32")
        chisq.append(chisq_statistic(gdl.sumstats_table[c]))
        scores.append(ld_scores_host(lop.leftmost_idx, lop.ld_indptr, lop.ld_data, True, None,
                                     ld_correction(gdl.ld[c], M[c]), 1.0))
        n.append(np.asarray(gdl.sumstats_table[c].n_per_snp, dtype=np.float64).ravel())
    want = ldsc_estimate(np.concatenate(chisq), np.concatenate(scores), np.concatenate(n))
    assert 0.0 < want <= 1.0
    assert simple_ldsc(gdl, score_fn=ld_scores_host) == want
    assert VIPRS(gdl, h2_init="ldsc", e_step_fn=_no_device_fn)._ldsc_h2()["*"] == want
    assert LDPredInf(gdl, h2=None, solve_fn=_no_device_fn, score_fn=ld_scores_host).h2 == want
