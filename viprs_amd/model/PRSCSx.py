"""``PRSCSx`` -- PRS-CSx (Ruan et al. 2022): one `PRSCS` chain per population, each on that population's own LD panel and
summary statistics, coupled through ONE local scale ``psi_j`` per SNP, so that a small GWAS borrows the sparsity pattern of a
large one.

Population k has ``beta_kj ~ N(0, sigma2_k / n_kj psi_j)`` with the shared ``psi_j ~ Gamma(1, delta_j)``, ``delta_j ~
Gamma(1/2, phi)``.  Given the scales every population is a PRS-CS chain: its own merged device plan, its own grid state with
one column per entry of `phi`, the LDpred2 Gibbs sweep with an inclusion probability of exactly 1 (`DeviceState.gibbs_sweep`,
untouched).  Between two rounds of sweeps `DeviceCoupling.update` makes ONE pass over the union of the SNP sets: it gathers the
effects of the populations that carry a SNP, draws ``delta_j`` and ``psi_j ~ GIG(1 - K_j / 2, 2 delta_j, sum_k n_kj beta_kj^2 /
sigma2_k)`` -- the closed form of PRS-CS for one carrying population, Devroye's rejection sampler on the device for two or more
-- and rewrites the three sweep inputs of every population (`viprs_amd.stats.csx` is the host definition).  Per chain the host
draws ``sigma2_k`` for every population (its own ``nbar``, ``m_k`` and sums) and, for auto chains, one shared ``phi`` from the
union's ``sum delta``, populations in ascending order from the chain's generator ``default_rng([seed, g])``.

SNPs are matched on the ``SNP`` column of each loader's ``snp_table``; the union is ordered by chromosome and, within one, by
first appearance (populations in the given order).  Where ``A1`` / ``A2`` are given and exchanged relative to the first
population that carries the SNP, that population's ``beta_hat`` is negated for the fit and its result negated back; any other
disagreement raises ``ValueError``.  A chain that diverges in any population (`divergence_rule`) is zeroed and dropped in all.

Results: ``post_mean_beta[pop]`` (each population's own SNP order and allele coding, laid out as `PRSCS`'s), ``sigma2_est[pop]``,
``phi_est``, ``grid_table``, ``predict(pop=...)``, ``to_table(pop=...)``, ``n_capped_total`` (draws of the rejection sampler that
ended at its attempt cap: expected 0) and `meta_beta`.  `meta_beta` averages the POSTERIOR MEANS of the populations with weights
``nbar_k / sigma2_est_k``; PRS-CSx's ``--meta`` averages the draws of every iteration with inverse-variance weights instead.

What differs from the PRS-CSx program:
  * an effect is drawn given all the others, SNP after SNP (single-site Gibbs), where PRS-CSx draws an LD block jointly;
  * ONE ``sigma2_k`` per population and ONE ``phi`` per chain over the whole genome (genome-wide scalars), where PRS-CSx runs
    chromosome by chromosome;
  * the sample size ``n_kj`` of every SNP where PRS-CSx takes one ``n_k``;
  * the posterior means average the conditional means of the kept iterations (Rao-Blackwellised), not the draws;
  * only ``a = 1, b = 1/2``.
Not built: other ``a``, ``b``; joint-block draws; float64 states; several ranks; a fast-math variant; populations on different
devices.  The reference has no such class.  (``sweep_fn`` runs the chains on the host with
`viprs_amd.stats.gibbs.gibbs_sweep_host`; ``draws_fn`` replaces the Gibbs draws, ``coupled_fn`` the coupled update; without
``sweep_fn`` and without a GPU the constructor raises.)
"""
import numpy as np

from ._chain_engines import divergence_rule, tail_mean
from .ClumpThreshold import ClumpThreshold
from .PRSCS import PRSCS


class _Population(ClumpThreshold):
    """What the chain engines, `predict` and `to_table` need of one population: its loader on one merged plan."""

    def __init__(self, owner, index, gdl, low_memory, dequantize_on_the_fly, device, comm):
        self._set_loader(gdl, comm)
        self.seed = (owner.seed + (index << 40)) & (2 ** 64 - 1)       # a Philox key of its own for the Gibbs draws
        self._sweep_fn, self._draws_fn, self._variates_fn = owner._sweep_fn, owner._draws_fn, None
        self._keep_draws_log, self.draws_log = owner._keep_draws_log, []
        self._load("float32", low_memory, dequantize_on_the_fly, device, owner._sweep_fn is not None,
                   "PRSCSx needs a HIP device (viprs_amd.stats.gibbs.gibbs_sweep_host is the sweep on the host: "
                   "pass it as sweep_fn)",
                   n_per_snp=True)
        self.n_models = owner.n_models
        self.post_mean_beta = self.grid_table = self.validation_result = self.best_model_idx = None


def match_snps(tables, shapes):
    """The union of the SNP sets of the populations.  `tables`: per population ``{chromosome: {"SNP", ["A1", "A2"]}}``
    (None allowed for a single population: its own order); `shapes`: per population ``{chromosome: m_c}``.  Returns
    ``(row_of, flip, union)``: ``(P, m_union)`` int64 rows in each population's merged SNP order or -1, per population the
    boolean ``(m_k,)`` mask of SNPs whose alleles are exchanged relative to the first population carrying them, and the
    ``(chromosome, SNP)`` pairs of the union -- chromosomes sorted, within one by first appearance."""
    P = len(shapes)
    chroms = sorted(set().union(*[set(s) for s in shapes]))
    offs = []
    for s in shapes:
        o, off = 0, {}
        for c in sorted(s):
            off[c] = o
            o += int(s[c])
        offs.append(off)
    if P == 1 and not tables[0]:
        m = sum(int(v) for v in shapes[0].values())
        union = [(c, j) for c in sorted(shapes[0]) for j in range(int(shapes[0][c]))]
        return np.arange(m, dtype=np.int64)[None, :], [np.zeros(m, dtype=bool)], union
    for k, t in enumerate(tables):
        if not t or any(c not in t or "SNP" not in t[c] for c in shapes[k]):
            raise ValueError(f"PRSCSx: population {k} has no snp_table with a SNP column for every chromosome")
    flip = [np.zeros(sum(int(v) for v in s.values()), dtype=bool) for s in shapes]
    cols, union = [[] for _ in range(P)], []
    for c in chroms:
        index, first = {}, []                              # SNP -> position in this chromosome's union; (population, row)
        for k in range(P):
            if c not in shapes[k]:
                continue
            names = [str(s) for s in np.asarray(tables[k][c]["SNP"])]
            if len(names) != int(shapes[k][c]):
                raise ValueError(f"PRSCSx: snp_table of population {k}, chromosome {c}: {len(names)} SNPs for {shapes[k][c]}")
            if len(set(names)) != len(names):
                raise ValueError(f"PRSCSx: population {k}, chromosome {c}: a SNP is listed twice")
            alleles = "A1" in tables[k][c] and "A2" in tables[k][c]
            for j, s in enumerate(names):
                if s not in index:
                    index[s] = len(first)
                    first.append((k, j))
                    continue
                k0, j0 = first[index[s]]
                t0 = tables[k0][c]
                if alleles and "A1" in t0 and "A2" in t0:
                    mine = (str(tables[k][c]["A1"][j]), str(tables[k][c]["A2"][j]))
                    ref = (str(t0["A1"][j0]), str(t0["A2"][j0]))
                    if mine == ref[::-1] and mine != ref:
                        flip[k][offs[k][c] + j] = True
                    elif mine != ref:
                        raise ValueError(f"PRSCSx: alleles of SNP {s} disagree between populations {k0} and {k}: "
                                         f"{ref[0]}/{ref[1]} and {mine[0]}/{mine[1]}")
        for k in range(P):
            col = np.full(len(first), -1, dtype=np.int64)
            if c in shapes[k]:
                names = [str(s) for s in np.asarray(tables[k][c]["SNP"])]
                col[[index[s] for s in names]] = offs[k][c] + np.arange(len(names))
            cols[k].append(col)
        inv = {v: s for s, v in index.items()}
        union += [(c, inv[i]) for i in range(len(first))]
    return np.stack([np.concatenate(c) if c else np.zeros(0, dtype=np.int64) for c in cols]), flip, union


class PRSCSx:

    def __init__(self, gdls, phi=None, a=1.0, b=0.5, n_iter=1000, n_burnin=500, thin=5, seed=0, psi_max=1.0,
                 float_precision="float32", low_memory=True, dequantize_on_the_fly=False, device=None, sweep_fn=None,
                 draws_fn=None, coupled_fn=None, keep_draws_log=False, comm=None):
        """:param gdls: an ordered ``{population: loader}``: per population the summary statistics, the LD matrices and a
            ``snp_table`` with a ``SNP`` column (``A1`` / ``A2`` optional) per chromosome.
        :param phi: the shared global scale: None (learnt), a number, or a sequence of numbers and None -- one chain per
            entry, all in lock step, a column of every population's state.
        :param a, b: the exponents of the gamma-gamma prior; only 1 and 1/2.
        :param n_iter, n_burnin, thin: iterations in all, those dropped first, and the stride of the kept ones.
        :param seed: of the device draws (Philox key; population k sweeps with ``seed + k 2^40``) and of the host `Generator`
            of each chain.
        :param psi_max: the upper bound of the local scales (PRS-CSx: 1).
        :param sweep_fn: test hook -- a callable with `viprs_amd.stats.gibbs.gibbs_sweep_host`'s signature: the chains run on
            the host.
        :param draws_fn: host path -- ``(seed, draw_index, half_var_tau, cols) -> (U, noise)`` in place of
            `viprs_amd.stats.gibbs.gibbs_draws_host`; with a dict ``{population: callable}`` each population has its own.
        :param coupled_fn: host path -- ``(draw_index, cols) -> (psi, delta)``, float32 ``(m_union, G)`` each, in place of the
            draws of the coupled update (tests feed the device's logged values): the three inputs are rewritten from them.
        :param keep_draws_log: `draws_log[pop][k]` keeps the ``(U, noise)`` of sweep k of a population (device path) and
            `coupled_log[k]` the shared ``(psi, delta)`` after update k.
        """
        if not isinstance(gdls, dict) or not gdls:
            raise ValueError("gdls: a non-empty ordered {population: loader}")
        if len(gdls) > 8:
            raise ValueError("gdls: at most 8 populations")
        if float(a) != 1.0 or float(b) != 0.5:
            raise NotImplementedError("PRSCSx: only a = 1, b = 0.5 (the draws of delta and psi need them)")
        if np.dtype(float_precision) != np.float32:
            raise ValueError("PRSCSx: float_precision must be 'float32' (the Gibbs sweep has no float64 form)")
        self.a, self.b = 1.0, 0.5
        self.n_iter, self.n_burnin, self.thin = int(n_iter), int(n_burnin), int(thin)
        if not (0 <= self.n_burnin < self.n_iter) or self.thin < 1 or (self.n_iter - self.n_burnin) // self.thin < 1:
            raise ValueError("0 <= n_burnin < n_iter, thin >= 1 and at least one kept iteration")
        self.psi_max = float(psi_max)
        if not (2.0 ** -40 < self.psi_max < np.inf):
            raise ValueError("psi_max must lie in (2^-40, inf)")
        entries = list(phi) if isinstance(phi, (list, tuple, np.ndarray)) else [phi]
        if not entries:
            raise ValueError("phi: at least one entry")
        self.phi = [None if v is None else float(v) for v in entries]
        if any(v is not None and not (np.isfinite(v) and v > 0) for v in self.phi):
            raise ValueError("phi: positive numbers or None")
        self.n_models = len(self.phi)
        self.seed = int(seed)
        self._sweep_fn, self._draws_fn, self._coupled_fn = sweep_fn, None, coupled_fn
        self._keep_draws_log = bool(keep_draws_log)
        self.populations = list(gdls)
        self._pops = []
        for k, (name, gdl) in enumerate(gdls.items()):
            pop = _Population(self, k, gdl, low_memory, dequantize_on_the_fly, device, comm)
            pop._draws_fn = draws_fn.get(name) if isinstance(draws_fn, dict) else draws_fn
            self._pops.append(pop)
        self.device = getattr(self._pops[0], "device", None)
        self.row_of, self._flip, self.union_snps = match_snps(
            [getattr(g, "snp_table", None) for g in gdls.values()], [p.shapes for p in self._pops])
        self.m_union = int(self.row_of.shape[1])
        for pop, f in zip(self._pops, self._flip):              # exchanged alleles: the fit sees the first population's coding
            for c, (s, e) in pop._seg.items():
                pop.std_beta[c] = np.where(f[s:e], -pop.std_beta[c], pop.std_beta[c]).astype(np.float32)
        self.draws_log, self.coupled_log = {name: [] for name in self.populations}, []
        self.post_mean_beta = self.grid_table = None
        self.phi_est = self.sigma2_est = self.phi_history = self.sigma2_history = None
        self.n_capped_total = 0

    # -- the coupled update on the two paths: the per-population engines are `PRSCS`'s ---------------------------------------
    class _DeviceCoupled:
        def __init__(self, model, engines):
            from ..plan import DeviceCoupling
            self.model = model
            self.coupling = DeviceCoupling([e.st for e in engines], model.row_of)

        def prepare(self, params):
            self.coupling.update(params, self.model.psi_max, prepare_only=True, sync=False)

        def sums(self, active):
            return self.coupling.sums(active)

        def update(self, params, draw_index):
            self.coupling.update(params, self.model.psi_max, seed=self.model.seed, draw_index=draw_index, sync=False)
            self.model.n_capped_total += self.coupling.last()[1]
            if self.model._keep_draws_log:
                self.model.coupled_log.append((self.coupling.download("psi"), self.coupling.download("delta")))

        def close(self):
            self.coupling.close()

    class _HostCoupled:
        def __init__(self, model, engines):
            self.model, self.engines = model, engines
            G = model.n_models
            self.psi = np.ones((model.m_union, G), dtype=np.float32, order="F")
            self.delta = np.zeros((model.m_union, G), dtype=np.float32, order="F")

        def _update(self, params, draw_index, prepare_only):
            from ..stats.csx import csx_update_host
            E = self.engines
            _, capped = csx_update_host(self.model.row_of, [p._n_per_snp for p in self.model._pops], [e._eta for e in E],
                                        self.psi, self.delta, [(e.psi, e.delta, e.mm, e.hvt, e.ulog) for e in E], params,
                                        self.model.psi_max, None, self.model.seed, draw_index, prepare_only)
            self.model.n_capped_total += capped

        def prepare(self, params):
            self._update(params, 0, True)

        def sums(self, active):
            from ..stats.csx import csx_sums_host
            return csx_sums_host(self.psi, self.delta, cols=active)

        def update(self, params, draw_index):
            if self.model._coupled_fn is not None:
                cols = np.asarray(params)[:, 0].astype(np.int64)
                psi, delta = self.model._coupled_fn(draw_index, cols)
                self.psi[:, cols], self.delta[:, cols] = np.asarray(psi)[:, cols], np.asarray(delta)[:, cols]
                self._update(params, draw_index, True)
            else:
                self._update(params, draw_index, False)
            if self.model._keep_draws_log:
                self.model.coupled_log.append((self.psi.copy(order="F"), self.delta.copy(order="F")))

        def close(self):
            pass

    def fit(self):
        """The chains in lock step: `n_iter` iterations of (one sweep and its sums per population, the scalar draws, one coupled
        update); after `n_burnin` every `thin`-th iteration adds its conditional means to the posterior means."""
        import pandas as pd
        from ..stats.cs import cs_phi_draw, cs_sigma2_draw
        pops, P, G = self._pops, len(self._pops), self.n_models
        host = self._sweep_fn is not None
        rules = [divergence_rule(p) for p in pops]
        nbar = [float(np.mean(p._n_per_snp)) for p in pops]
        auto = np.array([v is None for v in self.phi])
        phi = np.array([1.0 if v is None else v for v in self.phi], dtype=np.float64)
        sigma2 = np.ones((P, G), dtype=np.float64)
        # one generator per chain: a chain depends on its own entry of `phi` and on its position, not on the other entries
        rngs = [np.random.default_rng([self.seed, g]) for g in range(G)]
        diverged = np.zeros(G, dtype=bool)
        phi_hist, s2_hist = np.full((self.n_iter, G), np.nan), np.full((P, self.n_iter, G), np.nan)
        n_kept = 0
        self.n_capped_total = 0
        self.coupled_log = []
        for p in pops:
            p.draws_log = []
        engines, coupled = [], None
        rows = lambda cols: np.concatenate([np.asarray(cols, dtype=np.float64)[:, None], phi[cols][:, None], sigma2[:, cols].T],
                                           axis=1)
        try:
            for p, (beta_hat, _) in zip(pops, rules):
                engines.append((PRSCS._Host if host else PRSCS._Device)(p, beta_hat, G))
            coupled = (self._HostCoupled if host else self._DeviceCoupled)(self, engines)
            coupled.prepare(rows(np.arange(G)))
            for it in range(self.n_iter):
                active = np.flatnonzero(~diverged).astype(np.int32)
                if active.shape[0] == 0:
                    break
                sums = [e.sweep(active, it) for e in engines]
                shared = coupled.sums(active)
                still = []
                for i, g in enumerate(active):
                    if any(rules[k][1](sums[k][0][i][3]) for k in range(P)):
                        diverged[g] = True
                        for e in engines:
                            e.zero_column(int(g))
                        continue
                    still.append(int(g))
                    for k in range(P):
                        row, c = sums[k][0][i], sums[k][1][i]
                        quad = row[3] + row[2] + c[0]
                        sigma2[k, g] = cs_sigma2_draw(rngs[g], nbar[k], pops[k].m, row[1], quad, c[1])
                    if auto[g]:
                        phi[g] = cs_phi_draw(rngs[g], self.m_union, self.b, phi[g], shared[i][0])
                    phi_hist[it, g], s2_hist[:, it, g] = phi[g], sigma2[:, g]
                still = np.asarray(still, dtype=np.int32)
                if still.shape[0]:
                    coupled.update(rows(still), it)
                kept = it + 1 > self.n_burnin and (it + 1 - self.n_burnin) % self.thin == 0
                if kept:
                    n_kept += 1
                    if still.shape[0]:
                        for e in engines:
                            e.accumulate(still)
            means = [e.mean_sum() / float(max(n_kept, 1)) for e in engines]
        finally:
            if coupled is not None:
                coupled.close()
            for e in engines:
                e.close()
        self.phi_history, self.sigma2_history = phi_hist, dict(zip(self.populations, s2_hist))
        self.phi_est = tail_mean(phi_hist, self.n_burnin, diverged)
        self.sigma2_est = {name: tail_mean(s2_hist[k], self.n_burnin, diverged) for k, name in enumerate(self.populations)}
        table = dict(phi=[np.nan if v is None else v for v in self.phi], auto=auto, phi_est=self.phi_est)
        table.update({f"sigma2_est_{name}": self.sigma2_est[name] for name in self.populations})
        self.grid_table = pd.DataFrame(dict(table, diverged=diverged))
        self.post_mean_beta = {}
        for name, p, mean, f in zip(self.populations, pops, means, self._flip):
            mean[:, diverged] = 0.0
            beta = np.where(f[:, None], -mean, mean).astype(np.float32)     # back to the population's own allele coding
            p.post_mean_beta = p._split(beta[:, 0] if G == 1 else beta)
            p.best_model_idx = 0 if G == 1 else None
            p.grid_table = p.validation_result = self.grid_table.copy()
            self.post_mean_beta[name] = p.post_mean_beta
            self.draws_log[name] = p.draws_log
        return self

    def _pop(self, pop):
        if pop not in self.populations:
            raise KeyError(f"unknown population {pop!r}: one of {self.populations}")
        return self._pops[self.populations.index(pop)]

    def get_posterior_mean_beta(self, pop=None):
        return self.post_mean_beta if pop is None else self.post_mean_beta[pop]

    def predict(self, pop, test_gdl=None, **kw):
        """Polygenic scores from the posterior mean effects of population `pop` (`MergedPlanModel.predict`)."""
        assert self.post_mean_beta is not None, "The effects are not set. Call `.fit()` first."
        return self._pop(pop).predict(test_gdl, **kw)

    def to_table(self, pop, per_chromosome=False):
        """The effects of population `pop` as a pandas table (`ClumpThreshold.to_table`)."""
        return self._pop(pop).to_table(per_chromosome=per_chromosome)

    def meta_beta(self):
        """``(m_union,)`` or ``(m_union, G)`` float64 in the order of `union_snps` and the allele coding of the first population
        carrying each SNP: the mean of the populations' posterior means over the populations that carry the SNP, with weights
        ``nbar_k / sigma2_est_k`` (the precision of a standardised effect).  PRS-CSx's ``--meta`` averages per iteration."""
        assert self.post_mean_beta is not None, "The effects are not set. Call `.fit()` first."
        G = self.n_models
        num, den = np.zeros((self.m_union, G)), np.zeros((self.m_union, G))
        for k, (name, p) in enumerate(zip(self.populations, self._pops)):
            b = p._concat(p.post_mean_beta).astype(np.float64).reshape(p.m, G)
            b = np.where(self._flip[k][:, None], -b, b)
            w = float(np.mean(p._n_per_snp)) / np.asarray(self.sigma2_est[name], dtype=np.float64).reshape(1, G)
            u = np.flatnonzero(self.row_of[k] >= 0)
            num[u] += w * b[self.row_of[k, u]]
            den[u] += w
        with np.errstate(invalid="ignore"):
            out = np.nan_to_num(num / den)
        return out[:, 0] if G == 1 else out
