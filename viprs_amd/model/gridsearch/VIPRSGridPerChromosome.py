"""``VIPRSGridPerChromosome`` -- one ``VIPRSGrid`` PER CHROMOSOME, every (chromosome, grid point) pair fitted in lock step on
one device plan.

The reference's CLI fits one model per chromosome whatever ``--hyp-search`` is (bin/viprs_fit:232-238, fan-out
:1079-1086); with ``GS`` / ``BMA`` every chromosome fits its own ``VIPRSGrid`` (:373-390) over a grid rebuilt for that
chromosome -- the ``pi`` grid from its SNP count, the ``lambda_min`` grid from its LD (:450-466) -- and one grid point is
selected, or the points are averaged, per chromosome (:534-551).  Only the INDEPENDENT grid mode is built here
(``fit(pathwise=False)``, ``--grid-search-mode independent``): every pair starts from the standard initialisation.

On the device the chromosomes are SNP groups of ONE grid state (``viprs_state_set_groups``) and a pair is a
(group, column) pair of it.  An EM round is one ``viprs_state_prep_grid_groups`` for the active pairs, ONE sweep under the
pair mask (``viprs_state_set_group_columns``: column g of chromosome c is swept only while the pair iterates), one
``viprs_state_sums_grid_groups_*`` call and the vectorised M-step / ELBO / stopping rules of ``LockstepEM`` over the
C x G pairs.  A converged pair leaves the mask, a chromosome whose pairs have all converged leaves the sweep
(``viprs_plan_set_active_blocks``).  A pair's prep, sweep and sums are bit-identical to those of the same grid point in
``VIPRSGrid(loader_of_c, grid_c).fit(batched=True)``, so the lock-step fit reproduces, bit for bit, those fits run one
chromosome after the other.

With ``e_step_fn=oracle.cpp_e_step_grid`` (CPU tests) the same host logic runs per chromosome on NumPy state with that
chromosome's active list.

Results are keyed by chromosome, in ``VIPRSGrid``'s per-model layout: ``var_gamma / var_mu / q / pip / post_mean_beta /
post_var_beta [c]`` of shape ``(m_c, G)``; ``pi / tau_beta / sigma_epsilon / _sigma_g / model_elbos [c]`` of length G;
``optim_results[c]`` (G results); ``validation_result[c]`` (the chromosome's grid table + ``ELBO``, ``Converged``,
``Optimization_message``); ``history[c]["ELBO"][g]`` (the trajectory of pair (c, g)).

The PATHWISE mode (the CLI's default ``--grid-search-mode``: grid point i starts from what point i-1 left) is
``VIPRSGridPathwisePerChromosome``; both classes share the grid building, the result layout and the summaries
(``GridPerChromosomeMixin``).
"""
import copy

import numpy as np

from .._lockstep import LockstepEM, f64, run_rounds
from .._per_chromosome import PerChromosomeGroups
from ..VIPRS import VIPRS
from .VIPRSGrid import VIPRSGrid

_RES = np.finfo(np.float64).resolution


class GridPerChromosomeMixin:
    """What the per-chromosome grid searches share (mixed in front of the model classes): one grid per chromosome, the
    per-chromosome result layout of ``VIPRSGrid``, the summaries of one chromosome's models."""

    def _set_grids(self, gdl, grid):
        """``grid``: one ``HyperparameterGrid`` -- regenerated per chromosome as the CLI does (``pi`` from the chromosome's
        SNP count, ``lambda_min`` scaled by its LD's ``get_lambda_min``, for grids built from steps) -- or a
        ``{chromosome: HyperparameterGrid}`` dict.  Every chromosome must end up with the same number of grid points."""
        lds = gdl.get_ld_matrices()
        self.grids = {}
        for gi, c in enumerate(self.groups):
            if isinstance(grid, dict):
                self.grids[c] = grid[c]
                continue
            g = copy.deepcopy(grid)
            gen = getattr(grid, "_generated", {})
            if "pi" in gen:                              # bin/viprs_fit:450-455
                g.n_snps = int(self._m_group[gi])
                g.generate_pi_grid(**gen["pi"])
            if "lambda_min" in gen:                      # bin/viprs_fit:457-462
                # (the CLI asks for `get_lambda_min(aggregate="min")`: |min(smallest eigenvalue, 0)|, no min / max ratio)
                g.generate_lambda_min_grid(steps=gen["lambda_min"]["steps"],
                                           emp_lambda_min=lds[c].get_lambda_min(min_max_ratio=0.0))
            self.grids[c] = g
        self.grid_tables = {c: g.to_table() for c, g in self.grids.items()}
        sizes = {len(t) for t in self.grid_tables.values()}
        if len(sizes) != 1:
            raise ValueError(f"every chromosome needs the same number of grid points, got {sorted(sizes)}")
        self.n_models = sizes.pop()

    def _publish_chromosomes(self, rec):
        """The (m_c, G) state arrays (var_gamma / var_mu / q / eta_diff [c], already set) and ``rec[c]`` = dict(var_tau=(m_c, G),
        theta=[(pi, sigma_epsilon, tau_beta)] * G, sigma_g=(G,), elbo=(G,) in the state precision, results=[G]) in the
        layout ``VIPRSGrid`` publishes."""
        T = self._T
        # (m_c, G) arrays in the layouts VIPRSGrid publishes (C order; eta_diff F order): reductions over them give its bits
        for name in ("var_gamma", "var_mu", "q"):
            d = getattr(self, name)
            for c in d:
                d[c] = np.ascontiguousarray(d[c])
        self.eta_diff = {c: np.asfortranarray(v) for c, v in self.eta_diff.items()}
        self.var_tau, self._log_var_tau = {}, {}
        self.pi, self.sigma_epsilon, self.tau_beta, self._sigma_g, self.model_elbos = {}, {}, {}, {}, {}
        self.optim_results, self.validation_result = {}, {}
        for c in self.groups:
            r = rec[c]
            self.var_tau[c] = r["var_tau"]
            self._log_var_tau[c] = np.log(r["var_tau"])
            theta = r["theta"]
            self.pi[c] = np.array([t[0] for t in theta], dtype=T)
            self.sigma_epsilon[c] = np.array([t[1] for t in theta], dtype=T)
            self.tau_beta[c] = np.array([t[2] for t in theta], dtype=T)
            self._sigma_g[c] = np.asarray(r["sigma_g"]).astype(T)
            elbo = r["elbo"]                                     # (VIPRSGrid keeps the ELBO column in the state precision)
            self.model_elbos[c] = elbo.astype(f64)
            self.optim_results[c] = list(r["results"])
            vr = self.grid_tables[c].copy()
            vr["ELBO"] = elbo
            vr["Converged"] = np.array([r.success for r in self.optim_results[c]])
            vr["Optimization_message"] = [r.message for r in self.optim_results[c]]
            self.validation_result[c] = vr
        self.eta = self.compute_eta()
        self.zeta = self.compute_zeta()
        self._host_stale = False
        self.update_posterior_moments()
        res = self.optim_result
        res.nit = max(r.nit for rs in self.optim_results.values() for r in rs)
        res.stop_iteration = True
        res.success = all(r.success for rs in self.optim_results.values() for r in rs)
        return self

    # ---- one chromosome's model through the base class's scalar code --------------------------------------------------
    @property
    def n_snps(self):
        """Variants of the model in scope: the whole loader, or one chromosome inside `m_step_of_chromosome`."""
        return self._chrom_m if getattr(self, "_chrom_m", None) is not None else self.m

    def m_step_of_chromosome(self, c):
        """`VIPRS.m_step` with nothing fixed over chromosome c's current (1-D) posterior, as the M-step of a model over
        chromosome c alone computes it (its SNP count, its lambda_min, one chromosome); returns (pi, tau_beta,
        sigma_epsilon, sigma_g).  (What `bayesian_model_average` runs after averaging a VIPRSGrid.)"""
        gi = self._gindex[c]
        keep = ("shapes", "lambda_min", "_n_chroms_total", "fix_params", "_sums", "_sums_valid", "_host_stale", "pi",
                "tau_beta", "sigma_epsilon", "_sigma_g")
        saved = {k: getattr(self, k) for k in keep}
        lam = self._T.type(self._lambda_group[gi])
        try:
            self.shapes, self._chrom_m = {c: self.shapes[c]}, int(self._m_group[gi])
            self.lambda_min = lam if np.isscalar(lam) else self._T.type(0.0)
            self._n_chroms_total, self.fix_params, self._sums, self._sums_valid, self._host_stale = 1, {}, None, False, False
            self.pi = self.tau_beta = self.sigma_epsilon = None
            VIPRS.m_step(self)
            return self.pi, self.tau_beta, self.sigma_epsilon, self._sigma_g
        finally:
            self._chrom_m = None
            for k, v in saved.items():
                setattr(self, k, v)

    # ---- summaries ---------------------------------------------------------------------------------------------------
    def to_validation_table(self, chrom=None):
        """The validation table of one chromosome, or of all of them with a ``Chromosome`` column."""
        import pandas as pd
        if not self.validation_result:
            raise ValueError("Validation result is not set!")
        if chrom is not None:
            return pd.DataFrame(self.validation_result[chrom])
        return pd.concat([pd.DataFrame(v).assign(Chromosome=c) for c, v in self.validation_result.items()], ignore_index=True)

    def pseudo_validate(self, validation_std_beta=None, chrom=None, validation_ld=None):
        """Pseudo-R^2 per grid point of one chromosome's models (``chrom``), or ``{chromosome: values}``.  `validation_ld`:
        the LD of an external validation panel per chromosome, as `VIPRS.pseudo_validate` takes it (one rank only)."""
        vb = validation_std_beta if validation_std_beta is not None else getattr(self, "validation_std_beta", None)
        assert vb is not None, "standardized betas of a validation set are required"
        chroms = [chrom] if chrom is not None else [c for c in self.groups if c in vb]
        out = {}
        for c in chroms:                # (VIPRS.pseudo_validate over a loader that holds chromosome c only, the same operations)
            if validation_ld is not None:
                if self.comm.world_size > 1:
                    raise NotImplementedError("pseudo_validate(validation_ld=...) runs on one rank only")
                from ..VIPRS import _pseudo_r2_external
                out[c] = _pseudo_r2_external({c: validation_ld[c]}, {c: vb[c]}, {c: self.post_mean_beta[c]},
                                              device=getattr(self, "device", 0))
                continue
            cat = lambda d: np.concatenate([np.asarray(d[c])], axis=0)
            r, b = cat(vb), cat(self.post_mean_beta)
            rb_w = cat({c: self.q[c] + self.post_mean_beta[c]})
            rb = np.sum((b.T * r).T, axis=0)
            out[c] = rb ** 2 / np.sum(b * rb_w, axis=0)
        return out[chrom] if chrom is not None else out

    def elbo(self, sum_axis=None):
        return {c: v.copy() for c, v in self.model_elbos.items()}

    objective = elbo


class VIPRSGridPerChromosome(GridPerChromosomeMixin, PerChromosomeGroups, VIPRSGrid):

    def __init__(self, gdl, grid, **kwargs):
        """``grid``: one ``HyperparameterGrid``, regenerated per chromosome, or a ``{chromosome: HyperparameterGrid}`` dict
        (``GridPerChromosomeMixin._set_grids``)."""
        if np.dtype(kwargs.get("float_precision", "float32")) != np.float32:
            raise NotImplementedError("VIPRSGridPerChromosome: float32 states only (the grid pair mask has no float64 kernels)")
        first = next(iter(grid.values())) if isinstance(grid, dict) else grid
        super().__init__(gdl, grid=first, **kwargs)
        if self.comm.world_size > 1:
            raise NotImplementedError("VIPRSGridPerChromosome runs on one GPU (world_size == 1)")
        if self._e_step_fn is None:
            from ... import _lib as L
            if self._plans["*"].info(L.INFO_N_RAGGED) > 0:
                raise NotImplementedError("VIPRSGridPerChromosome: LD with ragged / banded blocks leaves the dense path, "
                                          "which the grid pair mask needs")
        self._set_grids(gdl, grid)
        self._pair_state = None

    def _make_device_state(self, plan):
        # (the spike-and-slab state of the base class is not swept by this model: no placement probe for it)
        from ...plan import DeviceState
        return DeviceState(plan, self.float_precision, "spike_slab", placement="off")

    # ---- initial hyper-parameters of every pair (VIPRSGrid._fit_batched per chromosome) ---------------------------------
    def _pair_theta(self, theta_0):
        T = self._T
        base_fixed = dict(self.fix_params)
        th = []
        for gi, c in enumerate(self.groups):
            m_c = int(self._m_group[gi])
            for params in self.grid_tables[c].to_dict(orient="records"):
                self.fix_params = {**base_fixed, **params}
                pi, sig, tau = self._theta_values(self._merge_theta(self._theta0_for(c, theta_0)), m_c)
                lam = T.type(params["lambda_min"]) if "lambda_min" in params else self._lambda_group[gi]
                th.append(dict(pi=T.type(pi), sigma_epsilon=T.type(sig), tau_beta=tau, lam=lam, fixed=set(self.fix_params)))
        self.fix_params = base_fixed
        return th

    # ---- state -------------------------------------------------------------------------------------------------------
    def _init_state(self, em):
        T, G = self._T, self.n_models
        for gi, c in enumerate(self.groups):
            m_c = int(self._m_group[gi])
            mk = lambda: np.zeros((m_c, G), dtype=T, order="F")
            self.var_gamma[c] = mk()
            for g in range(G):
                self.var_gamma[c][:, g] = em.pi[gi * G + g]
            self.var_mu[c], self.eta[c], self.q[c], self.eta_diff[c] = mk(), mk(), mk(), mk()
        if self._e_step_fn is not None:
            self._inputs = {c: {k: np.zeros((int(self._m_group[gi]), G), dtype=T, order="F")
                                for k in ("u_logs", "half_var_tau", "mu_mult")} for gi, c in enumerate(self.groups)}
            return
        from ...plan import DeviceState
        ds = self._pair_state
        if ds is None:
            ds = self._pair_state = DeviceState(self._plans["*"], self.float_precision, "grid", G)
            chroms = self.chromosomes
            ds.upload("std_beta", np.concatenate([self.std_beta[c] for c in chroms]))
            ds.set_n_per_snp(np.concatenate([np.asarray(self.n_per_snp[c], dtype=np.float64).ravel() for c in chroms]))
            ds.set_groups(self._group_start)
        for name in ("var_gamma", "var_mu", "eta", "q", "eta_diff"):
            ds.upload(name, np.asfortranarray(np.concatenate([getattr(self, name)[c] for c in self.chromosomes])))
        ds.set_group_columns(np.ones((len(self.groups), G), dtype=np.uint8))
        self._mask = None

    def _sweep(self, ka, em):
        G = self.n_models
        ci, gc = np.divmod(ka, G)
        rows = em.prep_rows(ka)
        if self._e_step_fn is None:
            ds = self._pair_state
            ds.prep_grid_groups(np.column_stack([ci.astype(f64), gc.astype(f64), rows[:, 1:]]))
            mask = np.zeros((len(self.groups), G), dtype=np.uint8)
            mask[ci, gc] = 1
            if self._mask is None or not np.array_equal(mask, self._mask):
                ds.set_group_columns(mask)
                self._mask = mask
            ds.e_step(self.dequantize_scale, active_model_idx=np.unique(gc).astype(np.int32), sync=False)
            return
        T = self._T
        for gi, c in enumerate(self.groups):                      # CPU test hook: the oracle's e_step_grid per chromosome
            sel = ci == gi
            if not sel.any():
                continue
            n, inp = np.asarray(self.n_per_snp[c], dtype=f64), self._inputs[c]
            for (g, logit, log_tau, sig, tau, lam1) in zip(gc[sel], *rows[sel, 1:].T):    # prep_grid_groups_kernel, host
                vt = n * lam1 / sig + tau
                inp["mu_mult"][:, g] = (n / (vt * sig)).astype(T)
                inp["u_logs"][:, g] = (logit + 0.5 * (log_tau - np.log(vt))).astype(T)
                inp["half_var_tau"][:, g] = (0.5 * vt).astype(T)
            self._e_step_fn(self.ld_left_bound[c], self.ld_indptr[c], self.ld_data[c], self.std_beta[c], self.var_gamma[c],
                            self.var_mu[c], self.eta[c], self.q[c], self.eta_diff[c], inp["u_logs"], inp["half_var_tau"],
                            inp["mu_mult"], self.dequantize_scale, np.ascontiguousarray(gc[sel], dtype=np.int32),
                            self.threads, self.low_memory)

    def _pair_sums(self, ka, em):
        """(len(ka), 11) rows in the layout of `viprs_state_sums`, [0] the plain sum of gamma over the chromosome."""
        G = self.n_models
        ci, gc = np.divmod(ka, G)
        if self._e_step_fn is None:
            ds = self._pair_state
            ds.sums_grid_groups_begin(ci, gc, em.lam1[ka])
            return ds.sums_grid_groups_end()
        s = np.zeros((len(ka), 11))
        for r, (gi, g, k) in enumerate(zip(ci, gc, ka)):
            c = self.groups[gi]
            gam, mu = self.var_gamma[c][:, g].astype(f64), self.var_mu[c][:, g].astype(f64)
            eta, q = self.eta[c][:, g], self.q[c][:, g]
            vt = np.asarray(self.n_per_snp[c], dtype=f64) * em.lam1[k] / em.sig_e[k] + em.tau_e[k]
            zeta = gam * (mu * mu + 1.0 / vt)
            lo, hi = _RES, 1.0 - _RES
            gcl, ng = np.clip(gam, lo, hi), np.clip(1.0 - gam, lo, hi)
            s[r] = (gam.sum(), zeta.sum(), (em.lam1[k] * zeta + (q * eta).astype(f64)).sum(),
                    self.std_beta[c].astype(f64) @ eta.astype(f64), (eta.astype(f64) ** 2).sum(), (gcl * np.log(gcl)).sum(),
                    (ng * np.log(ng)).sum(), gcl.sum(), ng.sum(), (gcl * np.log(vt)).sum(),
                    float(np.max(np.abs(self.eta_diff[c][:, g]))) if gam.size else 0.0)
        return s

    # ---- the fit -----------------------------------------------------------------------------------------------------
    def fit(self, pathwise=True, max_iter=1000, theta_0=None, min_iter=3, f_abs_tol=1e-6, x_abs_tol=1e-6, patience=10,
            on_iteration=None, **kwargs):
        """All (chromosome, grid point) pairs in lock step, each from the standard start (independent mode).  Arguments of
        ``VIPRSGrid.fit(batched=True)``; ``theta_0`` is one dict for every chromosome or ``{chromosome: dict}``."""
        if pathwise:
            raise NotImplementedError("VIPRSGridPerChromosome fits the independent grid mode only: call fit(pathwise=False)")
        kwargs.pop("disable_pbar", None)
        kwargs.pop("batched", None)
        T, G, C = self._T, self.n_models, len(self.groups)
        th = self._pair_theta(theta_0)
        em = self._em = LockstepEM(T, th, np.repeat(self._m_group, G), np.repeat(self._n_group, G), n_chroms_total=1,
                                   m_mean=np.repeat(self._m_group, G).astype(f64), min_iter=min_iter, f_abs_tol=f_abs_tol,
                                   x_abs_tol=x_abs_tol, patience=patience)
        self._init_state(em)
        self._set_active(np.arange(C))
        self.history = {c: {"ELBO": [[] for _ in range(G)]} for c in self.groups}

        def settle(a, code, i):
            for k in a:
                self.history[self.groups[k // G]]["ELBO"][k % G].append(float(em.elbos[k]))
            active = a[code == 0]
            if active.size < a.size:                     # a chromosome whose pairs have all stopped leaves the sweep
                ga = np.unique(a // G)
                self._narrow(ga, np.isin(ga, active // G))
            return active

        run_rounds(em, np.arange(C * G), lambda a: self._sweep(a, em), lambda a: self._pair_sums(a, em), settle,
                   max_rounds=max_iter, on_iteration=on_iteration)
        em.finish()
        self._set_active(np.arange(C))
        return self._publish_pairs(em, th)

    def _publish_pairs(self, em, th):
        T, G = self._T, self.n_models
        if self._e_step_fn is None:
            ds = self._pair_state
            for name in ("var_gamma", "var_mu", "eta", "q", "eta_diff"):
                full = ds.download(name)
                for c, (a, b) in self._seg.items():
                    getattr(self, name)[c] = full[a:b]
        rec = {}
        for gi, c in enumerate(self.groups):
            ks = gi * G + np.arange(G)
            vt = np.empty((int(self._m_group[gi]), G), dtype=T)
            for g, k in enumerate(ks):                           # what the LAST E-step of the pair was built from
                vt[:, g] = self._var_tau_of(c, th[k]["lam"], em.sig_e[k], em.tau_e[k])
            rec[c] = dict(var_tau=vt, theta=[em.theta(k) for k in ks], sigma_g=em.sigma_g[ks], elbo=em.elbos[ks].astype(T),
                          results=[em.results[k] for k in ks])
        return self._publish_chromosomes(rec)
