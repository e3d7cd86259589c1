"""``VIPRSGridPathwisePerChromosome`` -- one PATHWISE ``VIPRSGrid`` per chromosome, all chromosomes in lock step on one device
plan.

The reference's CLI fits one ``VIPRSGrid`` per chromosome with ``--hyp-search GS`` / ``BMA`` (bin/viprs_fit:238, fan-out
:1079-1086), and unless ``--grid-search-mode independent`` is given (default :885, switch :501-504) each of those fits is
pathwise: grid point i starts from the state and hyper-parameters point i-1 left (VIPRSGrid.py:190-215,
``continued=i > 0``).  Within a chromosome the points run one after the other; across chromosomes they are independent, so
at any moment every chromosome sits at exactly one grid point -- one spike-and-slab model.  That is the batch of
``VIPRSPerChromosome``: the chromosomes are SNP groups of one spike-and-slab state, and an EM round is one
``viprs_state_prep_groups`` with each chromosome's current scalars, ONE sweep, one ``viprs_state_sums_groups_*`` and
``LockstepEM.update`` (one iteration number per chromosome).  A chromosome whose point stops this round

* stores its state as column i of its (m_c, G) result: one ``viprs_state_commit_groups`` launch for all of them into a grid
  state on the same plan that is never swept (the result store);
* moves on to point i + 1 with its state left in place (the warm start) -- ``LockstepEM.advance`` does the host side of
  ``set_fixed_params(point)`` + ``VIPRS.fit(continued=True)`` -- or, after its last point, leaves the sweep
  (``viprs_plan_set_active_blocks``).

Every round of a chromosome is the round its own ``VIPRSGrid(loader_of_c, grid_c).fit(pathwise=True)`` runs on a plan of
that chromosome alone (``VIPRSGrid._fit_serial`` + ``VIPRS.fit(continued=True)``, VIPRS.py:822-855), so the lock-step fit
reproduces those fits bit for bit.  The sweep runs the spike-and-slab kernels: every LD kind and state precision of
``VIPRSPerChromosome`` works (float64 states, banded / ragged LD), unlike the independent batch
(``VIPRSGridPerChromosome``), whose pair mask needs the fp32 dense grid kernels.

With ``e_step_fn=oracle.cpp_e_step`` (CPU tests) the same host logic runs on NumPy state and a commit is a NumPy column copy.

Results have ``VIPRSGridPerChromosome``'s layout (``GridPerChromosomeMixin``); ``history[c]["ELBO"]`` is chromosome c's
WHOLE pathwise trajectory (its initial ELBO, then one entry per iteration of every point), as ``VIPRSGrid`` leaves it.
"""
import numpy as np

from ...utils.optim import OptimizeResult
from .._lockstep import RESTART, LockstepEM, run_rounds
from ..VIPRS import VIPRS
from ..VIPRSPerChromosome import VIPRSPerChromosome
from .VIPRSGridPerChromosome import GridPerChromosomeMixin

_FIELDS = ("var_gamma", "var_mu", "eta", "q", "eta_diff")


class VIPRSGridPathwisePerChromosome(GridPerChromosomeMixin, VIPRSPerChromosome):

    def __init__(self, gdl, grid, **kwargs):
        """``grid``: one ``HyperparameterGrid``, regenerated per chromosome as the CLI does, or a
        ``{chromosome: HyperparameterGrid}`` dict (``GridPerChromosomeMixin._set_grids``)."""
        super().__init__(gdl, **kwargs)
        if self.comm.world_size > 1:
            raise NotImplementedError("VIPRSGridPathwisePerChromosome runs on one GPU (world_size == 1)")
        self._set_grids(gdl, grid)
        assert self.n_models > 1, "Grid search requires at least 2 models."
        self._lambda_base = list(self._lambda_group)
        self._store = None

    # ---- the result store: column g of chromosome c holds the state its grid point g stopped with ----------------------
    def _new_store(self):
        G = self.n_models
        if self._e_step_fn is not None:
            return {name: {c: np.zeros((int(self._m_group[gi]), G), dtype=self._T, order="F")
                           for gi, c in enumerate(self.groups)} for name in _FIELDS}
        if self._store is None:
            from ...plan import DeviceState
            self._store = DeviceState(self._plans["*"], self.float_precision, "grid", G, placement="off")
        return self._store

    def _commit(self, store, groups, columns):
        if self._e_step_fn is None:
            store.commit_groups(self._dstate["*"], groups, columns)
            return
        for g, col in zip(groups, columns):
            c = self.groups[g]
            if c in self.shapes:
                for name in _FIELDS:
                    store[name][c][:, col] = getattr(self, name)[c]

    def _download(self, store):
        if self._e_step_fn is not None:
            for name in _FIELDS:
                setattr(self, name, store[name])
            return
        for name in _FIELDS:
            full = store.download(name)
            setattr(self, name, {c: full[a:b] for c, (a, b) in self._seg.items()})

    # ---- the fit -----------------------------------------------------------------------------------------------------
    def fit(self, pathwise=True, max_iter=1000, theta_0=None, min_iter=3, f_abs_tol=1e-6, x_abs_tol=1e-6, patience=10,
            on_iteration=None, **kwargs):
        """Every chromosome's pathwise grid search in lock step.  Arguments of ``VIPRSGrid.fit(pathwise=True)``: ``max_iter``
        bounds every grid point's fit, ``theta_0`` is one dict for every chromosome or ``{chromosome: dict}``.
        ``on_iteration(r)`` is called after every EM round r."""
        if not pathwise:
            raise NotImplementedError("VIPRSGridPathwisePerChromosome fits the pathwise grid mode; the independent mode is "
                                      "VIPRSGridPerChromosome")
        T, C, G = self._T, len(self.groups), self.n_models
        points = {c: self.grid_tables[c].to_dict(orient="records") for c in self.groups}
        base_fixed = dict(self.fix_params)
        # ---- point 0: the standard start with the point's values fixed (set_fixed_params + VIPRS.fit) ----
        fixed = [{**base_fixed, **points[c][0]} for c in self.groups]
        raw = []
        for g, c in enumerate(self.groups):
            self.fix_params = fixed[g]
            raw.append(self._theta_for(c, theta_0))
        theta = self._cast_group_theta(raw)
        # (`_lambda_group[g]`: the lambda_min of chromosome g's current point -- what the CPU hook's prep and, after the fit,
        #  `m_step_of_chromosome` see, as the serial fit's `lambda_min` is the one its last `set_fixed_params` set)
        lam = self._lambda_group = [T.type(points[c][0]["lambda_min"]) if "lambda_min" in points[c][0]
                                    else T.type(self._lambda_base[g]) for g, c in enumerate(self.groups)]
        th = [dict(pi=theta[g][0], sigma_epsilon=theta[g][1], tau_beta=theta[g][2], lam=lam[g], fixed=set(fixed[g]))
              for g in range(C)]
        em = self._em = LockstepEM(T, th, self._m_group, self._n_group, n_chroms_total=1, min_iter=min_iter,
                                   f_abs_tol=f_abs_tol, x_abs_tol=x_abs_tol, patience=patience, restart_free_sigma=True)
        self.var_mu, self.var_tau, self.var_gamma, self._log_var_tau = {}, {}, {}, {}
        self.eta, self.zeta, self.eta_diff, self.q = {}, {}, {}, {}
        for c in self.chromosomes:
            self._init_chromosome_state(c, *theta[self._gindex[c]])
        self._host_stale = False
        self._push_state()
        self._set_active(np.arange(C))
        store = self._new_store()
        names = [t if isinstance(t, str) else t.__name__ for t in self.tracked_params]
        self.history = {c: dict({"ELBO": []}, **{n: [] for n in names}) for c in self.groups}
        all_groups = np.arange(C)
        s0 = self._group_sums(all_groups, em, on_host=True)
        for g, c in enumerate(self.groups):
            self.fix_params = fixed[g]
            with self._as_group(g, *theta[g]):
                self._sums, self._sums_valid = s0[g, :10], True
                self.history[c]["ELBO"].append(VIPRS.elbo(self))
        self._sums, self._sums_valid = None, False
        self._track(all_groups, em)

        # ---- lock-step rounds: chromosome g is on its grid point point[g], iteration number it[g] of its history ----
        point = np.zeros(C, dtype=np.int64)
        it = np.ones(C, dtype=np.int64)                 # VIPRS.fit: 1 on point 0, then len(history["ELBO"]) + 1
        n_point = np.zeros(C, dtype=np.int64)           # iterations of the current point (max_iter bounds each point)
        rec = {c: dict(var_tau=np.empty((int(self._m_group[g]), G), dtype=T), theta=[None] * G, sigma_g=np.zeros(G),
                       elbo=np.empty(G, dtype=T), results=[None] * G) for g, c in enumerate(self.groups)}

        def settle(a, code, rnd):
            self._track(a, em, elbo=True)
            for g in a[code == RESTART]:
                self.fix_params = fixed[g]
                self._restart_group(int(g), em, theta_0, int(it[g]))
                fixed[g]["sigma_epsilon"] = 0.95
            it[a] += 1
            n_point[a] += 1
            stopped = (code != 0) & (code != RESTART)
            out = a[stopped | (~stopped & (n_point[a] >= max_iter))]
            if not out.size:
                return a
            em.finish(out)
            self._commit(store, out, point[out])
            for g in out:
                self._record(rec[self.groups[g]], int(point[g]), int(g), em, lam[g])
            moving = out[point[out] + 1 < G]
            for g in moving:
                c = self.groups[g]
                point[g] += 1
                p = points[c][point[g]]
                fixed[g].update(p)
                if "lambda_min" in p:
                    lam[g] = T.type(p["lambda_min"])
                em.advance(int(g), p)
                it[g] = len(self.history[c]["ELBO"]) + 1
                n_point[g] = 0
            return self._narrow(a, ~np.isin(a, np.setdiff1d(out, moving)))       # (after its last point: out of the sweep)

        # (`max_iter` bounds every grid point, not the run: no bound on the rounds)
        run_rounds(em, all_groups, lambda a: self._sweep(a, em), lambda a: self._group_sums(a, em), settle,
                   iteration=lambda a: it[a], on_iteration=on_iteration)
        self._set_active(all_groups)
        self.fix_params = base_fixed
        self._sums, self._sums_valid = None, False
        self._download(store)
        self.optim_result = OptimizeResult()
        return self._publish_chromosomes(rec)

    def _record(self, r, i, g, em, lam):
        """Point i of chromosome g has stopped: what ``VIPRSGrid._fit_serial`` keeps of it (its result, ``elbo[i] =
        history["ELBO"][-1]``, ``_collect``'s scalars and var_tau as the point's last E-step built it)."""
        c = self.groups[g]
        r["results"][i] = em.results[g]
        r["elbo"][i] = self.history[c]["ELBO"][-1]
        r["theta"][i] = em.theta(g)
        r["sigma_g"][i] = em.sigma_g[g]
        r["var_tau"][:, i] = self._var_tau_of(c, lam, em.sig_e[g], em.tau_e[g])
