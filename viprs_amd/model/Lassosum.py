"""``Lassosum`` -- the L1 / elastic-net estimate from marginal effects and an LD panel (Mak et al. 2017), the third baseline
of every summary-statistics PRS comparison beside `LDPredInf` and `ClumpThreshold`, with its coordinate descent on MI355X.

For every ``(s, lambda)`` of the grid the estimate minimises ``b'((1 - s) R + s I) b - 2 b'beta_hat + 2 lambda sum_j w_j
|b_j|`` (``w``: the optional per-SNP penalty factor).  Every ``s < 1`` is one column of ONE grid state on the device; the
path runs from the largest lambda down, each lambda warm-started from the one before, and at each lambda the columns that
have not converged are swept in lock step (`DeviceState.enet_sweep`: cyclic coordinate descent over each LD block, the
E-step's serial sweep with a soft threshold; `viprs_amd.stats.enet` is its host definition) until the largest change of a
coefficient is at most `tol`.  ``s = 1`` has no LD term: the closed form ``soft(beta_hat, lambda w)`` on the host.  A column
whose coefficients stop being finite -- small ``s`` on an LD panel that is not positive definite -- is marked ``diverged``,
set to zero for this and every smaller lambda and leaves the sweeps.

The LD of every chromosome lives in one device plan, as for `ClumpThreshold`, whose result layout, `predict`,
`pseudo_validate`, `select_best` and `to_table` this class takes over unchanged (``post_mean_beta[c]`` of shape ``(m_c,
n_models)``, model ``i_s * n_lambda + k``).  The reference has no such class.  One rank only.  (``sweep_fn`` lets the CPU
tests drive the host logic with `viprs_amd.stats.enet.enet_sweep_host`; without it and without a GPU the constructor raises.)
"""
import numpy as np

from ._chain_engines import DeviceColumns, HostColumns
from .ClumpThreshold import ClumpThreshold


class Lassosum(ClumpThreshold):

    def __init__(self, gdl, s=(0.2, 0.5, 0.9, 1.0), lambdas=None, penalty_factor=None, tol=1e-4, max_sweeps=1000,
                 float_precision="float32", low_memory=True, dequantize_on_the_fly=False, device=None, sweep_fn=None,
                 comm=None):
        """:param gdl: the data loader (summary statistics and LD matrices per chromosome).
        :param s: the shrinkage values of the LD matrix, each in (0, 1]; the grid is ``s x lambdas``, s outermost.
        :param lambdas: the penalties (any order: the path runs over them descending; the models keep that descending
            order); None: `viprs_amd.stats.enet.lambda_path()`, 20 values from 0.1 down to 0.001.
        :param penalty_factor: per-SNP factors >= 0 of the penalty, ``{chromosome: array}`` or one array over all SNPs.
        :param tol: a column stops at a lambda when the largest |change of a coefficient| of a sweep is <= tol.
        :param max_sweeps: sweeps per lambda at most.
        :param float_precision: 'float32' (the device sweep has no float64 form).
        :param low_memory: load the upper-triangular form of the LD matrices (never expanded on the device).
        :param dequantize_on_the_fly: keep integer LD in its stored dtype on the device (as in `ClumpThreshold`).
        :param device: HIP device index (default 0).
        :param sweep_fn: test hook -- a callable with `viprs_amd.stats.enet.enet_sweep_host`'s signature that replaces the
            device sweep (called once per column and sweep).
        """
        self._set_loader(gdl, comm)
        self._configure(s, lambdas, tol, max_sweeps, float_precision, sweep_fn)
        self._set_penalty(penalty_factor)
        self._load("float32", low_memory, dequantize_on_the_fly, device, sweep_fn is not None,
                   "Lassosum needs a HIP device (viprs_amd.stats.enet.enet_sweep_host is the sweep on the host: "
                   "pass it as sweep_fn)")

    def _configure(self, s, lambdas, tol, max_sweeps, float_precision, sweep_fn):
        """What a fit needs beside the data and the penalty factors: checked and stored by both constructors."""
        if np.dtype(float_precision) != np.float32:
            raise ValueError("Lassosum: float_precision must be 'float32' (the elastic-net sweep has no float64 form)")
        self.s = np.atleast_1d(np.asarray(s, dtype=np.float64))
        lam = np.atleast_1d(np.asarray(lambdas, dtype=np.float64)) if lambdas is not None else None
        if self.s.ndim != 1 or self.s.shape[0] < 1 or not np.all((self.s > 0) & (self.s <= 1)):
            raise ValueError("s: at least one value, each in (0, 1]")
        if lam is not None and (lam.ndim != 1 or lam.shape[0] < 1 or not np.all(np.isfinite(lam)) or np.any(lam < 0)):
            raise ValueError("lambdas: at least one finite value >= 0")
        if lam is None:
            from ..stats.enet import lambda_path
            lam = lambda_path()
        self.lambdas = np.sort(lam)[::-1].copy()
        if not (tol >= 0) or int(max_sweeps) < 1:
            raise ValueError("tol >= 0 and max_sweeps >= 1")
        self.tol, self.max_sweeps = float(tol), int(max_sweeps)
        self._sweep_fn = sweep_fn
        self.n_models = int(self.s.shape[0] * self.lambdas.shape[0])
        self.post_mean_beta = None
        self.grid_table = None
        self.validation_result = None
        self.best_model_idx = None

    def _set_penalty(self, penalty_factor):
        if penalty_factor is None:
            w = np.ones(self.m)
        elif isinstance(penalty_factor, dict):
            w = np.concatenate([np.asarray(penalty_factor[c], dtype=np.float64) for c in self.chromosomes])
        else:
            w = np.asarray(penalty_factor, dtype=np.float64)
        if w.shape != (self.m,) or not np.all(np.isfinite(w)) or np.any(w < 0):
            raise ValueError("penalty_factor: one finite value >= 0 per SNP")
        self.penalty_factor = w

    @classmethod
    def from_plan(cls, plan, std_beta, dq_scale, s=(0.2, 0.5, 0.9, 1.0), lambdas=None, penalty_factor=None, tol=1e-4,
                  max_sweeps=1000):
        """A model on an existing `LDPlan` (`MergedPlanModel._attach`: one chromosome, the LD may exist on the device only).
        Device sweep only; the plan stays the caller's."""
        self = cls.__new__(cls)
        self._configure(s, lambdas, tol, max_sweeps, "float32", None)
        self._attach(plan, dq_scale, std_beta)
        self._set_penalty(penalty_factor)
        return self

    # -- the two engines of the path: a grid state on the device, or arrays swept by the hook -------------------------------
    class _Device(DeviceColumns):
        def __init__(self, plan, beta, mult, dq):
            from ..plan import DeviceState
            self.dq = dq
            self.st = DeviceState(plan, "float32", model="grid", width=mult.shape[1], placement="off")
            zero = np.zeros(mult.shape, dtype=np.float32, order="F")
            self.st.upload("std_beta", beta)
            self.st.upload("mu_mult", mult)
            for k in ("u_logs", "var_gamma", "var_mu", "eta", "q", "eta_diff"):
                self.st.upload(k, zero)

        def set_penalty(self, pen):
            self.st.upload("half_var_tau", pen)

        def sweep(self, active):
            self.st.enet_sweep(self.dq, active_model_idx=active, sync=False)
            return self.st.enet_sums(active)

        def eta(self):
            return self.st.download("eta")

    class _Host(HostColumns):
        def __init__(self, fn, ld, low_memory, beta, mult, dq):
            self.fn, self.ld, self.low_memory, self.beta, self.mult, self.dq = fn, ld, low_memory, beta, mult, dq
            self._eta, self.q, self.ed = (np.zeros(mult.shape, dtype=np.float32, order="F") for _ in range(3))
            self.pen = None

        def set_penalty(self, pen):
            self.pen = pen

        def sweep(self, active):
            from ..stats.enet import enet_sums_host
            lb, ip, data = self.ld
            for g in active:
                self.ed[:, g] = self.fn(lb, ip, data, self.low_memory, self.beta, self.mult[:, g], self.pen[:, g],
                                        self._eta[:, g], self.q[:, g], self.dq)[0]
            return enet_sums_host(self.beta, self.pen, self._eta, self.q, self.ed, cols=active, grid=True)

        def eta(self):
            return self._eta.copy()

    def fit(self):
        """The path over `lambdas` (descending, warm starts) for every `s`; model ``i_s * n_lambda + k``."""
        import pandas as pd
        from ..stats.enet import enet_objective
        f32 = np.float32
        m, n_lam = self.m, self.lambdas.shape[0]
        beta_hat = self._concat(self.std_beta)
        path_s = [i for i, v in enumerate(self.s) if v < 1.0]                 # column g of the state: s[path_s[g]]
        G = len(path_s)
        beta = np.zeros((m, self.n_models), dtype=f32)
        rows = [dict(s=float(sv), **{"lambda": float(lv)}, n_sweeps=0, converged=True, diverged=False, n_nonzero=0,
                     objective=np.nan) for sv in self.s for lv in self.lambdas]
        pens = [(lv * self.penalty_factor).astype(f32) for lv in self.lambdas]
        # s = 1: no LD term, the minimiser is the soft threshold of the marginal effects
        for i, sv in enumerate(self.s):
            if sv < 1.0:
                continue
            for k, pen in enumerate(pens):
                a = np.abs(beta_hat) - pen
                b = np.where(a > 0, np.copysign(a, beta_hat), f32(0.0)).astype(f32)
                beta[:, i * n_lam + k] = b
                b64 = b.astype(np.float64)
                rows[i * n_lam + k].update(n_nonzero=int(np.count_nonzero(b)), objective=float(
                    b64 @ b64 - 2.0 * (b64 @ beta_hat.astype(np.float64)) + 2.0 * (pen.astype(np.float64) @ np.abs(b64))))
        if G:
            mult = np.asfortranarray(np.repeat((1.0 - self.s[path_s]).astype(f32)[None, :], m, axis=0))
            s_eff = 1.0 - mult[0].astype(np.float64)                          # the s the rounded multiplier stands for
            eng = (self._Host(self._sweep_fn, self._ld, self.low_memory, beta_hat, mult, self.dequantize_scale)
                   if self._sweep_fn is not None else self._Device(self._plan, beta_hat, mult, self.dequantize_scale))
            try:
                diverged = np.zeros(G, dtype=bool)
                for k, pen in enumerate(pens):
                    eng.set_penalty(np.asfortranarray(np.repeat(pen[:, None], G, axis=1)))
                    active = [g for g in range(G) if not diverged[g]]
                    last = {}
                    n_sweeps = np.zeros(G, dtype=np.int64)
                    done = np.zeros(G, dtype=bool)
                    while active and n_sweeps[active[0]] < self.max_sweeps:
                        sums = eng.sweep(np.asarray(active, dtype=np.int32))
                        still = []
                        for g, row in zip(active, sums):
                            n_sweeps[g] += 1
                            last[g] = row
                            if not np.isfinite(row[3]):
                                diverged[g] = True
                                eng.zero_column(g)
                            elif row[0] <= self.tol:
                                done[g] = True
                            else:
                                still.append(g)
                        active = still
                    eta = eng.eta()
                    for g in range(G):
                        r = rows[path_s[g] * n_lam + k]
                        r.update(n_sweeps=int(n_sweeps[g]), converged=bool(done[g]), diverged=bool(diverged[g]))
                        if not diverged[g]:
                            beta[:, path_s[g] * n_lam + k] = eta[:, g]
                            r.update(n_nonzero=int(last[g][5]), objective=float(enet_objective(last[g], s_eff[g])))
            finally:
                eng.close()
        self.post_mean_beta = self._split(beta)
        self.grid_table = pd.DataFrame(rows, columns=["s", "lambda", "n_sweeps", "converged", "diverged", "n_nonzero",
                                                      "objective"])
        self.validation_result = self.grid_table.copy()
        self.best_model_idx = None
        return self
