"""The engines of the lock-step Gibbs chains -- every chain a column of ONE grid state -- and the two rules their fit loops
share.  `DeviceChains` / `HostChains` are what `LDpred2` and `PRSCS` have in common: the state, one sweep with its sums, the
accumulated Rao-Blackwellised means.  A model adds how the inputs of a sweep are made (`LDpred2`: ``prep``; `PRSCS`:
``prepare``, ``update``, and `sums` widened by the continuous-shrinkage sums).  `DeviceColumns` / `HostColumns` below them
are the little that `Lassosum`'s path, another sweep policy, shares with the chains.  (`SBayesR` runs a mixture state per
chain: its engines stay with it; it takes the two rules.)
"""
import warnings

import numpy as np


def divergence_rule(model):
    """``(beta_hat, diverged)``: the marginal effects over all SNPs, and the predicate of a chain's ``sum eta^2`` -- not
    finite, or beyond ``sum beta_hat^2``."""
    beta_hat = model._concat(model.std_beta)
    limit = float(beta_hat.astype(np.float64) @ beta_hat.astype(np.float64))
    return beta_hat, lambda sum_eta2: not np.isfinite(sum_eta2) or sum_eta2 > limit


def tail_mean(history, start, diverged):
    """The mean over ``history[start:]`` (iterations first) that skips nan, and nan where `diverged`; silent about tails
    without any number."""
    with np.errstate(invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.where(diverged, np.nan, np.nanmean(history[start:], axis=0))


class DeviceColumns:
    """A grid `DeviceState` (`st`) whose columns leave the sweeps one by one."""

    def zero_column(self, g):
        for k in ("eta", "q"):
            a = self.st.download(k)
            a[:, g] = 0
            self.st.upload(k, a)

    def close(self):
        self.st.close()


class HostColumns:
    """The same on the host: `_eta` and `q`, Fortran-ordered ``(m, G)``."""

    def zero_column(self, g):
        self._eta[:, g] = 0
        self.q[:, g] = 0

    def close(self):
        pass


class DeviceChains(DeviceColumns):
    def __init__(self, model, beta, G):
        from ..plan import DeviceState
        self.model, self.dq = model, model.dequantize_scale
        self.st = DeviceState(model._plan, "float32", model="grid", width=G, placement="off")
        self.st.upload("std_beta", beta)
        self.st.set_n_per_snp(model._n_per_snp)
        self.st.gibbs_reset_mean()

    def sums(self, active):
        return self.st.enet_sums(active)

    def sweep(self, active, draw_index):
        self.st.gibbs_sweep(self.dq, active_model_idx=active, seed=self.model.seed, draw_index=draw_index, sync=False)
        sums = self.sums(active)
        if self.model._keep_draws_log:
            self.model.draws_log.append((self.st.gibbs_download("unif"), self.st.gibbs_download("noise")))
        return sums

    def accumulate(self, active):
        self.st.gibbs_accumulate(active)

    def mean_sum(self):
        return self.st.gibbs_download("mean_sum")


class HostChains(HostColumns):
    def __init__(self, model, beta, G):
        from ..stats.gibbs import gibbs_draws_host
        self.model, self.beta, self.dq = model, beta, model.dequantize_scale
        self.draws = model._draws_fn or gibbs_draws_host
        self.mm, self.hvt, self.ulog, self._eta, self.q, self.ed, self.mu, self.gam = (
            np.zeros((model.m, G), dtype=np.float32, order="F") for _ in range(8))
        self.mean = np.zeros((model.m, G), dtype=np.float64, order="F")

    def sums(self, active):
        from ..stats.enet import enet_sums_host
        return enet_sums_host(self.beta, self.hvt, self._eta, self.q, self.ed, cols=active, grid=True)

    def sweep(self, active, draw_index):
        lb, ip, data = self.model._ld
        a = np.asarray(active)
        unif, noise = self.draws(self.model.seed, draw_index, self.hvt, a)
        pick = lambda x: np.asfortranarray(x[:, a])
        eta, q = pick(self._eta), pick(self.q)
        res = self.model._sweep_fn(lb, ip, data, self.model.low_memory, self.beta, pick(self.mm), pick(self.hvt),
                                   pick(self.ulog), pick(unif), pick(noise), eta, q, self.dq)
        for dst, src in zip((self.ed, self.mu, self.gam, self._eta, self.q), tuple(res) + (eta, q)):
            dst[:, a] = src
        return self.sums(active)

    def accumulate(self, active):
        for g in active:
            self.mean[:, g] += self.gam[:, g].astype(np.float64) * self.mu[:, g].astype(np.float64)

    def mean_sum(self):
        return self.mean.copy()
