"""What the lock-step fits share (`viprs_amd/model/_lockstep.py`): the round loop `run_rounds` over a fake EM object and
recording callables, and the stopping rules `LockstepRules.stop_codes` driven through both EM classes on the same sums."""
import numpy as np

from viprs_amd.model._lockstep import RESTART, LockstepEM, keeps_going, run_rounds
from viprs_amd.model._lockstep_mix import LockstepMixEM


# ---- the round loop -----------------------------------------------------------------------------------------------------
class FakeEM:
    """Stop codes from a script {round: {model: code}}; every call goes into `log`."""

    def __init__(self, log, script):
        self.log, self.script, self.round = log, script, 0

    def mark_e_step(self, a):
        self.round += 1
        self.log.append(("mark", self.round, list(a)))

    def update(self, a, s, i):
        self.log.append(("update", list(a), s, i if np.ndim(i) == 0 else list(i)))
        return np.array([self.script.get(self.round, {}).get(int(g), 0) for g in a])


def drive(script, n=4, iteration=None, max_rounds=None):
    log = []
    em = FakeEM(log, script)

    def settle(a, code, rnd):
        log.append(("settle", list(a), list(code), rnd))
        return a[keeps_going(code)]

    def sums(a):
        log.append(("sums", list(a)))
        return "S", list(a)

    run_rounds(em, np.arange(n), lambda a: log.append(("sweep", list(a))), sums, settle, iteration=iteration,
               max_rounds=max_rounds, on_iteration=lambda r: log.append(("on_iteration", r)))
    return log


def rounds_of(log):
    """The log cut into rounds: each one starts at `mark_e_step`."""
    cuts = [k for k, rec in enumerate(log) if rec[0] == "mark"] + [len(log)]
    return [log[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def test_round_loop_order_and_active_set():
    # model 1 converges in round 1, model 2 restarts in round 2 and stops in round 3, the others in round 4
    log = drive({1: {1: 5}, 2: {2: RESTART}, 3: {2: 8}, 4: {0: 6, 3: 1}})
    rounds = rounds_of(log)
    assert len(rounds) == 4                                               # the set is empty after round 4: no fifth round
    active = [[0, 1, 2, 3], [0, 2, 3], [0, 2, 3], [0, 3]]                 # non-zero code: out; RESTART: stays
    for r, (rec, a) in enumerate(zip(rounds, active), start=1):
        assert [x[0] for x in rec] == ["mark", "sweep", "sums", "update", "settle", "on_iteration"]
        assert rec[0] == ("mark", r, a) and rec[1] == ("sweep", a) and rec[2] == ("sums", a)
        assert rec[3] == ("update", a, ("S", a), r)                       # the sums go to update, the round number is `i`
        assert rec[4][1] == a and rec[4][3] == r and rec[5] == ("on_iteration", r)
    assert [x for x in log if x[0] == "on_iteration"] == [("on_iteration", r) for r in (1, 2, 3, 4)]


def test_round_loop_bound_and_empty_start():
    rounds = rounds_of(drive({}, max_rounds=3))
    assert len(rounds) == 3 and all(rec[0][2] == [0, 1, 2, 3] for rec in rounds)
    assert drive({}, max_rounds=0) == [] and drive({}, n=0) == []


def test_round_loop_iteration_per_model():
    it = np.array([7, 1, 30, 4])
    log = drive({1: {1: 5}}, iteration=lambda a: it[a] + 100, max_rounds=2)
    upd = [x for x in log if x[0] == "update"]
    assert upd[0][1:] == ([0, 1, 2, 3], ("S", [0, 1, 2, 3]), [107, 101, 130, 104])
    assert upd[1][1:] == ([0, 2, 3], ("S", [0, 2, 3]), [107, 130, 104])   # aligned with the active set


# ---- the shared rules through both classes ----------------------------------------------------------------------------------
G, ROUNDS = 5, 8


def both(T=np.float32):
    """The same G models with EVERY hyper-parameter fixed (both M-steps are the identity) as spike-and-slab models and as
    K = 1 mixtures."""
    kw = dict(min_iter=3, patience=1)
    m, n = np.array([100, 120, 140, 160, 180]), np.array([1e4, 2e4, 3e4, 4e4, 5e4])
    ss = [dict(pi=T(0.01), sigma_epsilon=T(0.8), tau_beta=T(200.0 + g), lam=T(0.0), fixed={"pi", "tau_beta", "sigma_epsilon"})
          for g in range(G)]
    mix = [dict(pi=np.array([0.01], dtype=T), sigma_epsilon=T(0.8), tau_beta=np.array([200.0 + g], dtype=T), lam=T(0.0),
                fixed={"pis": None, "tau_betas": None, "sigma_epsilon": 0.8}) for g in range(G)]
    return LockstepEM(np.dtype(T), ss, m, n, **kw), LockstepMixEM(np.dtype(T), mix, np.ones(1, dtype=T), m, n, **kw)


def sums(rnd):
    """(G, 11) rows in the layout of `viprs_state_sums`.  Model 0: random (its ELBO goes up and down); 1: the same sums
    every round; 2: a rising ELBO over a sigma_g and a max |eta_diff| that have settled; 3: a negative MSE from round 6;
    4: a heritability out of bounds from round 5."""
    s = np.abs(np.random.default_rng(rnd).normal(size=(G, 11))) + 0.1
    s[1:] = np.abs(np.random.default_rng(0).normal(size=(G - 1, 11))) + 0.1
    s[:, 0], s[:, 3], s[:, 10] = 0.02, 0.05, 1e-3
    s[1:, 1], s[1:, 4] = 0.3, 1.5               # (an MSE above zero whatever sigma_g is)
    s[2, 5] -= 0.01 * rnd
    s[2, 10] = 5e-6
    s[3:, 5] -= 0.01 * rnd
    if rnd >= 6:
        s[3, 3] = 5.0
    if rnd >= 5:
        s[4, 2] = -0.9
    return s


def as_mixture(s):
    """The same sums in the layout of `viprs_state_sums_mixture_end` for K = 1."""
    return s[:, [1, 2, 3, 4, 6, 8, 0, 1, 5, 7, 9, 1, 10]]


def test_stopping_rules_agree_between_the_two_classes():
    a, b = both()
    assert not b.fresh.any()
    idx, seen = np.arange(G), set()
    for i in range(1, ROUNDS + 1):
        s = sums(i)
        ca, cb = a.update(idx, s, i), b.update(idx, as_mixture(s), i)
        assert np.array_equal(ca, cb), (i, ca, cb)
        assert np.array_equal(a.plateau_n, b.plateau_n) and np.array_equal(a.dropping_n, b.dropping_n)
        assert [r.message for r in a.results] == [r.message for r in b.results]
        state = lambda em: [(r.stop_iteration, r.success, r.nit) for r in em.results]
        assert state(a) == state(b)
        seen |= set(int(c) for c in ca)
    # the sums are built so that the rules have something to decide: dropping, plateau, converged ELBO, heritability, MSE
    assert {0, 1, 4, 5, 7, 8} <= seen, seen
    a.finish()
    b.finish()
    assert [r.message for r in a.results] == [r.message for r in b.results]
