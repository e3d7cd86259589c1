"""CPU: the host implementation of greedy LD clumping (`viprs_amd.stats.clump.clump_host`, the yardstick of the device
tests) against a hand-worked case, against a brute force over the dense matrix, and against the invariants of the
definition in include/viprs_hip.h; `clump_order`; the prefix property `ClumpThreshold` rests on."""
import functools

import numpy as np
import pytest

from tests.test_gpu_ld_dot import _banded_windows
from viprs_amd.stats.clump import clump_host, clump_order
from viprs_amd.utils import synthetic as syn

SIZES = (1, 2, 63, 64, 65, 130)
R2 = (0.05, 0.1, 0.2, 0.5)


def dense_entries(lb, ip, data, low_memory):
    """(X, E): the stored elements as float64 and the entry set of the symmetric matrix the arrays stand for, dense."""
    m = lb.shape[0]
    X, E = np.zeros((m, m)), np.zeros((m, m), dtype=bool)
    for j in range(m):
        for t in range(int(ip[j + 1] - ip[j])):
            c = int(lb[j]) + t
            if c == j:
                continue
            X[j, c], E[j, c] = float(data[ip[j] + t]), True
            if low_memory:
                X[c, j], E[c, j] = X[j, c], True
    return X, E


def brute_force(X, E, order, thr, member):
    """The per-column procedure of the header, entry by entry over the dense matrix."""
    m = X.shape[0]
    out = np.full((m, len(thr)), -1, dtype=np.int32)
    for g, t in enumerate(thr):
        avail = np.ones(m, dtype=bool) if member is None else np.array(member, dtype=bool)
        for j in order:
            if not avail[j]:
                continue
            out[j, g] = j
            avail[j] = False
            for k in range(m):
                if E[j, k] and avail[k] and X[j, k] * X[j, k] >= t:
                    out[k, g] = j
                    avail[k] = False
    return out


def chisq_draw(m, seed):
    """chi^2 (1 d.f.) statistics with 2 % inflated SNPs."""
    rng = np.random.default_rng(seed)
    chisq = rng.chisquare(1, m)
    hot = rng.random(m) < 0.02
    chisq[hot] += rng.chisquare(1, int(hot.sum())) * 25.0
    return chisq


def test_hand_worked_case():
    """Six SNPs in one block; |r|: (0,1) .9, (2,3) .8, (3,5) .7, (4,5) .6, (1,2) .5, (0,4) .2, every other pair .1.
    Order 2, 0, 4, 1, 5, 3.
    r2 = .3: 2 takes 3 (.64; 1 is at .25); 0 takes 1 (.81); 4 takes 5 (.36); 1, 5, 3 are claimed    -> 0 0 2 2 4 4
    r2 = .2: 2 takes 3 and 1 (.25); 0 finds 1 gone and 4 at .04; 4 takes 5                          -> 0 2 2 2 4 4"""
    R = np.full((6, 6), 0.1)
    for (a, b), v in {(0, 1): .9, (2, 3): -.8, (3, 5): .7, (4, 5): -.6, (1, 2): .5, (0, 4): .2}.items():
        R[a, b] = R[b, a] = v
    np.fill_diagonal(R, 1.0)
    order = np.array([2, 0, 4, 1, 5, 3])
    sym = (np.zeros(6, np.int32), np.arange(0, 37, 6), R.ravel().astype(np.float32), False)
    up = (np.minimum(np.arange(1, 7), 5).astype(np.int32), np.concatenate([[0], np.cumsum(np.arange(5, -1, -1))]),
          np.concatenate([R[j, j + 1:] for j in range(6)]).astype(np.float32), True)
    for arrays in (sym, up):
        assert clump_host(*arrays, order, 0.3).tolist() == [0, 0, 2, 2, 4, 4]
        assert clump_host(*arrays, order, 0.2).tolist() == [0, 2, 2, 2, 4, 4]
        got = clump_host(*arrays, order, (0.3, 0.2))
        assert got.shape == (6, 2) and got.dtype == np.int32
        assert got[:, 0].tolist() == [0, 0, 2, 2, 4, 4] and got[:, 1].tolist() == [0, 2, 2, 2, 4, 4]
        # a non-member is never claimed and is no entry of the order; SNPs behind the order's end stay unclaimed
        member = np.array([1, 1, 1, 0, 1, 1], dtype=bool)
        assert clump_host(*arrays, order[:5], 0.3, member).tolist() == [0, 0, 2, -1, 4, 4]
        assert clump_host(*arrays, order[:2], 0.3).tolist() == [0, 0, 2, 2, -1, -1]
        assert clump_host(*arrays, order[:0], 0.3).tolist() == [-1] * 6
        # r2 = 0: every entry passes (one clump); above every entry: every SNP of the order is its own index SNP
        assert clump_host(*arrays, order, 0.0).tolist() == [2] * 6
        assert clump_host(*arrays, order, 0.9).tolist() == [0, 1, 2, 3, 4, 5]
        # the natural order: LD pruning
        assert clump_host(*arrays, np.arange(6), 0.3).tolist() == [0, 0, 2, 2, 4, 4]
        # ... and the reverse one: 5 takes 3 (.49) and 4 (.36); 2 finds 3 gone and 1 at .25; 1 takes 0
        assert clump_host(*arrays, np.arange(6)[::-1], 0.3).tolist() == [1, 1, 2, 5, 5, 5]


@functools.lru_cache(maxsize=None)
def _cases():
    out = []
    for low_memory in (False, True):
        for kind, dt in (("ar1", np.float32), ("longrange", np.int8), ("sample", np.int16)):
            ld = syn.make_ld(SIZES, low_memory=low_memory, ld_dtype=dt, kind=kind, seed=5, rho_range=(0.5, 0.95))
            out.append((f"{kind}-{np.dtype(dt).name}", ld.ld_left_bound, ld.ld_indptr, ld.ld_data, low_memory, ld.dq_scale))
        lb, ip = _banded_windows(400, 30, 45, low_memory, seed=14, jitter=20)
        data = np.random.default_rng(15).uniform(-1, 1, int(ip[-1])).astype(np.float32)
        out.append(("banded-float32", lb, ip, data, low_memory, 1.0))
    return out


def test_host_implementation_against_the_brute_force():
    for name, lb, ip, data, low_memory, dq in _cases():
        m = lb.shape[0]
        chisq = chisq_draw(m, 7)
        X, E = dense_entries(lb, ip, data, low_memory)
        thr = np.asarray(R2) / (dq * dq)
        for order, member in ((clump_order(chisq, 1.0), chisq >= 0.3), (clump_order(chisq), None),
                              (np.arange(m), None), (np.arange(m)[::-1], None)):
            got = clump_host(lb, ip, data, low_memory, order, R2, member, dq)
            want = brute_force(X, E, order, thr, member)
            assert np.array_equal(got, want), (name, low_memory)
            assert np.array_equal(clump_host(lb, ip, data, low_memory, order, R2[2], member, dq), want[:, 2])


def test_both_ld_forms_agree():
    cases = _cases()
    half = len(cases) // 2
    for (name, lb, ip, data, _, dq), (name_u, lb_u, ip_u, data_u, _, dq_u) in zip(cases[:half - 1], cases[half:-1]):
        assert name == name_u
        m = lb.shape[0]
        chisq = chisq_draw(m, 8)
        order, member = clump_order(chisq, 1.0), chisq >= 0.3
        sym = clump_host(lb, ip, data, False, order, R2, member, dq)
        up = clump_host(lb_u, ip_u, data_u, True, order, R2, member, dq_u)
        assert np.array_equal(sym, up), name
        assert np.any(sym != np.arange(m)[:, None])


def test_invariants():
    for name, lb, ip, data, low_memory, dq in _cases():
        m = lb.shape[0]
        chisq = chisq_draw(m, 9)
        order, member = clump_order(chisq, 1.0), chisq >= 0.3
        rank = np.full(m, m)
        rank[order] = np.arange(order.shape[0])
        X, E = dense_entries(lb, ip, data, low_memory)
        got = clump_host(lb, ip, data, low_memory, order, R2, member, dq)
        for g, r2 in enumerate(R2):
            P = E & (X * X >= r2 / (dq * dq))
            idx = got[:, g]
            is_index = idx == np.arange(m)
            assert np.array_equal(np.flatnonzero(is_index), np.sort(order[is_index[order]])), "index SNPs come from the order"
            assert np.all(idx[~member] == -1)
            claimed = np.flatnonzero((idx >= 0) & ~is_index)
            assert claimed.size, name
            # every claimed SNP's index is an index SNP that precedes it in the order and passes the threshold with it
            assert np.all(is_index[idx[claimed]]) and np.all(rank[idx[claimed]] < rank[claimed]) and np.all(P[idx[claimed], claimed])
            # ... and it is the FIRST index SNP of the order that does
            for k in claimed[:50]:
                first = min((rank[j], j) for j in np.flatnonzero(P[:, k] & is_index))[1]
                assert idx[k] == first
            # the index SNPs are pairwise below the threshold (row of the earlier one: the banded case's random windows are
            # no symmetric matrix); a member nobody claimed passes with no index SNP
            ii = np.flatnonzero(is_index)
            assert not (P[np.ix_(ii, ii)] & (rank[ii][:, None] < rank[ii][None, :])).any()
            if not name.startswith("banded"):
                assert not P[np.ix_(ii, ii)].any()
            left = np.flatnonzero(member & (idx < 0))
            assert not P[np.ix_(ii, left)].any()


@pytest.mark.parametrize("low_memory", [False, True])
def test_the_pass_test_is_greater_or_equal(low_memory):
    """Integer entries k with dq_scale = 1 / 16 and r2 = (k0 / 16)^2: the threshold on the stored element is k0^2 exactly, an
    entry of +-k0 passes, one of +-(k0 - 1) does not."""
    k0 = 9
    for dt in (np.int8, np.int16, np.int32, np.int64, np.float32, np.float64):
        sk = syn.make_ld((40, 7), low_memory=low_memory, ld_dtype=np.float32, data=False)
        lb, ip = sk.ld_left_bound, sk.ld_indptr
        rng = np.random.default_rng(3)
        ints = rng.choice(np.array([k0, -k0, k0 - 1, 1 - k0]), int(ip[-1]))
        if not low_memory:                          # (a symmetric matrix: mirror the upper triangle, block by block)
            o = 0
            for b in (40, 7):
                K = np.triu(ints[o:o + b * b].reshape(b, b), 1)
                ints[o:o + b * b] = (K + K.T + 16 * np.eye(b, dtype=K.dtype)).ravel()
                o += b * b
        floating = np.issubdtype(dt, np.floating)
        data = (ints / 16.0).astype(dt) if floating else ints.astype(dt)
        dq = 1.0 if floating else 1.0 / 16.0
        X, E = dense_entries(lb, ip, ints, low_memory)
        order = np.arange(47)
        got = clump_host(lb, ip, data, low_memory, order, (k0 / 16.0) ** 2, None, dq)
        want = brute_force(X, E, order, [float(k0 * k0)], None)[:, 0]
        assert np.array_equal(got, want)
        strict = brute_force(X, E, order, [float(k0 * k0) + 0.5], None)[:, 0]
        assert np.array_equal(strict, np.arange(47)) and np.any(got != strict)


def test_clump_order():
    chisq = np.array([3.0, np.nan, 7.0, 3.0, 0.5, 7.0, 0.0, np.inf])
    assert clump_order(chisq).tolist() == [7, 2, 5, 0, 3, 4, 6]
    assert clump_order(chisq, 3.0).tolist() == [7, 2, 5, 0, 3]
    assert clump_order(chisq, 3.5).tolist() == [7, 2, 5]
    assert clump_order(chisq, 100.0).tolist() == [7] and clump_order(chisq[:7], 100.0).shape == (0,)
    assert clump_order(chisq).dtype == np.int32


def test_prefix_property():
    """A SNP's fate depends only on the SNPs in front of it: the index SNPs above a cut-off of a clumping over a longer order
    are the index SNPs of the clumping of the order cut there."""
    for name, lb, ip, data, low_memory, dq in _cases():
        m = lb.shape[0]
        chisq = chisq_draw(m, 10)
        full = clump_host(lb, ip, data, low_memory, clump_order(chisq), R2, None, dq)
        is_index = full == np.arange(m)[:, None]
        for cut in (0.5, 2.0, 6.0):
            part = clump_host(lb, ip, data, low_memory, clump_order(chisq, cut), R2, None, dq)
            assert np.array_equal(part == np.arange(m)[:, None], is_index & (chisq >= cut)[:, None]), (name, cut)
            # ... and what they claimed among the SNPs of the shorter order is the same
            assert np.array_equal(part[chisq >= cut], full[chisq >= cut])


def test_refusals():
    lb, ip, data = np.zeros(3, np.int32), np.arange(0, 10, 3), np.ones(9, np.float32)
    for kw in (dict(order=[0, 0]), dict(order=[3]), dict(order=[-1]), dict(order=[0], member=[0, 1, 1]),
               dict(order=[0], r2=-0.1), dict(order=[0], r2=np.nan), dict(order=[0], r2=[0.1] * 33), dict(order=[0], r2=[]),
               dict(order=[0], dq_scale=0.0), dict(order=[0], dq_scale=np.inf), dict(order=[0], member=[1, 1])):
        args = dict(dict(r2=0.1, member=None, dq_scale=1.0), **kw)
        with pytest.raises(ValueError):
            clump_host(lb, ip, data, False, np.asarray(args["order"], dtype=np.int64), args["r2"], args["member"], args["dq_scale"])
