"""A host replay of the order `include/viprs_hip.h` fixes for `viprs_genotypes_class_sums`, written from the header's text and
independently of viprs_amd/genotypes.py: the 64 slot chains, then the xor butterfly on a 64-vector.  NumPy float64 additions
are IEEE additions with one rounding each, the device's `__dadd_rn`.  Plus the exact value by `math.fsum`, the header's
rounding bound, and the tolerance the association statistics inherit from it."""
import math

import numpy as np

from viprs_amd.io.plink_bed import pack_codes, unpack_codes

SLOTS = 64                               # VIPRS_CLASS_SUM_SLOTS
CODES = (0, 2, 3)                        # the code of class k: two copies of A1, one, none
U = 2.0 ** -53


def terms(packed, n, Y):
    """t[j, k, i, c] of the header: Y[i, c] where sample i of SNP j is of class k, +0.0 elsewhere."""
    codes = unpack_codes(packed, n)
    Y2 = np.asarray(Y, dtype=np.float64).reshape(n, -1)
    is_k = np.stack([codes == code for code in CODES], axis=1)           # (m, 3, n)
    return np.where(is_k[:, :, :, None], Y2[None, None, :, :], 0.0)


def slot_chains(t):
    """P[..., s, c]: the samples of slot s = (i >> 4) & 63 added in ascending i, from +0.  `t`: (m, 3, n, n_cols)."""
    m, _, n, n_cols = t.shape
    rounds = -(-n // 1024)
    padded = np.zeros((m, 3, rounds * 1024, n_cols))
    padded[:, :, :n] = t
    by_slot = padded.reshape(m, 3, rounds, SLOTS, 16, n_cols)            # sample i = 1024 round + 16 slot + q
    P = np.zeros((m, 3, SLOTS, n_cols))
    for r in range(rounds):
        for q in range(16):
            P = P + by_slot[:, :, r, :, q, :]
    return P


def butterfly(P):
    """for d in 32 .. 1: P[s] <- P[s] + P[s ^ d], all slots at once.  -> the 64 values per output (all equal)."""
    s = np.arange(SLOTS)
    for d in (32, 16, 8, 4, 2, 1):
        P = P + P[:, :, s ^ d, :]
    return P


def replay(packed, n, Y):
    """(m, 3, n_cols) float64: what the device must give, bit for bit."""
    if n == 0:
        return np.zeros((packed.shape[0], 3, np.asarray(Y).reshape(0, -1).shape[1] if np.ndim(Y) == 2 else 1))
    return butterfly(slot_chains(terms(packed, n, Y)))[:, :, 0, :]


def ascending(packed, n, Y):
    """The plain sum in ascending sample order: another order, for telling the two apart."""
    t = terms(packed, n, Y)
    out = np.zeros(t.shape[:2] + t.shape[3:])
    for i in range(n):
        out = out + t[:, :, i, :]
    return out


def exact(packed, n, Y):
    """The correctly rounded sums (`math.fsum`)."""
    t = terms(packed, n, Y)
    out = np.zeros(t.shape[:2] + t.shape[3:])
    for idx in np.ndindex(*out.shape):
        out[idx] = math.fsum(t[idx[0], idx[1], :, idx[2]])
    return out


def bound(packed, n, Y):
    """The header's bound (16 ceil(n / 1024) + 6) 2^-53 sum|t| per output, as it stands: the longest chain has one addition
    fewer than it counts (the first one adds to +0, exactly), which covers `fsum`'s own rounding and the second-order terms."""
    return (16 * -(-n // 1024) + 6) * U * np.abs(terms(packed, n, Y)).sum(axis=2)


def random_codes(rng, m, n, missing=0.1):
    freq = rng.uniform(0.1, 0.9, size=(m, 1))
    dose = (rng.random((m, n)) < freq).astype(np.int64) + (rng.random((m, n)) < freq)
    codes = np.array([3, 2, 0], dtype=np.uint8)[dose]
    if missing:
        codes[rng.random((m, n)) < missing] = 1
    return codes


def random_case(rng, m, n, missing=0.1):
    """(packed rows with random trailing bits, codes)."""
    codes = random_codes(rng, m, n, missing)
    return pack_codes(codes, trailing_bits=rng.integers(0, 256, m)), codes


def association_rtol(n):
    """Relative tolerance of BETA, SE, R against an independent double evaluation (np.corrcoef, np.linalg.lstsq) for a SNP
    whose dose variance and |correlation| are not tiny (the tests' data: MAF >= 0.1, the phenotype carries each tested
    SNP's effect or is checked with an absolute tolerance): both sides sum n terms (relative error <= n u each, sequential
    or pairwise), the centred moments cxx, cyy, cxy combine three such sums whose cancellation is bounded because y is
    centred first and var(x) / mean(x^2) >= 0.05 at MAF >= 0.1 (a factor <= 20), and a quotient and a square root add a
    few u.  64 n u covers 2 sides x 20 x (n u) with room for the least-squares solve's own conditioning."""
    return 64.0 * max(n, 16) * U
