"""Host references of the genotype scoring (include/viprs_hip.h, `viprs_genotypes_score`).

* `replay`        THE ORDER of the header executed in NumPy: vectorised over samples and columns, a loop over the SNPs;
                  ``acc = (acc + (B[j, c] * D[j, code])).astype(T)`` per chunk of L SNPs, then a double sum over the chunks.
                  NumPy rounds every float32 operation once, so this IS the definition on the host: the device is compared
                  with ``==``.
* `exact_int`     the scores of integer effects and integer dose tables as an int64 matrix product.
* `abs_terms`     S[i, c] = sum_j |B[j, c] D[j, code]| in float64, what the rounding bound scales with.
* `random_case`   packed rows with a chosen missing rate, monomorphic SNPs, all-missing SNPs and random trailing bits.
"""
import numpy as np

from viprs_amd.genotypes import ADDITIVE, SCORE_CHUNK, score_host
from viprs_amd.io.plink_bed import pack_codes, unpack_codes

L = SCORE_CHUNK


def _table(D, m, T):
    if D is None:
        return np.broadcast_to(np.array(ADDITIVE, dtype=T), (m, 4))
    return np.asarray(D, dtype=T).reshape(m, 4)


def replay(packed, n, B, D, T):
    """-> (n, n_cols) scores in T, in the order of the header."""
    T = np.dtype(T).type
    codes = unpack_codes(packed, n).astype(np.intp)
    m = codes.shape[0]
    B = np.asarray(B, dtype=T).reshape(m, -1)
    Dm = _table(D, m, T)
    total = np.zeros((n, B.shape[1]), dtype=np.float64)
    for j0 in range(0, m, L):
        acc = np.zeros((n, B.shape[1]), dtype=T)
        for j in range(j0, min(j0 + L, m)):
            dose = Dm[j][codes[j]]                              # (n,) in T
            term = dose[:, None] * B[j][None, :]                # one rounded multiply
            acc = acc + term                                    # one rounded addition
            assert acc.dtype == T
        total = total + acc.astype(np.float64)
    return total.astype(T)


def exact_int(packed, n, B, D=None):
    """-> (n, n_cols) int64 scores of integer B and integer D."""
    codes = unpack_codes(packed, n).astype(np.intp)
    m = codes.shape[0]
    Bi = np.asarray(B).reshape(m, -1).astype(np.int64)
    Di = np.broadcast_to(np.array(ADDITIVE, dtype=np.int64), (m, 4)) if D is None else np.asarray(D).astype(np.int64)
    X = np.take_along_axis(Di, codes, axis=1)                   # (m, n)
    return X.T @ Bi


def abs_terms(packed, n, B, D=None):
    m = packed.shape[0]
    return score_host(packed, n, np.abs(np.asarray(B, dtype=np.float64).reshape(m, -1)),
                      np.abs(np.asarray(_table(D, m, np.float64))))


def rounding_bound(packed, n, B, D, T):
    """The header's bound: 1.001 (L + 2) u_T S + n_chunks 2^-53 S."""
    u = 2.0 ** -24 if np.dtype(T) == np.float32 else 2.0 ** -53
    S = abs_terms(packed, n, B, D)
    n_chunks = -(-packed.shape[0] // L)
    return 1.001 * (L + 2) * u * S + n_chunks * 2.0 ** -53 * S


def random_codes(rng, n, m, missing=0.1, special=True):
    """(m, n) codes: allele frequency per SNP uniform in (0.05, 0.95), `missing` of the entries missing; with `special` a
    monomorphic SNP and an all-missing SNP where there is room."""
    f = rng.uniform(0.05, 0.95, size=(m, 1))
    copies = (rng.random((m, n)) < f).astype(np.int64) + (rng.random((m, n)) < f)
    codes = np.array([3, 2, 0], dtype=np.uint8)[copies]
    codes[rng.random((m, n)) < missing] = 1
    if special and m >= 3:
        codes[m // 3] = 0                                       # monomorphic
        codes[(2 * m) // 3] = 1                                 # every sample missing
    if special and m >= 7:
        codes[m // 7] = 3
    return codes


def random_case(rng, n, m, missing=0.1, special=True):
    """-> (packed rows with random trailing bits, codes)."""
    codes = random_codes(rng, n, m, missing, special)
    return pack_codes(codes, rng.integers(0, 256, size=m).astype(np.uint8)), codes


def other_trailing_bits(rng, codes):
    return pack_codes(codes, rng.integers(0, 256, size=codes.shape[0]).astype(np.uint8))


def first_difference(got, want):
    """None when the arrays are equal bit for bit, else a message with the first (row, column) that differs."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(got.reshape(got.shape[0], -1) != want.reshape(want.shape[0], -1))
    if bad.shape[0] == 0:
        return None
    i, c = (int(v) for v in bad[0])
    g, w = got.reshape(got.shape[0], -1)[i, c], want.reshape(want.shape[0], -1)[i, c]
    return f"{bad.shape[0]} of {got.size} entries differ; first at sample {i}, column {c}: got {g!r}, expected {w!r}"
