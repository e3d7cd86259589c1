"""Genotypes on the device: packed PLINK .bed rows, per-SNP code counts, dose tables and polygenic scores.

The reference turns posterior effect sizes into scores through magenpy and plink2 (``BayesPRSModel.predict`` ->
``GWADataLoader.predict``); neither is part of the reference tree, so nothing here claims parity with them.  The definition
is stated in full in ``include/viprs_hip.h`` (viprs_genotypes_*):

    score[i, c] = sum_j B[j, c] * D[j, code(i, j)]

with ``code`` the 2-bit .bed code (0 = two copies of A1, 1 = missing, 2 = one copy, 3 = no copy) and ``D`` a per-SNP dose
table indexed by the code.  Everything a user means by "additive", "mean-imputed", "standardised" or "alleles swapped" is a
dose table, built here on the host in double from the exact counts and rounded once to the scoring precision.

* ``score_host``         NumPy float64 straight from the definition: the CPU fallback and the base of the tests;
* ``dose_table``         the tables from the counts;
* ``DeviceGenotypes``    the rows on a HIP device (`viprs_genotypes_*`): ``counts``, ``dose_table``, ``score``;
* ``HostGenotypes``      the same surface over `score_host` (what a loader uses when no device is visible);
* ``ld_host``            the LD matrix of the rows from the definition (`viprs_genotypes_ld`), ``ld_windows`` the windows of
                         an estimator; both classes have ``ld()``;
* ``class_sums_host``    per SNP and genotype class (two / one / no copy of A1) the sums of the columns of ``Y`` over the
                         samples of the class (`viprs_genotypes_class_sums`); both classes have ``class_sums()`` and, built on
                         it and the counts alone, ``association()``: the per-SNP linear regression of a GWAS;
* ``open_genotypes``     a loader's genotype entry -- one of the two above, ``(packed_rows, n)`` or a .bed prefix -- opened;
* ``model_predict``      ``predict()`` of the model classes.
"""
import ctypes

import numpy as np

from .io.plink_bed import bytes_per_row, read_bed, unpack_codes

SCORE_CHUNK = 1024                       # VIPRS_SCORE_CHUNK (include/viprs_hip.h): part of the definition of the device sum
ADDITIVE = (2.0, 0.0, 1.0, 0.0)          # the dose table of a NULL `dose`
DOSE_MODES = ("mean", "zero", "standardize")
_HOST_SLAB = 2048                        # SNPs `score_host` unpacks at a time


def _check_rows(packed_rows, n):
    n = int(n)
    if n < 0:
        raise ValueError("n must not be negative")
    p = packed_rows if isinstance(packed_rows, np.ndarray) else np.asarray(packed_rows)
    if p.dtype != np.uint8 or p.ndim != 2 or p.shape[1] != bytes_per_row(n):
        raise ValueError(f"packed rows: an (m, {bytes_per_row(n)}) uint8 array for n = {n}, got {p.dtype} {p.shape}")
    return p, n


def counts_host(packed_rows, n):
    """(m, 4) int64: the samples ``i < n`` of every SNP per code."""
    p, n = _check_rows(packed_rows, n)
    out = np.zeros((p.shape[0], 4), dtype=np.int64)
    for a in range(0, p.shape[0], _HOST_SLAB):
        codes = unpack_codes(p[a:a + _HOST_SLAB], n)
        for k in range(4):
            out[a:a + _HOST_SLAB, k] = (codes == k).sum(axis=1)
    return out


def dose_table(counts, mode="mean", swapped=None, dtype=np.float32):
    """The (m, 4) dose table of `mode` from the exact (m, 4) code counts, computed in double and rounded once to `dtype`.

    ``"zero"``         additive, missing = 0: ``{2, 0, 1, 0}``
    ``"mean"``         mean-imputed: ``{2, mu, 1, 0}``, ``mu = (2 c0 + c2) / (c0 + c2 + c3)`` (0 when every sample is missing)
    ``"standardize"``  ``{(2 - mu) / s, 0, (1 - mu) / s, -mu / s}``, ``s`` the population standard deviation of the non-missing
                       doses; a monomorphic SNP (and one without any sample) gets an all-zero table
    `swapped`: None or an (m,) boolean mask of the SNPs whose A1 / A2 are exchanged relative to the effect sizes: entries 0
    and 3 change places and ``mu' = 2 - mu``.  Exact -- not a sign flip of the effect, which would change every score by a
    constant."""
    if mode not in DOSE_MODES:
        raise ValueError(f"dose mode {mode!r}: one of {DOSE_MODES}")
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 4)
    m = c.shape[0]
    sw = np.zeros(m, dtype=bool) if swapped is None else np.asarray(swapped, dtype=bool).reshape(m)
    # copies of the allele the effect sizes count: A1, or A2 where swapped
    c_two = np.where(sw, c[:, 3], c[:, 0]).astype(np.float64)
    c_one = c[:, 2].astype(np.float64)
    c_none = np.where(sw, c[:, 0], c[:, 3]).astype(np.float64)
    nn = c_two + c_one + c_none
    some = nn > 0
    mu = np.where(some, (2.0 * c_two + c_one) / np.where(some, nn, 1.0), 0.0)
    D = np.zeros((m, 4), dtype=np.float64)              # columns: dose of two copies, missing, one copy, no copy
    if mode == "zero":
        D[:, 0], D[:, 2] = 2.0, 1.0
    elif mode == "mean":
        D[:, 0], D[:, 1], D[:, 2] = 2.0, mu, 1.0
    else:
        poly = some & (np.maximum(np.maximum(c_two, c_one), c_none) < nn)
        var = (c_two * (2.0 - mu) ** 2 + c_one * (1.0 - mu) ** 2 + c_none * mu ** 2) / np.where(some, nn, 1.0)
        sd = np.sqrt(np.where(poly, var, 1.0))
        D[:, 0], D[:, 2], D[:, 3] = (2.0 - mu) / sd, (1.0 - mu) / sd, -mu / sd
        D[~poly] = 0.0
    D[sw] = D[sw][:, [3, 1, 2, 0]]
    return np.ascontiguousarray(D.astype(dtype))


def score_host(packed_rows, n, B, D=None):
    """``score[i, c] = sum_j B[j, c] D[j, code(i, j)]`` in float64: ``(n,)`` for ``(m,)`` effects, ``(n, n_cols)`` for
    ``(m, n_cols)``.  `D`: an (m, 4) dose table or None (``{2, 0, 1, 0}``).  Nothing depends on the trailing bits of a row."""
    p, n = _check_rows(packed_rows, n)
    B = np.asarray(B)
    m = p.shape[0]
    B2 = B.reshape(m, B.shape[1] if B.ndim == 2 else 1).astype(np.float64)
    Dm = np.broadcast_to(np.array(ADDITIVE), (m, 4)) if D is None else np.asarray(D, dtype=np.float64).reshape(m, 4)
    out = np.zeros((n, B2.shape[1]), dtype=np.float64)
    for a in range(0, m, _HOST_SLAB):
        codes = unpack_codes(p[a:a + _HOST_SLAB], n)
        X = np.take_along_axis(Dm[a:a + _HOST_SLAB], codes.astype(np.intp), axis=1)       # (slab, n) doses
        out += X.T @ B2[a:a + _HOST_SLAB]
    return out[:, 0] if B.ndim == 1 else out


# ---- LD from genotypes (include/viprs_hip.h, viprs_genotypes_ld) ----------------------------------------------------------
LD_MAX_SAMPLES = 1 << 19                 # 4 n^3 4 < 2^63: the numerator stays inside int64
LD_DTYPES = {np.dtype(np.int8): 127.0, np.dtype(np.int16): 32767.0, np.dtype(np.float32): None, np.dtype(np.float64): None}
LD_ESTIMATORS = ("sample", "windowed", "windowed_bp", "block")
_LD_TILE = 64                            # kLdTile (viprs_amd/csrc/geno_ld.h): the rows of a device call are whole tiles
_LD_HOST_SLAB = 256                      # rows `ld_host` computes at a time


def _ld_dtype(dtype):
    T = np.dtype(dtype)
    if T not in LD_DTYPES:
        raise ValueError(f"LD dtype: int8, int16, float32 or float64, got {T}")
    return T


def ld_dq_scale(dtype):
    """What turns a stored element into a correlation: 1 / 127, 1 / 32767, or 1 for the float types."""
    q = LD_DTYPES[_ld_dtype(dtype)]
    return 1.0 if q is None else 1.0 / q


def ld_stats(counts):
    """``(nn, a, w)`` of the definition from the exact (m, 4) code counts: non-missing samples and dose sums (int64), and
    ``w = sqrt((double)(nn d))``, ``d = nn q - a^2``, ``q = 4 c0 + c2`` (float64; 0 for a monomorphic or all-missing SNP)."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 4)
    nn = c[:, 0] + c[:, 2] + c[:, 3]
    a = 2 * c[:, 0] + c[:, 2]
    q = 4 * c[:, 0] + c[:, 2]
    d = nn * q - a * a
    return nn, a, np.sqrt((nn * d).astype(np.float64))


def _check_right_end(right_end, m):
    """The windows of the compact upper store as (m,) int64: ``j + 1 <= right_end[j] <= m``, non-decreasing."""
    re = np.ascontiguousarray(right_end, dtype=np.int64)
    if re.shape != (int(m),):
        raise ValueError(f"right_end: ({int(m)},), got {re.shape}")
    if m and (np.any(re < np.arange(1, m + 1)) or np.any(re > m)):
        raise ValueError("right_end[j] must lie in [j + 1, m]")
    if m and np.any(np.diff(re) < 0):
        raise ValueError("right_end must be non-decreasing")
    return re


def ld_indptr(right_end):
    """Row pointers of the compact upper store: ``indptr[j + 1] - indptr[j] = right_end[j] - j - 1`` (no diagonal)."""
    re = np.asarray(right_end, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(re - np.arange(1, re.shape[0] + 1))]).astype(np.int64)


def ld_windows(estimator, m):
    """``right_end`` (m,) int64 of an LD estimator:

    ``("sample",)``                            every pair
    ``("windowed", n_snps)``                   the `n_snps` SNPs that follow
    ``("windowed_bp", distance, positions)``   the SNPs within `distance` base pairs; `positions`: the .bim's POS, sorted
                                               (SNPs at one position are inside each other's window)
    ``("block", boundaries)``                  block starts (0 and m may be left out); a row ends with its block"""
    m = int(m)
    if isinstance(estimator, str):
        estimator = (estimator,)
    kind = estimator[0]
    j = np.arange(m, dtype=np.int64)
    if kind == "sample" and len(estimator) == 1:
        re = np.full(m, m, dtype=np.int64)
    elif kind == "windowed" and len(estimator) == 2:
        k = int(estimator[1])
        if k < 0:
            raise ValueError("windowed: the SNP count must not be negative")
        re = np.minimum(j + 1 + k, m)
    elif kind == "windowed_bp" and len(estimator) == 3:
        pos = np.asarray(estimator[2], dtype=np.int64)
        if pos.shape != (m,):
            raise ValueError(f"windowed_bp: ({m},) positions, got {pos.shape}")
        if np.any(np.diff(pos) < 0):
            raise ValueError("windowed_bp: the positions must be sorted")
        if int(estimator[1]) < 0:
            raise ValueError("windowed_bp: the distance must not be negative")
        re = np.searchsorted(pos, pos + int(estimator[1]), side="right").astype(np.int64)
    elif kind == "block" and len(estimator) == 2:
        b = np.asarray(estimator[1], dtype=np.int64).reshape(-1)
        if b.size and (b.min() < 0 or b.max() > m):
            raise ValueError(f"block: boundaries must lie in [0, {m}]")
        b = np.unique(np.concatenate([[0], b, [m]]))
        re = b[np.searchsorted(b, j, side="right")] if m else np.zeros(0, dtype=np.int64)
    else:
        raise ValueError(f"LD estimator {estimator!r}: ('sample',), ('windowed', n_snps), "
                         "('windowed_bp', distance, positions) or ('block', boundaries)")
    return _check_right_end(re, m)


def _ld_planes(packed_rows, n):
    """(dose, presence) of the rows as float64 (k, n): integers, so that every product below is exact."""
    codes = unpack_codes(packed_rows, n)
    x = np.where(codes == 0, 2.0, np.where(codes == 2, 1.0, 0.0))
    return x, (codes != 1).astype(np.float64)


def ld_block_host(rows_i, rows_j, n, stats_i=None, stats_j=None):
    """``r`` (len(rows_i), len(rows_j)) float64 between two sets of packed rows, straight from the definition.  The four sums
    are float64 matrix products of small integers (every partial sum is an integer below 2^53, hence exact in any order),
    `num` is int64.  `stats_*`: ``ld_stats`` of the rows when the caller has them."""
    pi, n = _check_rows(rows_i, n)
    pj, _ = _check_rows(rows_j, n)
    if n > LD_MAX_SAMPLES:
        raise ValueError(f"n = {n} samples: LD needs n <= 2^19 = {LD_MAX_SAMPLES} (beyond it the numerator leaves int64)")
    nn_i, a_i, w_i = stats_i if stats_i is not None else ld_stats(counts_host(pi, n))
    nn_j, a_j, w_j = stats_j if stats_j is not None else ld_stats(counts_host(pj, n))
    xi, qi = _ld_planes(pi, n)
    xj, qj = _ld_planes(pj, n)
    S = np.rint(xi @ xj.T).astype(np.int64)
    U_ij = np.rint(xi @ qj.T).astype(np.int64)
    U_ji = np.rint(qi @ xj.T).astype(np.int64)
    N = np.rint(qi @ qj.T).astype(np.int64)
    num = ((nn_i[:, None] * nn_j[None, :]) * S - (nn_i[:, None] * a_j[None, :]) * U_ij
           - (a_i[:, None] * nn_j[None, :]) * U_ji + (a_i[:, None] * a_j[None, :]) * N)
    den = w_i[:, None] * w_j[None, :]
    live = den != 0.0                                  # (w >= 0 and finite: the product is 0 only when a factor is)
    return np.where(live, num.astype(np.float64) / np.where(live, den, 1.0), 0.0)


def _ld_quantize(r, dtype):
    """A float64 correlation as a stored element: itself, ``(float)r``, or ``rint(r max)`` clamped to ``+-max``."""
    T = _ld_dtype(dtype)
    q = LD_DTYPES[T]
    if q is None:
        return np.asarray(r, dtype=np.float64).astype(T)
    return np.clip(np.rint(np.asarray(r, dtype=np.float64) * q), -q, q).astype(T)


def ld_host(packed_rows, n, right_end, dtype=np.float32):
    """``(indptr, data)``: the LD of the rows inside the windows `right_end` as the compact upper store, in NumPy int64 and
    float64 from the definition in ``include/viprs_hip.h``.  The CPU fallback and the yardstick of the device kernels."""
    p, n = _check_rows(packed_rows, n)
    m = p.shape[0]
    T = _ld_dtype(dtype)
    if n > LD_MAX_SAMPLES:
        raise ValueError(f"n = {n} samples: LD needs n <= 2^19 = {LD_MAX_SAMPLES} (beyond it the numerator leaves int64)")
    re = _check_right_end(right_end, m)
    ip = ld_indptr(re)
    data = np.zeros(int(ip[-1]), dtype=T)
    nn, a, w = ld_stats(counts_host(p, n))
    for r0 in range(0, m, _LD_HOST_SLAB):
        r1 = min(m, r0 + _LD_HOST_SLAB)
        c1 = int(re[r1 - 1])
        if ip[r1] == ip[r0]:
            continue
        R = ld_block_host(p[r0:r1], p[r0 + 1:c1], n, (nn[r0:r1], a[r0:r1], w[r0:r1]),
                          (nn[r0 + 1:c1], a[r0 + 1:c1], w[r0 + 1:c1]))
        for j in range(r0, r1):
            data[ip[j]:ip[j + 1]] = _ld_quantize(R[j - r0, j - r0:int(re[j]) - r0 - 1], T)
    return ip, data


# ---- per-genotype-class column sums and the association test (include/viprs_hip.h, viprs_genotypes_class_sums) ------------
CLASS_SUM_SLOTS = 64                     # VIPRS_CLASS_SUM_SLOTS: part of the definition of the device sum
CLASS_CODES = (0, 2, 3)                  # the .bed code of class k = 0, 1, 2: two copies of A1, one, none
ASSOCIATION_FIELDS = ("N", "BETA", "SE", "Z", "R", "A1_FREQ")


def _check_columns(Y, n):
    """`Y` of `class_sums` as C-contiguous float64 (n, n_cols) -> (Y2, whether it was (n,))."""
    Y = np.asarray(Y)
    if Y.ndim not in (1, 2) or Y.shape[0] != n or (Y.ndim == 2 and Y.shape[1] < 1):
        raise ValueError(f"Y: ({n},) or ({n}, n_cols), got {Y.shape}")
    Y2 = np.ascontiguousarray(Y.reshape(n, Y.shape[1] if Y.ndim == 2 else 1), dtype=np.float64)
    if not np.all(np.isfinite(Y2)):
        raise ValueError("Y holds NaN or inf: class_sums needs finite values (`association` takes NaN as an unknown "
                         "phenotype and leaves those samples out)")
    return Y2, Y.ndim == 1


def class_sums_host(packed_rows, n, Y):
    """``sums[j, k, c] = sum of Y[i, c] over the samples i < n whose code at SNP j is CLASS_CODES[k]`` in float64: ``(m, 3)``
    for ``(n,)`` values, ``(m, 3, n_cols)`` for ``(n, n_cols)``.  Indicator planes times `Y`, in slabs of rows.  The CPU
    fallback: within the header's rounding bound of the device's sums, not bit-identical to them."""
    p, n = _check_rows(packed_rows, n)
    Y2, flat = _check_columns(Y, n)
    out = np.zeros((p.shape[0], 3, Y2.shape[1]), dtype=np.float64)
    for a in range(0, p.shape[0], _HOST_SLAB):
        codes = unpack_codes(p[a:a + _HOST_SLAB], n)
        for k, code in enumerate(CLASS_CODES):
            out[a:a + _HOST_SLAB, k] = (codes == code).astype(np.float64) @ Y2
    return out[:, :, 0] if flat else out


class _Genotypes:
    """What the two genotype classes share: everything that follows from the counts and the class sums."""

    n = m = 0

    def counts(self):
        raise NotImplementedError

    def class_sums(self, Y, max_bytes=1 << 30):
        """Per SNP and genotype class the column sums of `Y` (``(n,)`` or ``(n, n_cols)``, finite) over the samples of the
        class: ``(m, 3)`` or ``(m, 3, n_cols)`` float64, classes in the order two copies of A1, one, none; missing genotypes
        belong to no class.  On the device in the order `include/viprs_hip.h` defines, in row ranges whose output stays
        within `max_bytes` (a row at least)."""
        raise NotImplementedError

    def association(self, Y, keep=None):
        """The linear regression of every phenotype column on every SNP's dose of A1 over the complete pairs -- a GWAS without
        covariates (residualise the phenotype first) -- from `class_sums` and `counts` alone.  `Y`: ``(n,)`` or ``(n, T)``,
        NaN = unknown phenotype.  `keep`: None, or an ``(n,)`` / ``(n, T)`` boolean mask of the samples that take part (a
        training subset; K folds of one trait are K columns of one pass).  Per trait the host centres ``y`` by the mean of its
        kept, known samples and sums the columns ``[u, y u, (y u)^2]`` (``u`` the 0 / 1 mask; dropped when every sample takes
        part: the class counts are then the exact `counts`) per genotype class; with ``N_k, Y_k, Q_k`` those sums, in double:

            n = N_0 + N_1 + N_2,  Sx = 2 N_0 + N_1,  Sxx = 4 N_0 + N_1,  Sy = sum Y_k,  Syy = sum Q_k,  Sxy = 2 Y_0 + Y_1
            cxx = n Sxx - Sx^2,  cyy = n Syy - Sy^2,  cxy = n Sxy - Sx Sy

        -> dict of ``(m,)`` / ``(m, T)`` float64: ``N = n``, ``BETA = cxy / cxx`` (per copy of A1),
        ``SE = sqrt(max(cxx cyy - cxy^2, 0) / (n - 2)) / cxx``, ``Z = BETA / SE``, ``R = cxy / sqrt(cxx cyy)`` (the Pearson
        correlation: the standardised effect the models read), ``A1_FREQ = Sx / (2 n)``.  A SNP with ``n < 3``,
        ``cxx <= 0`` or ``cyy <= 0`` gets ``BETA = SE = Z = R = 0`` and its true ``N``.  No P-value."""
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim not in (1, 2) or Y.shape[0] != self.n or (Y.ndim == 2 and Y.shape[1] < 1):
            raise ValueError(f"phenotype: ({self.n},) or ({self.n}, T), got {Y.shape}")
        flat = Y.ndim == 1
        T = 1 if flat else Y.shape[1]
        Y2 = Y.reshape(self.n, T)
        if np.any(np.isinf(Y2)):
            raise ValueError("the phenotype holds inf (NaN marks an unknown phenotype)")
        u = np.isfinite(Y2)
        if keep is not None:
            k = np.asarray(keep)
            if k.dtype != np.bool_ or k.shape not in ((self.n,), (self.n, T)):
                raise ValueError(f"keep: a boolean mask of shape ({self.n},) or ({self.n}, {T}), got {k.dtype} {k.shape}")
            u = u & (k if k.ndim == 2 else k[:, None])
        n_u = u.sum(axis=0)
        mean = np.where(u, Y2, 0.0).sum(axis=0) / np.maximum(n_u, 1)
        yc = np.where(u, Y2 - mean, 0.0)
        everyone = u.all(axis=0) if self.n else np.ones(T, dtype=bool)
        cols, at = [], []
        for t in range(T):
            at.append(len(cols))
            if not everyone[t]:
                cols.append(u[:, t].astype(np.float64))
            cols += [yc[:, t], yc[:, t] * yc[:, t]]
        S = self.class_sums(np.stack(cols, axis=1)) if self.n else np.zeros((self.m, 3, len(cols)))
        out = {f: np.zeros((self.m, T), dtype=np.float64) for f in ASSOCIATION_FIELDS}
        exact = self.counts()[:, list(CLASS_CODES)].astype(np.float64) if np.any(everyone) else None
        for t in range(T):
            a = at[t]
            if everyone[t]:
                Nk = exact
            else:
                Nk, a = S[:, :, a], a + 1
            Yk, Qk = S[:, :, a], S[:, :, a + 1]
            n = Nk.sum(axis=1)
            Sx, Sxx = 2.0 * Nk[:, 0] + Nk[:, 1], 4.0 * Nk[:, 0] + Nk[:, 1]
            Sy, Syy, Sxy = Yk.sum(axis=1), Qk.sum(axis=1), 2.0 * Yk[:, 0] + Yk[:, 1]
            cxx, cyy, cxy = n * Sxx - Sx * Sx, n * Syy - Sy * Sy, n * Sxy - Sx * Sy
            live = (n >= 3) & (cxx > 0) & (cyy > 0)
            sxx, syy, dof = np.where(live, cxx, 1.0), np.where(live, cyy, 1.0), np.where(live, n - 2.0, 1.0)
            beta = np.where(live, cxy / sxx, 0.0)
            se = np.where(live, np.sqrt(np.maximum(sxx * syy - cxy * cxy, 0.0) / dof) / sxx, 0.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                z = np.where(live, beta / se, 0.0)             # (a perfect fit: SE = 0 and Z = +-inf)
            out["N"][:, t] = n
            out["BETA"][:, t], out["SE"][:, t], out["Z"][:, t] = beta, se, z
            out["R"][:, t] = np.where(live, cxy / np.sqrt(sxx * syy), 0.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                out["A1_FREQ"][:, t] = np.where(n > 0, Sx / (2.0 * n), np.nan)
        return {f: (v[:, 0] if flat else v) for f, v in out.items()}

    def _right_end(self, window):
        """`window` of `ld`: None (every pair), an estimator of `ld_windows`, or the (m,) right ends themselves."""
        if window is None:
            return ld_windows(("sample",), self.m)
        if isinstance(window, str) or (isinstance(window, tuple) and window and isinstance(window[0], str)):
            return ld_windows(window, self.m)
        return _check_right_end(window, self.m)

    def ld(self, window=None, dtype=np.float32, max_bytes=1 << 30):
        """``(indptr, data)``: the LD matrix of the SNPs inside `window` as the compact upper store in `dtype` (int8, int16,
        float32, float64; `ld_dq_scale` turns an element into a correlation).  On the device the rows are computed in ranges
        of at most `max_bytes` of the store (a tile row of 64 SNPs at least)."""
        raise NotImplementedError

    def allele_frequency(self):
        """Frequency of A1 among the non-missing samples, (m,) float64 (NaN where every sample is missing)."""
        c = self.counts().astype(np.float64)
        nn = c[:, 0] + c[:, 2] + c[:, 3]
        with np.errstate(invalid="ignore", divide="ignore"):
            return (2.0 * c[:, 0] + c[:, 2]) / (2.0 * nn)

    def dose_table(self, mode="mean", swapped=None, dtype=np.float32):
        return dose_table(self.counts(), mode, swapped, dtype)

    def _score_args(self, B, dose, float_precision):
        B = np.asarray(B)
        if float_precision is None:
            float_precision = B.dtype if B.dtype in (np.float32, np.float64) else np.float32
        T = np.dtype(float_precision)
        if T not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError(f"float_precision: float32 or float64, got {T}")
        if B.ndim not in (1, 2) or B.shape[0] != self.m or (B.ndim == 2 and B.shape[1] < 1):
            raise ValueError(f"effects: ({self.m},) or ({self.m}, n_cols), got {B.shape}")
        B2 = np.ascontiguousarray(B.reshape(self.m, B.shape[1] if B.ndim == 2 else 1), dtype=T)
        if dose is None or isinstance(dose, str):
            D = None if dose is None else self.dose_table(dose, dtype=T)
        else:
            D = np.ascontiguousarray(dose, dtype=T)
            if D.shape != (self.m, 4):
                raise ValueError(f"dose table: ({self.m}, 4), got {D.shape}")
        return B2, D, T, B.ndim == 1


class HostGenotypes(_Genotypes):
    """`DeviceGenotypes`' surface on the host (`counts_host`, `score_host`): scores are float64 sums rounded to the asked
    precision."""

    def __init__(self, packed_rows, n):
        self.rows, self.n = _check_rows(packed_rows, n)
        self.m = int(self.rows.shape[0])
        self._counts = None

    def counts(self):
        if self._counts is None:
            self._counts = counts_host(self.rows, self.n)
        return self._counts

    def score(self, B, dose=None, float_precision=None):
        B2, D, T, flat = self._score_args(B, dose, float_precision)
        s = score_host(self.rows, self.n, B2, D).astype(T)
        return s[:, 0] if flat else s

    def ld(self, window=None, dtype=np.float32, max_bytes=1 << 30):
        return ld_host(self.rows, self.n, self._right_end(window), dtype)

    def class_sums(self, Y, max_bytes=1 << 30):
        return class_sums_host(self.rows, self.n, Y)

    def close(self):
        pass


class DeviceGenotypes(_Genotypes):
    """Packed .bed rows of one chromosome (or any set of SNPs) resident on a HIP device.

    `packed_rows`: (m, ceil(n / 4)) uint8, e.g. `read_bed`'s memory map -- uploaded in slices of `slice_bytes`, never
    unpacked on the host."""

    def __init__(self, packed_rows, n, device=0, slice_bytes=256 << 20):
        from . import _lib as L
        self._L = L
        rows, self.n = _check_rows(packed_rows, n)
        self.m = int(rows.shape[0])
        self.device = int(device)
        self._h = ctypes.c_void_p()
        self._counts = None
        L.check(L.lib.viprs_genotypes_create(ctypes.byref(self._h), self.n, self.m, self.device))
        bpr = bytes_per_row(self.n)
        step = max(1, int(slice_bytes) // max(bpr, 1))
        for a in range(0, self.m if bpr else 0, step):
            part = np.ascontiguousarray(rows[a:a + step])
            L.check(L.lib.viprs_genotypes_upload_rows(self._h, a, part.shape[0], part.ctypes.data_as(ctypes.c_void_p)))

    @property
    def handle(self):
        if not self._h:
            raise ValueError("DeviceGenotypes is closed")
        return self._h

    def counts(self):
        """(m, 4) int64 code counts of the samples ``i < n`` (`viprs_genotypes_counts`; kept after the first call)."""
        if self._counts is None:
            c = np.zeros((self.m, 4), dtype=np.int64)
            self._L.check(self._L.lib.viprs_genotypes_counts(self.handle, c.ctypes.data_as(ctypes.c_void_p)))
            self._counts = c
        return self._counts

    def score(self, B, dose=None, float_precision=None):
        """Scores of the ``(m,)`` / ``(m, n_cols)`` effects `B`: ``(n,)`` / ``(n, n_cols)`` in `float_precision` (default:
        B's own when it is float32 / float64, else float32), in the order `include/viprs_hip.h` defines.  `dose`: None (the
        additive table ``{2, 0, 1, 0}``, no table is uploaded), a mode of `dose_table`, or an (m, 4) table."""
        B2, D, T, flat = self._score_args(B, dose, float_precision)
        out = np.zeros((self.n, B2.shape[1]), dtype=T)
        L = self._L
        L.check(L.lib.viprs_genotypes_score(self.handle, L.F32 if T == np.float32 else L.F64, B2.shape[1],
                                            B2.ctypes.data_as(ctypes.c_void_p),
                                            None if D is None else D.ctypes.data_as(ctypes.c_void_p),
                                            out.ctypes.data_as(ctypes.c_void_p)))
        return out[:, 0] if flat else out

    def ld_rows(self, row0, row1, right_end, w, out):
        """Rows ``[row0, row1)`` of the compact upper store of the windows `right_end` into `out` (`viprs_genotypes_ld`): a
        C-contiguous array of an LD dtype with ``indptr[row1] - indptr[row0]`` elements.  `w`: ``ld_stats(counts)[2]``."""
        L = self._L
        code = {np.dtype(np.int8): L.LD_I8, np.dtype(np.int16): L.LD_I16, np.dtype(np.float32): L.LD_F32,
                np.dtype(np.float64): L.LD_F64}[_ld_dtype(out.dtype)]
        re = np.ascontiguousarray(right_end, dtype=np.int64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        if re.shape != (self.m,) or w.shape != (self.m,):
            raise ValueError(f"right_end and w: ({self.m},) each")
        if not 0 <= row0 <= row1 <= self.m:
            raise ValueError(f"rows [{row0}, {row1}) of {self.m}")
        ip = ld_indptr(re)
        if not out.flags.c_contiguous or not out.flags.writeable or out.size != int(ip[row1] - ip[row0]):
            raise ValueError(f"out: a writeable C-contiguous array of {int(ip[row1] - ip[row0])} elements")
        spare = np.zeros(1, dtype=out.dtype)           # (an empty array may have no address to hand over)
        L.check(L.lib.viprs_genotypes_ld(self.handle, int(row0), int(row1), re.ctypes.data_as(ctypes.c_void_p),
                                         w.ctypes.data_as(ctypes.c_void_p), code,
                                         (out if out.size else spare).ctypes.data_as(ctypes.c_void_p)))
        return out

    def ld(self, window=None, dtype=np.float32, max_bytes=1 << 30):
        T = _ld_dtype(dtype)
        re = self._right_end(window)
        if self.n > LD_MAX_SAMPLES:
            raise ValueError(f"n = {self.n} samples: LD needs n <= 2^19 = {LD_MAX_SAMPLES} (beyond it the numerator "
                             "leaves int64)")
        ip = ld_indptr(re)
        data = np.zeros(int(ip[-1]), dtype=T)
        w = ld_stats(self.counts())[2]
        budget = max(int(max_bytes) // T.itemsize, 1)
        r0 = 0
        while r0 < self.m:                             # whole tile rows while they fit the budget, one at least
            r1 = min(self.m, r0 + _LD_TILE)
            while r1 < self.m and ip[min(self.m, r1 + _LD_TILE)] - ip[r0] <= budget:
                r1 = min(self.m, r1 + _LD_TILE)
            if ip[r1] > ip[r0]:
                self.ld_rows(r0, r1, re, w, data[ip[r0]:ip[r1]])
            r0 = r1
        return ip, data

    def class_sums(self, Y, max_bytes=1 << 30):
        Y2, flat = _check_columns(Y, self.n)
        n_cols = Y2.shape[1]
        out = np.zeros((self.m, 3, n_cols), dtype=np.float64)
        step = max(1, int(max_bytes) // (3 * n_cols * 8))
        L = self._L
        spare = np.zeros(1, dtype=np.float64)          # (an empty array may have no address to hand over)
        for r0 in range(0, self.m, step):
            r1 = min(self.m, r0 + step)
            L.check(L.lib.viprs_genotypes_class_sums(self.handle, r0, r1, n_cols,
                                                     (Y2 if Y2.size else spare).ctypes.data_as(ctypes.c_void_p),
                                                     out[r0:r1].ctypes.data_as(ctypes.c_void_p)))
        return out[:, :, 0] if flat else out

    def last_class_sums_ms(self):
        """HIP-event time (ms) of the kernels of the last device call of `class_sums` on this object (one row range)."""
        ms = ctypes.c_double(0.0)
        self._L.check(self._L.lib.viprs_genotypes_last_class_sums_ms(self.handle, ctypes.byref(ms)))
        return ms.value

    def last_ld_ms(self):
        """HIP-event time (ms) of the kernels of the last device call of `ld` / `ld_rows` on this object."""
        ms = ctypes.c_double(0.0)
        self._L.check(self._L.lib.viprs_genotypes_last_ld_ms(self.handle, ctypes.byref(ms)))
        return ms.value

    def last_score_ms(self):
        """HIP-event time (ms) of the kernels of the last `score` on this object."""
        ms = ctypes.c_double(0.0)
        self._L.check(self._L.lib.viprs_genotypes_last_score_ms(self.handle, ctypes.byref(ms)))
        return ms.value

    def last_counts_ms(self):
        """HIP-event time (ms) of the counts kernel of the last device `counts` on this object (no download)."""
        ms = ctypes.c_double(0.0)
        self._L.check(self._L.lib.viprs_genotypes_last_counts_ms(self.handle, ctypes.byref(ms)))
        return ms.value

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.lib.viprs_genotypes_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def open_genotypes(entry, device=0):
    """A loader's genotype entry opened: -> ``(genotypes, owned, bed)``.  `entry`: a `DeviceGenotypes` / `HostGenotypes`
    (returned as it is), ``(packed_rows, n)``, or the prefix of a .bed / .bim / .fam triple.  New objects live on HIP device
    `device`, or on the host when no device is visible; `owned` says the caller closes them; `bed`: None or what `read_bed`
    returned for a prefix."""
    if isinstance(entry, _Genotypes):
        return entry, False, None
    bed = None
    if isinstance(entry, (str, bytes)) or hasattr(entry, "__fspath__"):
        bed = read_bed(entry)
        entry = bed[:2]
    rows, n = entry
    from . import _lib
    if _lib.device_count() < 1:
        return HostGenotypes(rows, n), True, bed
    return DeviceGenotypes(rows, n, device=device), True, bed


# ---- predict() of the model classes ---------------------------------------------------------------------------------------
def _align(model_table, test_table, beta, c):
    """Effects of the model's SNPs laid out over the test table's SNPs by SNP id: absent SNPs score 0, SNPs whose A1 / A2
    are exchanged are marked as swapped, any other allele pair is dropped.  -> (beta over the test SNPs, swapped mask)."""
    for t, who in ((model_table, "the model's loader"), (test_table, "the test loader")):
        if any(k not in t for k in ("SNP", "A1", "A2")):
            raise ValueError(f"chromosome {c}: the SNP table of {who} needs the columns SNP, A1 and A2")
    ids = np.asarray(model_table["SNP"], dtype=str)
    if ids.shape[0] != beta.shape[0]:
        raise ValueError(f"chromosome {c}: the model's SNP table has {ids.shape[0]} SNPs, its effects {beta.shape[0]}")
    t_ids = np.asarray(test_table["SNP"], dtype=str)
    for who, v in (("the model's loader", ids), ("the test loader", t_ids)):
        u, n_of = np.unique(v, return_counts=True)
        if np.any(n_of > 1):
            raise ValueError(f"chromosome {c}: the SNP table of {who} lists {u[n_of > 1][0]!r} more than once "
                             f"({int(np.sum(n_of > 1))} duplicated ids): the alignment by SNP id needs unique ids")
    where = {s: k for k, s in enumerate(ids)}
    at = np.array([where.get(s, -1) for s in t_ids], dtype=np.int64)
    found = at >= 0
    a1m, a2m = np.asarray(model_table["A1"], dtype=str)[at[found]], np.asarray(model_table["A2"], dtype=str)[at[found]]
    a1t, a2t = np.asarray(test_table["A1"], dtype=str)[found], np.asarray(test_table["A2"], dtype=str)[found]
    same = (a1m == a1t) & (a2m == a2t)
    swap = (a1m == a2t) & (a2m == a1t) & ~same
    out = np.zeros((t_ids.shape[0],) + beta.shape[1:], dtype=beta.dtype)
    rows = np.nonzero(found)[0]
    keep = same | swap
    out[rows[keep]] = beta[at[found][keep]]
    swapped = np.zeros(t_ids.shape[0], dtype=bool)
    swapped[rows[swap]] = True
    return out, swapped


def model_predict(model, test_gdl=None, per_chromosome=False, **kw):
    """``BayesPRSModel.predict`` (viprs/model/BayesPRSModel.py:229-250): the polygenic scores of the training loader's samples,
    or of `test_gdl`'s, from the model's posterior mean effects -- ``(n,)``, or ``(n, n_models)`` for a grid.  A `test_gdl`
    with SNP tables (and a model whose loader has them) is aligned by SNP id (`_align`); without tables the SNP counts must
    agree.  `per_chromosome`: ``{chromosome: scores}`` instead of their sum.  `kw` goes to the loader's ``predict``."""
    beta = getattr(model, "post_mean_beta", None)
    if beta is None:
        raise ValueError("The posterior means for BETA are not set. Call `.fit()` first.")
    gdl = model.gdl if test_gdl is None else test_gdl
    if getattr(gdl, "genotype", None) is None:
        raise ValueError("The data loader holds no genotypes: predict() needs them.  Remedy: build the loader with "
                         "ArrayDataLoader(..., genotype={chromosome: bed prefix | (packed_rows, n) | DeviceGenotypes}).")
    if not hasattr(gdl, "predict"):
        raise TypeError(f"{type(gdl).__name__} has no predict(beta_by_chromosome)")
    beta = {c: np.asarray(b) for c, b in beta.items()}
    swapped = None
    if hasattr(gdl, "_open_genotypes"):                        # (a .bed prefix brings its SNP table when it is opened)
        for c in sorted(gdl.genotype):
            gdl._open_genotypes(c)
    test_tables = getattr(gdl, "snp_table", None) if test_gdl is not None else None
    model_tables = getattr(model.gdl, "snp_table", None)
    if test_tables and model_tables:
        # every chromosome of the effects needs genotypes and both SNP tables, as on the path without tables
        aligned, swapped = {}, {}
        for c in sorted(beta):
            if c not in gdl.genotype:
                raise ValueError(f"chromosome {c} of the effects has no genotypes in the test loader")
            if c not in test_tables:
                raise ValueError(f"chromosome {c} of the test loader has genotypes but no SNP table")
            if c not in model_tables:
                raise ValueError(f"chromosome {c} of the effects has no SNP table in the model's loader")
            aligned[c], swapped[c] = _align(model_tables[c], test_tables[c], beta[c], c)
        beta = aligned
    from .data import ArrayDataLoader
    if not isinstance(gdl, ArrayDataLoader):
        return gdl.predict(beta)                               # a foreign loader: the reference's call
    return gdl.predict(beta, swapped=swapped, per_chromosome=per_chromosome, **kw)
