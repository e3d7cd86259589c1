"""Array-backed stand-ins for the slice of magenpy's data layer that the E-step path touches.

The reference reads its inputs from a magenpy ``GWADataLoader`` (an un-vendored dependency):
``gdl.get_ld_matrices()[c].load(return_symmetric=..., dtype=...)`` -> ``.ld_data / .ld_indptr /
.leftmost_idx`` (VIPRS.py:153-172), ``gdl.sumstats_table[c].n_per_snp`` and
``.get_snp_pseudo_corr()`` (BayesPRSModel.py:133-136), ``gdl.shapes``, ``gdl.m``, ``gdl.n``.
``viprs_amd.model.VIPRS`` is duck-typed on exactly those attributes, so a real magenpy loader
works unchanged; these classes provide the same surface over plain NumPy arrays.
"""
import numpy as np


class LDArrays:
    """LD of one chromosome in the contiguous-window layout.  Holds the
    symmetric and/or the upper-triangular form; ``load`` hands out the one asked for."""

    def __init__(self, symmetric=None, upper=None, stored_dtype=None, dq_scale=1.0, lambda_min=0.0, sample_size=None):
        if symmetric is None and upper is None:
            raise ValueError("need at least one LD form")
        self._forms = {True: symmetric, False: upper}      # key: return_symmetric
        any_form = symmetric if symmetric is not None else upper
        self.stored_dtype = np.dtype(stored_dtype if stored_dtype is not None else any_form[2].dtype)
        self.dq_scale = float(dq_scale)
        self._lambda_min = lambda_min
        self._extremal = None
        self.sample_size = sample_size                      # of the panel the LD was estimated from (None: unknown)
        self._ld_score = None

    class _Loaded:
        def __init__(self, lb, ip, data):
            self.leftmost_idx, self.ld_indptr, self.ld_data = lb, ip, data

    def load(self, return_symmetric=False, dtype=None):
        form = self._forms[bool(return_symmetric)]
        if form is None:
            raise ValueError(f"LD form return_symmetric={return_symmetric} was not provided")
        lb, ip, data = form
        if dtype is not None and np.dtype(dtype) != data.dtype:
            # dequantise at load time, as magenpy does when the caller asks for a float dtype
            data = (data * self.dq_scale).astype(dtype) if np.issubdtype(data.dtype, np.integer) \
                else data.astype(dtype)
        return LDArrays._Loaded(lb, ip, data)

    # which candidate formula `get_lambda_min` applies to the extremes for a min / max ratio > 0 (None: it refuses);
    # see viprs_amd.stats.spectrum.lambda_min_from_extremes
    lambda_min_formula = None

    def set_extremal(self, lam_min, lam_max):
        """The extremal eigenvalues of this LD matrix (`viprs_amd.stats.spectrum.annotate_spectrum` computes them on the
        device): from now on `get_lambda_min` answers from them."""
        self._extremal = (float(lam_min), float(lam_max))

    def set_ld_score(self, ld_score):
        """The per-SNP LD scores of this matrix (`viprs_amd.stats.ldsc.annotate_ld_scores` computes them on the device):
        from now on `ld_score` answers."""
        self._ld_score = np.asarray(ld_score, dtype=np.float64)

    @property
    def ld_score(self):
        if self._ld_score is None:
            raise ValueError("LDArrays: no LD scores attached; compute them with "
                             "viprs_amd.stats.ldsc.annotate_ld_scores(gdl) (or set_ld_score)")
        return self._ld_score

    def get_lambda_min(self, min_max_ratio=1e-3, formula=None):
        if self._extremal is None:
            return self._lambda_min
        from .stats.spectrum import lambda_min_from_extremes
        return lambda_min_from_extremes(*self._extremal, min_max_ratio, formula or self.lambda_min_formula,
                                        where="LDArrays")


class SumstatsArrays:
    def __init__(self, std_beta, n_per_snp, chisq=None):
        self._std_beta = np.asarray(std_beta)
        self.n_per_snp = np.asarray(n_per_snp, dtype=np.float64)
        self._chisq = None if chisq is None else np.asarray(chisq, dtype=np.float64)

    def get_snp_pseudo_corr(self):
        return self._std_beta

    def get_chisq_statistic(self):
        """The association statistic per SNP: the one the caller gave (`chisq=`), else N_j beta_hat_j^2 from the
        standardised effects the models use."""
        if self._chisq is not None:
            return self._chisq
        return self.n_per_snp * np.asarray(self._std_beta, dtype=np.float64) ** 2


class ArrayDataLoader:
    """Minimal ``GWADataLoader`` look-alike: ``ld`` / ``sumstats_table`` dicts keyed by chromosome."""

    def __init__(self, ld, sumstats, n=None, genotype=None, phenotype=None, snp_table=None, device=0):
        """`genotype`: None, or ``{chromosome: DeviceGenotypes | HostGenotypes | (packed_rows, n) | .bed prefix}`` (opened at
        the first `predict`; a prefix also supplies the chromosome's SNP table and, when none is given, the phenotype).
        `phenotype`: (n_samples,) values of the genotyped samples.  `snp_table`: ``{chromosome: {"SNP", "A1", "A2", ...}}``
        arrays per SNP -- of the genotypes when there are any, else of the summary statistics; what `predict` of a model
        aligns by.  `ld` / `sumstats` may be empty dicts for a loader that only carries genotypes."""
        self.ld = dict(ld)
        self.sumstats_table = dict(sumstats)
        self.genotype = dict(genotype) if genotype is not None else None
        self.phenotype = None if phenotype is None else np.asarray(phenotype, dtype=np.float64)
        self.snp_table = {c: dict(t) for c, t in snp_table.items()} if snp_table else None
        self.device = int(device)
        self._own_genotypes = []
        self.shapes = {c: int(s.n_per_snp.shape[0]) for c, s in self.sumstats_table.items()}
        if n is not None:
            self.n = float(n)
        elif self.sumstats_table:
            self.n = float(max(s.n_per_snp.max() for s in self.sumstats_table.values()))
        else:
            self.n = None

    @property
    def chromosomes(self):
        return sorted(self.shapes)

    @property
    def m(self):
        return int(sum(self.shapes.values()))

    def get_ld_matrices(self):
        return self.ld

    # ---- genotypes: polygenic scores of the loader's samples (magenpy's ``GWADataLoader.predict``) ----
    def _open_genotypes(self, c):
        """The genotypes of chromosome `c`, opened once (`viprs_amd.genotypes.open_genotypes`)."""
        from .genotypes import _Genotypes, open_genotypes
        g = self.genotype[c]
        if not isinstance(g, _Genotypes):
            g, owned, bed = open_genotypes(g, device=self.device)
            self.genotype[c] = g
            if owned:
                self._own_genotypes.append(g)
            if bed is not None:
                if self.snp_table is None or c not in self.snp_table:
                    self.snp_table = dict(self.snp_table or {})
                    self.snp_table[c] = bed[2]
                if self.phenotype is None and not np.all(np.isnan(bed[3])):
                    self.phenotype = bed[3]
        return g

    @property
    def n_samples(self):
        """Genotyped samples (None without genotypes)."""
        if not self.genotype:
            return None
        return int(self._open_genotypes(sorted(self.genotype)[0]).n)

    def predict(self, beta_by_chromosome, swapped=None, dose="mean", float_precision=None, per_chromosome=False):
        """Polygenic scores of the genotyped samples: every chromosome of `beta_by_chromosome` (``(m_c,)`` or
        ``(m_c, n_models)`` effects per copy of A1) is scored on its genotypes (`DeviceGenotypes.score`; on the host without a
        device) in `float_precision` (default: the effects' own), and the chromosomes are added on the host in double in
        ascending chromosome order: ``(n,)`` or ``(n, n_models)`` float64.  `dose`: a mode of
        `viprs_amd.genotypes.dose_table` or None (additive, missing = 0); `swapped`: None or ``{chromosome: (m_c,) mask}``
        of the SNPs whose A1 / A2 are exchanged relative to the effects.  `per_chromosome`: the ``{chromosome: scores}``
        (float64) dict instead of the sum."""
        if self.genotype is None:
            raise ValueError("this loader holds no genotypes.  Remedy: ArrayDataLoader(..., genotype={chromosome: "
                             ".bed prefix | (packed_rows, n) | DeviceGenotypes}).")
        parts = {}
        for c in sorted(beta_by_chromosome):
            if c not in self.genotype:
                raise ValueError(f"chromosome {c} of the effects has no genotypes in this loader")
            g = self._open_genotypes(c)
            b = np.asarray(beta_by_chromosome[c])
            if b.shape[0] != g.m:
                raise ValueError(f"chromosome {c}: {b.shape[0]} effects against {g.m} genotyped SNPs (give both loaders "
                                 "SNP tables to have them aligned by SNP id)")
            sw = None if swapped is None else swapped.get(c)
            table = None if dose is None and sw is None else g.dose_table(
                dose or "zero", swapped=sw, dtype=float_precision or (b.dtype if b.dtype == np.float64 else np.float32))
            parts[c] = np.asarray(g.score(b, dose=table, float_precision=float_precision), dtype=np.float64)
        if not parts:
            raise ValueError("no effects were given")
        if per_chromosome:
            return parts
        total = None
        for c in sorted(parts):
            total = parts[c].copy() if total is None else total + parts[c]
        return total

    # ---- genotypes: the LD of the loader's own panel --------------------------------------------------------------------
    def compute_ld(self, estimator=("sample",), dtype=np.float32, max_bytes=1 << 30):
        """LD of every chromosome that has genotypes, from the genotypes (`DeviceGenotypes.ld`: int8 matrix cores; on the
        host without a device): ``self.ld[c]`` becomes an `LDArrays` with the compact upper-triangular form, the quantisation
        scale of `dtype` (int8, int16, float32, float64) and the panel's sample size.  `estimator`: one of
        `viprs_amd.genotypes.ld_windows`, or ``{chromosome: estimator}``; ``("windowed_bp", distance)`` takes the positions
        from the chromosome's SNP table (``POS``).  A model built on the loader afterwards reads this LD like any other;
        `write_ld_stores` saves it.  Returns ``self.ld``."""
        from .genotypes import ld_dq_scale, ld_windows
        if not self.genotype:
            raise ValueError("this loader holds no genotypes.  Remedy: ArrayDataLoader(..., genotype={chromosome: "
                             ".bed prefix | (packed_rows, n) | DeviceGenotypes}).")
        self.ld_estimator = dict(getattr(self, "ld_estimator", {}))
        for c in sorted(self.genotype):
            g = self._open_genotypes(c)
            if c in self.shapes and self.shapes[c] != g.m:
                raise ValueError(f"chromosome {c}: {g.m} genotyped SNPs against {self.shapes[c]} SNPs of the summary "
                                 "statistics: the LD would not line up with them (subset the genotypes to the SNPs of "
                                 "the summary statistics, in their order)")
            est = estimator[c] if isinstance(estimator, dict) else estimator
            est = (est,) if isinstance(est, str) else tuple(est)
            if est[0] == "windowed_bp" and len(est) == 2:
                if not self.snp_table or c not in self.snp_table or "POS" not in self.snp_table[c]:
                    raise ValueError(f"chromosome {c}: ('windowed_bp', distance) needs POS in the SNP table")
                est = est + (self.snp_table[c]["POS"],)
            indptr, data = g.ld(ld_windows(est, g.m), dtype=dtype, max_bytes=max_bytes)
            self.ld[c] = LDArrays(upper=(np.arange(1, g.m + 1, dtype=np.int32), indptr, data),
                                  dq_scale=ld_dq_scale(dtype), sample_size=int(g.n))
            self.ld_estimator[c] = est[0]
        return self.ld

    # ---- genotypes: the loader's own summary statistics (magenpy's ``GWADataLoader.perform_gwas``) -----------------------
    def perform_gwas(self, phenotype=None, keep=None):
        """Summary statistics of every chromosome that has genotypes, from the genotypes and the phenotype (`phenotype`,
        ``(n_samples,)``, or the loader's own; NaN = unknown; a .bed prefix brings the .fam's): the per-SNP linear regression
        of `viprs_amd.genotypes._Genotypes.association` over the samples of `keep` (None: all).
        ``self.sumstats_table[c]`` becomes ``SumstatsArrays(std_beta=R, n_per_snp=N, chisq=Z**2)``, ``self.gwas_table[c]`` keeps
        the full table (N, BETA, SE, Z, R, A1_FREQ), ``self.shapes`` and ``self.n`` follow.  The effect allele is the .bed's
        A1.  Returns ``self.sumstats_table``."""
        if not self.genotype:
            raise ValueError("this loader holds no genotypes: perform_gwas() needs them.  Remedy: ArrayDataLoader(..., "
                             "genotype={chromosome: .bed prefix | (packed_rows, n) | DeviceGenotypes}).")
        opened = {c: self._open_genotypes(c) for c in sorted(self.genotype)}    # (a prefix may bring the phenotype)
        y = self.phenotype if phenotype is None else phenotype
        if y is None:
            raise ValueError("this loader has no phenotype: perform_gwas() needs one.  Remedy: perform_gwas(phenotype="
                             "<(n_samples,) array>), ArrayDataLoader(..., phenotype=...), or a .fam file with a phenotype "
                             "column.")
        y = np.asarray(y, dtype=np.float64)
        self.gwas_table = dict(getattr(self, "gwas_table", {}))
        for c, g in opened.items():
            if y.shape != (g.n,):
                raise ValueError(f"chromosome {c}: a phenotype of shape {y.shape} against {g.n} genotyped samples")
            table = g.association(y, keep=keep)
            self.gwas_table[c] = table
            self.sumstats_table[c] = SumstatsArrays(std_beta=table["R"], n_per_snp=table["N"], chisq=table["Z"] ** 2)
            self.shapes[c] = int(g.m)
        self.n = float(max(s.n_per_snp.max() if s.n_per_snp.size else 0.0 for s in self.sumstats_table.values()))
        return self.sumstats_table

    def write_ld_stores(self, ld_dir, **kw):
        """The LD of `compute_ld` as one zarr store per chromosome under `ld_dir` (``chr_<c>``), with the attributes
        `ZarrLDMatrix` reads back: ``{chromosome: path}``.  `kw` goes to `viprs_amd.io.zarr_ld.write_ld_store`."""
        import os
        from .io.zarr_ld import write_ld_store
        paths = {}
        for c, name in sorted(getattr(self, "ld_estimator", {}).items()):
            lb, ip, data = self.ld[c]._forms[False]
            paths[c] = os.path.join(str(ld_dir), f"chr_{c}")
            write_ld_store(paths[c], ip, data, attrs={"Chromosome": c, "LD estimator": name,
                                                      "Sample size": self.ld[c].sample_size}, **kw)
        return paths

    def close_genotypes(self):
        for g in self._own_genotypes:
            g.close()
        self._own_genotypes = []

    def split_by_chromosome(self):
        """One loader per chromosome, as magenpy's ``GWADataLoader.split_by_chromosome()`` hands to the reference's
        per-chromosome fits (bin/viprs_fit:232-238)."""
        return {c: ArrayDataLoader({c: self.ld[c]}, {c: self.sumstats_table[c]},
                                   genotype=None if self.genotype is None or c not in self.genotype else {c: self.genotype[c]},
                                   phenotype=self.phenotype, device=self.device,
                                   snp_table=None if not self.snp_table or c not in self.snp_table else {c: self.snp_table[c]})
                for c in self.chromosomes}

    @classmethod
    def synthetic(cls, chrom_sizes, ld_dtype=np.float32, seed=7209, n=1e5, forms=("symmetric", "upper"), h2=0.2,
                  kind="ar1", ld_sample_size=None):
        """Synthetic block LD (`kind`: "ar1" | "longrange" | "sample") + simulated summary statistics
        (viprs_amd.utils.synthetic) per chromosome; the total heritability `h2` is shared between the
        chromosomes in proportion to their SNP counts.  `ld_sample_size`: the size of the panel the LD stands for
        (`LDArrays.sample_size`, what corrected LD scores need); None: unknown, as for LD given as bare arrays."""
        m_total = float(sum(int(np.sum(s)) for s in chrom_sizes.values()))
        from .utils import synthetic as syn
        ld, ss = {}, {}
        for ci, (chrom, sizes) in enumerate(chrom_sizes.items()):
            sym = syn.make_ld(sizes, low_memory=False, ld_dtype=ld_dtype, seed=seed + ci, kind=kind)
            up = syn.make_ld(sizes, low_memory=True, ld_dtype=ld_dtype, seed=seed + ci, kind=kind) \
                if "upper" in forms else None
            s = syn.make_sumstats(sym, n=n, seed=seed + ci, h2=h2 * float(np.sum(sizes)) / m_total)
            ld[chrom] = LDArrays(
                symmetric=(sym.ld_left_bound, sym.ld_indptr, sym.ld_data) if "symmetric" in forms else None,
                upper=(up.ld_left_bound, up.ld_indptr, up.ld_data) if up is not None else None,
                stored_dtype=ld_dtype, dq_scale=sym.dq_scale, sample_size=ld_sample_size)
            ss[chrom] = SumstatsArrays(s.std_beta, s.n_per_snp)
        return cls(ld, ss, n=n)


def merge_ld_arrays(chroms, shapes, ld_left_bound, ld_indptr, ld_data):
    """Concatenate the per-chromosome CSR-like LD arrays into one (LD blocks never span chromosomes, so
    the merged matrix is block diagonal): window starts shifted by the SNP offset of their chromosome,
    row pointers by its entry offset.  Returns (left_bound int32, indptr int64, data, {chrom: (start, end)})."""
    snp_off = np.concatenate([[0], np.cumsum([int(shapes[c]) for c in chroms])]).astype(np.int64)
    nnz_off = np.concatenate([[0], np.cumsum([int(ld_indptr[c][-1]) for c in chroms])]).astype(np.int64)
    seg = {c: (int(snp_off[i]), int(snp_off[i + 1])) for i, c in enumerate(chroms)}
    lb = np.concatenate([np.asarray(ld_left_bound[c], dtype=np.int64) + snp_off[i]
                         for i, c in enumerate(chroms)]).astype(np.int32)
    ip = np.concatenate([np.asarray(ld_indptr[c][:-1], dtype=np.int64) + nnz_off[i]
                         for i, c in enumerate(chroms)] + [nnz_off[-1:]])
    data = np.concatenate([ld_data[c] for c in chroms])
    return lb, ip, data, seg


def mirror_upper_ld(ld_indptr, ld_data, diag_value=None):
    """Host model of ``LDPlan.from_upper`` / ``viprs_plan_create_expanded``: the symmetric windowed
    arrays ``(left_bound int32, indptr int64, data)`` of the compact upper-triangular store (row j =
    correlations with SNPs j+1 .. j+len_j).  Row j of the result is [mirror of the rows that reach j |
    diagonal | row j].  Used by the CPU tests and the ``e_step_fn`` test hook; the device path never
    builds the symmetric copy on the host."""
    ip_u = np.asarray(ld_indptr, dtype=np.int64)
    m = ip_u.shape[0] - 1
    if diag_value is None:
        diag_value = np.iinfo(ld_data.dtype).max if np.issubdtype(ld_data.dtype, np.integer) else 1
    length = np.diff(ip_u)
    reach = np.arange(m, dtype=np.int64) + length
    if m and (np.any(np.diff(reach) < 0) or reach[-1] >= m):
        raise ValueError("the upper-triangular windows do not mirror into contiguous symmetric windows")
    # first row whose window reaches j (reach is non-decreasing)
    first = np.minimum(np.searchsorted(reach, np.arange(m), side="left"), np.arange(m))
    lb = first.astype(np.int32)
    ip = np.concatenate([[0], np.cumsum(np.arange(m) - first + 1 + length)]).astype(np.int64)
    data = np.empty(int(ip[-1]), dtype=ld_data.dtype)
    for j in range(m):
        o = int(ip[j])
        n_left = j - int(first[j])
        if n_left:
            rows = np.arange(first[j], j)
            data[o:o + n_left] = ld_data[ip_u[rows] + (j - rows - 1)]
        data[o + n_left] = diag_value
        data[o + n_left + 1:int(ip[j + 1])] = ld_data[ip_u[j]:ip_u[j + 1]]
    return lb, ip, data
