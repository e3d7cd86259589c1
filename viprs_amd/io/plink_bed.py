"""PLINK 1 binary genotype files (.bed / .bim / .fam), SNP-major.

The .bed file is three magic bytes ``6C 1B 01`` followed by ``m`` rows of ``ceil(n / 4)`` bytes; sample ``i`` of SNP ``j`` is
bits ``2 (i % 4) .. 2 (i % 4) + 1`` of byte ``i // 4`` of row ``j``.  Codes: 0 = two copies of A1, 1 = missing, 2 = one copy,
3 = no copy.  The unused bits of a row's last byte are arbitrary.  `read_bed` hands the rows out as they are (a memory map
past the magic: nothing is unpacked on the host), `write_bed` is its inverse.
"""
import os

import numpy as np

BED_MAGIC = bytes([0x6C, 0x1B, 0x01])
BIM_COLUMNS = ("CHR", "SNP", "CM", "POS", "A1", "A2")


def bytes_per_row(n):
    return (int(n) + 3) // 4


def pack_codes(codes, trailing_bits=0):
    """(m, n) codes 0..3 -> (m, ceil(n / 4)) packed bytes.  `trailing_bits`: what the unused slots of the last byte hold
    (a code 0..3, or an (m,) array of bytes whose slots beyond n are used)."""
    codes = np.asarray(codes)
    if codes.ndim != 2:
        raise ValueError("codes: an (m, n) array")
    if codes.size and (codes.min() < 0 or codes.max() > 3):
        raise ValueError("codes must be 0, 1, 2 or 3")
    m, n = codes.shape
    bpr = bytes_per_row(n)
    full = np.zeros((m, bpr * 4), dtype=np.uint8)
    if np.ndim(trailing_bits) == 0:
        full[:, n:] = int(trailing_bits) & 3
    elif bpr * 4 > n:
        t = np.asarray(trailing_bits, dtype=np.uint8).reshape(m, 1)
        full[:, n:] = (t >> (2 * (np.arange(n, bpr * 4) % 4))) & 3
    full[:, :n] = codes
    q = full.reshape(m, bpr, 4)
    return np.ascontiguousarray(q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6))


def unpack_codes(packed_rows, n):
    """(m, ceil(n / 4)) packed bytes -> (m, n) codes (uint8)."""
    p = np.asarray(packed_rows, dtype=np.uint8)
    if p.ndim != 2 or p.shape[1] != bytes_per_row(n):
        raise ValueError(f"packed rows: an (m, {bytes_per_row(n)}) uint8 array for n = {n}")
    out = np.empty((p.shape[0], p.shape[1], 4), dtype=np.uint8)
    for k in range(4):
        out[:, :, k] = (p >> (2 * k)) & 3
    return out.reshape(p.shape[0], -1)[:, :int(n)]


def _read_table(path, n_columns):
    rows = []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line:
                parts = line.split()
                if len(parts) < n_columns:
                    raise ValueError(f"{path}: a line with {len(parts)} fields, expected {n_columns}")
                rows.append(parts)
    return rows


def read_bed(prefix):
    """-> ``(packed_rows, n, bim, phenotype)``: the (m, ceil(n / 4)) rows as a read-only ``np.memmap`` past the magic, the
    sample count (lines of the .fam), the .bim columns ``{"CHR", "SNP", "POS", "A1", "A2"}`` as arrays, and the .fam phenotype
    column as float64 (``-9`` and ``NA`` become NaN).  Refuses a wrong magic, a sample-major file and a size other than
    ``m * ceil(n / 4) + 3``."""
    prefix = str(prefix)
    fam = _read_table(prefix + ".fam", 6)
    bim = _read_table(prefix + ".bim", 6)
    n, m = len(fam), len(bim)
    path = prefix + ".bed"
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        magic = f.read(3)
    if len(magic) < 3 or magic[:2] != BED_MAGIC[:2]:
        raise ValueError(f"{path}: not a PLINK 1 .bed file (magic bytes {magic.hex()}, expected 6c1b01)")
    if magic[2] != 1:
        raise ValueError(f"{path}: sample-major .bed files are not supported (mode byte {magic[2]:#04x}); "
                         "rewrite it SNP-major (plink --make-bed)")
    bpr = bytes_per_row(n)
    if size != m * bpr + 3:
        raise ValueError(f"{path}: {size} bytes, but {m} SNPs x {n} samples need {m * bpr + 3}")
    if m * bpr:
        rows = np.memmap(path, dtype=np.uint8, mode="r", offset=3, shape=(m, bpr))
    else:
        rows = np.zeros((m, bpr), dtype=np.uint8)
    cols = {name: np.array([r[k] for r in bim], dtype=object) for k, name in enumerate(BIM_COLUMNS)}
    table = {"CHR": cols["CHR"].astype(str), "SNP": cols["SNP"].astype(str),
             "POS": np.array([int(p) for p in cols["POS"]], dtype=np.int64),
             "A1": cols["A1"].astype(str), "A2": cols["A2"].astype(str)}

    def pheno(s):
        try:
            v = float(s)
        except ValueError:
            return np.nan
        return np.nan if v == -9 else v

    return rows, n, table, np.array([pheno(r[5]) for r in fam], dtype=np.float64)


def write_bed(prefix, codes, bim=None, fam=None, trailing_bits=0):
    """Writes ``prefix.bed / .bim / .fam`` from (m, n) codes 0..3.  `bim`: a dict with any of CHR / SNP / POS / A1 / A2
    ((m,) each; defaults ``1``, ``snp<j>``, ``j + 1``, ``A``, ``G``); `fam`: None, an (n,) phenotype array, or a dict with
    ``IID`` and / or ``phenotype``.  NaN phenotypes are written as ``-9``."""
    prefix = str(prefix)
    codes = np.asarray(codes)
    m, n = codes.shape
    bim = dict(bim or {})
    chr_ = np.asarray(bim.get("CHR", np.full(m, "1")), dtype=str)
    snp = np.asarray(bim.get("SNP", [f"snp{j}" for j in range(m)]), dtype=str)
    pos = np.asarray(bim.get("POS", np.arange(1, m + 1)), dtype=np.int64)
    a1 = np.asarray(bim.get("A1", np.full(m, "A")), dtype=str)
    a2 = np.asarray(bim.get("A2", np.full(m, "G")), dtype=str)
    for name, a in (("CHR", chr_), ("SNP", snp), ("POS", pos), ("A1", a1), ("A2", a2)):
        if a.shape != (m,):
            raise ValueError(f"bim[{name!r}]: expected {m} entries")
    if fam is None or not isinstance(fam, dict):
        fam = {"phenotype": fam}
    iid = np.asarray(fam.get("IID") if fam.get("IID") is not None else [f"s{i}" for i in range(n)], dtype=str)
    ph = fam.get("phenotype")
    ph = np.full(n, np.nan) if ph is None else np.asarray(ph, dtype=np.float64)
    if iid.shape != (n,) or ph.shape != (n,):
        raise ValueError(f"fam: expected {n} samples")
    with open(prefix + ".bed", "wb") as f:
        f.write(BED_MAGIC)
        f.write(pack_codes(codes, trailing_bits).tobytes())
    with open(prefix + ".bim", "w") as f:
        for j in range(m):
            f.write(f"{chr_[j]}\t{snp[j]}\t0\t{int(pos[j])}\t{a1[j]}\t{a2[j]}\n")
    with open(prefix + ".fam", "w") as f:
        for i in range(n):
            f.write(f"{iid[i]}\t{iid[i]}\t0\t0\t0\t{'-9' if np.isnan(ph[i]) else repr(float(ph[i]))}\n")
