"""Plans whose LD offsets need more than 31 and more than 32 bits -- what tests/test_large_offset_plans.py (CPU) and
tests/test_gpu_large_offsets.py build -- and the host arithmetic that says where an LD entry lies and what it holds.

The largest plan of every other test and of the benchmark (cfg3) keeps element offsets below 2^31 and byte offsets below 2^32:
a kernel that narrowed `BlockDesc::ld_off`, `rowstart[j]` or `ip[j]` to 32 bits would stay `==` every reference there.  Here
"longrange" LD is generated on the device (`LDPlan.synthetic`), so a plan of several 10^9 entries costs milliseconds and no
host memory, and LD blocks are independent: the expected result of a block placed far into the buffer is the existing oracle
or replay run on a small host-built LD that holds only that block (`sub_ld`).

A layout is a block list [fillers A][group G2][fillers B][group G3] (two marks, int8 LD) or [fillers][group G] (one mark):

    filler   12 800 SNPs (a multiple of 64 below kMaxDenseBlock = 13 184: the dense route), only there to push offsets;
             the last filler in front of the last group has 16 384 SNPs: above kMaxDenseBlock, so the planner keeps a ragged
             block, the raw buffer stays, and the row-by-row kernels read it behind the marks
    group    the role list of a family's existing bit test: SWEEP_GROUP (tests/test_gpu_panel_roles.py) or SOLVER_GROUP
             (SIZES of tests/test_gpu_ridge.py)

    name               LD     form    blocks                                         first-element offsets of the groups
    i8-sym             int8   sym     14 F, G2, 14 F, 16384, G3                      raw 2.29e9 / 4.86e9, dense 2.29e9 / 4.60e9
    i8-upper           int8   upper   the same                                       raw 1.15e9 / 2.43e9, dense as above
    i8-upper-solvers   int8   upper   the same with SOLVER_GROUP                     raw 1.15e9 / 2.43e9, dense 2.29e9 / 4.60e9
    f32-upper          fp32   upper   14 F, 16384, G                                 raw 1.28e9, dense 2.29e9 (x 4 bytes)
    i16-sym            int16  sym     14 F, 16384, G                                 raw 2.56e9, dense 2.29e9 (x 2 bytes)

(2^30 = 1.07e9, 2^31 = 2.15e9, 2^32 = 4.29e9.)  tests/test_large_offset_plans.py asserts the conditions on these numbers."""
import functools

import numpy as np

from viprs_amd.utils import synthetic as syn

PANEL = 64
MAX_DENSE_BLOCK = 13184                     # kMaxDenseBlock (abi_plan.hip)
FILLER, OVERSIZE = 12800, 16384
N_FILLERS = 14                              # 14 x 12800^2 = 2.29e9 > 2^31; 14 x 12800 x 12799 / 2 = 1.15e9 > 2^30
SWEEP_GROUP = (2370, 1601, 130, 64, 1)      # tests/test_gpu_panel_roles.py
SOLVER_GROUP = (1, 2, 63, 64, 65, 257, 513, 1025, 2305)      # SIZES of tests/test_gpu_ridge.py
SEED = 61

LAYOUTS = {                                 # name: (low_memory, LD dtype, group, number of groups)
    "i8-sym": (False, np.int8, SWEEP_GROUP, 2),
    "i8-upper": (True, np.int8, SWEEP_GROUP, 2),
    "i8-upper-solvers": (True, np.int8, SOLVER_GROUP, 2),
    "f32-upper": (True, np.float32, SWEEP_GROUP, 1),
    "i16-sym": (False, np.int16, SWEEP_GROUP, 1),
}


class Layout:
    """The block list of a layout: `sizes`, `roles` ("A" / "B" fillers, the group names), `groups` {name: block indices},
    `oversize` (index of the 16 384-SNP block) and `far_filler` (the last dense-route filler in front of the last group)."""

    def __init__(self, name):
        self.name = name
        self.low_memory, dt, group, n_groups = LAYOUTS[name]
        self.ld_dtype = np.dtype(dt)
        g = list(group)
        if n_groups == 2:
            sizes = [FILLER] * N_FILLERS + g + [FILLER] * N_FILLERS + [OVERSIZE] + g
            roles = ["A"] * N_FILLERS + ["G2"] * len(g) + ["B"] * (N_FILLERS + 1) + ["G3"] * len(g)
        else:
            sizes = [FILLER] * N_FILLERS + [OVERSIZE] + g
            roles = ["A"] * (N_FILLERS + 1) + ["G"] * len(g)
        self.sizes = np.array(sizes, dtype=np.int64)
        self.roles = roles
        self.groups = {r: np.array([i for i, x in enumerate(roles) if x == r]) for r in roles if r.startswith("G")}
        self.oversize = sizes.index(OVERSIZE)
        self.far_filler = self.oversize - 1
        self.block_start = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.m = int(self.block_start[-1])

    def snps(self, blocks):
        """The SNP range [s, e) of consecutive blocks."""
        blocks = np.atleast_1d(blocks)
        assert np.array_equal(blocks, np.arange(blocks[0], blocks[-1] + 1))
        return int(self.block_start[blocks[0]]), int(self.block_start[blocks[-1] + 1])

    @property
    def n_dense(self):
        return int((self.sizes <= MAX_DENSE_BLOCK).sum())

    @property
    def n_ragged(self):
        return int((self.sizes > MAX_DENSE_BLOCK).sum())


@functools.lru_cache(maxsize=None)
def layout(name):
    return Layout(name)


@functools.lru_cache(maxsize=None)
def skeleton(name):
    """The `SyntheticLD` skeleton of a layout (index arrays and block parameters, no entries): what `LDPlan.synthetic` takes."""
    lay = layout(name)
    return syn.make_ld(lay.sizes, low_memory=lay.low_memory, ld_dtype=lay.ld_dtype, seed=SEED, kind="longrange", data=False)


@functools.lru_cache(maxsize=None)
def device_vectors(name):
    """The per-SNP float32 parameter vectors of the whole layout (`synthetic.longrange_device_params`)."""
    full = skeleton(name)
    return syn.longrange_device_params(np.diff(full.block_start), full.rho, full.params)


def sub_ld_of(full, blocks):
    """Host-built LD of the listed blocks of `full` alone, with their parameters: the reference's LD."""
    blocks = [int(b) for b in np.atleast_1d(blocks)]
    sizes = np.diff(full.block_start)[blocks]
    return syn.make_ld(sizes, low_memory=full.low_memory, ld_dtype=full.ld_dtype, rho=full.rho[blocks],
                       params=[full.params[b] for b in blocks], kind="longrange")


@functools.lru_cache(maxsize=None)
def sub_ld(name, group):
    """The reference LD of a group of a layout.  Computed once, never modified."""
    ld = sub_ld_of(skeleton(name), layout(name).groups[group])
    for a in (ld.ld_left_bound, ld.ld_indptr, ld.ld_data):
        a.setflags(write=False)
    return ld


@functools.lru_cache(maxsize=None)
def sumstats(name):
    """Marginal effects for the whole layout, a seeded vector as tests/test_band.py draws it: noise of the size 1 / sqrt(n)
    has at n = 1e5 and an effect of 0.05 at one SNP in 50.  (`synthetic.make_sumstats` takes seconds at this size.)"""
    m = layout(name).m
    rng = np.random.default_rng(SEED + 2)
    beta = (rng.standard_normal(m) * 0.004).astype(np.float32)
    beta[rng.integers(0, m, m // 50)] += np.float32(0.05)
    beta.setflags(write=False)
    return syn.SyntheticSumstats(beta, np.full(m, 1e5), np.zeros(m, np.float32), 1e5)


# ---- where an entry lies ------------------------------------------------------------------------------------------------------
def dense_layout(sizes):
    """Python restatement of the `ld_off` rule (abi_plan.hip, the loop that fills `BlockDesc`): a block of at most
    kMaxDenseBlock SNPs becomes a padded square of `stride = ceil(size / 64) * 64` columns at the running offset, which is then
    rounded up to a multiple of 64 elements.  Returns (ld_off per block, -1 for a block that stays ragged; stride per block;
    dense_elems)."""
    ld_off = np.full(len(sizes), -1, dtype=np.int64)
    stride = np.zeros(len(sizes), dtype=np.int64)
    off = 0
    for i, b in enumerate(int(x) for x in sizes):
        if b > MAX_DENSE_BLOCK:
            continue
        stride[i] = (b + PANEL - 1) // PANEL * PANEL
        ld_off[i] = off
        off += b * int(stride[i])
        off = (off + 63) // 64 * 64
    return ld_off, stride, off


def raw_row_offsets(full):
    """First-element offset of every row in the caller's row-concatenated layout: `ld_indptr[j]`."""
    return np.asarray(full.ld_indptr[:-1], dtype=np.int64)


def dense_row_offsets(full):
    """First-element offset of every row in the repacked layout (`rowstart_dense`, abi_plan.hip): ld_off + r * stride, plus
    r + 1 in the upper form; -1 for the rows of a ragged block."""
    sizes = np.diff(full.block_start)
    ld_off, stride, _ = dense_layout(sizes)
    out = np.full(full.m, -1, dtype=np.int64)
    for i, b in enumerate(int(x) for x in sizes):
        if ld_off[i] < 0:
            continue
        r = np.arange(b, dtype=np.int64)
        out[int(full.block_start[i]):int(full.block_start[i + 1])] = ld_off[i] + r * stride[i] + (r + 1 if full.low_memory else 0)
    return out


# ---- what an entry holds ------------------------------------------------------------------------------------------------------
def generated(vecs, ld_dtype, s, i, j):
    """NumPy restatement of `synth_entry` / `synth_store` (csrc/synth.hip), entry (i, j) of the block whose first SNP is `s`
    (arrays of equal shape): five float32 operations, each rounded on its own, then rint(v * qmax) for integer LD.
    tests/test_large_offset_plans.py shows it `==` the library's host generator."""
    pw, uf0, uf1, sa, sf = vecs
    s, i, j = (np.asarray(a, dtype=np.int64) for a in (s, i, j))
    mm = uf0[s + i] * uf0[s + j] + uf1[s + i] * uf1[s + j]
    t = (pw[s + np.abs(i - j)] * sa[s + i]) * sf[s + j]
    v = np.where(i == j, np.float32(1.0), mm + t).astype(np.float32)
    dt = np.dtype(ld_dtype)
    if dt == np.float32:
        return v
    return np.rint(v * np.float32(np.iinfo(dt).max)).astype(dt)


def raw_window(full, vecs, off, n=64):
    """The `n` consecutive elements of the raw buffer from each offset of `off`: (values (len(off), n), valid) -- `valid`
    False beyond the end of the buffer."""
    ip = np.asarray(full.ld_indptr, dtype=np.int64)
    p = np.asarray(off, dtype=np.int64)[:, None] + np.arange(n, dtype=np.int64)[None, :]
    valid = (p >= 0) & (p < ip[-1])
    q = np.where(valid, p, 0)
    row = np.searchsorted(ip, q, side="right") - 1              # (skips the empty rows that share an offset)
    col = full.ld_left_bound[row].astype(np.int64) + (q - ip[row])
    blk = np.searchsorted(full.block_start, row, side="right") - 1
    s = np.asarray(full.block_start, dtype=np.int64)[blk]
    return np.where(valid, generated(vecs, full.ld_dtype, s, row - s, col - s), 0), valid


def dense_window(full, vecs, off, n=64):
    """The `n` consecutive elements of the repacked buffer from each offset of `off`, as the panel kernels sweep it: whole
    rows of a padded square, zeros in the padding and between the squares and behind the last one; in the upper form the
    lower triangle mirrors the upper one and the diagonal is 0.  `valid` False in front of the buffer."""
    sizes = np.diff(full.block_start)
    ld_off, stride, total = dense_layout(sizes)
    dense = np.nonzero(ld_off >= 0)[0]
    p = np.asarray(off, dtype=np.int64)[:, None] + np.arange(n, dtype=np.int64)[None, :]
    valid = p >= 0
    q = np.clip(p, 0, total - 1)
    k = dense[np.searchsorted(ld_off[dense], q, side="right") - 1]
    rel = q - ld_off[k]
    r, c = rel // stride[k], rel % stride[k]
    inside = valid & (p < total) & (r < sizes[k]) & (c < sizes[k])
    if full.low_memory:
        inside &= r != c
    s = np.asarray(full.block_start, dtype=np.int64)[k]
    rr, cc = np.where(inside, r, 0), np.where(inside, c, 0)
    return np.where(inside, generated(vecs, full.ld_dtype, s, rr, cc), 0), valid


def landing(full, off, layout_kind):
    """(block, row in the block, column in the block's square) of the element at offset `off` of a layout ("raw" / "dense"):
    where a truncated offset lands."""
    off = int(off)
    if layout_kind == "raw":
        ip = np.asarray(full.ld_indptr, dtype=np.int64)
        row = int(np.searchsorted(ip, off, side="right") - 1)
        blk = int(np.searchsorted(full.block_start, row, side="right") - 1)
        s = int(full.block_start[blk])
        return blk, row - s, int(full.ld_left_bound[row]) + off - int(ip[row]) - s
    ld_off, stride, _ = dense_layout(np.diff(full.block_start))
    dense = np.nonzero(ld_off >= 0)[0]
    blk = int(dense[np.searchsorted(ld_off[dense], off, side="right") - 1])
    rel = off - int(ld_off[blk])
    return blk, rel // int(stride[blk]), rel % int(stride[blk])


# ---- one UPLOADED plan: a windowed component behind 2^31 raw entries -------------------------------------------------------------
# The device generator builds dense blocks only.  This plan (int8, upper form) puts a windowed component and a dense block
# behind ONE zero-valued windowed filler whose rows hold just over 2^31 entries: 143 000 rows of up to 15 936 entries -- 250
# panels to the right, inside the band kernel's q ring of 256, so that the band kernel still serves the plan.
W_FILL, M_FILL = 15936, 143000
WINDOWED = (1500, 130, 70, 40)              # banded_ld(m, w_left, w_right, jitter=) of tests/test_gpu_per_snp_inputs.py
WINDOWED_DENSE = 130


@functools.lru_cache(maxsize=None)
def windowed_plan():
    """(left_bound, indptr, first SNP behind the filler, `SyntheticLD` of the part behind the filler alone): the index arrays of
    the uploaded plan and its reference LD.  The entries of the whole plan: `windowed_plan_data`."""
    from tests.test_band import banded_ld
    j = np.arange(M_FILL, dtype=np.int64)
    length = np.minimum(j + W_FILL + 1, M_FILL) - (j + 1)
    lb_f = np.minimum(j + 1, M_FILL - 1)
    m_w, wl, wr, jitter = WINDOWED
    band = banded_ld(m_w, wl, wr, True, np.int8, seed=m_w, jitter=jitter)
    dense = syn.make_ld([WINDOWED_DENSE], low_memory=True, ld_dtype=np.int8, seed=SEED, kind="longrange")
    sub_lb = np.concatenate([band.ld_left_bound, dense.ld_left_bound + m_w]).astype(np.int32)
    sub_ip = np.concatenate([band.ld_indptr, dense.ld_indptr[1:] + band.ld_indptr[-1]]).astype(np.int64)
    sub = syn.SyntheticLD(sub_lb, sub_ip, np.concatenate([band.ld_data, dense.ld_data]), np.array([0, m_w, m_w + WINDOWED_DENSE]),
                          np.zeros(2), True, band.dq_scale)
    assert band.dq_scale == dense.dq_scale
    nnz_f = int(length.sum())
    lb = np.concatenate([lb_f, sub_lb.astype(np.int64) + M_FILL]).astype(np.int32)
    ip = np.concatenate([[0], np.cumsum(length), sub_ip[1:] + nnz_f]).astype(np.int64)
    for a in (lb, ip, sub.ld_left_bound, sub.ld_indptr, sub.ld_data):
        a.setflags(write=False)
    return lb, ip, M_FILL, sub


def windowed_plan_data():
    """The entries of the uploaded plan: zeros (pages the host never touches before the upload), then the reference LD's.
    Not cached: 2.15 GB."""
    lb, ip, start, sub = windowed_plan()
    data = np.zeros(int(ip[-1]), dtype=np.int8)
    data[int(ip[start]):] = sub.ld_data
    return data


# ---- comparing a group of the whole plan's result with its reference --------------------------------------------------------------
def group_rows(lay, group, arrays):
    """The rows of the SNPs of `group` of every array of the dict `arrays` (contiguous copies in the arrays' memory order)."""
    s, e = lay.snps(lay.groups[group])
    return {k: np.array(v[s:e], order="F" if (v.ndim == 2 and v.flags.f_contiguous and not v.flags.c_contiguous) else "C")
            for k, v in arrays.items()}


def assert_group_equal(got, ref, lay, group, fields, what=""):
    """`==` between the rows of `group` in `got` (arrays over the whole plan) and `ref` (arrays over the group's SNPs); a
    failure names the group, the block of the plan and the row (`per_snp_inputs.first_difference`)."""
    from tests import per_snp_inputs as P
    blocks = lay.groups[group]
    sub = syn.SyntheticLD(None, None, None, lay.block_start[blocks[0]:blocks[-1] + 2] - lay.block_start[blocks[0]], None,
                          lay.low_memory)
    msg = P.first_difference(group_rows(lay, group, {k: got[k] for k in fields}), ref, sub, fields)
    assert msg is None, (f"{what} {lay.name} group {group} (blocks {int(blocks[0])} .. {int(blocks[-1])} of the plan, SNPs from "
                         f"{lay.snps(blocks)[0]}): {msg}")


def assert_all_finite(arrays, what=""):
    for k, v in arrays.items():
        assert np.isfinite(v).all(), f"{what}: {k} has {int((~np.isfinite(v)).sum())} non-finite values"
