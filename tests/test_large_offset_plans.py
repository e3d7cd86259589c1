"""CPU: the plans of tests/large_offset_plans.py -- that their groups lie where tests/test_gpu_large_offsets.py says they
do, that the reference LD of a group is what the device generates for it, and that the plans can SEE a truncated offset: for
every row of every group, in the caller's layout and in the repacked one, the 64 buffer elements from the row's first-element
offset truncated to 32 or to 31 bits differ from the 64 elements at the true offset.  That is the statement that a kernel which
narrowed an LD offset would not be `==` its reference; no mutated kernel is run on a GPU.  (Truncated as a SIGNED 32-bit
value, an offset with bit 31 set is negative: a read in front of the buffer.)"""
import numpy as np
import pytest

from tests import large_offset_plans as LO
from viprs_amd import _lib as L
from viprs_amd.plan import _LD_CODE, _ptr

TWO_MARKS = ("i8-sym", "i8-upper", "i8-upper-solvers")
ALL = tuple(LO.LAYOUTS)


def _first(full, lay, group, offsets):
    """Offset of the group's first row with an offset in that layout."""
    s, e = lay.snps(lay.groups[group])
    return int(offsets[s])


# ---- the conditions of the issue ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_the_groups_lie_beyond_the_marks(name):
    lay, full = LO.layout(name), LO.skeleton(name)
    raw, dense = LO.raw_row_offsets(full), LO.dense_row_offsets(full)
    es = lay.ld_dtype.itemsize
    first = {g: (_first(full, lay, g, raw), _first(full, lay, g, dense)) for g in lay.groups}
    print(name, {g: (f"raw {r:.4e}", f"dense {d:.4e}") for g, (r, d) in first.items()}, "nnz", full.nnz,
          "dense_elems", LO.dense_layout(lay.sizes)[2])
    if name == "i8-sym":
        assert first["G2"][0] > 2 ** 31 and first["G2"][1] > 2 ** 31
        assert first["G3"][0] > 2 ** 32 and first["G3"][1] > 2 ** 32
    elif name in ("i8-upper", "i8-upper-solvers"):
        assert first["G2"][1] > 2 ** 31 and first["G3"][1] > 2 ** 32          # the dense layout
        assert first["G3"][0] > 2 ** 31                                       # raw offsets pass 2^31
    elif name == "f32-upper":
        assert first["G"][0] > 2 ** 30 and first["G"][1] > 2 ** 30 and first["G"][0] * es > 2 ** 32
    else:
        assert name == "i16-sym" and first["G"][0] > 2 ** 31 and first["G"][1] > 2 ** 31
    # the oversize block stays ragged and is read from the raw buffer behind a mark of its layout; the far filler of the plans
    # with two marks is a dense-route block behind 2^32
    mark = {"i8-sym": 2 ** 32, "i8-upper": 2 ** 31, "i8-upper-solvers": 2 ** 31, "f32-upper": 2 ** 30, "i16-sym": 2 ** 31}[name]
    assert lay.sizes[lay.oversize] > LO.MAX_DENSE_BLOCK and raw[lay.block_start[lay.oversize]] > mark
    assert lay.sizes[lay.far_filler] == LO.FILLER and LO.FILLER % 64 == 0 and LO.FILLER <= LO.MAX_DENSE_BLOCK
    if name in TWO_MARKS:                                   # (one mark: the last filler BEGINS in front of it)
        assert dense[lay.block_start[lay.far_filler]] > 2 ** 32
    assert lay.n_ragged == 1 and lay.n_dense == len(lay.sizes) - 1
    assert lay.m < 2 ** 31 and full.nnz == int(full.ld_indptr[-1])
    # the groups are the role lists of the existing bit tests
    from tests.test_gpu_panel_roles import SIZES as ROLES
    from tests.test_gpu_ridge import SIZES as SOLVER
    want = tuple(SOLVER) if name.endswith("solvers") else tuple(ROLES)
    for g, blocks in lay.groups.items():
        assert tuple(int(b) for b in lay.sizes[blocks]) == want


def test_dense_layout_restates_the_planner_on_a_small_plan():
    """The rule on a list with sizes around a panel and one ragged block: offsets are multiples of 64, squares do not overlap,
    rows start where `rowstart_dense` puts them."""
    sizes = np.array([1, 63, 64, 65, 13184, 13185, 130])
    ld_off, stride, total = LO.dense_layout(sizes)
    assert ld_off.tolist() == [0, 64, 64 + 63 * 64, 64 + 63 * 64 + 64 * 64, 64 + 63 * 64 + 64 * 64 + 65 * 128 + 0, -1,
                               64 + 63 * 64 + 64 * 64 + 65 * 128 + 13184 * 13184]
    assert stride.tolist() == [64, 64, 64, 128, 13184, 0, 192] and total == ld_off[-1] + 130 * 192
    assert np.all(ld_off[ld_off >= 0] % 64 == 0)


# ---- the reference LD is what the device generates ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_reference_ld_equals_the_host_generator_on_the_parameter_slices(name):
    lay, full, vecs = LO.layout(name), LO.skeleton(name), LO.device_vectors(name)
    for g, blocks in lay.groups.items():
        sub = LO.sub_ld(name, g)
        s, e = lay.snps(blocks)
        sizes = np.ascontiguousarray(lay.sizes[blocks], dtype=np.int64)
        sl = [np.ascontiguousarray(v[s:e]) for v in vecs]
        out = np.full(sub.nnz + 3, 77, dtype=lay.ld_dtype)
        L.check(L.lib.viprs_synthetic_ld_host(int(sizes.shape[0]), _ptr(sizes), *[_ptr(v) for v in sl], _LD_CODE[lay.ld_dtype],
                                              int(lay.low_memory), _ptr(out), sub.nnz))
        assert np.array_equal(out[:sub.nnz], sub.ld_data) and (out[sub.nnz:] == 77).all()
        # ... its windows are the whole plan's, moved
        assert np.array_equal(sub.ld_left_bound, full.ld_left_bound[s:e] - s)
        assert np.array_equal(sub.ld_indptr, full.ld_indptr[s:e + 1] - full.ld_indptr[s])
        # ... and the NumPy restatement of one entry gives the same values from the WHOLE plan's vectors and offsets
        raw = LO.raw_row_offsets(full)[s:e]
        n = np.minimum(64, np.diff(sub.ld_indptr))
        got, valid = LO.raw_window(full, vecs, raw)
        for r in np.nonzero(n > 0)[0]:
            o = int(sub.ld_indptr[r])
            assert valid[r, :n[r]].all() and np.array_equal(got[r, :n[r]], sub.ld_data[o:o + n[r]]), (g, r)


# ---- the plans can see a truncated offset -------------------------------------------------------------------------------------
def _truncations(off, itemsize, name):
    """{label: offsets in elements} of the truncations of element offsets (and, for LD of more than one byte, of byte
    offsets) to 32 and to 31 bits."""
    out = {"elements & (2^32 - 1)": off & 0xFFFFFFFF, "elements & (2^31 - 1)": off & 0x7FFFFFFF}
    if itemsize > 1:
        out["bytes & (2^32 - 1)"] = ((off * itemsize) & 0xFFFFFFFF) // itemsize
        out["bytes & (2^31 - 1)"] = ((off * itemsize) & 0x7FFFFFFF) // itemsize
    return out


@pytest.mark.parametrize("kind", ["raw", "dense"])
@pytest.mark.parametrize("name", ALL)
def test_a_truncated_offset_reads_other_entries(name, kind):
    lay, full, vecs = LO.layout(name), LO.skeleton(name), LO.device_vectors(name)
    offsets = LO.raw_row_offsets(full) if kind == "raw" else LO.dense_row_offsets(full)
    window = LO.raw_window if kind == "raw" else LO.dense_window
    rowlen = np.diff(full.ld_indptr)
    changed_by = {}
    for g, blocks in lay.groups.items():
        s, e = lay.snps(blocks)
        rows = np.arange(s, e)[rowlen[s:e] > 0]            # (upper form: the last row of a block stores nothing and is never read)
        off = offsets[rows]
        assert (off >= 0).all()
        true, tv = window(full, vecs, off)
        for label, t in _truncations(off, lay.ld_dtype.itemsize, name).items():
            moved = t != off
            changed_by[(g, label)] = bool(moved.all())
            if not moved.any():
                continue
            assert moved.all(), (g, label)
            got, gv = window(full, vecs, t[moved])
            both = tv[moved] & gv
            assert both.any(axis=1).all()
            same = ((got == true[moved]) | ~both).all(axis=1)
            if same.any():
                r = int(np.nonzero(same)[0][0])
                blk, row, col = LO.landing(full, t[moved][r], kind)
                raise AssertionError(f"{name} {kind} {g} {label}: {int(same.sum())} rows read the same 64 elements at the "
                                     f"truncated offset, first SNP {int(rows[moved][r])}: offset {int(off[moved][r])} -> "
                                     f"{int(t[moved][r])} lands on block {blk} row {row} column {col}")
            # as a signed 32-bit value: negative where bit 31 is set -- in front of the buffer
            if label == "elements & (2^32 - 1)":
                signed = t.astype(np.uint32).view(np.int32)
                assert np.array_equal(signed < 0, (off >> 31) & 1 == 1)
    # what has to move for the GPU cases to mean what they say
    if name == "i8-sym" or kind == "dense" and name in TWO_MARKS:
        assert changed_by[("G2", "elements & (2^31 - 1)")] and changed_by[("G3", "elements & (2^32 - 1)")]
        assert changed_by[("G3", "elements & (2^31 - 1)")]
    elif name in TWO_MARKS:
        assert changed_by[("G3", "elements & (2^31 - 1)")]
    elif name == "f32-upper":
        assert changed_by[("G", "bytes & (2^32 - 1)")] and changed_by[("G", "bytes & (2^31 - 1)")]
        assert changed_by[("G", "elements & (2^31 - 1)")] == (kind == "dense")
    else:
        assert changed_by[("G", "elements & (2^31 - 1)")] and changed_by[("G", "bytes & (2^32 - 1)")]


def test_uploaded_plan_puts_a_windowed_component_behind_2_to_the_31():
    """The index arrays of the one uploaded plan: three blocks for the planner (the filler, the windowed component, the dense
    block), every row behind the filler starts beyond 2^31 raw entries, the filler's windows fit the band kernel's q ring,
    and a row offset truncated to 31 or 32 bits lands in the filler's zeros while the row itself starts with an entry != 0."""
    from viprs_amd.plan import plan_blocks
    lb, ip, start, sub = LO.windowed_plan()
    m = lb.shape[0]
    starts, kinds = plan_blocks(lb, ip, True)
    assert starts.tolist() == [0, start, start + LO.WINDOWED[0], m] and m == start + sub.m
    assert int(ip[start]) > 2 ** 31 and int(ip[-1]) < 2 ** 32 and int(ip[-1]) == int(ip[start]) + sub.nnz
    assert np.array_equal(ip[start:] - ip[start], sub.ld_indptr) and np.array_equal(lb[start:] - start, sub.ld_left_bound)
    reach = int(np.max(lb[:start] + np.diff(ip[:start + 1]) - 1 - np.arange(start)))
    assert reach == LO.W_FILL and 1 + (reach // 64 + 1) + 2 <= 256            # band_left + band_right + 2 (abi_plan.hip)
    rows = np.nonzero(np.diff(sub.ld_indptr) > 0)[0]
    assert np.all(sub.ld_data[sub.ld_indptr[rows]] != 0)
    off = ip[start + rows]
    assert np.all((off & 0x7FFFFFFF) + 64 < ip[start])                         # 31 bits: inside the filler, zeros
    assert np.all((off & 0xFFFFFFFF).astype(np.uint32).view(np.int32) < 0)     # 32 bits, signed: in front of the buffer


def test_landing_names_block_row_and_column():
    full = LO.skeleton("i8-sym")
    lay = LO.layout("i8-sym")
    j = int(lay.block_start[14]) + 5                         # row 5 of the first block of G2
    assert LO.landing(full, int(full.ld_indptr[j]) + 7, "raw") == (14, 5, 7)
    assert LO.landing(full, int(LO.dense_row_offsets(full)[j]) + 7, "dense") == (14, 5, 7)
    up = LO.skeleton("i8-upper")
    assert LO.landing(up, int(up.ld_indptr[j]) + 7, "raw") == (14, 5, 13)          # row 5 of the upper form starts at column 6
    assert LO.landing(up, int(LO.dense_row_offsets(up)[j]) + 7, "dense") == (14, 5, 13)
