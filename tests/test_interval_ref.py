"""The model of interval_merge / interval_overlap (tests/interval_ref.py) held to the reference's own cgranges and to hand cases, without
a device: 'any' and 'contain' are cr_overlap and cr_contain of oracle/_ref/libcgranges.so, 'within' is 'contain' with the sides swapped,
the merge rule on nested, touching and gapped rows, and which rows are invalid."""
import ctypes as C
import os

import numpy as np
import pytest

import interval_ref as R
from conftest import ROOT

import region_oracle   # noqa: E402  (interval_ref put oracle/ on the path)

CGR = os.path.join(ROOT, "oracle", "_ref", "libcgranges.so")
SIZES = (1, 7, 64, 65, 2000)


def cgranges_contain(lib_path, names, tid, beg, end, queries):
    """cr_contain of the reference's cgranges, bound as region_oracle.cgranges_overlap binds cr_overlap: the labels of the intervals that lie
    inside every query (name, st, en), sorted"""
    L = C.CDLL(lib_path)
    L.cr_init.restype = C.c_void_p
    L.cr_add.restype = C.c_void_p
    L.cr_add.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int32]
    L.cr_index.argtypes = [C.c_void_p]
    L.cr_destroy.argtypes = [C.c_void_p]
    L.cr_contain.restype = C.c_int64
    L.cr_contain.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.POINTER(C.c_int64)), C.POINTER(C.c_int64)]

    class Intv(C.Structure):
        _fields_ = [("x", C.c_uint64), ("y", C.c_uint32), ("label", C.c_int32)]

    class Cr(C.Structure):
        _fields_ = [("n_r", C.c_int64), ("m_r", C.c_int64), ("r", C.POINTER(Intv))]

    cr = L.cr_init()
    for i in range(len(tid)):
        L.cr_add(cr, names[int(tid[i])].encode(), int(beg[i]), int(end[i]), i)
    L.cr_index(cr)
    r = C.cast(cr, C.POINTER(Cr)).contents.r
    b, mb, out = C.POINTER(C.c_int64)(), C.c_int64(0), []
    for name, st, en in queries:
        n = L.cr_contain(cr, name.encode(), int(st), int(en), C.byref(b), C.byref(mb))
        out.append(np.sort(np.array([r[b[k]].label for k in range(n)], np.int64)))
    C.CDLL(None).free(b)
    L.cr_destroy(cr)
    return out


def _case(n):
    """n intervals and 40 queries (a fifth of each empty, and a few queries on the intervals' own edges) on three chroms inside int32"""
    right = R.seeded_bed(100 + n, n)
    left = R.seeded_bed(200 + n, 30) + [(c, s, e) for c, s, e in right[:5]] + [(c, s, s) for c, s, e in right[:3]] + [(c, e, e) for c, s, e in right[:2]]
    return left, right


@pytest.mark.skipif(not os.path.exists(CGR), reason="oracle/_ref/libcgranges.so is built only where the reference lies")
@pytest.mark.parametrize("n", SIZES)
def test_any_and_contain_are_cgranges(n):
    left, right = _case(n)
    names = sorted({c.decode() for c, _, _ in left + right})
    tid = [names.index(c.decode()) for c, _, _ in right]
    beg, end = [s for _, s, _ in right], [e for _, _, e in right]
    queries = [(c.decode(), s, e) for c, s, e in left]
    ltext, rtext = R.bed_text(left), R.bed_text(right)
    for mode, ref in (("any", region_oracle.cgranges_overlap), ("contain", cgranges_contain)):
        exp = ref(CGR, names, tid, beg, end, queries)
        got = [[] for _ in left]
        for row in R.overlap(ltext, rtext, mode):
            got[row[3]].append(row[6])
        assert [sorted(g) for g in got] == [e.tolist() for e in exp], mode
        assert sum(len(g) for g in got) > 0 or n == 1


@pytest.mark.parametrize("n", SIZES)
def test_within_is_contain_with_the_sides_swapped(n):
    left, right = _case(n)
    ltext, rtext = R.bed_text(left), R.bed_text(right)
    a = sorted((r[3], r[6], r[7]) for r in R.overlap(ltext, rtext, "within"))
    b = sorted((r[6], r[3], r[7]) for r in R.overlap(rtext, ltext, "contain"))
    assert a == b


def test_overlap_order_and_the_overlap_column():
    left = R.bed_text([(b"c", 10, 20), (b"d", 0, 5), (b"c", 0, 100)])
    right = R.bed_text([(b"c", 15, 30), (b"c", 5, 12), (b"c", 15, 16), (b"c", 20, 25), (b"e", 0, 9)])
    got = R.overlap(left, right, "any")
    assert [(r[3], r[6]) for r in got] == [(0, 1), (0, 0), (0, 2), (2, 1), (2, 0), (2, 2), (2, 3)]         # by left_row, then (right_start, right_row)
    assert [r[7] for r in got] == [2, 5, 1, 7, 15, 1, 5]
    assert [(r[3], r[6]) for r in R.overlap(left, right, "contain")] == [(0, 2), (2, 1), (2, 0), (2, 2), (2, 3)]
    assert [(r[3], r[6]) for r in R.overlap(left, right, "within")] == []
    # touching rows are no pair; an empty row inside another is one, with overlap 0
    assert R.overlap(R.bed_text([(b"c", 0, 10)]), R.bed_text([(b"c", 10, 20)]), "any") == []
    assert R.overlap(R.bed_text([(b"c", 5, 5)]), R.bed_text([(b"c", 0, 10)]), "any") == [(b"c", 5, 5, 0, 0, 10, 0, 0)]
    assert R.overlap(R.bed_text([(b"c", 5, 5)]), R.bed_text([(b"c", 5, 10)]), "any") == []                    # rs < e fails


def test_merge_hand_cases():
    m = R.merge
    assert m(R.bed_text([(b"c", 0, 100), (b"c", 10, 20), (b"c", 50, 60)])) == [(b"c", 0, 100, 3)]                        # nested
    assert m(R.bed_text([(b"c", 0, 10), (b"c", 10, 20)])) == [(b"c", 0, 20, 2)]                                           # touching
    assert m(R.bed_text([(b"c", 0, 10), (b"c", 11, 20)])) == [(b"c", 0, 10, 1), (b"c", 11, 20, 1)]
    assert m(R.bed_text([(b"c", 0, 10), (b"c", 15, 20)]), 5) == [(b"c", 0, 20, 2)]                                       # a gap of exactly max_gap
    assert m(R.bed_text([(b"c", 0, 10), (b"c", 16, 20)]), 5) == [(b"c", 0, 10, 1), (b"c", 16, 20, 1)]                    # max_gap + 1
    assert m(R.bed_text([(b"c", 30, 40), (b"b", 5, 6), (b"c", 0, 35), (b"b", 1, 5)])) == [(b"b", 1, 6, 2), (b"c", 0, 40, 2)]   # unsorted input
    assert m(R.bed_text([(b"a", 0, 100), (b"b", 50, 60)])) == [(b"a", 0, 100, 1), (b"b", 50, 60, 1)]                     # a run ends at a chrom change
    assert m(R.bed_text([(b"c", 7, 7)])) == [(b"c", 7, 7, 1)]                                                             # an empty row on its own
    assert m(R.bed_text([(b"c", 0, 50), (b"c", 3, 9), (b"c", 40, 41), (b"c", 51, 52)])) == [(b"c", 0, 50, 3), (b"c", 51, 52, 1)]   # run_end is the largest end seen
    assert [r[0] for r in m(R.bed_text([(b"chr10", 0, 1), (b"chr1_alt", 0, 1), (b"chr1", 0, 1), (b"chr2", 0, 1)]))] == [b"chr1", b"chr10", b"chr1_alt", b"chr2"]
    for bad in (-1, (1 << 40) + 1):
        with pytest.raises(ValueError, match="max_gap must be between 0 and 1099511627776"):
            m(b"c\t0\t1\n", bad)
    assert m(b"c\t0\t1\n", 1 << 40) == [(b"c", 0, 1, 1)]


def test_invalid_rows_keep_their_number_and_take_no_part():
    lim = 1 << 62
    rows = [(b"c", None, 5), (b"c", 9, 3), (b"c", -lim, lim - 1), (b"c", lim, lim), (b"c", -lim - 1, 0), (b"c", 0, lim), (b"c", b"1x", 5), (b"c", 1, 2)]
    text = R.bed_text(rows)
    got, ok = R.rows_of(text)
    assert len(got) == 8 and ok == [2, 7]
    assert R.table_stats(text) == {"n_rows": 8, "n_skipped": 6, "n_chroms": 1}
    assert R.merge(text) == [(b"c", -lim, lim - 1, 2)]
    assert [(r[3], r[6]) for r in R.overlap(text, text, "any")] == [(2, 2), (2, 7), (7, 2), (7, 7)]
    with pytest.raises(ValueError, match="fewer than 3 tab-delimited fields"):
        R.rows_of(b"c\t0\t1\nc\t5\n")


def test_the_sort_model():
    start = np.array([5, -1, 0, -(1 << 62), (1 << 62) - 1, 5], np.int64)
    rank = np.array([1, 1, 0, 1, 0, 1], np.uint32)
    assert R.sort_rows(R.sort_key(start), rank).tolist() == [2, 4, 3, 1, 0, 5]
    assert R.name_runs(b"a\t0\t1\na\t1\t2\n#x\na\t2\t3\nb\t0\t1\n\nb\t1\t2\n") == 4
