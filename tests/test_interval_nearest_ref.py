"""The brute-force model of interval_nearest (interval_nearest_ref) on hand-written cases whose answers are written out here: touching rows,
an upstream and a downstream row at equal distance under both tie rules, k larger than the chrom, max_distance 0, empty rows on both sides, the
order of the result, invalid rows and the refusals."""
import pytest

import interval_nearest_ref as N
import interval_ref as R


def bed(rows):
    return R.bed_text(rows)


def test_distance():
    assert N.distance(10, 20, 20, 30) == 0 and N.distance(10, 20, 0, 10) == 0          # rows that touch
    assert N.distance(10, 20, 21, 30) == 1 and N.distance(10, 20, 0, 9) == 1
    assert N.distance(10, 20, 12, 15) == 0 and N.distance(10, 20, 0, 100) == 0
    assert N.distance(-(1 << 62), -(1 << 62), (1 << 62) - 1, (1 << 62) - 1) == (1 << 63) - 1


def test_touching_rows_are_at_distance_0():
    left, right = bed([(b"c", 10, 20)]), bed([(b"c", 0, 10), (b"c", 20, 30), (b"c", 40, 50)])
    assert N.nearest(left, right) == [(b"c", 10, 20, 0, 0, 10, 0, 0, 0), (b"c", 10, 20, 0, 20, 30, 1, 0, 0)]
    assert N.nearest(left, right, ties="first") == [(b"c", 10, 20, 0, 0, 10, 0, 0, 0)]
    assert N.nearest(left, right, k=3) == [(b"c", 10, 20, 0, 0, 10, 0, 0, 0), (b"c", 10, 20, 0, 20, 30, 1, 0, 0), (b"c", 10, 20, 0, 40, 50, 2, 0, 20)]


def test_upstream_and_downstream_at_equal_distance():
    left, right = bed([(b"c", 100, 110)]), bed([(b"c", 115, 120), (b"c", 90, 95), (b"c", 300, 400)])
    up, down = (b"c", 100, 110, 0, 90, 95, 1, 0, 5), (b"c", 100, 110, 0, 115, 120, 0, 0, 5)
    assert N.nearest(left, right) == [up, down]                                       # 'all': both rows of the tie, in (right_start, right_row) order
    assert N.nearest(left, right, ties="first") == [up]                               # 'first': the smaller right_start wins
    assert N.nearest(left, right, k=2, ties="first") == [up, down]
    assert N.nearest(left, right, k=2) == [up, down]
    # equal starts: the smaller row number wins
    right = bed([(b"c", 120, 130), (b"c", 120, 125)])
    assert N.nearest(left, right, ties="first") == [(b"c", 100, 110, 0, 120, 130, 0, 0, 10)]


def test_k_larger_than_the_chrom_and_the_order_of_the_result():
    left, right = bed([(b"c", 50, 60), (b"d", 0, 1)]), bed([(b"c", 200, 210), (b"c", 0, 10), (b"c", 55, 58), (b"e", 0, 1)])
    exp = [(b"c", 50, 60, 0, 0, 10, 1, 0, 40), (b"c", 50, 60, 0, 55, 58, 2, 3, 0), (b"c", 50, 60, 0, 200, 210, 0, 0, 140)]
    for ties in N.TIES:
        st = {}
        assert N.nearest(left, right, k=7, ties=ties, stats=st) == exp and st == {"n_pairs": 3, "n_unmatched": 1}
    assert N.nearest(left, right, k=2) == exp[:2]                                      # by right_start, not by distance


def test_max_distance_0_and_other_bounds():
    left, right = bed([(b"c", 10, 20), (b"c", 100, 101)]), bed([(b"c", 0, 10), (b"c", 15, 16), (b"c", 21, 30)])
    st = {}
    assert N.nearest(left, right, k=5, max_distance=0, stats=st) == [(b"c", 10, 20, 0, 0, 10, 0, 0, 0), (b"c", 10, 20, 0, 15, 16, 1, 1, 0)]
    assert st == {"n_pairs": 2, "n_unmatched": 1}
    assert [r[6] for r in N.nearest(left, right, k=5, max_distance=1)] == [0, 1, 2]
    assert [r[3:] for r in N.nearest(left, right, k=1, max_distance=70)] == [(0, 0, 10, 0, 0, 0), (0, 15, 16, 1, 1, 0), (1, 21, 30, 2, 0, 70)]
    assert [r[3] for r in N.nearest(left, right, k=1, max_distance=69)] == [0, 0]


def test_empty_rows_on_both_sides():
    left, right = bed([(b"c", 10, 10), (b"c", 0, 0)]), bed([(b"c", 10, 10), (b"c", 5, 15), (b"c", 12, 12), (b"c", 0, 10)])
    got = N.nearest(left, right, k=9)
    assert [r[3:] for r in got] == [(0, 0, 10, 3, 0, 0), (0, 5, 15, 1, 0, 0), (0, 10, 10, 0, 0, 0), (0, 12, 12, 2, 0, 2),
                                    (1, 0, 10, 3, 0, 0), (1, 5, 15, 1, 0, 5), (1, 10, 10, 0, 0, 10), (1, 12, 12, 2, 0, 12)]
    assert [r[6] for r in N.nearest(left, right)] == [3, 1, 0, 3]


def test_invalid_rows_keep_their_numbers():
    left = bed([(b"c", 9, 3), (b"c", 5, 6)])
    right = bed([(b"c", None, 5), (b"c", 100, 200), (b"c", 1 << 62, 1 << 62)])
    st = {}
    assert N.nearest(left, right, stats=st) == [(b"c", 5, 6, 1, 100, 200, 1, 0, 94)] and st["n_unmatched"] == 0


def test_refusals():
    text = bed([(b"c", 0, 1)])
    for k in (0, -1, (1 << 20) + 1):
        with pytest.raises(ValueError, match="^" + N.ERR_K + "$"):
            N.nearest(text, text, k=k)
    with pytest.raises(ValueError, match="^" + N.ERR_MAX_DISTANCE + "$"):
        N.nearest(text, text, max_distance=-1)
    with pytest.raises(ValueError, match="^" + N.ERR_TIES + "$"):
        N.nearest(text, text, ties="any")
    assert N.nearest(text, text, k=1 << 20, max_distance=(1 << 63) - 1, ties="first") == [(b"c", 0, 1, 0, 0, 1, 0, 1, 0)]
    assert N.NEAREST_COLUMNS == R.OVERLAP_COLUMNS + ["distance"] and len(N.NEAREST_COLUMNS) == 9
