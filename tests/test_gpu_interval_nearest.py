"""interval_nearest on the device (dhts_ivl_nearest_*, csrc/interval_nearest.hip) through duckhts_amd.interval_nearest against the brute-force
model interval_nearest_ref, row for row and column for column: seeded files plain and bgzipped under every k, ties and max_distance, the walk
back over 64-row blocks, disjoint rows (every answer from the upstream or downstream sequence), many equal rows, end order against start order,
positions at the limits, chroms on one side, invalid rows, batches of one block, pages, projections, the stats, the refusals and the switch
between the results of one context."""
import numpy as np
import pytest

import duckhts_amd
import interval_nearest_ref as N
import interval_ref as R
from bamwriter import bgzf_file

pytestmark = pytest.mark.gpu
LIM = 1 << 62
KS, MDS = (1, 2, 5, 3000), (None, 0, 3, 10 ** 9)


def same(got, exp_rows):
    exp = R.columns(exp_rows, N.NEAREST_COLUMNS)
    assert got["n_rows"] == exp["n_rows"] == sum(got["pages"])
    assert got["chrom"] == exp["chrom"]
    for k in N.NEAREST_COLUMNS[1:]:
        assert got[k].dtype == np.int64 and len(got[k]) == exp["n_rows"], k
        bad = np.flatnonzero(got[k] != exp[k])
        assert not len(bad), (k, bad[:5].tolist(), got[k][bad[:5]].tolist(), exp[k][bad[:5]].tolist())


def check(left, right, k=1, max_distance=None, ties="all", lsrc=None, rsrc=None, **kw):
    st, est = {}, {}
    got = duckhts_amd.interval_nearest(left if lsrc is None else lsrc, right if rsrc is None else rsrc, k=k, max_distance=max_distance, ties=ties, stats=st, **kw)
    exp = N.nearest(left, right, k, max_distance, ties, stats=est)
    same(got, exp)
    assert got["status"] == 1 and st["n_pairs"] == est["n_pairs"] and st["n_unmatched"] == est["n_unmatched"], (st, est)
    assert {k_: st[k_] for k_ in ("n_rows", "n_skipped", "n_chroms")} == R.table_stats(left)
    assert {k_: st["right"][k_] for k_ in ("n_rows", "n_skipped", "n_chroms")} == R.table_stats(right)
    return got, st


def check_all(left, right, ks=KS, mds=MDS, **kw):
    n = 0
    for k in ks:
        for md in mds:
            for ties in N.TIES:
                n += check(left, right, k, md, ties, **kw)[0]["n_rows"]
    return n


@pytest.mark.parametrize("n", (1, 7, 64, 65, 2000))
def test_seeded_files_plain_and_bgzipped(n, tmp_path):
    right = R.seeded_bed(300 + n, n)
    left = R.seeded_bed(400 + n, 30) + right[:5] + [(c, s, s) for c, s, e in right[:3]] + [(c, e, e) for c, s, e in right[:2]]
    ltext, rtext = R.bed_text(left), R.bed_text(right)
    assert check_all(ltext, rtext) > 0
    lp, rp = tmp_path / "l.bed", tmp_path / "r.bed.gz"
    lp.write_bytes(ltext)
    rp.write_bytes(bgzf_file(rtext))
    for ties in N.TIES:
        check(ltext, rtext, 2, None, ties, lsrc=str(lp), rsrc=str(rp))
        check(ltext, rtext, 5, 3, ties, lsrc=bgzf_file(ltext), rsrc=str(rp))


def test_the_walk_back_reaches_a_row_that_spans_its_chrom():
    """the first right row spans the chrom, so it is at distance 0 of every left row and the walk starts at the chrom's first row; the left rows
    lie around the 64-row block edges, the blocks in between are skipped by bmax"""
    right = [(b"c", 0, 10 ** 6)] + [(b"c", 10 * i, 10 * i + 5) for i in range(1, 400)] + [(b"d", 5, 6)]
    left = [(b"c", 10 * i - 3, 10 * i + 12) for i in (62, 63, 64, 65, 127, 128, 129, 255, 256)] + [(b"c", 10 * i + 6, 10 * i + 8) for i in (63, 64, 128, 256, 399)] + [(b"d", 0, 100), (b"c", 10 ** 6 + 7, 10 ** 6 + 9)]
    ltext, rtext = R.bed_text(left), R.bed_text(right)
    got, _ = check(ltext, rtext)
    assert (np.bincount(got["left_row"], minlength=len(left))[:9] == 3).all() and (got["right_row"][got["left_row"] < 14] == 0).sum() == 14
    check_all(ltext, rtext, ks=(1, 2, 5, 3000), mds=(None, 0, 3))
    check_all(rtext, ltext, ks=(1, 3), mds=(None, 3))


def test_disjoint_rows_every_answer_from_the_two_sequences():
    """400 disjoint right rows; the left rows lie in the gaps, in front of the first and behind the last: no row is at distance 0"""
    right = [(b"c", 100 * i, 100 * i + 40) for i in range(1, 401)]
    left = [(b"c", 100 * i + 45 + i % 50, 100 * i + 47 + i % 50) for i in range(1, 400, 7)] + [(b"c", 0, 10), (b"c", -500, -400), (b"c", 50000, 50001), (b"c", 40141, 40199), (b"c", 170, 170)]
    ltext, rtext = R.bed_text(left), R.bed_text(right)
    assert not N.nearest(ltext, rtext, k=1, max_distance=0)
    got, st = check(ltext, rtext)
    assert st["n_unmatched"] == 0 and got["distance"].min() > 0
    check_all(ltext, rtext, ks=(1, 2, 5, 64, 399, 400, 401), mds=(None, 0, 3, 160))


def test_many_equal_right_rows():
    around = [(b"c", 100, 200)] * 200 + [(b"c", 0, 10), (b"c", 500, 510)]
    left = R.bed_text([(b"c", 150, 160)])
    for ties in N.TIES:
        got, _ = check(left, R.bed_text(around), 3, None, ties)
        assert got["n_rows"] == (200 if ties == "all" else 3)
    assert check(left, R.bed_text(around), 3, None, "first")[0]["right_row"].tolist() == [0, 1, 2]
    groups = R.bed_text([(b"c", 200, 210)] * 70 + [(b"c", 0, 100)] * 70)            # the left row midway: both groups at distance 50
    mid = R.bed_text([(b"c", 150, 150)])
    got, _ = check(mid, groups, 3, None, "all")
    assert got["n_rows"] == 140 and set(got["distance"].tolist()) == {50}
    got, _ = check(mid, groups, 3, None, "first")
    assert got["right_row"].tolist() == [70, 71, 72] and got["right_start"].tolist() == [0, 0, 0]      # the upstream group wins
    check_all(mid, groups, ks=(1, 69, 70, 71, 139, 140, 141), mds=(None, 49, 50))


def test_end_order_differs_from_start_order():
    same_start = [(b"c", 100, 100 + 7 * ((i * 37) % 41)) for i in range(41)]         # equal starts, ends in no order
    same_end = [(b"c", 1000 + 5 * ((i * 29) % 43), 2000) for i in range(43)]         # equal ends, starts in no order
    nested = [(b"c", 3000 - 10 * i, 3000 + 10 * i) for i in range(30)]               # the later the start, the earlier the end
    right = R.bed_text(same_start + same_end + nested)
    left = R.bed_text([(b"c", p, p + w) for p in (0, 99, 100, 150, 400, 900, 1100, 2000, 2001, 2500, 2990, 3000, 3005, 3400, 9000) for w in (0, 1, 30)])
    check_all(left, right, ks=(1, 2, 5, 40, 3000), mds=(None, 0, 3, 10 ** 9))


def test_positions_at_the_limits():
    far = (1 << 63) - 1
    left, right = R.bed_text([(b"c", -LIM, -LIM)]), R.bed_text([(b"c", LIM - 1, LIM - 1)])
    for ties in N.TIES:
        got, _ = check(left, right, 1, far, ties)
        assert got["distance"].tolist() == [far]
        check(left, right, 1, None, ties)
        check(right, left, 1, far, ties)
        assert check(left, right, 1, far - 1, ties)[0]["n_rows"] == 0
    rows = [(b"c", -LIM, -LIM), (b"c", -LIM, LIM - 1), (b"c", LIM - 1, LIM - 1), (b"c", -LIM + 5, -LIM + 9), (b"c", LIM - 9, LIM - 2), (b"c", 0, 0), (b"c", -7, 7)]
    text = R.bed_text(rows)
    check_all(text, text, ks=(1, 2, 5, 3000), mds=(None, 0, 3, far, far - 1, LIM))
    check_all(text, R.bed_text(rows[::2]), ks=(1, 2), mds=(None, far))


def test_chroms_on_one_side_and_names_that_are_prefixes():
    names = [b"chr1", b"chr10", b"chr1_alt", b"chr2", b"chr", b"chr1\xff", b"Chr1"]
    ltext = R.bed_text(R.seeded_bed(1, 200, names=names[:5], span=300))
    rtext = R.bed_text(R.seeded_bed(2, 200, names=names[2:], span=300))
    got, st = check(ltext, rtext, 2)
    assert set(got["chrom"]) == {b"chr1_alt", b"chr2", b"chr"} and st["n_unmatched"] > 0
    check_all(ltext, rtext, ks=(1, 5), mds=(None, 3))
    got, st = check(R.bed_text([(b"a", 0, 9)]), R.bed_text([(b"b", 0, 9)]))
    assert got["n_rows"] == 0 and st["n_unmatched"] == 1


def test_invalid_rows_on_both_sides():
    rows = R.seeded_bed(5, 40, n_chroms=2, span=200)
    invalid = [(b"chr1", None, 5), (b"chr1", 9, 3), (b"chr2", LIM, LIM), (b"chr1", -LIM - 1, 0), (b"chr2", 0, LIM), (b"chr1", b"1x", 5), (b"chr1", 3, None), (b"e", 1, b"")]
    ltext = R.bed_text(invalid[:3] + rows[:20] + invalid[3:])
    rtext = R.bed_text(rows[20:30] + invalid + rows[30:])
    got, st = check(ltext, rtext, 2)
    assert st["n_skipped"] == 8 and st["right"]["n_skipped"] == 8 and got["left_row"].min() == 3 and got["left_row"].max() == 22
    assert not set(got["right_row"].tolist()) & set(range(10, 18))
    check_all(ltext, rtext, ks=(1, 5, 3000), mds=(None, 0))
    got, st = check(ltext, R.bed_text(invalid))                                       # a right file without a valid row: its chroms have no rows
    assert got["n_rows"] == 0 and st["n_unmatched"] == 20


def test_files_read_one_block_a_batch():
    rows = sorted(R.seeded_bed(7, 6000, n_chroms=4, span=100000), key=lambda r: r[0])
    text = b"#head\n" + R.bed_text(rows)
    z = bgzf_file(text, payload=9000)
    part = R.bed_text(rows[:900])
    other = R.bed_text(R.seeded_bed(8, 60, n_chroms=5, span=100000, max_len=900))
    for ties in N.TIES:
        check(other, text, 3, None, ties, rsrc=z, max_blocks=1)
        check(part, other, 2, 500, ties, lsrc=bgzf_file(part, payload=3000), max_blocks=1)


def test_pages_of_every_size_give_one_result():
    right = R.seeded_bed(31, 300, n_chroms=2, span=400, max_len=60)
    left = [(b"zz", 0, 5), (b"zz", 1, 5)] + R.seeded_bed(32, 20, n_chroms=2, span=400) + [(b"zz", 3, 4), (b"chr1", 0, 1000)] + R.seeded_bed(33, 20, n_chroms=2, span=400) + [(b"zz", 7, 9)]
    ltext, rtext = R.bed_text(left), R.bed_text(right)
    per_row = np.bincount([r[3] for r in N.nearest(ltext, rtext, 2)], minlength=len(left))
    assert per_row[:2].tolist() == [0, 0] and per_row[22] == 0 and per_row[-1] == 0 and per_row[23] > 100
    for max_rows in (1, 2, 1000, 0):
        got, _ = check(ltext, rtext, 2, max_rows=max_rows)
        assert sum(got["pages"]) == got["n_rows"]
        if max_rows in (1, 2):
            at = np.cumsum([0] + got["pages"])
            for a, b in zip(at[:-1], at[1:]):
                rows = got["left_row"][a:b]
                assert b - a <= max_rows or len(np.unique(rows)) == 1              # more than max_rows rows only in a page of a single left row
                assert a == 0 or b == a or got["left_row"][a - 1] != rows[0]        # a cut falls between two left rows
            assert max(got["pages"]) == per_row[23] and len(got["pages"]) > 3
        check(ltext, rtext, 5, 3, "first", max_rows=max_rows)


def test_projections():
    ltext, rtext = R.bed_text(R.seeded_bed(41, 200, span=500)), R.bed_text(R.seeded_bed(42, 200, span=500))
    full = duckhts_amd.interval_nearest(ltext, rtext, k=3)
    for cols in (["distance"], ["chrom"], ["right_row", "left_row"], ["start", "right_end", "distance", "overlap"]):
        got = duckhts_amd.interval_nearest(ltext, rtext, k=3, columns=cols, max_rows=50)
        assert got["n_rows"] == full["n_rows"]
        for k in N.NEAREST_COLUMNS:
            assert (got[k] is None) == (k not in cols)
            if k in cols:
                assert list(got[k]) == list(full[k])


def test_the_stats_and_the_end_sort():
    ltext, rtext = R.bed_text(R.seeded_bed(51, 100, span=5000)), R.bed_text(R.seeded_bed(52, 100, span=5000))
    st, ost = {}, {}
    got = duckhts_amd.interval_nearest(ltext, rtext, k=2, max_distance=5, stats=st)
    duckhts_amd.interval_overlap(ltext, rtext, stats=ost)
    est = {}
    N.nearest(ltext, rtext, 2, 5, stats=est)
    assert st["n_pairs"] == got["n_rows"] == est["n_pairs"] and st["n_unmatched"] == est["n_unmatched"] > 0
    assert st["end_sort_passes"] > 0 and st["right"] == ost["right"] and st["right"]["sort_passes"] > 0      # the end sort leaves the right context's stats alone
    assert set(st) == {"n_rows", "n_skipped", "n_chroms", "n_name_runs", "sort_passes", "n_pairs", "n_unmatched", "end_sort_passes", "right"}


def test_distance_0_rows_are_the_overlapping_and_touching_ones():
    ltext, rtext = R.bed_text(R.seeded_bed(61, 300, span=6000)), R.bed_text(R.seeded_bed(62, 300, span=6000))
    got = duckhts_amd.interval_nearest(ltext, rtext, k=1, max_distance=0)
    exp = {r[3] for r in N.nearest(ltext, rtext, k=1 << 20) if r[8] == 0}
    assert set(got["left_row"].tolist()) == exp and 0 < len(exp) < 300 and not got["distance"].any()


def test_the_abi_states_refusals_and_the_switch_of_results():
    text = b"c\t0\t1\n"
    for k in (0, (1 << 20) + 1):
        with pytest.raises(duckhts_amd.DhtsError, match="^" + N.ERR_K + "$"):
            duckhts_amd.interval_nearest(text, text, k=k)
    with pytest.raises(duckhts_amd.DhtsError, match="^" + N.ERR_MAX_DISTANCE + "$"):
        duckhts_amd.interval_nearest(text, text, max_distance=-1)
    with pytest.raises(duckhts_amd.DhtsError, match="^" + N.ERR_TIES + "$"):
        duckhts_amd.interval_nearest(text, text, ties="any")
    with pytest.raises(duckhts_amd.DhtsError, match="^" + N.ERR_RIGHT_PATH + "$"):
        duckhts_amd.interval_nearest(text, None)
    ltext, rtext = b"c\t0\t10\nc\t5\t20\nd\t1\t2\n", b"c\t30\t40\nc\t12\t14\n"
    a, b = duckhts_amd.Context(0), duckhts_amd.Context(0)
    try:
        for c, t in ((a, ltext), (b, rtext)):
            c.open(t)
            c.L.dhts_bgzf_index(c.h)
            c._chk(c.L.dhts_bed_open(c.h))
        with pytest.raises(duckhts_amd.DhtsError, match="interval_nearest: dhts_ivl_load not called"):
            a.ivl_nearest_open(b)
        a.ivl_load()
        with pytest.raises(duckhts_amd.DhtsError, match="interval_nearest: dhts_ivl_nearest_open not called"):
            a.ivl_nearest_next()
        with pytest.raises(duckhts_amd.DhtsError, match="interval_nearest: dhts_ivl_nearest_open not called"):
            a.ivl_nearest_stats()
        with pytest.raises(duckhts_amd.DhtsError, match="interval_nearest: dhts_ivl_load not called on the right context"):
            a.ivl_nearest_open(b)
        with pytest.raises(duckhts_amd.DhtsError, match="interval_nearest: no right context"):
            a.ivl_nearest_open(None)
        b.ivl_load()
        before = b.ivl_stats()
        with pytest.raises(duckhts_amd.DhtsError, match="interval_nearest: ties must be 'all' or 'first'"):
            a._chk(a.L.dhts_ivl_nearest_open(a.h, b.h, 1, -1, 2))
        with pytest.raises(duckhts_amd.DhtsError, match="interval_nearest: k must be between 1 and 1048576"):
            a._chk(a.L.dhts_ivl_nearest_open(a.h, b.h, 0, -1, 0))
        with pytest.raises(duckhts_amd.DhtsError, match="interval_nearest: max_distance must not be negative"):
            a._chk(a.L.dhts_ivl_nearest_open(a.h, b.h, 1, -2, 0))
        # overlap and merge answer on the same contexts before and after a nearest result
        a.ivl_overlap_open(b, "any")
        ov, st = a.ivl_overlap_next()
        assert st == 1 and ov["right_row"].tolist() == [1] and ov["left_row"].tolist() == [1]
        a.ivl_nearest_open(b, 1)
        with pytest.raises(duckhts_amd.DhtsError, match="interval_overlap: dhts_ivl_overlap_open not called"):
            a.ivl_overlap_next()
        with pytest.raises(duckhts_amd.DhtsError, match="interval_merge: dhts_ivl_merge_open not called"):
            a.ivl_merge_next()
        cols, st = a.ivl_nearest_next()
        assert st == 1 and cols["left_row"].tolist() == [0, 1] and cols["right_row"].tolist() == [1, 1] and cols["distance"].tolist() == [2, 0] and cols["overlap"].tolist() == [0, 2]
        assert a.ivl_nearest_stats() == {"n_pairs": 2, "n_unmatched": 1, "end_sort_passes": a.ivl_nearest_stats()["end_sort_passes"], "status": 1}
        assert a.ivl_nearest_stats()["end_sort_passes"] > 0 and b.ivl_stats() == before and a.ivl_stats()["n_pairs"] == 0
        a.ivl_merge_open()
        with pytest.raises(duckhts_amd.DhtsError, match="interval_nearest: dhts_ivl_nearest_open not called"):
            a.ivl_nearest_next()
        cols, st = a.ivl_merge_next()
        assert st == 1 and cols["end"].tolist() == [20, 2]
        a.ivl_nearest_open(b, 2, 100, "first")                                   # the end order is there already
        cols, st = a.ivl_nearest_next(columns=["right_row", "distance"])
        assert cols["right_row"].tolist() == [1, 0, 1, 0] and cols["distance"].tolist() == [2, 20, 0, 10] and cols["chrom"] is None
        a.ivl_overlap_open(b, "any")
        with pytest.raises(duckhts_amd.DhtsError, match="interval_nearest: dhts_ivl_nearest_open not called"):
            a.ivl_nearest_next()
        assert a.ivl_overlap_next()[0]["n_rows"] == 1
        b.ivl_nearest_open(a, 1)                                                  # the roles swapped: a gets its end order
        assert b.ivl_nearest_next()[0]["right_row"].tolist() == [1, 1]
        a.ivl_nearest_open(b, 1)
        b.ivl_load()
        with pytest.raises(duckhts_amd.DhtsError, match="interval_nearest: the right context was loaded anew or closed since dhts_ivl_nearest_open"):
            a.ivl_nearest_next()
        a.ivl_nearest_open(b, 1)
        assert a.ivl_nearest_next()[0]["distance"].tolist() == [2, 0]
    finally:
        a.close()
        b.close()
