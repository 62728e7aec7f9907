"""interval_merge and interval_overlap on the device (dhts_ivl_*, csrc/interval_sort.hip, csrc/interval_algebra.hip) through the Python
functions against the brute-force model interval_ref, row for row and column for column: plain and bgzipped files, rows, row numbers and name
runs that cross batches, chrom names that are prefixes of each other, the walk back over 64-row blocks, every edge of the predicates, empty and
negative and huge rows, CRLF and meta lines, read_bed's error, pages of every size, projections and the stats."""
import numpy as np
import pytest

import duckhts_amd
import interval_ref as R
from bamwriter import bgzf_file

pytestmark = pytest.mark.gpu
LIM = 1 << 62


def same(got, exp_rows, names):
    exp = R.columns(exp_rows, names)
    assert got["n_rows"] == exp["n_rows"] == sum(got["pages"])
    assert got["chrom"] == exp["chrom"]
    for k in names[1:]:
        assert got[k].dtype == np.int64 and len(got[k]) == exp["n_rows"], k
        bad = np.flatnonzero(got[k] != exp[k])
        assert not len(bad), (k, bad[:5].tolist(), got[k][bad[:5]].tolist(), exp[k][bad[:5]].tolist())


def check_merge(text, max_gap=0, src=None, **kw):
    st = {}
    got = duckhts_amd.interval_merge(text if src is None else src, max_gap=max_gap, stats=st, **kw)
    exp = R.merge(text, max_gap)
    same(got, exp, R.MERGE_COLUMNS)
    assert got["status"] == 1 and st["n_runs"] == len(exp)
    assert {k: st[k] for k in ("n_rows", "n_skipped", "n_chroms")} == R.table_stats(text)
    return got, st


def check_overlap(left, right, mode="any", lsrc=None, rsrc=None, **kw):
    st = {}
    got = duckhts_amd.interval_overlap(left if lsrc is None else lsrc, right if rsrc is None else rsrc, mode=mode, stats=st, **kw)
    exp = R.overlap(left, right, mode)
    same(got, exp, R.OVERLAP_COLUMNS)
    assert got["status"] == 1 and st["n_pairs"] == len(exp)
    assert {k: st[k] for k in ("n_rows", "n_skipped", "n_chroms")} == R.table_stats(left)
    assert {k: st["right"][k] for k in ("n_rows", "n_skipped", "n_chroms")} == R.table_stats(right)
    return got, st


def check_all(left, right, **kw):
    n = 0
    for mode in R.MODES:
        n += check_overlap(left, right, mode, **kw)[0]["n_rows"]
    check_merge(left)
    check_merge(right, 3)
    return n


@pytest.mark.parametrize("n", (1, 7, 64, 65, 2000))
def test_seeded_files_plain_and_bgzipped(n, tmp_path):
    right = R.seeded_bed(100 + n, n)
    left = R.seeded_bed(200 + n, 30) + right[:5] + [(c, s, s) for c, s, e in right[:3]] + [(c, e, e) for c, s, e in right[:2]]
    ltext, rtext = R.bed_text(left), R.bed_text(right)
    assert check_all(ltext, rtext) > 0 or n == 1
    lp, rp = tmp_path / "l.bed", tmp_path / "r.bed.gz"
    lp.write_bytes(ltext)
    rp.write_bytes(bgzf_file(rtext))
    for mode in R.MODES:
        check_overlap(ltext, rtext, mode, lsrc=str(lp), rsrc=str(rp))
    check_merge(rtext, src=str(rp))
    check_merge(ltext, 7, src=bgzf_file(ltext))


def test_rows_and_name_runs_cross_batches():
    """a bgzipped file of several BGZF blocks read one block a batch: lines, row numbers and runs of one chrom span the batches"""
    rows = sorted(R.seeded_bed(7, 6000, n_chroms=4, span=100000), key=lambda r: r[0])
    text = b"#head\n" + R.bed_text(rows)
    z = bgzf_file(text, payload=9000)
    nblocks = -(-len(text) // 9000)
    assert nblocks > 8
    got, st = check_merge(text, src=z, max_blocks=1)
    assert R.name_runs(text) == 4 and 4 < st["n_name_runs"] <= 4 + nblocks        # one head per batch beside the chrom changes
    _, st1 = check_merge(text, src=z)
    assert st1["n_name_runs"] == 4
    other = R.bed_text(R.seeded_bed(8, 300, n_chroms=5, span=100000, max_len=900))
    for mode in R.MODES:
        check_overlap(text, other, mode, lsrc=z, max_blocks=1)
        check_overlap(other, text, mode, rsrc=z, max_blocks=1)


def test_a_chrom_that_changes_on_every_line():
    rows = [(b"c%d" % (i % 37), (i * 7919) % 5000, (i * 7919) % 5000 + i % 50) for i in range(3000)]
    text = R.bed_text(rows)
    _, st = check_merge(text)
    assert st["n_name_runs"] == 3000 and st["n_chroms"] == 37
    check_all(text, R.bed_text(rows[::-1][:500]))


def test_chroms_on_one_side_and_names_that_are_prefixes():
    names = [b"chr1", b"chr10", b"chr1_alt", b"chr2", b"chr", b"chr1\xff", b"Chr1"]
    left = R.seeded_bed(1, 400, names=names[:5], span=300)
    right = R.seeded_bed(2, 400, names=names[2:], span=300)
    ltext, rtext = R.bed_text(left), R.bed_text(right)
    assert check_all(ltext, rtext) > 0
    got, _ = check_merge(ltext + rtext)
    seen = list(dict.fromkeys(got["chrom"]))
    assert seen == sorted(names) and seen.index(b"chr1") < seen.index(b"chr10") < seen.index(b"chr1_alt") < seen.index(b"chr1\xff")
    assert check_overlap(R.bed_text([(b"a", 0, 9)]), R.bed_text([(b"b", 0, 9)]))[0]["n_rows"] == 0


def test_the_walk_back_reaches_a_row_that_spans_its_chrom():
    """the first right row spans the chrom, so the running maximum end admits it from every query; the short rows around 64-row block
    edges are hit on both sides of an edge, and whole blocks in between are skipped"""
    right = [(b"c", 0, 10 ** 6)] + [(b"c", 10 * i, 10 * i + 5) for i in range(1, 400)] + [(b"d", 5, 6)]
    left = [(b"c", 10 * i - 3, 10 * i + 12) for i in (1, 62, 63, 64, 65, 127, 128, 129, 255, 256, 399)] + [(b"c", 625, 1295), (b"c", 999999, 10 ** 6), (b"c", 10 ** 6, 10 ** 6 + 5), (b"d", 0, 100)]
    ltext, rtext = R.bed_text(left), R.bed_text(right)
    got, _ = check_overlap(ltext, rtext)
    assert (np.bincount(got["left_row"], minlength=len(left))[:11] >= 2).all() and 0 in got["right_row"][got["left_row"] == 12]
    check_all(ltext, rtext)
    check_all(rtext, ltext)


def test_touching_rows_and_the_edges_of_the_predicates():
    right = [(b"c", 10, 20)]
    left = [(b"c", a, b) for a in (0, 9, 10, 11, 19, 20, 21) for b in (9, 10, 11, 19, 20, 21, 30) if b >= a]
    ltext, rtext = R.bed_text(left), R.bed_text(right)
    check_all(ltext, rtext)
    check_all(rtext, ltext)
    assert check_overlap(R.bed_text([(b"c", 0, 10)]), R.bed_text([(b"c", 10, 20)]))[0]["n_rows"] == 0        # rows that touch are no pair ...
    assert check_merge(R.bed_text([(b"c", 10, 20), (b"c", 0, 10)]))[0]["n_merged"].tolist() == [2]           # ... and one run
    assert check_merge(R.bed_text([(b"c", 0, 10), (b"c", 15, 20)]), 5)[0]["n_rows"] == 1
    assert check_merge(R.bed_text([(b"c", 0, 10), (b"c", 16, 20)]), 5)[0]["n_rows"] == 2


def test_empty_negative_and_huge_rows():
    rows = [(b"c", 5, 5), (b"c", 0, 10), (b"c", -50, -40), (b"c", -45, 5), (b"c", -(LIM - 1), LIM - 1), (b"c", LIM - 1, LIM - 1), (b"c", -(LIM - 1), -(LIM - 1)),
            (b"c", -LIM, -LIM), (b"c", 5, 10), (b"c", 10, 10), (b"c", 0, 0)]
    text = R.bed_text(rows)
    check_all(text, text)
    check_merge(text, 1 << 40)
    invalid = [(b"c", None, 5), (b"c", 9, 3), (b"c", LIM, LIM), (b"c", -LIM - 1, 0), (b"c", 0, LIM), (b"c", b"1x", 5), (b"c", 3, None), (b"e", 1, b"")]
    mixed = R.bed_text(invalid[:4] + rows + invalid[4:])
    got, st = check_merge(mixed)
    assert st["n_skipped"] == 8 and st["n_rows"] == 19 and st["n_chroms"] == 2
    got, st = check_overlap(mixed, text)
    assert got["left_row"].min() == 4 and st["n_skipped"] == 8
    check_overlap(text, mixed, "within")


def test_crlf_meta_lines_and_the_short_line():
    text = b"track name=x\r\n#c\r\nc\t0\t10\r\n\r\nbrowser position\r\nc\t5\t20\textra\r\nd\t1\t2\r\n#tail\r\nc\t20\t25"
    got, st = check_merge(text)
    assert got["chrom"] == [b"c", b"d"] and got["end"].tolist() == [25, 2] and st["n_rows"] == 4
    check_all(text, b"c\t9\t10\nd\t0\t9\r\n")
    for bad in (b"c\t0\t10\nc\t5\n", b"c\t0\t10\n#x\n\nc\t5\nc\t7\t9\n"):
        line = bad.split(b"\n").index(b"c\t5") + 1
        with pytest.raises(duckhts_amd.DhtsError, match=r"read_bed: BED line has fewer than 3 tab-delimited fields \(line %d\)" % line):
            duckhts_amd.interval_merge(bad)
        with pytest.raises(duckhts_amd.DhtsError, match=r"fewer than 3 tab-delimited fields \(line %d\)" % line):
            duckhts_amd.interval_overlap(b"c\t0\t1\n", bad)
    assert duckhts_amd.interval_merge(b"")["n_rows"] == 0 and duckhts_amd.interval_merge(b"#only\n")["n_rows"] == 0
    assert duckhts_amd.interval_overlap(b"", b"c\t0\t1\n")["n_rows"] == 0 and duckhts_amd.interval_overlap(b"c\t0\t1\n", b"\n")["n_rows"] == 0


def test_pages_of_every_size_give_one_result():
    right = R.seeded_bed(31, 300, n_chroms=2, span=400, max_len=60)
    # left rows with no pair at the start, in the middle and at the end (chrom zz is not on the right), and one with very many pairs
    left = [(b"zz", 0, 5), (b"zz", 1, 5)] + R.seeded_bed(32, 20, n_chroms=2, span=400) + [(b"zz", 3, 4), (b"chr1", 0, 1000)] + R.seeded_bed(33, 20, n_chroms=2, span=400) + [(b"zz", 7, 9)]
    ltext, rtext = R.bed_text(left), R.bed_text(right)
    exp = R.overlap(ltext, rtext)
    per_row = np.bincount([r[3] for r in exp], minlength=len(left))
    assert per_row[:2].tolist() == [0, 0] and per_row[22] == 0 and per_row[-1] == 0 and per_row[23] > 100
    for max_rows in (1, 7, 0):
        got, _ = check_overlap(ltext, rtext, max_rows=max_rows)
        if max_rows:
            # a page is whole left rows: it holds more than max_rows rows only when it is a single left row
            at = np.cumsum([0] + got["pages"])
            for a, b in zip(at[:-1], at[1:]):
                rows = got["left_row"][a:b]
                assert b - a <= max_rows or len(np.unique(rows)) == 1
                assert a == 0 or b == a or got["left_row"][a - 1] != rows[0]         # a cut falls between two left rows
            assert max(got["pages"]) == per_row[23] and len(got["pages"]) > 3
        for mode in ("contain", "within"):
            check_overlap(ltext, rtext, mode, max_rows=max_rows)
        check_merge(rtext, max_rows=max_rows)
    assert check_merge(R.bed_text([(b"c", 10 * i, 10 * i + 5) for i in range(20)]), max_rows=7)[0]["pages"] == [7, 7, 6]


def test_projections():
    ltext, rtext = R.bed_text(R.seeded_bed(41, 200, span=500)), R.bed_text(R.seeded_bed(42, 200, span=500))
    full = duckhts_amd.interval_overlap(ltext, rtext)
    for cols in (["overlap"], ["chrom"], ["right_row", "left_row"], ["start", "right_end"]):
        got = duckhts_amd.interval_overlap(ltext, rtext, columns=cols, max_rows=50)
        assert got["n_rows"] == full["n_rows"]
        for k in R.OVERLAP_COLUMNS:
            assert (got[k] is None) == (k not in cols)
            if k in cols:
                assert list(got[k]) == list(full[k])
    fm = duckhts_amd.interval_merge(ltext)
    got = duckhts_amd.interval_merge(ltext, columns=["n_merged", "chrom"])
    assert got["start"] is None and got["end"] is None and got["chrom"] == fm["chrom"] and got["n_merged"].tolist() == fm["n_merged"].tolist()


def test_the_abi_states_and_refusals():
    for bad in (-1, (1 << 40) + 1):
        with pytest.raises(duckhts_amd.DhtsError, match="^interval_merge: max_gap must be between 0 and 1099511627776$"):
            duckhts_amd.interval_merge(b"c\t0\t1\n", max_gap=bad)
    with pytest.raises(duckhts_amd.DhtsError, match="^interval_overlap: mode must be 'any', 'contain' or 'within'$"):
        duckhts_amd.interval_overlap(b"c\t0\t1\n", b"c\t0\t1\n", mode="touch")
    a, b = duckhts_amd.Context(0), duckhts_amd.Context(0)
    try:
        with pytest.raises(duckhts_amd.DhtsError, match="dhts_ivl_load: dhts_bed_open not called"):
            a.ivl_load()
        for c in (a, b):
            c.open(b"c\t0\t10\nc\t5\t20\n")
            c.L.dhts_bgzf_index(c.h)
            c._chk(c.L.dhts_bed_open(c.h))
        with pytest.raises(duckhts_amd.DhtsError, match="interval_merge: dhts_ivl_load not called"):
            a.ivl_merge_open()
        a.ivl_load()
        with pytest.raises(duckhts_amd.DhtsError, match="interval_merge: dhts_ivl_merge_open not called"):
            a.ivl_merge_next()
        with pytest.raises(duckhts_amd.DhtsError, match="interval_overlap: dhts_ivl_overlap_open not called"):
            a.ivl_overlap_next()
        with pytest.raises(duckhts_amd.DhtsError, match="interval_overlap: dhts_ivl_load not called on the right context"):
            a.ivl_overlap_open(b)
        with pytest.raises(duckhts_amd.DhtsError, match="interval_overlap: no right context"):
            a.ivl_overlap_open(None)
        with pytest.raises(duckhts_amd.DhtsError, match="interval_overlap: mode must be"):
            a._chk(a.L.dhts_ivl_overlap_open(a.h, a.h, 3))
        with pytest.raises(duckhts_amd.DhtsError, match="interval_merge: max_gap must be between"):
            a._chk(a.L.dhts_ivl_merge_open(a.h, -1))
        b.ivl_load()
        a.ivl_overlap_open(b, "any")
        cols, st = a.ivl_overlap_next()
        assert st == 1 and cols["n_rows"] == 4 and a.ivl_stats()["n_pairs"] == 4 and a.ivl_stats()["n_runs"] == 0
        a.ivl_merge_open()                                                       # a merge on a loaded table after an overlap, and the other way round
        cols, st = a.ivl_merge_next()
        assert st == 1 and cols["end"].tolist() == [20] and a.ivl_stats()["n_runs"] == 1
        assert a.ivl_chrom_names() == [b"c"] and a.ivl_stats()["sort_passes"] == 1
    finally:
        a.close()
        b.close()
