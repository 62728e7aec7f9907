"""The CPU model of bam_depth on inputs whose results are written out by hand, against bam_coverage's model where the two must agree, and the
BED merge against literals."""
import pytest

import bam_coverage_cases as K
import bam_coverage_ref as CM
import bam_depth_cases as D
import bam_depth_ref as M


def rows_of(res):
    return list(zip(res["tid"], res["pos"], res["depth"]))


@pytest.fixture(scope="module")
def hand():
    return M.reads_from_bam(D.bam(D.HAND_REFS, D.HAND_READS))


def test_the_hand_written_table(hand):
    refs, reads = hand
    assert refs == [(n.encode(), l) for n, l in D.HAND_REFS]
    res = M.depth(reads, refs, **D.HAND_PARAMS)
    assert rows_of(res) == D.HAND_ROWS and res["stats"] == D.HAND_STATS and res["touched"] == D.HAND_TOUCHED
    assert rows_of(M.depth(reads, refs, include_deletions=1, **D.HAND_PARAMS)) == D.HAND_ROWS_DEL


@pytest.mark.parametrize("mode", [1, 2])
def test_the_hand_written_table_with_all_positions(hand, mode):
    refs, reads = hand
    res = M.depth(reads, refs, all_positions=mode, **D.HAND_PARAMS)
    assert rows_of(res) == D.hand_rows_all(mode) and res["n_rows"] == 60 + 30 + 0 + 8


def test_all_positions_1_leaves_an_untouched_contig_out(hand):
    refs, reads = hand
    # without the 4S read c4 is untouched: -a emits nothing of it, -aa all eight positions
    reads = reads[:9]
    one, two = M.depth(reads, refs, all_positions=1, **D.HAND_PARAMS), M.depth(reads, refs, all_positions=2, **D.HAND_PARAMS)
    assert one["n_rows"] == 90 and two["n_rows"] == 98 and rows_of(two)[90:] == [(3, p, 0) for p in range(1, 9)]


def test_a_deletion_counts_whatever_the_qualities_are():
    refs = [(b"c1", 1000)]
    for low in ({19}, {20}, {19, 20}, set(range(40))):
        reads = M.reads_from_bam(K.bam([("c1", 1000)], [K.read(0, 0, 100, 30, "20M3D20M", [3 if k in low else 30 for k in range(40)])]))[1]
        res = M.depth(reads, refs, min_baseq=20, include_deletions=1)
        assert [p for p in res["pos"] if 121 <= p <= 123] == [121, 122, 123] and res["n_rows"] == 43 - len(low)
        assert not [p for p in M.depth(reads, refs, min_baseq=20)["pos"] if 121 <= p <= 123]


@pytest.mark.parametrize("kw", [dict(), dict(min_baseq=20), dict(min_mapq=25, min_read_len=5), dict(exclude_flags=0)], ids=str)
def test_without_deletions_the_depths_are_bam_coverages(hand, kw):
    refs, reads = hand
    rows = [(0, 5, 50), (1, 0, 30), (0, 50, 60)]
    assert M.depth(reads, refs, rows=rows, **kw)["per_row"] == CM.coverage(reads, refs, rows=rows, **kw)["depth"]
    assert M.depth(reads, refs, **kw)["stats"] == CM.coverage(reads, refs, **kw)["stats"]
    refs2, reads2 = M.reads_from_bam(K.bam(K.HAND_REFS, K.HAND_READS))
    assert M.depth(reads2, refs2, **kw)["per_row"] == CM.coverage(reads2, refs2, **kw)["depth"]


def test_regions_are_answered_in_the_order_given(hand):
    refs, reads = hand
    res = M.depth(reads, refs, rows=[(0, 42, 44), (0, 10, 12)], **D.HAND_PARAMS)
    assert rows_of(res) == [(0, 43, 1), (0, 44, 1), (0, 11, 1), (0, 12, 1)]


def test_the_bed_merge():
    refs = [(n.encode(), l) for n, l in D.BED_REFS]
    assert M.merge_bed(D.BED_ROWS, refs) == (D.BED_MERGED, D.BED_SKIPPED)
    assert M.merge_bed([], refs) == ([], 0)
    assert M.merge_bed([(b"c1", 0, 10), (b"c1", 10, 20)], refs) == ([(0, 0, 20)], 0)                    # adjacent
    assert M.merge_bed([(b"c1", 0, 10), (b"c1", 11, 20)], refs) == ([(0, 0, 10), (0, 11, 20)], 0)      # a gap of one base
    assert M.merge_bed([(b"c1", 5, 50), (b"c1", 10, 20), (b"c1", 5, 50)], refs) == ([(0, 5, 50)], 0)  # nested, duplicate
    assert M.parse_bed(D.bed_text(D.BED_ROWS)) == D.BED_ROWS
    assert M.table_bytes(D.BED_MERGED) == 6 * 4096 and M.err_table(8192, 4096).startswith("bam_depth: the depth table needs 8192 bytes")
