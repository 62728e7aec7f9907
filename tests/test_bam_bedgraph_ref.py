"""The CPU model of bam_bedgraph held against the identity that defines the function: without breaks, its rows expanded per position are
bam_depth_ref's positions (all_positions = 2 with zero_runs, 0 without), on every small case the device tests use; and the classes, on a table
written out by hand."""
import numpy as np
import pytest

import bam_bedgraph_cases as G
import bam_bedgraph_ref as M
import bam_depth_cases as D
import bam_depth_ref as DM

SMALL = {"tile_edges": G.tile_edges(), "row_lengths": G.row_lengths(), "classes": (G.CLASS_REFS, G.CLASS_READS), "gap": (G.GAP_REFS, G.GAP_READS),
         "touch": (G.TOUCH_REFS, G.TOUCH_READS), "hand": (D.HAND_REFS, D.HAND_READS)}


def expanded_equals_depth(reads, refs, rows=None, **kw):
    for zero_runs, mode in ((1, 2), (0, 0)):
        res = M.bedgraph(reads, refs, rows=rows, zero_runs=zero_runs, **kw)
        exp = DM.depth(reads, refs, rows=rows, all_positions=mode, **kw)
        tid, pos, depth = M.expand(res)
        assert tid.tolist() == exp["tid"] and pos.tolist() == exp["pos"] and depth.tolist() == exp["depth"]
        assert res["stats"] == exp["stats"]
        assert np.all(res["end"] > res["start"]) and (zero_runs or np.all(res["depth"] > 0))
        # maximal: two rows of one target row that touch differ in depth (here every contig is one target row unless rows are given)
        if rows is None:
            touch = (res["tid"][1:] == res["tid"][:-1]) & (res["start"][1:] == res["end"][:-1])
            assert np.all(res["depth"][1:][touch] != res["depth"][:-1][touch])


@pytest.mark.parametrize("name", sorted(SMALL))
@pytest.mark.parametrize("kw", [dict(), dict(min_baseq=20, include_deletions=1), dict(min_mapq=10, min_read_len=4, exclude_flags=0x704)])
def test_the_model_expanded_is_bam_depth(name, kw):
    refs, reads = SMALL[name]
    expanded_equals_depth(DM.reads_from_bam(G.bam(refs, reads))[1], refs, **kw)


def test_every_cigar_operation_and_low_bases():
    cigars = ["10M", "5M2D5M", "3S7M", "5M20N5M", "4M2I4M", "2H8M", "3M1P3M", "5=2X3=", "2D8M", "8M2D"]
    reads = [D.R(0, i % 3, 1000 + 7 * i, 30, cg, lambda k: 12 + (k * 5) % 17) for i, cg in enumerate(cigars)]
    _, mreads = DM.reads_from_bam(G.bam(G.REFS, reads))
    for kw in (dict(), dict(min_baseq=20), dict(include_deletions=1), dict(min_baseq=15, include_deletions=1)):
        expanded_equals_depth(mreads, G.REFS, **kw)


def test_rows_of_regions_and_of_a_bed():
    _, mreads = DM.reads_from_bam(G.bam(G.REFS, G.SEAM_READS))
    two = [(0, 90, 100), (0, 100, 110)]
    expanded_equals_depth(mreads, G.REFS, rows=two)
    res = M.bedgraph(mreads, G.REFS, rows=two)
    assert list(zip(res["tid"], res["start"], res["end"], res["depth"])) == [(0, 90, 100, 2), (0, 100, 110, 2)]        # a run never spans two rows
    res = M.bedgraph(mreads, G.REFS, rows=two[::-1])
    assert list(zip(res["start"], res["end"])) == [(100, 110), (90, 100)]                                              # the order the rows are answered in
    assert list(zip(*[M.bedgraph(mreads, G.REFS, rows=[(0, 90, 110)])[k] for k in ("start", "end", "depth")])) == [(90, 110, 2)]
    refs, mreads = DM.reads_from_bam(G.bam(G.TOUCH_REFS, G.TOUCH_READS))
    rows, skipped = M.merge_bed(G.TOUCH_BED, refs)
    assert rows == [(0, 100, 300), (0, 1500, 2600)] and skipped == 0
    expanded_equals_depth(mreads, G.TOUCH_REFS, rows=rows)
    res = M.bedgraph(mreads, G.TOUCH_REFS, rows=rows)
    assert list(zip(res["start"], res["end"], res["depth"])) == [(150, 250, 3), (1500, 2600, 1)]


def test_classes_on_the_hand_written_table():
    assert M.classes([0, 1, 2, 3, 4, 5, 149, 150, 2**31 - 1], [1, 5, 150]).tolist() == [0, 1, 1, 1, 1, 2, 2, 3, 3]
    assert M.class_depth([0, 1, 2, 3], [1, 5, 150]).tolist() == [0, 1, 5, 150]
    assert M.classes([0, 7], []).tolist() == [0, 7] and M.class_depth([0, 7], []).tolist() == [0, 7]
    assert M.parse_breaks("2,4") == [2, 4] and M.parse_breaks(None) == [] and M.parse_breaks([3]) == [3]
    _, mreads = DM.reads_from_bam(G.bam(G.CLASS_REFS, G.CLASS_READS))
    for (zero_runs, breaks), rows in G.CLASS_ROWS.items():
        res = M.bedgraph(mreads, G.CLASS_REFS, zero_runs=zero_runs, breaks=breaks)
        assert list(zip(res["tid"], res["start"], res["end"], res["depth"])) == rows
    # one omitted zero run between two emitted ones: the first ends where the zero run starts
    _, mreads = DM.reads_from_bam(G.bam(G.GAP_REFS, G.GAP_READS))
    res = M.bedgraph(mreads, G.GAP_REFS)
    assert list(zip(res["start"], res["end"], res["depth"])) == [(1000, 1020, 2), (2100, 2120, 2)]
    # an untouched contig: one row with zero_runs, none without
    res = M.bedgraph([], [("u", 77), ("e", 0)], zero_runs=1)
    assert list(zip(res["tid"], res["start"], res["end"], res["depth"])) == [(0, 0, 77, 0)] and M.bedgraph([], [("u", 77)])["n_rows"] == 0


def test_the_long_rows_stay_fast():
    for reads, kw, rows in ((G.LONG_ENDS, dict(zero_runs=1), [(0, 10, 1), (10, G.LONG - 10, 0), (G.LONG - 10, G.LONG, 1)]),
                            (G.LONG_DELETION, dict(include_deletions=1), [(20000, 20000 + 4250020, 1)]),
                            (G.LONG_DELETION, dict(), [(20000, 20010, 1), (4270010, 4270020, 1)])):
        _, mreads = DM.reads_from_bam(G.bam(G.LONG_REFS, reads))
        res = M.bedgraph(mreads, G.LONG_REFS, **kw)
        assert list(zip(res["start"], res["end"], res["depth"])) == rows
