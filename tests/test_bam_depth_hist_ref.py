"""The CPU model of bam_depth_hist (bam_depth_hist_ref) held to itself and to bam_bedgraph_ref, on every case of bam_depth_hist_cases: the summed
run lengths of bedgraph(zero_runs = 1) per group and min(depth, depth_cap) are n_positions; n_at_least of a group's lowest bin and the sum of its
n_positions are its length; the groups, a few results by hand, and the bytes of the histogram table."""
import numpy as np
import pytest

import bam_bedgraph_ref as B
import bam_depth_hist_cases as H
import bam_depth_hist_ref as M


def built(name):
    case = H.ALL[name]()
    refs, reads = M.reads_from_bam(H.bam(case["refs"], case["reads"]))
    if "region" in case:
        rows = H.rows_of_region(refs, case["region"])
    elif "bed" in case:
        rows, _ = M.merge_bed(case["bed"], refs)
    else:
        rows = [(t, 0, l) for t, (_, l) in enumerate(refs)]
    return refs, reads, rows


@pytest.fixture(scope="module")
def cases():
    return {name: built(name) for name in H.ALL}


@pytest.mark.parametrize("per", H.PERS)
@pytest.mark.parametrize("name", sorted(H.ALL))
def test_the_model_against_the_bedgraph_model_and_itself(cases, name, per):
    refs, reads, rows = cases[name]
    runs = B.bedgraph(reads, refs, rows=rows, zero_runs=1, exclude_flags=M.DEFAULT_EXCLUDE)
    for cap in ((1, 5, 1000) + (H.CAPS if name == "stack" else ())):
        got = M.hist(reads, refs, rows=rows, depth_cap=cap, per=per, exclude_flags=M.DEFAULT_EXCLUDE)
        exp = M.from_bedgraph(runs, rows, cap, per)
        for k in M.COLUMNS:
            assert np.array_equal(got[k], exp[k]), (k, cap)
        assert got["stats"] == runs["stats"] and got["n_rows"] > 0 and got["depth"].max() <= cap and got["n_positions"].min() > 0
        # per group: ascending bins, the lowest bin's n_at_least and the sum of n_positions are the length
        key = list(zip(got["tid"].tolist(), got["start"].tolist(), got["end"].tolist()))
        assert len(set(key)) == got["n_groups"] == len(M.groups_of(rows, per))
        for g in set(key):
            sel = np.array([k == g for k in key])
            d, n, al, ln = got["depth"][sel], got["n_positions"][sel], got["n_at_least"][sel], got["length"][sel]
            assert (np.diff(d) > 0).all() and al[0] == ln[0] == n.sum() and (ln == ln[0]).all() and al[-1] == n[-1]
            assert np.array_equal(al, np.cumsum(n[::-1])[::-1])


def test_groups():
    rows = [(0, 300, 400), (0, 90, 100), (2, 100, 100), (1, 0, 200), (0, 5000, 5050)]
    assert M.groups_of(rows, "row") == [(0, 300, 400, 100, [0]), (0, 90, 100, 10, [1]), (1, 0, 200, 200, [3]), (0, 5000, 5050, 50, [4])]
    assert M.groups_of(rows, "contig") == [(0, 90, 5050, 160, [1, 0, 4]), (1, 0, 200, 200, [3])]
    assert M.hist_bytes(rows, 1000, "row") == 4 * 1001 * 8 and M.hist_bytes(rows, 1000, "contig") == 2 * 1001 * 8
    # the intended steer: 200,000 targets at the default cap are past 1 GiB per row and fit per contig
    targets = [(t % 24, 1000 * (t // 24), 1000 * (t // 24) + 200) for t in range(200000)]
    assert M.hist_bytes(targets, 1000, "row") > M.MAX_HIST_BYTES > M.hist_bytes(targets, 1000, "contig")


def test_results_by_hand():
    refs, reads = M.reads_from_bam(H.bam([("k", 400), ("u", 7)], H.at(0, 100, 40) + H.at(0, 110, 30) + H.at(0, 110, 10) + H.at(0, 130, 10, 3)))
    got = M.hist(reads, refs, exclude_flags=M.DEFAULT_EXCLUDE)                 # depth 1 on 100 .. 109, 3 on 110 .. 119, 2 on 120 .. 129, 5 on 130 .. 139
    rows = list(zip(*(got[k].tolist() for k in M.COLUMNS)))
    assert rows == [(0, 0, 400, 0, 360, 400, 400), (0, 0, 400, 1, 10, 40, 400), (0, 0, 400, 2, 10, 30, 400), (0, 0, 400, 3, 10, 20, 400), (0, 0, 400, 5, 10, 10, 400),
                    (1, 0, 7, 0, 7, 7, 7)]                                     # an untouched contig: the single row (chrom, 0, L, 0, L, L, L)
    got = M.hist(reads, refs, depth_cap=2, exclude_flags=M.DEFAULT_EXCLUDE)
    assert list(zip(*(got[k].tolist() for k in M.COLUMNS)))[:3] == [(0, 0, 400, 0, 360, 400, 400), (0, 0, 400, 1, 10, 40, 400), (0, 0, 400, 2, 30, 30, 400)]
    stacked = M.hist(*M.reads_from_bam(H.bam(*[H.stack()[k] for k in ("refs", "reads")]))[::-1], depth_cap=5000, exclude_flags=M.DEFAULT_EXCLUDE)
    # the stack stands on depth 1 (700 .. 799); 4,096 reads on 2000 .. 2004 and one more on 2002; the untouched contig's row comes last
    assert stacked["depth"].tolist()[-4:] == [H.LDS, H.LDS + 1, H.STACK + 1, 0] and stacked["n_positions"].tolist()[-4:] == [4, 1, 1, 10]
