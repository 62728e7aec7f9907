"""The CPU model of bam_bedcov (bam_bedcov_ref) against per-base depth arrays on the golden file and against a table written out by hand."""
import numpy as np
import pytest

import bam_bedcov_cases as K
import bam_bedcov_ref as M
import orc
import read_bed_ref as B
from conftest import read_golden


def depth_arrays(c, count_deletions, count_ref_skips, **flt):
    """independent of the model's walk: every read's CIGAR is expanded into one letter per reference position; depth[tid][x] counts the
    letters that are depth, (beg, end) per contig are the read intervals"""
    n_ref = c["n_ref"]
    size = [int(n) + 4096 for n in c["ref_len"]]
    depth = [np.zeros(n, np.int64) for n in size]
    ivs = [[] for _ in range(n_ref)]
    yes = set("M=X") | ({"D"} if count_deletions else set()) | ({"N"} if count_ref_skips else set())
    for i in range(c["n_rows"]):
        flag, tid, pos0, mapq = int(c["FLAG"][i]), int(c["tid"][i]), int(c["POS"][i]) - 1, int(c["MAPQ"][i])
        if flag & flt.get("exclude_flags", 0) or mapq < flt.get("min_mapq", 0) or tid < 0 or pos0 < 0:
            continue
        letters = "" if flag & 4 else "".join(op * n for n, op in M.cigar_ops(c["CIGAR"][i]) if op in "MDN=X")
        mask = np.array([ch in yes for ch in letters], bool)
        depth[tid][pos0:pos0 + len(letters)] += mask
        ivs[tid].append((pos0, pos0 + max(1, len(letters))))
    return depth, ivs


@pytest.mark.parametrize("count_deletions,count_ref_skips", K.OPTIONS)
@pytest.mark.parametrize("flt", [dict(), dict(min_mapq=1, exclude_flags=0x10)], ids=["all", "filtered"])
def test_model_against_depth_arrays(count_deletions, count_ref_skips, flt):
    c = orc.bam_read(read_golden("range.bam"))
    assert c["n_rows"] == 112
    got = M.bedcov(c, c["ref_names"], K.GOLDEN_BED, count_deletions=count_deletions, count_ref_skips=count_ref_skips, **flt)
    bed = B.read_bed(K.GOLDEN_BED)
    assert got["n_rows"] == bed["n_rows"] == 14
    depth, ivs = depth_arrays(c, count_deletions, count_ref_skips, **flt)
    names = list(c["ref_names"])
    some = 0
    for r in range(14):
        chrom, s, e = bed["chrom"][r], bed["start"][r], bed["end"][r]
        bases = count = 0
        if chrom in names and s is not None and e is not None and e > s:
            t = names.index(chrom)
            bases = int(depth[t][max(s, 0):max(e, 0)].sum())
            count = sum(1 for p, q in ivs[t] if p < e and q > s)
        assert (got["bases_covered"][r], got["read_count"][r]) == (bases, count), r
        some += bases > 0
    assert some >= 4                                                     # (the check is not vacuous: rows with depth exist under either filter)
    assert [got[k] for k in M.COLUMNS[:6]] == [bed[k] for k in M.COLUMNS[:6]]
    assert sum(v for k, v in got["stats"].items() if k != "n_rows") == got["stats"]["n_rows"] == 112
    if not flt:
        assert got["stats"]["n_counted"] == 112
        # two reads of the file have a deletion: the whole-contig sums differ by their two bases
        whole = M.bedcov(c, c["ref_names"], b"CHROMOSOME_II\t0\t5000\nCHROMOSOME_I\t0\t2000000\nCHROMOSOME_III\t0\t5000\nCHROMOSOME_IV\t0\t5000\n",
                         count_deletions=count_deletions, count_ref_skips=count_ref_skips)
        assert sum(whole["read_count"]) == 112
        assert sum(whole["bases_covered"]) == 108 * 100 + 100 + 100 + 28 + 99 + (2 if count_deletions else 0)


@pytest.mark.parametrize("k", range(4))
def test_model_against_the_hand_written_table(k):
    cd, cs = K.OPTIONS[k]
    data = K.bam(K.REFS, K.HAND_ROWS)
    c = orc.bam_read(data)
    assert c["n_rows"] == len(K.HAND_ROWS) and [bytes(x) for x in c["CIGAR"]] == [r[4].encode() for r in K.HAND_ROWS]
    got = M.bedcov(c, c["ref_names"], K.HAND_BED, count_deletions=cd, count_ref_skips=cs, **K.HAND_PARAMS)
    assert got["stats"] == K.HAND_STATS
    assert K.pairs(got) == [row[k] for row in K.HAND_EXPECTED]


def test_read_geometry():
    g = M.read_geometry
    assert g(0, 10, "5M2D5M2D5M") == (19, [(10, 29)])
    assert g(0, 10, "5M2D5M2D5M", count_deletions=False) == (19, [(10, 15), (17, 22), (24, 29)])
    assert g(0, 10, "5M100N5M", count_ref_skips=False) == (110, [(10, 15), (115, 120)])
    assert g(0, 10, "5M3D2N5M", False, True) == (15, [(10, 15), (18, 25)])
    assert g(0, 10, "2H5M1P5M3S") == (10, [(10, 20)]) and g(0, 10, "2H5M1P5M3S", False, False) == (10, [(10, 20)])
    assert g(0, 10, "5M0D5M", False, False) == (10, [(10, 20)])                  # an operation of length 0 covers nothing and parts nothing
    assert g(0, 10, "4S") == (0, []) and g(0, 10, "*") == (0, []) and g(0, 10, b"*") == (0, [])
    assert g(0, 10, "3D") == (3, [(10, 13)]) and g(0, 10, "3D", count_deletions=False) == (3, [])
    assert g(4, 10, "10M") == (0, [])
