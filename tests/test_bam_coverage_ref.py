"""The CPU model of bam_coverage (bam_coverage_ref) held to a table worked out by hand and to numpy depth arrays built straight from the
golden file's CIGAR and QUAL columns."""
import numpy as np
import pytest

import bam_coverage_cases as K
import bam_coverage_ref as M
import orc
from conftest import read_golden


def test_hand_written_table():
    data = K.bam(K.HAND_REFS, K.HAND_READS)
    refs, reads = M.reads_from_bam(data)
    assert refs == [(n.encode(), l) for n, l in K.HAND_REFS] and len(reads) == len(K.HAND_READS)
    got = M.coverage(reads, refs, **K.HAND_PARAMS)
    assert got["stats"] == K.HAND_STATS and got["n_rows"] == 3
    for r, exp in enumerate(K.HAND_EXPECTED):
        assert tuple(got[k][r] for k in M.COLUMNS + M.SUMS) == exp, r
    # the file's own bytes and the columns of a read_bam result describe the same reads
    assert M.reads_from_cols(orc.bam_read(data)) == reads


def test_hand_table_without_thresholds():
    refs, reads = M.reads_from_bam(K.bam(K.HAND_REFS, K.HAND_READS))
    got = M.coverage(reads, refs, exclude_flags=0x704)
    # reads 4 and 5 come in (10..19 and 10..12), read 1's second half and position 97 count: 26 + 10 + 3 + 5 + 1 bases
    assert got["sum_depth"] == [45, 5, 0] and got["numreads"] == [7, 1, 0] and got["covbases"][0] == 17 + 4            # 10..26 and 95..98
    assert got["stats"]["n_counted"] == 8 and got["stats"]["n_short"] == 0 and got["stats"]["n_low_mapq"] == 0


def test_rows_and_ratios():
    refs, reads = M.reads_from_bam(K.bam(K.HAND_REFS, K.HAND_READS))
    rows = [(0, 15, 20), (0, 20, 23), (1, 48, 50), (0, 60, 60)]
    got = M.coverage(reads, refs, rows=rows, exclude_flags=0x704)
    assert got["numreads"] == [4, 2, 1, 0]                                  # [15, 20): reads 0, 1, 2, 4 (5 ends at 13); [20, 23): read 1 (its deletion counts for the interval) and 2
    assert got["sum_depth"] == [5 * 2 + 5 + 2, 1 + 3, 2, 0]                 # 15..19: reads 0 and 4 five each, read 1 five, read 2 two; 20..22: read 1 at 22, read 2 three times
    assert got["coverage"] == [100.0, 100.0, 100.0, 0.0] and got["meandepth"][3] == 0.0
    assert M.ratio(1, 3) == float(np.float64(1) / np.float64(3)) and M.ratio(5, 0) == 0.0


def test_cg_tag_and_raw_qualities():
    reads = [K.read(0, 0, 100, 30, "1S1N", cg="4M2D4M", qual=[1, 2, 3, 4, 5, 6, 7, 255]), K.read(0, 0, 200, 30, "4M", raw_qual=b"\xff" * 4, qual=0)]
    _, got = M.reads_from_bam(K.bam(K.REFS, reads))
    assert got[0][5] == [(4, "M"), (2, "D"), (4, "M")] and got[0][6] == bytes([1, 2, 3, 4, 5, 6, 7, 255]) and got[1][6] == b"\xff" * 4
    res = M.coverage(got, [(b"c1", 100000)], min_baseq=4)
    assert res["sum_depth"] == [5 + 4] and res["sum_baseq"] == [4 + 5 + 6 + 7 + 255 + 4 * 255] and sorted(res["depth"][0]) == [103, 106, 107, 108, 109, 200, 201, 202, 203]


@pytest.mark.parametrize("min_baseq", [0, 20, 30])
def test_golden_file_against_numpy_depth(min_baseq):
    """depth arrays made with numpy slices from the CIGAR and QUAL text of the golden file: another way to the same numbers"""
    c = orc.bam_read(read_golden("range.bam"))
    names, lens = list(c["ref_names"]), [int(x) for x in c["ref_len"]]
    refs = [(n.encode() if isinstance(n, str) else bytes(n), l) for n, l in zip(names, lens)]
    depth = [np.zeros(l, np.int64) for l in lens]
    sum_q, nreads, sum_mq = [0] * len(refs), [0] * len(refs), [0] * len(refs)
    for i in range(c["n_rows"]):
        flag, tid, pos0, mapq = int(c["FLAG"][i]), int(c["tid"][i]), int(c["POS"][i]) - 1, int(c["MAPQ"][i])
        if flag & 0x704 or tid < 0 or pos0 >= lens[tid]:
            continue
        nreads[tid] += 1
        sum_mq[tid] += mapq
        qual = np.frombuffer(c["QUAL"][i].encode("latin-1") if isinstance(c["QUAL"][i], str) else bytes(c["QUAL"][i]), np.uint8).astype(np.int64) - 33
        x, q = pos0, 0
        for n, op in M.cigar_ops(c["CIGAR"][i]):
            if op in "M=X":
                n_in = max(0, min(n, lens[tid] - x))
                ok = qual[q:q + n_in] >= min_baseq
                depth[tid][x:x + n_in] += ok
                sum_q[tid] += int(qual[q:q + n_in][ok].sum())
            if op in "M=XDN":
                x += n
            if op in "M=XIS":
                q += n
    got = M.coverage(M.reads_from_cols(c), refs, exclude_flags=0x704, min_baseq=min_baseq)
    assert got["numreads"] == nreads and got["sum_mapq"] == sum_mq and got["sum_baseq"] == sum_q
    assert got["sum_depth"] == [int(d.sum()) for d in depth] and got["covbases"] == [int((d >= 1).sum()) for d in depth]
    assert got["meandepth"] == [float(np.float64(d.sum()) / np.float64(len(d))) for d in depth]
    assert sum(got["sum_depth"]) > 1000 and got["stats"]["n_counted"] == sum(nreads)
