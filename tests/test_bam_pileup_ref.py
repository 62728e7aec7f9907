"""The CPU model of bam_pileup on inputs whose results are written out by hand, and against bam_depth's model where the two must agree: per
position the bases of both strands sum to the depth, and with the deletions to the depth that counts them."""
import pytest

import bam_depth_ref as DM
import bam_pileup_cases as P
import bam_pileup_ref as M
from conftest import read_golden


@pytest.fixture(scope="module")
def hand():
    return M.reads_from_bam(P.hand_bam())


@pytest.mark.parametrize("extra,rows", P.HAND_SETS, ids=[str(e) for e, _ in P.HAND_SETS])
def test_the_hand_written_table(hand, extra, rows):
    refs, reads = hand
    assert refs == [(n.encode(), l) for n, l in P.HAND_REFS]
    res = M.pileup(reads, refs, **{**P.HAND_PARAMS, **extra})
    assert M.as_rows(res) == rows and res["stats"] == P.HAND_STATS and res["n_rows"] == len(rows)


def test_the_reads_carry_the_codes_of_seq(hand):
    _, reads = hand
    assert reads[4][7] == list(range(16)) and reads[0][7] == [1, 2, 4, 8, 15, 1] and [M.symbol_of(c) for c in range(16)] == list("=ACNGNNNTNNNNNNN")
    assert reads[1][5] == [(3, "M"), (2, "D"), (3, "M")] and reads[1][4] == 6


def test_insertion_anchors():
    refs = [(b"c", 200)]
    for cigar, want in (("5S3I10M", []), ("10M2I5D3I10M", [110, 115]), ("10M100N2I10M", []), ("10M2I2P3I10M", [110, 110]), ("3D2I", [103]), ("4M0D2N0M3I4M", []),
                        ("4M2N0D3I4M", []), ("4M2N1D3I4M", [107]), ("2I4M1I", [104]), ("4M3H2S1I", [104])):
        reads = M.reads_from_bam(P.bam([("c", 200)], [P.R(0, 0, 100, 30, cigar, 30)]))[1]
        res = M.pileup(reads, refs, include_insertions=1)
        got = sorted(p for p, n, c in zip(res["pos"], res["nucleotide"], res["count"]) for _ in range(c) if n == "+")
        assert got == want, cigar
    # the anchor must lie inside a row: the last position of a row counts, one position in front of the row does not
    reads = M.reads_from_bam(P.bam([("c", 200)], [P.R(0, 0, 100, 30, "10M2I10M", 30)]))[1]
    assert [(p, n) for p, n in zip(*[M.pileup(reads, refs, rows=[(0, 100, 110)], include_insertions=1)[k] for k in ("pos", "nucleotide")]) if n == "+"] == [(110, "+")]
    assert "+" not in M.pileup(reads, refs, rows=[(0, 110, 120)], include_insertions=1)["nucleotide"]


def sums(res, with_deletions):
    """per row {position 0-based: the sum over A..= (and -) of both strands}"""
    out = {}
    for (r, x, _, sym), n in res["counts"].items():
        if sym in "ACGTN=" or (with_deletions and sym == "-"):
            out.setdefault(r, {})
            out[r][x] = out[r].get(x, 0) + n
    return out


def depth_rows(res):
    return {r: d for r, d in enumerate(res["per_row"]) if d}


FILTERS = [dict(), dict(min_baseq=20), dict(min_mapq=25, min_read_len=5, exclude_flags=0x704), dict(require_flags=1), dict(include_flags=16, min_baseq=35)]


@pytest.fixture(scope="module", params=["range.bam", "random"])
def some_reads(request):
    if request.param == "range.bam":
        return M.reads_from_bam(read_golden("range.bam"))
    return M.reads_from_bam(P.bam(P.RANDOM_REFS, P.random_reads(11, 300)))


@pytest.mark.parametrize("strands", [0, 1])
@pytest.mark.parametrize("kw", FILTERS, ids=str)
def test_the_bases_sum_to_bam_depths_depth(some_reads, kw, strands):
    refs, reads = some_reads
    plain = [r[:7] for r in reads]
    res = M.pileup(reads, refs, include_deletions=1, include_insertions=1, distinguish_strands=strands, **kw)
    assert sums(res, False) == depth_rows(DM.depth(plain, refs, **kw)) and sums(res, True) == depth_rows(DM.depth(plain, refs, include_deletions=1, **kw))
    assert res["stats"] == DM.depth(plain, refs, **kw)["stats"] and res["n_rows"] > 100
    off = M.pileup(reads, refs, distinguish_strands=strands, **kw)                      # the switches off: no '-' and no '+' row
    assert not set(off["nucleotide"]) & {"-", "+"} and sums(off, True) == sums(res, False)


def test_regions_are_answered_in_the_order_given(hand):
    refs, reads = hand
    res = M.pileup(reads, refs, rows=[(0, 30, 32), (0, 10, 12)], **P.HAND_PARAMS)
    assert M.as_rows(res) == [(0, 31, "+", "A", 1), (0, 32, "+", "C", 1), (0, 11, "+", "A", 1), (0, 12, "+", "C", 1)]
    assert M.table_bytes([(0, 0, 1023), (1, 5, 5), (0, 2000, 3024)], 1) == (1024 + 2048) * 64 and M.table_bytes([(0, 0, 10)], 0) == 1024 * 32
    assert M.err_table(65536, 4096, 1).startswith("bam_pileup: the count table needs 65536 bytes (64 per position of every row); at most 4096")
