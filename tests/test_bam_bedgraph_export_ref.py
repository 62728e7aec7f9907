"""The CPU model of bam_bedgraph_export (bam_bedgraph_export_ref) pinned on the golden file: the text it makes of the bedGraph model's rows, parsed
back line by line, reproduces those rows; its sizes and first and last lines are written down here; the helpers the device tests lean on
(blocks, rows across block boundaries, tabix overlap, the file order of regions) on small hand-made inputs.  No device."""
import hashlib

import numpy as np
import pytest

import bam_bedgraph_export_ref as X
import bam_bedgraph_ref as M
from conftest import read_golden

PINS = {(0, None): (192, 5024, "5dd8ae1452e529aa", b"CHROMOSOME_I\t913\t933\t1\n", b"CHROMOSOME_IV\t2534\t2584\t1\n"),
        (1, None): (225, 5861, "68d7f20dc4f96296", b"CHROMOSOME_I\t0\t913\t0\n", b"CHROMOSOME_MtDNA\t0\t5000\t0\n"),
        (1, "2,4"): (115, 2981, "381e0b45b25d2e51", b"CHROMOSOME_I\t0\t933\t0\n", b"CHROMOSOME_MtDNA\t0\t5000\t0\n")}


@pytest.fixture(scope="module")
def rng():
    return M.reads_from_bam(read_golden("range.bam"))


@pytest.mark.parametrize("zero_runs,breaks", sorted(PINS, key=str))
def test_the_text_of_the_golden_file(rng, zero_runs, breaks):
    refs, reads = rng
    text, res = X.export(reads, refs, exclude_flags=M.DEFAULT_EXCLUDE, zero_runs=zero_runs, breaks=breaks)
    n, size, digest, first, last = PINS[(zero_runs, breaks)]
    assert (res["n_rows"], len(text), hashlib.sha256(text).hexdigest()[:16]) == (n, size, digest)
    lines = text.splitlines(keepends=True)
    assert len(lines) == n and lines[0] == first and lines[-1] == last
    # every line parsed back is the bedGraph model's row
    parsed = X.parse(text)
    assert parsed == X.rows_of(res, refs)
    names = [nm for nm, _ in refs]
    assert [names.index(p[0]) for p in parsed] == res["tid"].tolist() and [p[1] for p in parsed] == res["start"].tolist()
    assert [p[2] for p in parsed] == res["end"].tolist() and [p[3] for p in parsed] == res["depth"].tolist()


def test_the_format_of_a_row():
    refs = [("a", 10), (b"chr with space", 10)]
    rows = {"tid": np.array([0, 1, 1]), "start": np.array([0, 9, 10**18]), "end": np.array([1, 10, 2**62]), "depth": np.array([0, 10, 2**31 - 1])}
    assert X.text(rows, refs) == b"a\t0\t1\t0\nchr with space\t9\t10\t10\nchr with space\t1000000000000000000\t4611686018427387904\t2147483647\n"
    assert X.text({k: v[:0] for k, v in rows.items()}, refs) == b"" and X.parse(b"") == []


def test_blocks_and_rows_across_their_boundaries():
    line = b"c\t1\t2\t3\n"                                                # 8 bytes: 0xff00 is a multiple of it
    assert X.BLOCK % len(line) == 0
    whole = line * (X.BLOCK // len(line))
    assert X.n_blocks(b"") == 0 and X.n_blocks(line) == 1 and X.n_blocks(whole) == 1 and X.n_blocks(whole + line) == 2
    assert X.straddlers(whole * 3) == 0                                    # every row ends where a block ends
    assert X.straddlers(b"xx\n" + whole * 3) == 3 and X.straddlers(b"xx\n" + whole * 2 + whole[:-8]) == 2      # three bytes in front: a row over every boundary
    assert len(X.EOF_BLOCK) == 28


def test_overlap_and_file_order():
    rows = [(b"a", 0, 10, 1), (b"a", 10, 20, 2), (b"b", 5, 6, 1)]
    assert X.overlapping(rows, b"a", 9, 10) == rows[:1] and X.overlapping(rows, b"a", 9, 11) == rows[:2] and X.overlapping(rows, b"a", 20, 30) == []
    assert X.overlapping(rows, b"b", 0, 100) == rows[2:] and X.overlapping(rows, b"c", 0, 100) == []
    assert X.in_file_order([(0, 0, 5), (0, 5, 9), (2, 0, 1), (1, 3, 4)])   # contigs in any order, each together and ascending
    assert not X.in_file_order([(0, 5, 9), (0, 0, 5)]) and not X.in_file_order([(0, 0, 5), (1, 0, 5), (0, 7, 9)])
    assert X.in_file_order([])


def test_the_error_strings():
    assert X.err_exists("/x/y.bed.gz") == "bam_bedgraph_export: output '/x/y.bed.gz' already exists (overwrite is off)"
    assert X.as_export(M.ERR_BREAKS) == "bam_bedgraph_export: breaks must be strictly increasing integers between 1 and 2147483647"
    for msg in (X.ERR_NOT_OPEN, X.ERR_ORDER, X.ERR_INDEX_KIND, X.ERR_OPEN_OUTPUT):
        assert msg.startswith("bam_bedgraph_export: ")
