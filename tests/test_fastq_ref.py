"""tests/fastq_encode_ref.py (the CPU restatement of fastq_parse1 + bam_set1 + bam_write1 that the device encoder is held to) against
htslib's own FASTQ / FASTA fixtures: tests/golden/htslib_fastq/ holds test/fastq/*.fq, *.fa and the SAM its test viewer wrote for them.
r1 / r2 / longline were written with aux tags turned on; columns 1-11 do not depend on that option and only they are compared."""
import os
import struct

import pytest

import fastq_encode_ref as F

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "htslib_fastq")
EXPECTED = [("minimal.fq", "minimal.sam"), ("minimal.fa", "minimal-q.sam"), ("multiline.fq", "multiline.sam"), ("multiline.fa", "multiline-q.sam"),
            ("single.fq", "single_noaux.sam"), ("single.fa", "single_noaux-q.sam"), ("interleaved.fq", "inter_noaux.sam"),
            ("interleaved.fa", "inter_noaux-q.sam"), ("r1.fq", "r1.sam"), ("r2.fq", "r2.sam"), ("r1.fa", "r1-q.sam"), ("r2.fa", "r2-q.sam"),
            ("longline.fq", "longline.sam")]


def _read(name):
    return open(os.path.join(GOLD, name), "rb").read()


@pytest.mark.parametrize("src,sam", EXPECTED)
def test_restatement_meets_htslib_expected_sam(src, sam):
    text = _read(src)
    assert F.detect(text) == ("fasta" if src.endswith(".fa") else "fastq")
    recs, stopped = F.encode_text(text)
    exp = [l.split("\t")[:11] for l in _read(sam).decode().split("\n") if l and not l.startswith("@")]
    assert not stopped and [F.sam_columns(r) for r in recs] == exp


def test_multiline_quality_line_of_at_signs():
    recs, stopped = F.encode_text(_read("multiline.fq"))
    cols = [F.sam_columns(r) for r in recs]
    assert not stopped and [c[0] for c in cols] == ["seq1", "seq2"]
    assert "@@@@@@@@@@" in cols[0][10] and cols[1][10].endswith("@@@@@@@@@")


def _cols(text, **kw):
    recs, stopped = F.encode_text(text, **kw)
    return [F.sam_columns(r) for r in recs], stopped


def test_crlf_and_missing_last_newline():
    a, sa = _cols(b"@r1 c\r\nACGT\r\n+\r\nIIII\r\n@r2\r\nAC\r\n+r2\r\nII")
    b, sb = _cols(b"@r1 c\nACGT\n+\nIIII\n@r2\nAC\n+r2\nII\n")
    assert a == b and not sa and not sb and [c[0] for c in a] == ["r1", "r2"] and a[1][9:] == ["AC", "II"]


def test_empty_read_takes_one_empty_quality_line():
    c, s = _cols(b"@e\n\n+\n\n@f\nA\n+\nI\n")
    assert not s and [x[0] for x in c] == ["e", "f"] and c[0][9:] == ["*", "*"]
    c, s = _cols(b"@e\n+\n\n@f\nA\n+\nI\n")
    assert not s and len(c) == 2
    c, s = _cols(b"@e\n+\nI\n@f\nA\n+\nI\n")                   # a quality line longer than the remainder (0)
    assert s and c == []


def test_pair_suffixes():
    c, s = _cols(b"@a/1\nA\n+\nI\n@a/2\nA\n+\nI\n@a/7\nA\n+\nI\n@a/x\nA\n+\nI\n@b/1 x/2\nA\n+\nI\n")
    assert not s and [(x[0], x[1]) for x in c] == [("a", "77"), ("a", "141"), ("a", "205"), ("a/x", "4"), ("b", "77")]


def test_two_byte_names():
    """fastq_parse1 strips when name.l > 2, and name.l counts the '@': the two-byte NAME LINE "@1" keeps everything, "@/" too; the
    two-byte name "/1" (line "@/1", name.l 3) is stripped to nothing, which bam_set1 stores as "*" """
    c, s = _cols(b"@1\nA\n+\nI\n@/\nA\n+\nI\n@/1\nA\n+\nI\n@x/1\nA\n+\nI\n")
    assert not s and [(x[0], x[1]) for x in c] == [("1", "4"), ("/", "4"), ("*", "77"), ("x", "77")]


def test_lowercase_and_iupac_bases():
    c, _ = _cols(b"@r\nacgtnRYKMSWBDHV=.x\n+\nIIIIIIIIIIIIIIIIII\n")
    assert c[0][9] == "ACGTNRYKMSWBDHV=NN"


def test_space_led_quality_reads_as_star():
    recs, s = F.encode_text(b"@r\nACG\n+\n II\n")
    n = struct.unpack_from("<I", recs[0], 20)[0]
    assert not s and n == 3 and recs[0][-3:] == bytes([0xff, ord("I") - 33, ord("I") - 33]) and F.sam_columns(recs[0])[10] == "*"


def test_over_long_name_ends_the_scan():
    ok, bad = b"n" * 254, b"n" * 255
    c, s = _cols(b"@a\nA\n+\nI\n@" + ok + b"\nA\n+\nI\n@" + bad + b"\nA\n+\nI\n@z\nA\n+\nI\n")
    assert s and [x[0] for x in c] == ["a", ok.decode()]
    c, s = _cols(b"@" + b"n" * 254 + b"/1\nA\n+\nI\n")       # (the suffix goes first)
    assert not s and c[0][1] == "77"


def test_truncated_last_record():
    for tail in (b"@t\n", b"@t\nACGT\n", b"@t\nACGT\n+\n", b"@t\nACGT\n+\nII\n"):
        c, s = _cols(b"@a\nA\n+\nI\n" + tail)
        assert s and [x[0] for x in c] == ["a"], tail
    c, s = _cols(b">a\nAC\n>t\n", fasta=True)                 # FASTA: the end of the file ends the sequence
    assert not s and [x[0] for x in c] == ["a", "t"] and c[1][9] == "*"


def test_bad_record_mid_file_stops_the_rows():
    c, s = _cols(b"@a\nA\n+\nI\n@b\nAC\n+\nIII\n@c\nA\n+\nI\n")
    assert s and [x[0] for x in c] == ["a"]
    c, s = _cols(b"@a\nA\n+\nI\nb\nAC\n+\nII\n")
    assert s and [x[0] for x in c] == ["a"]
    c, s = _cols(b"@a\nA\n+\nI\n\n")                           # a blank line where a name is expected
    assert s and len(c) == 1


def test_wrapped_record_with_marker_led_quality_lines():
    c, s = _cols(b"@w x\nACGT\nAC\n\nG\n+w\n@III\n+I\n>\n@n\nA\n+\n@\n")
    assert not s and [x[0] for x in c] == ["w", "n"] and c[0][9:] == ["ACGTACG", "@III+I>"] and c[1][10] == "@"


def test_detection_order():
    assert F.detect(b"@HD\tVN:1.6\n") == "sam" and F.detect(b"@CO\tx\nACGT\n") == "sam"
    assert F.detect(b"@XY\tAA:b\n") == "fastq"                                          # (htslib reads it as FASTQ with no reads)
    assert F.detect(b"@XY\tAA:b\nr\t0\t*\t0\t0\t*\t*\t0\t0\tA\tI\n") is None        # the second line is not bases
    assert F.detect(b">c\nAC=T\n") is None and F.detect(b">c\nACGT\n") == "fasta" and F.detect(b"@r\r\nACGT\r\n") == "fastq"
    assert F.detect(b"r\t0\t*\t0\t0\t*\t*\t0\t0\tA\tI\n") is None
