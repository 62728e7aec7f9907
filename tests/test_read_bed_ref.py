"""The CPU model of read_bed (tests/read_bed_ref.py) pinned on tests/golden/targets.bed against the reference's own answers
(test/sql/duckhts.test:241-258, 276-284), and on the corners of next_bed_line / read_bed_scan."""
import pytest

import read_bed_ref as M
from conftest import read_golden


def test_targets_bed_pins():
    t = M.read_bed(read_golden("targets.bed"))
    assert t["n_rows"] == 4 and t["status"] == 1 and t["error"] is None
    row0 = [t[k][0] for k in ("chrom", "start", "end", "name", "score", "strand", "thick_start", "block_count")]
    assert row0 == [b"CHROMOSOME_I", 0, 10, b"target1", b"100", b"+", 0, 2]
    assert t["extra"][t["name"].index(b"target4")] == b"extra_note=foo"
    assert t["extra"][:3] == [None, None, None]
    assert t["name"][2] == b"target3" and t["score"][2] is None and t["thick_start"][2] is None     # a 4-field line: the rest is NULL


def test_targets_bed_region():
    text = read_golden("targets.bed")
    assert M.tabix_names(text, M.R.CONF_BED) == ["CHROMOSOME_I", "CHROMOSOME_II", "CHROMOSOME_III"]
    assert M.read_bed(text, region="CHROMOSOME_I:1-20")["n_rows"] == 2
    assert M.read_bed(text, region=".")["n_rows"] == 4
    assert M.read_bed(text, region="CHROMOSOME_I:11-20")["name"] == [b"target2"]        # [10, 20) against rows [0, 10) and [10, 20)
    assert M.read_bed(text, region="CHROMOSOME_I:10-10")["name"] == [b"target1"]
    with pytest.raises(M.BedIteratorError):
        M.read_bed(text, region="nope:1-2")


def test_custom_one_based_columns_change_the_row_set():
    text = b"c\t10\t20\tA\nc\t20\t30\tB\n"
    # bed preset: [10, 20) and [20, 30); sc=1 bc=2 ec=3 without the UCSC flag: [9, 20) and [19, 30)
    assert M.read_bed(text, region="c:20-20")["name"] == [b"A"]
    assert M.read_bed(text, region="c:20-20", conf=(0, 1, 2, 3, ord("#"), 0))["name"] == [b"A", b"B"]
    assert M.read_bed(text, region="c:21-21")["name"] == [b"B"]


def test_lines_and_meta():
    text = b"#c\ntrack x\nbrowser y\ntracker1\t1\t2\n\n\r\n\0c\t1\t2\nc\t1\t2\r\nd\t3\t4\tna\0me\tz\ne\t5\t6"
    t = M.read_bed(text)
    assert t["chrom"] == [b"c", b"d", b"e"] and t["name"] == [None, b"na", None] and t["end"] == [2, 4, 6]


def test_integers():
    f = [b" 12", b"+5", b"-7", b"-", b"12 ", b"0x10", b"1e3", b"\v12", b"9223372036854775807", b"9223372036854775808", b"-9223372036854775808",
         b"-9223372036854775809", b"99999999999999999999", b""]
    text = b"".join(b"c\t" + x + b"\t1\n" for x in f)
    assert M.read_bed(text)["start"] == [12, 5, -7, None, None, None, None, 12, 2**63 - 1, 2**63 - 1, -2**63, -2**63, 2**63 - 1, None]


def test_extra_and_empty_fields():
    t = M.read_bed(b"c\t1\t2\t\t\t\t\t\t\t\t\t\tx\ty\t\nc\t1\t2\t3\t4\t5\t6\t7\t8\t9\t10\t11\t\nc\t1\t\n")
    assert t["extra"] == [b"x\ty\t", None, None] and t["name"] == [None, b"3", None] and t["end"] == [2, 2, None]
    assert t["block_starts"] == [None, b"11", None]


def test_short_line_ends_the_scan():
    t = M.read_bed(b"c\t1\t2\n#x\nc\t1\nc\t3\t4\n")
    assert t["n_rows"] == 1 and t["status"] < 0 and t["error"] == M.ERR + " (line 3)"
    assert M.read_bed(b"c\t1\n")["n_rows"] == 0
    assert M.read_bed(b"c\t1\t2\n", columns=[])["n_rows"] == 1
