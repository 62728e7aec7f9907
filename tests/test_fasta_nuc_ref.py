"""The CPU model of fasta_nuc (tests/fasta_nuc_ref.py) pinned on the reference's published answers (test/sql/duckhts.test:286-317,
README.md:204-221), computed on the first 100 bases of each sequence of its test/data/ce.fa (tests/golden/ce_heads.fa) with its
test/data/targets.bed, and on hand-written text for every row rule of next_fasta_nuc_bed_interval / fasta_nuc_scan."""
import struct

import pytest

import fasta_index_ref as F
import fasta_nuc_ref as M
from conftest import read_golden


@pytest.fixture(scope="module")
def ce():
    fa = read_golden("ce_heads.fa")
    fai = F.save(F.build(fa))
    return fa, fai, read_golden("targets.bed")


def bits(x):
    return struct.pack("<d", x)


def test_the_fixture_is_the_heads_of_ce_fa(ce):
    names, tab = F.read(ce[1])
    assert names == [n for n, _ in F.CE_NAMES]
    assert all(tab[n][0] == 100 and tab[n][2:] == (50, 51) for n in names)


def test_readme_rows(ce):
    """README.md:209-213"""
    got = M.fasta_nuc(ce[0], ce[1], bed_text=ce[2])
    assert got["n_rows"] == 4
    assert got["chrom"] == [b"CHROMOSOME_I", b"CHROMOSOME_I", b"CHROMOSOME_II", b"CHROMOSOME_III"]
    assert got["start"] == [0, 10, 0, 0] and got["end"] == [10, 20, 8, 6]
    assert [bits(x) for x in got["pct_gc"]] == [bits(x) for x in (0.6, 0.5, 0.625, 0.5)]
    assert list(zip(got["num_a"], got["num_c"], got["num_g"], got["num_t"])) == [(2, 4, 2, 2), (4, 3, 2, 1), (2, 4, 1, 1), (2, 2, 1, 1)]
    assert "seq" not in got


def test_first_target_row(ce):
    """duckhts.test:286-295"""
    got = M.fasta_nuc(ce[0], ce[1], bed_text=ce[2])
    i = [k for k in range(4) if got["chrom"][k] == b"CHROMOSOME_I" and got["start"][k] == 0][0]
    row = [got[c][i] for c in ("pct_at", "pct_gc", "num_a", "num_c", "num_g", "num_t", "num_n", "num_other", "seq_len")]
    assert row == [0.4, 0.6, 2, 4, 2, 2, 0, 0, 10] and bits(row[0]) == bits(0.4) and bits(row[1]) == bits(0.6)


def test_bins_of_a_region(ce):
    """duckhts.test:297-305 and README.md:215-221"""
    got = M.fasta_nuc(ce[0], ce[1], bin_width=10, region="CHROMOSOME_I:1-20")
    assert got["n_rows"] == 2 and sum(got["seq_len"]) == 20
    assert got["chrom"] == [b"CHROMOSOME_I"] * 2 and got["start"] == [0, 10] and got["end"] == [10, 20] and got["pct_gc"] == [0.6, 0.5]


def test_include_seq(ce):
    """duckhts.test:307-317"""
    got = M.fasta_nuc(ce[0], ce[1], bed_text=ce[2], include_seq=True)
    assert got["seq"][0] == b"GCCTAAGCCT" and got["seq"][2] == ce[0].split(b"\n")[4][:8]


def test_bins_without_a_region_walk_every_sequence(ce):
    got = M.fasta_nuc(ce[0], ce[1], bin_width=30)
    assert got["n_rows"] == 7 * 4 and got["end"][:4] == [30, 60, 90, 100] and got["chrom"][4] == b"CHROMOSOME_II" and sum(got["seq_len"]) == 700
    one = M.fasta_nuc(ce[0], ce[1], bin_width=1000000)
    assert one["n_rows"] == 7 and one["seq_len"] == [100] * 7
    for k in range(7):
        seq = b"".join(ce[0].split(b"\n")[3 * k + 1:3 * k + 3])
        assert one["num_a"][k] == seq.count(b"A") and one["num_other"][k] == 0


def test_bind_errors(ce):
    for kw, msg in (({"fasta_path": ""}, M.ERR_PATH), ({}, M.ERR_ONE_OF), ({"bed_text": ce[2], "bin_width": 5}, M.ERR_ONE_OF), ({"bin_width": 0}, M.ERR_BIN_WIDTH),
                    ({"bin_width": -3}, M.ERR_BIN_WIDTH)):
        with pytest.raises(M.NucError, match=msg):
            M.fasta_nuc(ce[0], ce[1], **kw)
    with pytest.raises(M.NucError, match=M.ERR_OPEN_INDEX):
        M.fasta_nuc(ce[0], None, bin_width=5)


@pytest.mark.parametrize("region", ["nope", "CHROMOSOME_I:0-5", "CHROMOSOME_I:5-3", "CHROMOSOME_I:102", "CHROMOSOME_I:1-101", "CHROMOSOME_I:200-300", "{CHROMOSOME_I"])
def test_invalid_regions(ce, region):
    """unknown and malformed, and everything fai_adjust_region had to move: a start behind the sequence, an explicit end behind it"""
    with pytest.raises(M.NucError, match=M.ERR_REGION):
        M.fasta_nuc(ce[0], ce[1], bin_width=10, region=region)


def test_regions_whose_open_end_is_clamped(ce):
    for region, rows in (("CHROMOSOME_II", [(0, 40), (40, 80), (80, 100)]), ("CHROMOSOME_II:61", [(60, 100)]), ("CHROMOSOME_II:95-", [(94, 100)]), ("CHROMOSOME_II:-7", [(0, 7)]),
                         ("CHROMOSOME_II:100-100", [(99, 100)]), ("CHROMOSOME_II:101", [])):
        got = M.fasta_nuc(ce[0], ce[1], bin_width=40, region=region)
        assert list(zip(got["start"], got["end"])) == rows and got["chrom"] == [b"CHROMOSOME_II"] * len(rows)


# ---- the row rules, on hand-written text ------------------------------------------------------------------------------------------
FA = b">s1\nACGTN\nacgtn\nRY\n>s2 comment\nAAAA\n>s3\nGG"
FAI = F.save(F.build(FA))


def run(bed, **kw):
    return M.fasta_nuc(FA, FAI, bed_text=bed, include_seq=True, **kw)


def test_lines_that_are_passed_over():
    got = run(b"#c\n\ntrack t\nbrowser b\ns1\t1\ns1\ns1\t0\t3\ns1\t\t3\ns1\t1\t\ns1\t1x\t3\ns1\t1\t3.0\ns1\t 1\t+3\ts\r\ns1\t1\t2 \ns2\t0\t1\0\t9\n")
    assert list(zip(got["chrom"], got["start"], got["end"])) == [(b"s1", 0, 3), (b"s1", 1, 3), (b"s2", 0, 1)]
    assert got["seq"] == [b"ACG", b"CG", b"A"]


def test_zero_and_negative_lengths_are_rows_without_a_fetch():
    got = run(b"s1\t5\t5\nnope\t9\t2\ns1\t-3\t-8\n\t0\t0\n")
    assert got["n_rows"] == 4 and got["seq_len"] == [0, -7, -5, 0] and got["seq"] == [None] * 4 and got["chrom"] == [b"s1", b"nope", b"s1", b""]
    for k in ("num_a", "num_c", "num_g", "num_t", "num_n", "num_other"):
        assert got[k] == [0] * 4
    assert [bits(x) for x in got["pct_at"] + got["pct_gc"]] == [bits(0.0)] * 8


def test_unknown_chrom_with_bases_is_dropped():
    got = run(b"nope\t0\t5\ns2\t0\t2\nS1\t0\t2\n")
    assert got["chrom"] == [b"s2"] and got["seq"] == [b"AA"]


def test_clamping_of_faidx_adjust_position():
    got = run(b"s1\t-5\t-1\ns1\t-5\t3\ns1\t12\t20\ns1\t30\t40\ns1\t10\t99\ns1\t0\t12\ns1\t3\t8\n")
    assert got["start"] == [-5, -5, 12, 30, 10, 0, 3] and got["end"] == [-1, 3, 20, 40, 99, 12, 8]
    assert got["seq"] == [b"A", b"ACG", b"", b"", b"RY", b"ACGTNacgtnRY", b"TNacg"]
    assert got["seq_len"] == [1, 3, 0, 0, 2, 12, 5]
    assert got["num_other"] == [0, 0, 0, 0, 2, 2, 0] and got["num_n"] == [0, 0, 0, 0, 0, 2, 1]
    assert [bits(x) for x in got["pct_at"]] == [bits(x) for x in (1.0, 1.0 / 3.0, 0.0, 0.0, 0.0, 4.0 / 12.0, 2.0 / 5.0)]


def test_a_file_that_ends_early_drops_the_row():
    cut = FA[:FA.index(b"acgtn") + 2]
    got = M.fasta_nuc(cut, FAI, bed_text=b"s1\t0\t5\ns1\t0\t7\ns1\t0\t8\ns1\t6\t7\ns1\t7\t8\ns2\t0\t1\ns2\t1\t1\n", include_seq=True)
    assert got["seq"] == [b"ACGTN", b"ACGTNac", b"c", None] and got["chrom"] == [b"s1", b"s1", b"s1", b"s2"]
    bins = M.fasta_nuc(cut, FAI, bin_width=3)
    assert list(zip(bins["chrom"], bins["start"], bins["end"])) == [(b"s1", 0, 3), (b"s1", 3, 6)]


def test_region_filters_bed_rows_by_overlap():
    bed = b"s1\t0\t3\ns1\t2\t9\ns1\t3\t9\ns1\t6\t6\ns1\t7\t5\ns2\t0\t4\ns1\t5\t6\ns1\t6\t7\n"
    got = run(bed, region="s1:4-6")                       # [3, 6)
    assert list(zip(got["start"], got["end"])) == [(2, 9), (3, 9), (5, 6)]
    assert got["seq"][0] == b"GTNacgt"                    # the row's own bases, not the overlap
    assert run(bed, region="s1:4-6", bed_indexed=True) == got
    assert run(bed, region="s2")["chrom"] == [b"s2"]
    with pytest.raises(M.NucError, match=M.ERR_BED_ITER):
        run(b"s1\t0\t3\n", region="s2", bed_indexed=True)


def test_count_nucleotides_is_toupper_of_every_byte():
    seq = bytes(range(256))
    a, c, g, t, n, other = M.count_nucleotides(seq)
    assert (a, c, g, t, n, other) == (2, 2, 2, 2, 2, 246)


def test_projection_and_order():
    got = M.fasta_nuc(FA, FAI, bin_width=4, columns=["seq_len", "chrom", "num_other"])
    assert list(got) == ["n_rows", "seq_len", "chrom", "num_other"]
    assert got["seq_len"] == [4, 4, 4, 4, 2] and got["num_other"] == [0, 0, 2, 0, 0]
