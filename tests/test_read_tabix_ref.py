"""The Python model of read_tabix / read_gtf / read_gff (tests/read_tabix_ref.py) on the answers the reference records in
test/sql/duckhts.test:406-519 for the fixtures in tests/golden/, and on the grammars it states itself.  No device."""
import collections
import gzip
import math
import os

import pytest

import read_tabix_ref as M
from conftest import ROOT

GOLD = os.path.join(ROOT, "tests", "golden")


def fixture(name):
    raw = open(os.path.join(GOLD, name), "rb").read()
    return gzip.decompress(raw), M.tbi_conf(open(os.path.join(GOLD, name + ".tbi"), "rb").read())


def test_gff_fixture_rows_features_and_maps():
    text, conf = fixture("gff_file.gff.gz")
    assert sum(1 for s, l in M.getlines(text) if s[:1] == b"#") == 8
    for mode in (M.GFF, M.GENERIC):
        rows = M.scan(text, mode, types=[M.T_VARCHAR] * 9)
        assert len(rows) == 62
    rows = M.scan(text, M.GFF)
    assert rows[0][:5] == [b"X", b"Vega", b"exon", 2934816, 2935190]
    assert all(M.count_fields(s) == 9 for s in M.data_lines(text, ord("#"), 0, False))
    assert all(r[5] is None for r in rows)                                  # every score is "."
    cnt = collections.Counter(r[2] for r in rows)
    assert cnt == {b"exon": 23, b"intron": 19, b"CDS": 15, b"transcript": 4, b"gene": 1}
    assert sum(1 for r in rows if r[9] is not None) == 62
    g = M.scan(text, M.GENERIC, types=[M.T_VARCHAR] * 9)
    assert [(r[0], r[2]) for r in g[:2]] == [(b"X", b"exon"), (b"X", b"gene")]


def test_gff_fixture_regions():
    text, conf = fixture("gff_file.gff.gz")
    assert conf[:4] == (0, 1, 4, 5)
    a = M.region_scan(text, conf, "X:2934816-2935190", M.GFF)
    b = M.region_scan(text, conf, "X:2937010-2937500", M.GFF)
    both = M.region_scan(text, conf, "X:2934816-2935190,X:2937010-2937500", M.GFF)
    assert (len(a), len(b), len(both)) == (4, 3, 7) and both == a + b
    assert M.region_scan(text, conf, "nosuch:1-10", M.GFF) == []
    assert M.region_scan(text, conf, " nosuch , X:2934816-2935190 ,, ", M.GFF) == a


def test_meta_tabix_fixture():
    text, conf = fixture("meta_tabix.tsv.gz")
    meta, skip = conf[4], conf[5]
    assert (meta, skip) == (ord("#"), 1)
    b = M.bind(text, meta_char=meta, line_skip=skip)
    rows = M.scan(text, M.GENERIC, b["types"], meta, skip, b["skip_header_line"])
    assert b["names"][:2] == ["column0", "column1"] and rows[0][:2] == [b"chr1", b"1"]
    b = M.bind(text, header_names=["chrom", "pos", "value"], meta_char=meta, line_skip=skip)
    assert b["names"] == ["chrom", "pos", "value"] and not b["skip_header_line"]
    assert M.scan(text, M.GENERIC, b["types"], meta, skip, b["skip_header_line"])[0][:2] == [b"chr1", b"1"]
    b = M.bind(text, auto_detect=True, meta_char=meta, line_skip=skip)
    assert b["types"][1] == M.T_BIGINT


def test_header_tabix_fixture():
    text, conf = fixture("header_tabix.tsv.gz")
    meta, skip = conf[4], conf[5]
    assert skip == 1
    b = M.bind(text, header=True, meta_char=meta, line_skip=skip)
    assert b["names"] == ["chrom", "pos", "value"] and not b["skip_header_line"]      # the candidate came from the skip prefix
    assert M.scan(text, M.GENERIC, b["types"], meta, skip, b["skip_header_line"])[0][:2] == [b"chr1", b"1"]
    b = M.bind(text, header=True, column_types=["VARCHAR", "BIGINT", "VARCHAR"], meta_char=meta, line_skip=skip)
    assert M.scan(text, M.GENERIC, b["types"], meta, skip, b["skip_header_line"])[0][1] + 1 == 2
    with pytest.raises(M.BindError, match="column_types length does not match detected column count"):
        M.bind(text, header=True, column_types=["VARCHAR", "BIGINT"], meta_char=meta, line_skip=skip)


def test_bind_rules():
    t = b"#m\nh1\t h2 \t\n\na\t1\t2.5\t9\nb\t2\tx\n"
    assert M.sniff(t, False, False) == (3, None, False)
    assert M.sniff(t, True, False) == (4, b"h1\t h2 \t", False)
    b = M.bind(t, header=True)
    assert b == {"n_cols": 3, "names": ["h1", "h2", "column2"], "types": [M.T_VARCHAR] * 3, "skip_header_line": True}
    b = M.bind(t, header=True, header_names=["a", "b"])
    assert b["n_cols"] == 2 and b["skip_header_line"]
    b = M.bind(t, header_names=["a", "b", "c", "d", "e"])
    assert b["n_cols"] == 5 and not b["skip_header_line"]
    b = M.bind(t, header=True, auto_detect=True)
    assert b["types"] == [M.T_VARCHAR, M.T_BIGINT, M.T_VARCHAR]
    b = M.bind(b"a\t1\t2.5\nb\t.\t3\n", auto_detect=True)
    assert b["types"] == [M.T_VARCHAR, M.T_BIGINT, M.T_DOUBLE]
    b = M.bind(t, column_types=["int", "Long", "nonsense"])
    assert b["types"] == [M.T_INTEGER, M.T_BIGINT, M.T_VARCHAR]
    assert M.bind(b"")["n_cols"] == 1
    assert M.bind(b"\t".join([b"x"] * 300) + b"\n")["n_cols"] == 256
    # the last skipped line wins; the line behind it gives the count
    assert M.sniff(b"s1\ts\n\ns2\nd\td\td\n", True, False, line_skip=2) == (3, b"s2", True)


def test_scan_rules():
    t = b"x\t1\r\n\n#meta\ny\0z\t2\t3\n\0\tq\nlast\t5"
    rows = M.scan(t, M.GENERIC, [M.T_VARCHAR, M.T_BIGINT])
    assert rows == [[b"x", 1], [b"y", None], [None, None], [b"last", 5]]
    rows = M.scan(b"a\nb\n#c\nd\ne\n", M.GENERIC, [M.T_VARCHAR], line_skip=3, skip_header_line=True)
    assert rows == [[b"e"]]                                                # the meta line counts against line_skip, the header line comes behind
    rows = M.scan(b"a\nb\n#c\nd\ne\n", M.GENERIC, [M.T_VARCHAR], line_skip=3, skip_header_line=True, in_region=True)
    assert rows == [[b"a"], [b"b"], [b"d"], [b"e"]]
    rows = M.scan(b"s\t.\t\t.\t\tx\n", M.GFF)
    assert rows == [[b"s", b".", b".", 0, 0, None, b".", b".", b".", None]]
    assert M.scan(b"s\n", M.GTF)[0][9] is None
    assert M.cell(b"0" * 126 + b"1", M.T_BIGINT, False) == 1 and M.cell(b"0" * 127 + b"1", M.T_BIGINT, False) is None
    assert M.cell(b"0" * 127 + b"1", M.T_DOUBLE, False) is None


def test_number_grammars():
    for tok, v in ((b"5", 5), (b" 5", 5), (b"+5", 5), (b"-0", 0), (b"99999999999999999999", (1 << 63) - 1), (b"-99999999999999999999", -(1 << 63))):
        assert M.strtoll_whole(tok) == v
    for tok in (b"5x", b"5 ", b"", b"-", b"0x10", b"1_0", b"1.0"):
        assert M.strtoll_whole(tok) is None
    for tok, v in ((b"0", 0.0), (b"1.5", 1.5), (b".5", 0.5), (b"5.", 5.0), (b"1e22", 1e22), (b" \t1e-3", 1e-3), (b"0x1p-3", 0.125), (b"0X.8", 0.5), (b"0x1.8p1", 3.0),
                   (b"1e400", math.inf), (b"-Infinity", -math.inf), (b"INF", math.inf), (b"4.9e-324", 5e-324)):
        assert M.strtod_whole(tok) == v, tok
    assert M.dbl_bits(M.strtod_whole(b"-0.0")) == 1 << 63
    assert math.isnan(M.strtod_whole(b"nan")) and math.isnan(M.strtod_whole(b"NaN(a_1)"))
    for tok in (b"1e", b"1.5x", b"1_0", b"1 ", b"", b".", b"e5", b"0x", b"infin", b"nan(", b"nan(-)", b"--1", b"1e+"):
        assert M.strtod_whole(tok) is None, tok
    for tok in (b"0", b"-0.0", b"1.5", b".5", b"5.", b"1e22", b"1e-22", b"123456789012345", b"1e23"):      # 1e23 = 10 * 1e22: a spare digit moves into the significand
        assert M.fast_path_takes(tok), tok
    for tok in (b"1234567890123456", b"1e38", b"1e-23", b"1e400", b"4.9e-324", b"inf", b"-Infinity", b"nan", b"0x1p-3", b"1e", b"1.5x"):
        assert not M.fast_path_takes(tok), tok


def test_attribute_grammars():
    G, T = M.gff_pairs, M.gtf_pairs
    assert G(b"ID=g1;Name=x y; Note = a=b ;") == [(b"ID", b"g1"), (b"Name", b"x y"), (b"Note", b"a=b")]
    assert G(b"flag;ID=1") == [(b"ID", b"1")]
    assert G(b";; ID=1;;=v;k=") == [(b"ID", b"1"), (b"k", b"")]
    assert G(b"keyonly") == [] and G(b"; ;") == []
    assert T(b'gene_id "g;1"; n 5; tag "open') == [(b"gene_id", b"g;1"), (b"n", b"5"), (b"tag", b"open")]
    assert T(b'a "1" junk; b') == [(b"a", b"1"), (b"b", b"")]
    assert T(b";; a  \"\";") == [(b"a", b"")]
    assert M.attr_map(b".", True) is None and M.attr_map(b"", False) is None and M.attr_map(None, True) is None
    assert M.attr_map(b"x", True) == []


def test_parse_regions():
    assert M.parse_regions(None) == [] and M.parse_regions("") == []
    assert M.parse_regions(" a:1-2 ,\tb,, ,c ") == ["a:1-2", "b", "c"]


def test_the_library_resolves_schemas_as_the_model_does():
    """dhts_tabix_resolve_schema is pure host code (no device): the rest of bind behind the peek, for the table functions and the mirror"""
    import duckhts_amd as D
    rows120 = b"#m\n" + b"".join(b"r%d\t%d\t%s\t%s\n" % (i, i, b"2.5" if i == 99 else b"7", b"x" if i == 100 else b".") for i in range(120))
    texts = [b"#m\nh1\t h2 \t\n\na\t1\t2.5\t9\nb\t2\tx\n", b"a\t1\t2.5\nb\t.\t0x1p3\nc\t+7\tinf\n", b"", b"\t".join([b"x"] * 300) + b"\n", rows120,
             b"s1\ts\n\ns2\t\ts3\nd\td\td\n"]
    cases = [{}, {"header": True}, {"header": True, "auto_detect": True}, {"auto_detect": True}, {"header_names": ["a", "", "c", "d", "e"]},
             {"header": True, "header_names": ["p", "q"]}, {"column_types": ["int", "Long", "nonsense"]}, {"auto_detect": True, "column_types": ["REAL", "string", "INTEGER"]},
             {"header": True, "line_skip": 2}, {"auto_detect": True, "line_skip": 1}]
    n_checked = n_errors = 0
    for text in texts:
        for kw in cases:
            kw = dict(kw)
            skip = kw.pop("line_skip", 0)
            try:
                exp = M.bind(text, line_skip=skip, **kw)
            except M.BindError as e:
                with pytest.raises(D.DhtsError, match=str(e)):
                    D.tabix_resolve_schema(M.sniff(text, kw.get("header", False), bool(kw.get("header_names")), line_skip=skip), **kw)
                n_errors += 1
                continue
            sn = M.sniff(text, kw.get("header", False), bool(kw.get("header_names")), line_skip=skip)
            got = D.tabix_resolve_schema(sn, **kw)
            if got["need_rows"]:
                assert kw.get("auto_detect") and not kw.get("column_types") and got["types"] == [M.T_VARCHAR] * got["n_cols"]
                lines = list(M.data_lines(text, ord("#"), skip, got["skip_header_line"]))[:100]
                got = D.tabix_resolve_schema(sn, rows=[[M.get_field(s, i) for i in range(got["n_cols"])] for s in lines], **kw)
            assert not got.pop("need_rows") and got == exp, (text[:40], kw)
            n_checked += 1
    assert n_checked > 40 and n_errors > 5
