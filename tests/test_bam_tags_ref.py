"""The model of the tag columns and the map (bam_tags_ref.py) against the C oracle on the hostile corpus (tag_corpus.py), and against cells
written by hand from htslib's sam.c and the reference's bam_reader.c.  CPU only."""
import functools
import struct

import pytest

import bam_tags_ref as R
import bcf_cases
import orc
import tag_corpus as TC

COL = {t: i for i, (t, _) in enumerate(R.STD_TAGS)}


def signed(v):
    return [signed(x) for x in v] if isinstance(v, list) else (v - (1 << 64) if isinstance(v, int) and v >= 1 << 63 else v)


@functools.lru_cache(maxsize=None)
def model():
    """per record: (the 56 cells, the map without the standard tags, the whole map); computed once, never changed"""
    return [(signed(R.std_tags(aux)), R.aux_map(aux, True), R.aux_map(aux, False)) for _, _, aux in TC.corpus()]


def table_cells(table):
    """a decoded canonical table -> rows of Python cells"""
    return list(zip(*[orc.bcf_col_py(c) for c in table["cols"]]))


def map_cells(table):
    k, v = (orc.bcf_col_py(c) for c in table["cols"])
    return [None if a is None else (a, b) for a, b in zip(k, v)]


def by_name(name):
    names = [n for n, _, _ in TC.corpus()]
    return model()[names.index(name)]


def test_the_corpus_holds_every_family():
    names = [n for n, _, _ in TC.corpus()]
    assert len(set(names)) == len(names)
    fam = {f: [n for n in names if n.startswith(f + " ")] for f in ("F1", "F2", "F3", "F4", "F5", "F6", "F7")}
    assert len(fam["F1"]) >= 256 * 7 and len(fam["F2"]) == 12 * 4 * 7 and len(fam["F5"]) == 5 * 7
    for tag in TC.CARRIERS:
        T = tag.decode()
        for t in range(256):
            assert "F1 %s type %d" % (T, t) in names
        for w in TC.F3_WORDS:
            for form in ("f", "B:f x1", "B:f x5"):
                assert any(n.startswith("F3 %s %s %08x " % (T, form, w)) for n in names), (T, form, w)
        assert sum(n.startswith("F3 %s d " % T) for n in names) == 13
        assert sum(n.startswith("F4 %s " % T) for n in names) == 27 + 2 + 5 + 4 + 5 == sum(n.startswith("F7 %s behind CG" % T) for n in names)
    for w in (0x00000001, 0x007fffff, 0x00800000, 0x80000001, 0x7f7fffff, 0, 0x80000000, 0x7f800000, 0xff800000, 0x7f800001, 0xffc12345):
        assert w in TC.F3_WORDS
    for k, rec in enumerate(bcf_cases.qual_records()):              # the twelve QUAL words, in that table's order
        assert struct.pack("<I", TC.QUAL_WORDS[k]) in rec
    assert len(TC.QUAL_WORDS) == len(bcf_cases.qual_records()) == 12 and TC.F3_WORDS[:12] == TC.QUAL_WORDS
    for p in TC.F7_POSITIONS:
        assert "F7 CG " + p in names
    assert "F7 CG shorter than the CIGAR stays" in names
    for key in (b"\0X", b"X\0", b"\0\0", b"\xffZ", b"NX", b"XM"):
        assert "F6 key %r" % key in names
    assert all(("F6 aux of %d bytes" % k) in names for k in range(4)) and "F6 Z of 70000" in names and "F6 3000 fields" in names
    # a swapped record is seen without its CG tag, every other record as it is stored
    for n, rec, aux in TC.corpus():
        if n.startswith("F7") and "stays" not in n:
            assert TC.cg_tag(40) in rec and TC.cg_tag(40) not in aux and len(rec) - len(rec.replace(TC.cg_tag(40), b"")) == len(TC.cg_tag(40)) and rec.replace(TC.cg_tag(40), b"").endswith(aux), n
        else:
            assert rec.endswith(aux) and TC.cg_tag(40) not in rec, n
    for data in TC.files():
        assert len(data) < 2 << 20
    raw = sum(len(r) for _, r, _ in TC.corpus())
    assert orc.bgzf_inflate_all(TC.files()[1])["n_blocks"] >= raw // 700 > 1000      # small blocks: records and the long Z straddle them


@pytest.mark.parametrize("which", [0, 1], ids=["default_payload", "payload_700"])
def test_every_case_is_a_row(which):
    """no case ends the scan: the oracle reads as many rows as the corpus has records"""
    exp = orc.bam_read(TC.files()[which])
    assert exp["status"] >= 0 and exp["n_rows"] == len(TC.corpus()), (exp["status"], exp["n_rows"], len(TC.corpus()))


@pytest.mark.parametrize("which", [0, 1], ids=["default_payload", "payload_700"])
def test_model_and_oracle_agree_on_the_tag_columns(which):
    exp = orc.bam_read_std_tags(TC.files()[which])
    assert [c["name"] for c in exp["cols"]] == [t for t, _ in R.STD_TAGS]
    rows = table_cells(exp)
    assert len(rows) == len(model())
    for (name, _, _), got, (want, _, _) in zip(TC.corpus(), rows, model()):
        for j, (g, w) in enumerate(zip(got, want)):
            assert g == w, f"{name}: column {R.STD_TAGS[j][0]}: oracle {g!r:.120} model {w!r:.120}"


@pytest.mark.parametrize("excl", [True, False], ids=["exclude_standard", "all"])
@pytest.mark.parametrize("which", [0, 1], ids=["default_payload", "payload_700"])
def test_model_and_oracle_agree_on_the_map(which, excl):
    rows = map_cells(orc.bam_read_aux_map(TC.files()[which], excl))
    assert len(rows) == len(model())
    for (name, _, _), got, m in zip(TC.corpus(), rows, model()):
        want = m[1] if excl else m[2]
        assert got == want, f"{name}: oracle {got!r:.200} model {want!r:.200}"


def test_the_widening_on_integers():
    """f32_to_f64_bits against struct for every word of the corpus that is no NaN; the two NaN rules by hand"""
    for w in TC.F3_WORDS + [0x3f800000, 0xc0490fdb, 0x00000002, 0x00400000, 0x807fffff]:
        if (w >> 23) & 0xff == 0xff and w & 0x7fffff:
            continue
        want = struct.unpack("<Q", struct.pack("<d", struct.unpack("<f", struct.pack("<I", w))[0]))[0]
        assert R.f32_to_f64_bits(w) == want, hex(w)
    assert R.f32_to_f64_bits(0x00000001) == 0x36A0000000000000      # 2^-149
    assert R.f32_to_f64_bits(0x007fffff) == 0x380FFFFFC0000000      # the largest denormal
    assert R.f32_to_f64_bits(0x80000001) == 0xB6A0000000000000
    assert R.f32_to_f64_bits(0x7f800001) == 0x7FF8000020000000      # a signalling NaN: payload << 29, the quiet bit set
    assert R.f32_to_f64_bits(0x7f800002) == 0x7FF8000040000000
    assert R.f32_to_f64_bits(0xffc12345) == 0xFFF82468A0000000      # a negative quiet NaN keeps its sign and its payload
    assert R.f32_to_f64_bits(0x7fc00000) == 0x7FF8000000000000


def test_percent_g():
    """%g as glibc prints it (bam_aux_to_string bam_reader.c:156-158, 172-174)"""
    d = lambda v: struct.unpack("<Q", struct.pack("<d", v))[0]
    assert R.fmt_g(d(1e6)) == b"1e+06" and R.fmt_g(d(100000.0)) == b"100000" and R.fmt_g(d(0.0001)) == b"0.0001" and R.fmt_g(d(1e-5)) == b"1e-05"
    assert R.fmt_g(d(123456789.0)) == b"1.23457e+08" and R.fmt_g(d(0.1)) == b"0.1" and R.fmt_g(d(-0.0)) == b"-0" and R.fmt_g(d(5e-324)) == b"4.94066e-324"
    assert R.fmt_g(d(float("inf"))) == b"inf" and R.fmt_g(d(float("-inf"))) == b"-inf"
    assert R.fmt_g(0x7ff8000000000000) == b"nan" and R.fmt_g(0xfff8000000000001) == b"-nan" and R.fmt_g(0x7ff0000000000001) == b"nan"


def test_cells_written_by_hand():
    """one cell or more per family, each with the line of the reference that decides it"""
    # F1: a stored type that is not the column's.  bam_aux2i of 'Z' is get_int_aux_val's default, 0 (sam.c:5103-5105), and the cell is valid
    cells, mx, ma = by_name("F1 NM type %d" % ord("Z"))
    assert cells[COL["NM"]] == 0 and cells[COL["UQ"]] == 7 and cells[COL["AS"]] == -5
    assert mx == ([b"YA", b"YB"], [b"ya", b"yb"]) and ma == ([b"UQ", b"YA", b"NM", b"AS", b"YB"], [b"7", b"ya", b"ab", b"-5", b"yb"])
    assert by_name("F1 TS type %d" % ord("Z"))[0][COL["TS"]] == b""          # bam_aux2A of a non-A is 0 (sam.c:5129-5131): the C string {0, 0}
    assert by_name("F1 TS type %d" % ord("A"))[0][COL["TS"]] == b"\x01"
    assert by_name("F1 MD type %d" % ord("i"))[0][COL["MD"]] is None         # bam_aux2Z of a non-Z/H is NULL (sam.c:5138-5140) -> set_null (bam_reader.c:941)
    assert by_name("F1 MD type %d" % ord("H"))[0][COL["MD"]] == b"ab"
    assert by_name("F1 ML type %d" % ord("Z"))[0][COL["ML"]] == []           # bam_auxB_len of a non-B is 0 (sam.c:5145-5148): an empty, valid list
    assert by_name("F1 ML type %d" % ord("B"))[0][COL["ML"]] == [1, 2]
    cells, mx, ma = by_name("F1 NM type %d" % ord("?"))                      # aux_type2size 0 -> skip_aux NULL (sam.c:4803): NM and all behind it absent
    assert cells[COL["NM"]] is None and cells[COL["AS"]] is None and cells[COL["UQ"]] == 7 and ma == ([b"UQ", b"YA", b"NM"], [b"7", b"ya", b""])
    assert by_name("F1 NM S 65535")[0][COL["NM"]] == 65535 and by_name("F1 NM s -32768")[0][COL["NM"]] == -32768     # le_to_u16 / le_to_i16 (sam.c:5099-5100)
    assert by_name("F1 NM I 4294967295")[0][COL["NM"]] == 4294967295 and by_name("F1 XT c -128")[2][1][2] == b"-128"
    # F2: B:Z x7 through bam_auxB2i: get_int_aux_val's default for every element (sam.c:5159, 5103-5105); B:d through bam_auxB2f likewise (5170)
    cells, mx, ma = by_name("F2 ML B:Z x7")
    assert cells[COL["ML"]] == [0] * 7 and cells[COL["AS"]] == -5 and ma[1][2] == b"Z,0,0,0,0,0,0,0"
    assert by_name("F2 FZ B:d x7")[0][COL["FZ"]] == [0] * 7 and by_name("F2 XT B:d x1")[2][1][2] == b"d,0"
    assert by_name("F2 FZ B:S x7")[0][COL["FZ"]] == [0, 65535, 0, 65534, 1, 1, 32767]
    assert by_name("F2 CG B:c x7")[0][COL["CG"]] == [-128, 127, 0, 126, -127, 1, 63] and len(by_name("F2 ML B:B x300")[0][COL["ML"]]) == 300
    assert by_name("F2 NM B:i x1")[0][COL["NM"]] == 0 and by_name("F2 MD B:C x0")[0][COL["MD"]] is None and by_name("F2 TS B:C x0")[0][COL["TS"]] == b""
    # F3: le_to_float then float -> double (sam.c:5169; bam_reader.c:134 writes the double into the BIGINT child)
    assert by_name("F3 ML B:f x1 00000001 #4")[0][COL["ML"]] == [0x36A0000000000000]
    assert by_name("F3 ML B:f x1 ffc12345 #11")[0][COL["ML"]] == [signed(0xFFF82468A0000000)]
    assert by_name("F3 XT f ffc12345 #11")[2][1][3] == b"-nan" and by_name("F3 XT f 7f800001 #6")[2][1][3] == b"nan" and by_name("F3 XT f 3dcccccd #7")[2][1][3] == b"0.1"
    assert by_name("F3 XT B:f x5 00000001 #4")[2][1][4] == b"f,1,1.4013e-45,-0,-1.4013e-45,-3.14159"
    assert by_name("F3 XT d #6")[2][1][3] == b"1e+06" and by_name("F3 XT d #12")[2][1][3] == b"-nan" and by_name("F3 NM f 7f7fffff #8")[0][COL["NM"]] == 0
    # F4: a truncated field is refused by bam_aux_get (skip_aux NULL, sam.c:4806 / 4841) and listed with an empty value
    cells, mx, ma = by_name("F4 NM i 1 short")
    assert cells[COL["NM"]] is None and cells[COL["UQ"]] == 7 and ma == ([b"UQ", b"YA", b"NM"], [b"7", b"ya", b""])
    cells, mx, ma = by_name("F4 MD Z without NUL")                           # skip_aux answers `end`; bam_aux_get wants the NUL (sam.c:4842)
    assert cells[COL["MD"]] is None and ma == ([b"UQ", b"YA", b"MD"], [b"7", b"ya", b"abc"])
    assert by_name("F4 ML B:I count 3 overruns")[0][COL["ML"]] is None and by_name("F4 CG B:I count 1073741825 overruns")[0][COL["CG"]] is None
    assert by_name("F4 NM 2 stray bytes")[2] == ([b"UQ", b"YA"], [b"7", b"ya"])                    # end - next <= 2 (sam.c:4824)
    assert by_name("F4 NM tag and i, no payload")[2] == ([b"UQ", b"YA", b"NM"], [b"7", b"ya", b""]) and by_name("F4 MD tag and Z, no payload")[0][COL["MD"]] is None
    # F5: the first field of a name is the only one bam_aux_get looks at (sam.c:4838-4844)
    assert by_name("F5 NM twice")[0][COL["NM"]] == 77 and by_name("F5 NM wrong type first")[0][COL["NM"]] == 0 and by_name("F5 MD wrong type first")[0][COL["MD"]] is None
    assert by_name("F5 NM then a corrupt copy")[0][COL["NM"]] == 77 and by_name("F5 NM then a corrupt copy")[2][0][-1] == b"NM"
    assert by_name("F5 NM behind a corrupt field")[0][COL["NM"]] is None and by_name("F5 NM in front of a corrupt field")[0][COL["NM"]] == 77
    assert by_name("F5 NM twice")[2] == ([b"UQ", b"YA", b"NM", b"NM", b"AS", b"YB"], [b"7", b"ya", b"77", b"-5", b"-5", b"yb"])
    # F6: the key is the C string of tagbuf (bam_reader.c:1006-1015); A 0x00 is the empty C string (bam_reader.c:933-934)
    assert by_name("F6 key %r" % b"X\0")[1] == ([b"YA", b"X", b"YB"], [b"ya", b"42", b"yb"]) and by_name("F6 key %r" % b"\0X")[1][0][1] == b""
    assert by_name("F6 key %r" % b"NX")[0][COL["NM"]] is None and by_name("F6 key %r" % b"NX")[1][0] == [b"YA", b"NX", b"YB"]
    assert by_name("F6 TS A 0x00")[0][COL["TS"]] == b"" and by_name("F6 TS A 0xe9")[0][COL["TS"]] == b"\xe9" and by_name("F6 XT A 0x00")[2][1][2] == b""
    assert len(by_name("F6 Z of 70000")[0][COL["MD"]]) == 70000 and by_name("F6 Z of 70000")[0][COL["AS"]] == -5
    assert by_name("F6 3000 fields")[0][COL["NM"]] == 2279 & 0xff and len(by_name("F6 3000 fields")[2][0]) == 3004
    assert by_name("F6 aux of 2 bytes")[2] is None and by_name("F6 aux of 3 bytes")[2] == ([b"NM"], [b""]) and by_name("F6 aux of 3 bytes")[0][COL["NM"]] is None
    # F7: a swapped CG tag is gone (sam.c:722-724): its column is NULL and the fields around it are all there
    for p in TC.F7_POSITIONS:
        cells, mx, ma = by_name("F7 CG " + p)
        assert cells[COL["CG"]] is None and (ma is None or b"CG" not in ma[0])
        if p != "only":
            assert (cells[COL["NM"]], cells[COL["MD"]], cells[COL["TS"]], cells[COL["ML"]], cells[COL["FZ"]], cells[COL["PG"]]) == (77, b"10A5", b"+", [1, 2, 255], [65535, 1], b"bwa"), p
            assert mx == ([b"YA", b"YB"], [b"ya", b"yb"])
    assert by_name("F7 CG only") == ([None] * 56, None, None)
    cells, mx, ma = by_name("F7 CG shorter than the CIGAR stays")             # CG_len < n_cigar: not moved (sam.c:707)
    assert cells[COL["CG"]] == [640] and ma[0] == [b"UQ", b"YA", b"CG", b"AS", b"YB"] and ma[1][2] == b"I,640"
    cells, mx, ma = by_name("F7 MD behind CG: Z without NUL")
    assert cells[COL["CG"]] is None and cells[COL["MD"]] is None and cells[COL["UQ"]] == 7 and ma == ([b"UQ", b"YA", b"MD"], [b"7", b"ya", b"abc"])
