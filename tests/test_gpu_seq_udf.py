"""The seq_* / cigar_* / SAM flag functions and seq_kmers on device columns (dhts_udf_*, seq_udf.hip) against the Python restatement of
src/kmer_udf.c (tests/kmer_udf_ref.py).  Every comparison is exact; DOUBLE is compared by bits against Python's gc / called (one IEEE
division on both sides, no fast-math in the build)."""
import json
import os
import struct

import pytest

import duckhts_amd
import kmer_udf_cases as cases
import kmer_udf_ref as ref
from conftest import GOLDEN, read_golden

pytestmark = pytest.mark.gpu

STATEMENTS = json.load(open(os.path.join(GOLDEN, "kmer_udf_statements.json")))
STRING_FUNCS = ["seq_revcomp", "seq_canonical", "seq_hash_2bit", "seq_encode_4bit", "seq_gc_content"]
CIGAR_FUNCS = [f for f in duckhts_amd.UDF_OPS if f.startswith("cigar_") and f != "cigar_has_op"]


@pytest.fixture(scope="module")
def ctx():
    c = duckhts_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(params=["default", "4", "16", "64"])
def group(request, monkeypatch):
    """the lanes per row of the text kernels: the library's own choice, and each group size forced"""
    if request.param != "default":
        monkeypatch.setenv("DHTS_UDF_GROUP", request.param)
    return request.param


def bits(x):
    return None if x is None else struct.pack("<d", x)


def _eq(g, e):
    if isinstance(e, float):
        return isinstance(g, float) and bits(g) == bits(e)
    return g == e and isinstance(g, bool) == isinstance(e, bool)


def same(got, exp):
    """exact equality row by row: floats by their bits, a boolean only equals a boolean"""
    return len(got) == len(exp) and all(_eq(g, e) for g, e in zip(got, exp))


def first_diff(got, exp):
    for i, (g, e) in enumerate(zip(got, exp)):
        if not same([g], [e]):
            return i, g if not isinstance(g, (bytes, list)) or len(g) < 80 else (len(g), g[:40]), e if not isinstance(e, (bytes, list)) or len(e) < 80 else (len(e), e[:40])
    return (len(got), len(exp))


def as_bytes(x):
    return x.encode() if isinstance(x, str) else x


# ---- 1. the reference's published statements ---------------------------------------------------------------------------------------
def test_published_statements_through_the_module_functions():
    for st in STATEMENTS["literals"]:
        f = getattr(duckhts_amd, st["fn"])
        args = [as_bytes(a) for a in st["args"]]
        got = f([args[0]], *args[1:])[0]
        if st.get("format"):
            got = st["format"] % got
        exp = st["expect"]
        assert got == (as_bytes(exp) if not st.get("format") else exp), (st, got)
    for st in STATEMENTS["seq_kmers"]:
        got = duckhts_amd.seq_kmers([st["seq"]], st["k"], canonical=st["canonical"])
        assert got["kmer"] == [e.encode() for e in st["expect"]] and got["pos"] == list(range(1, len(st["expect"]) + 1)) and got["row"] == [0] * len(st["expect"]), (st, got)


def test_published_statements_and_the_model_on_a_batch_kept_in_hbm():
    data = read_golden("range.bam")
    c = duckhts_amd.Context(0)
    try:
        c.open(data); c.bgzf_index(); hdr = c.bam_open()
        b = c.next_batch()
        n = int(b.n_rows)
        assert n == 112
        host = c.batch_to_host(b, hdr)
        seq, cigar, flag = host["SEQ"], host["CIGAR"], [int(x) for x in host["FLAG"]]
        for f in STRING_FUNCS:
            got = c.udf(f, b.seq, n_rows=n)
            assert same(got, [ref.call(f, s) for s in seq]), (f, first_diff(got, [ref.call(f, s) for s in seq]))
        for f in CIGAR_FUNCS:
            assert c.udf(f, b.cigar, n_rows=n) == [ref.call(f, s) for s in cigar], f
        for op in (b"M", b"S", b"I", b"s", b"B"):
            assert c.udf("cigar_has_op", b.cigar, op, n_rows=n) == [ref.cigar_has_op(s, op) for s in cigar], op
        for f in ref.FLAG_FIELDS + ["is_forward_aligned", "sam_flag_bits"]:
            assert c.udf(f, b.flag, n_rows=n, width=2) == [ref.call(f, v) for v in flag], f
        for m in (1, 16, 1024):
            assert c.udf("sam_flag_has", b.flag, m, n_rows=n, width=2) == [ref.sam_flag_has(v, m) for v in flag]
        km = c.udf_seq_kmers(b.seq, 31, canonical=True, hash=True, n_rows=n)
        exp = ref.seq_kmers_column(seq, 31, True)
        assert list(zip(km["row"], km["pos"], km["kmer"], km["hash"])) == exp
        # the first row, as the statements select it
        fr = STATEMENTS["first_row"]
        for f, e in fr["flag"].items():
            assert c.udf(f, b.flag, n_rows=n, width=2)[0] is e
        bits12 = c.udf("sam_flag_bits", b.flag, n_rows=n, width=2)[0]
        for f, e in fr["sam_flag_bits"].items():
            assert bits12[ref.FLAG_FIELDS.index(f)] is e
        for m, e in fr["sam_flag_has"].items():
            assert c.udf("sam_flag_has", b.flag, int(m), n_rows=n, width=2)[0] is e
        assert c.udf("cigar_has_op", b.cigar, "M", n_rows=n)[0] is True and c.udf("cigar_has_soft_clip", b.cigar, n_rows=n)[0] is False
        assert c.udf("cigar_reference_length", b.cigar, n_rows=n)[0] > 0
        # the batch is still there, untouched
        again = c.batch_to_host(b, hdr)
        for k in ("QNAME", "CIGAR", "SEQ", "QUAL"):
            assert again[k] == host[k]
        assert list(again["FLAG"]) == list(host["FLAG"]) and list(again["POS"]) == list(host["POS"])
        # packed SEQ is 4-bit codes, not text
        c.set_seq_packed(True)
        c.rewind()
        b2 = c.next_batch()
        assert b2.seq_packed == 1
        for call in (lambda: c.udf("seq_revcomp", b2.seq, n_rows=int(b2.n_rows)), lambda: c.udf_seq_kmers(b2.seq, 3, n_rows=int(b2.n_rows))):
            with pytest.raises(duckhts_amd.DhtsError, match="packed SEQ"):
                call()
        assert c.udf("cigar_query_length", b2.cigar, n_rows=int(b2.n_rows)) == [ref.call("cigar_query_length", s) for s in cigar]
    finally:
        c.close()


# ---- 2. the edge table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", sorted({e[0] for e in cases.EDGE}))
def test_edge_table(ctx, fn, group):
    rows = [e for e in cases.EDGE if e[0] == fn]
    kind = "list" if fn == "seq_decode_4bit" else "int" if duckhts_amd.UDF_OPS.index(fn) >= 14 else "str"
    a0 = ctx.udf_upload([r[1][0] for r in rows], 0, kind=kind)
    a1 = None
    if len(rows[0][1]) == 2:
        a1 = ctx.udf_upload([r[1][1] for r in rows], 1, kind="int" if fn == "sam_flag_has" else "str")
    got = ctx.udf(fn, a0, a1)
    exp = [r[2] for r in rows]
    assert same(got, exp), (fn, first_diff(got, exp), rows[first_diff(got, exp)[0]])
    if a1 is not None:                                          # one second argument for every row
        for second in sorted({r[1][1] for r in rows if r[1][1] is not None}, key=repr):
            sub = [r for r in rows if r[1][1] == second]
            a0 = ctx.udf_upload([r[1][0] for r in sub], 0, kind=kind)
            assert ctx.udf(fn, a0, second) == [r[2] for r in sub], (fn, second)


# ---- 3. / 4. seeded rows, both input layouts -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def expected():
    col = cases.seq_column()
    short = [s for s in col if s is None or len(s) <= 33] + [s[:32] for s in col if s and len(s) > 33] + [s[-17:] for s in col if s and len(s) > 33]
    exp = {f: [ref.call(f, s) for s in col] for f in STRING_FUNCS}
    exp["short"] = short
    exp["seq_hash_2bit/short"] = [ref.seq_hash_2bit(s) for s in short]
    exp["seq_decode_4bit"] = [ref.seq_decode_4bit(r) for r in cases.code_column()]
    return exp


@pytest.mark.parametrize("reserve", [0, 37])
@pytest.mark.parametrize("fn", STRING_FUNCS + ["seq_decode_4bit", "seq_hash_2bit/short"])
def test_seeded_rows(ctx, expected, fn, reserve, group):
    col = cases.code_column() if fn == "seq_decode_4bit" else expected["short"] if fn.endswith("/short") else cases.seq_column()
    assert len(col) >= 2900 and (fn != "seq_revcomp" or max(len(s) for s in col if s) == 70001)
    a = ctx.udf_upload(col, 0, kind="list" if fn == "seq_decode_4bit" else "str", reserve=reserve)
    got = ctx.udf(fn.split("/")[0], a)
    exp = expected[fn]
    assert sum(e is not None for e in exp) > 400 and sum(e is None for e in exp) > 400
    assert same(got, exp), (fn, first_diff(got, exp))


def test_seeded_cigars_and_flags(ctx):
    col = cases.cigar_column()
    a = ctx.udf_upload(col, 0, reserve=3)
    for f in CIGAR_FUNCS:
        exp = [ref.call(f, s) for s in col]
        got = ctx.udf(f, a)
        assert got == exp and all(type(g) is type(e) for g, e in zip(got, exp)), (f, first_diff(got, exp))
    for op in b"MIDNSHP=X":
        assert ctx.udf("cigar_has_op", a, bytes([op])) == [ref.cigar_has_op(s, bytes([op])) for s in col], op
    flags = cases.flag_column()
    fa = ctx.udf_upload(flags, 0, kind="int")
    for f in ref.FLAG_FIELDS + ["is_forward_aligned", "sam_flag_bits"]:
        assert ctx.udf(f, fa) == [ref.call(f, v) for v in flags], f
    masks = list(reversed(flags))
    assert ctx.udf("sam_flag_has", fa, ctx.udf_upload(masks, 1, kind="int")) == [ref.sam_flag_has(v, m) for v, m in zip(flags, masks)]


@pytest.mark.parametrize("fn", [f for f in duckhts_amd.UDF_OPS])
def test_all_null_column_and_no_rows(ctx, fn):
    idx = duckhts_amd.UDF_OPS.index(fn)
    kind = "list" if fn == "seq_decode_4bit" else "int" if idx >= 14 else "str"
    second = {"cigar_has_op": "M", "sam_flag_has": 1}.get(fn)
    assert ctx.udf(fn, ctx.udf_upload([None] * 300, 0, kind=kind), second) == [None] * 300
    assert ctx.udf(fn, ctx.udf_upload([], 0, kind=kind), second) == []
    r = ctx.udf(fn, ctx.udf_upload([], 0, kind=kind), second, fetch=False)
    assert r.n_rows == 0


# ---- 5. seq_kmers ------------------------------------------------------------------------------------------------------------------
KMER_ROWS = [b"", b"A", b"AC", b"ACG", b"ACGTA", None, b"acgtnACGTN" * 4, b"TTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTT", b"ACGTXACGT-acgt" * 5, b"GATTACA" * 9 + b"\xc3\xa9" + b"CATTAG" * 8,
             b"N" * 31, b"A" * 31, b"C" * 32, b"G" * 33, b"ACGT" * 8 + b"A", bytes(cases.seq_column()[5] or b"")] + [s for s in cases.seq_column()[:400] if s is not None and len(s) <= 257]


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [1, 3, 31, 32, 33])
def test_seq_kmers(ctx, k, canonical):
    exp = ref.seq_kmers_column(KMER_ROWS, k, canonical)
    assert len(exp) > 1000
    a = ctx.udf_upload(KMER_ROWS, 0)
    text = ctx.udf_seq_kmers(a, k, canonical=canonical, text=True, hash=False)
    assert list(zip(text["row"], text["pos"], text["kmer"])) == [e[:3] for e in exp]
    if k <= 32:
        both = ctx.udf_seq_kmers(a, k, canonical=canonical, text=True, hash=True)
        only = ctx.udf_seq_kmers(a, k, canonical=canonical, text=False, hash=True)
        assert list(zip(both["row"], both["pos"], both["kmer"], both["hash"])) == exp
        assert list(zip(only["row"], only["pos"], only["hash"])) == [(e[0], e[1], e[3]) for e in exp] and "kmer" not in only
        assert any(e[3] is None for e in exp) and any(e[3] is not None for e in exp)
    else:
        with pytest.raises(duckhts_amd.DhtsError, match="k <= 32"):
            ctx.udf_seq_kmers(a, k, canonical=canonical, text=False, hash=True)
    rows = [s for s in KMER_ROWS[:40]]
    a = ctx.udf_upload(rows, 0, reserve=5)
    one = ctx.udf_seq_kmers(a, k, canonical=canonical, hash=k <= 32)
    stepped = ctx.udf_seq_kmers(a, k, canonical=canonical, hash=k <= 32, max_rows=7)
    assert one == stepped and len(one["row"]) == len(ref.seq_kmers_column(rows, k, canonical)) > 7


def test_seq_kmers_errors_and_empty(ctx):
    a = ctx.udf_upload([b"ACGT"], 0)
    for k in (0, -3):
        with pytest.raises(duckhts_amd.DhtsError, match="seq_kmers: k must be > 0"):
            ctx.udf_seq_kmers(a, k)
    assert ctx.udf_seq_kmers(a, 5) == {"row": [], "pos": [], "kmer": []}
    assert ctx.udf_seq_kmers(ctx.udf_upload([], 0), 3, hash=True) == {"row": [], "pos": [], "kmer": [], "hash": []}
    assert duckhts_amd.seq_kmers(["ACGTA", None, "ac"], 2, canonical=True, hash=True) == {
        "row": [0, 0, 0, 0, 2], "pos": [1, 2, 3, 4, 1], "kmer": [b"AC", b"CG", b"AC", b"TA", b"AC"], "hash": [1, 6, 1, 12, 1]}


# ---- 6. seq_encode_4bit -> seq_decode_4bit ------------------------------------------------------------------------------------------
def test_encode_decode_round_trip_and_compacted_children(ctx, group):
    col = [s for s in cases.seq_column() if s is None or len(s) <= 4097][:1500]
    col[3:3] = [b"ACGTRYSWKMBDHVN", b"AC-GT", b"", None, b"acgtryswkmbdhvn" * 7, b"ACGU", b"N"]
    a = ctx.udf_upload(col, 0, reserve=2)
    enc = ctx.udf("seq_encode_4bit", a, fetch=False)
    raw = ctx.udf_fetch(enc, raw=True)
    exp = [ref.seq_encode_4bit(s) for s in col]
    off = [0]
    for e in exp:
        off.append(off[-1] + (len(e) if e is not None else 0))                     # no children are kept for a NULL row
    assert raw["off"].tolist() == off and len(raw["bytes"]) == off[-1]
    assert raw["bytes"].tolist() == [c for e in exp if e is not None for c in e]
    assert ctx.udf_fetch(enc) == exp
    dec = ctx.udf("seq_decode_4bit", ctx.udf_as_arg(enc))                           # the list column just made, still on the device
    assert dec == [None if e is None else s.upper() for s, e in zip(col, exp)]
    assert sum(d is not None for d in dec) > 300 and sum(d is None for d in dec) > 300
