"""The Python restatement of src/kmer_udf.c (tests/kmer_udf_ref.py) against the reference's published statements
(tests/golden/kmer_udf_statements.json, from test/sql/duckhts.test:624-782) and a hand-written edge table; the C ABI and the module
functions exist and fail loudly without a device.  No GPU needed."""
import json
import os

import pytest

import duckhts_amd
import kmer_udf_cases as cases
import kmer_udf_ref as ref
import orc
from conftest import GOLDEN, read_golden

STATEMENTS = json.load(open(os.path.join(GOLDEN, "kmer_udf_statements.json")))


def as_bytes(x):
    return x.encode() if isinstance(x, str) else x


def test_model_gives_the_published_results():
    assert len(STATEMENTS["literals"]) == 23
    for st in STATEMENTS["literals"]:
        got = ref.call(st["fn"], *[as_bytes(a) for a in st["args"]])
        if st.get("format"):
            assert st["format"] % got == st["expect"], st
        else:
            assert got == as_bytes(st["expect"]) and isinstance(got, bool) == isinstance(st["expect"], bool), (st, got)
    for st in STATEMENTS["seq_kmers"]:
        got = ref.seq_kmers(st["seq"].encode(), st["k"], st["canonical"])
        assert [k for _, k in got] == [e.encode() for e in st["expect"]] and [p for p, _ in got] == list(range(1, len(got) + 1))


def test_model_gives_the_published_results_on_the_first_row_of_range_bam():
    t = orc.bam_read(read_golden("range.bam"))
    flag, cigar = int(t["FLAG"][0]), t["CIGAR"][0]
    fr = STATEMENTS["first_row"]
    for f, e in fr["flag"].items():
        assert ref.call(f, flag) is e, f
    bits = ref.sam_flag_bits(flag)
    for f, e in fr["sam_flag_bits"].items():
        assert bits[ref.FLAG_FIELDS.index(f)] is e, f
    for m, e in fr["sam_flag_has"].items():
        assert ref.sam_flag_has(flag, int(m)) is e
    assert ref.cigar_has_op(cigar, b"M") is True and ref.call("cigar_has_soft_clip", cigar) is False and ref.call("cigar_reference_length", cigar) > 0


@pytest.mark.parametrize("fn", sorted({e[0] for e in cases.EDGE}))
def test_model_on_the_edge_table(fn):
    rows = [e for e in cases.EDGE if e[0] == fn]
    assert rows
    for _, args, exp in rows:
        got = ref.call(fn, *args)
        assert got == exp and type(got) is type(exp), (fn, args, got, exp)


def test_edge_table_covers_the_quirks():
    """the rows the rules single out are in the table with the value the cited lines give"""
    e = {(f, a): x for f, a, x in cases.EDGE if all(not isinstance(v, list) for v in a)}
    assert e[("seq_canonical", (b"ACGT",))] == b"ACGT" and e[("seq_canonical", (b"AAT",))] == b"AAT" and e[("seq_canonical", (b"ATT",))] == b"AAT"
    assert e[("seq_hash_2bit", (b"",))] == 0 and e[("seq_hash_2bit", (b"A" * 32,))] == 0 and e[("seq_hash_2bit", (b"A" * 33,))] is None
    assert e[("seq_gc_content", (b"nnnn",))] is None and e[("seq_gc_content", (b"acgt",))] == e[("seq_gc_content", (b"ACGT",))] == 0.5
    assert ref.seq_decode_4bit([0]) is None and ref.seq_decode_4bit([16]) is None
    assert e[("cigar_has_op", (b"*", b"M"))] is False and e[("cigar_reference_length", (b"*",))] is None
    assert e[("cigar_has_op", (b"5M!", b"M"))] is True and e[("cigar_reference_length", (b"5M!",))] is None
    for s in (b"0M", b"M", b"5"):
        assert e[("cigar_query_length", (s,))] is None and e[("cigar_has_op", (s, b"M"))] is None
    assert e[("cigar_has_op", (b"5M", b"B"))] is None and e[("cigar_has_op", (b"5S90M", b"s"))] is e[("cigar_has_op", (b"5S90M", b"S"))] is True
    assert e[("cigar_has_op", (b"5M", b"MM"))] is None
    for v in (-1, 65536, 4):
        assert e[("is_forward_aligned", (v,))] is None


def test_the_function_ids_follow_the_registration_order():
    names = [r[0] for r in ref.REGISTERED]
    assert len(names) == 30 and names[6] == "seq_kmers"           # the 30 register_* calls of :1224-1253: 29 scalar functions and the table function
    assert duckhts_amd.UDF_OPS == [n for n in names if n != "seq_kmers"]
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "duckhts_amd.h")).read()
    enum = hdr[hdr.index("enum { DHTS_UDF_SEQ_REVCOMP = 0"):hdr.index("DHTS_UDF_OP_COUNT")]
    ids = [x.strip().split(" ")[0] for x in enum[len("enum {"):].split(",") if x.strip()]
    assert [i[len("DHTS_UDF_"):].lower() for i in ids] == duckhts_amd.UDF_OPS


def test_seeded_columns_are_what_the_gpu_tests_expect():
    col = cases.seq_column()
    assert len(col) == 3000 and max(len(s) for s in col if s is not None) == 70001
    assert {len(s) for s in col if s is not None} >= set(cases.LENGTHS)
    assert col == cases.seq_column() and any(s is None for s in col)
    ties = [s for s in col if s and len(s) > 16 and ref.seq_revcomp(s) == s.upper()]
    late = [s for s in col if s and len(s) >= 64 and ref.seq_revcomp(s) not in (None, s.upper())
            and min(i for i in range(len(s)) if s.upper()[i] != ref.seq_revcomp(s)[i]) >= len(s) // 2 - 1]
    assert len(ties) > 20 and len(late) > 20
    assert any(ref.seq_canonical(s) == s.upper() for s in late) and any(ref.seq_canonical(s) != s.upper() for s in late)


def test_without_a_device_the_functions_fail_loudly():
    L = duckhts_amd.lib()
    for n in ("dhts_udf_upload", "dhts_udf_apply", "dhts_udf_fetch", "dhts_udf_result_host_bytes", "dhts_udf_seq_kmers", "dhts_udf_kmers_fetch", "dhts_udf_kmers_host_bytes"):
        assert hasattr(L, n), n
    assert L.dhts_udf_apply(None, 0, None, None, 0, None) == -1 and L.dhts_udf_seq_kmers(None, None, 0, 3, 0, 1, 0, 0, 0, None) == -1
    if L.dhts_device_count() == 0:
        for call in (lambda: duckhts_amd.seq_revcomp([b"ACGT"]), lambda: duckhts_amd.cigar_has_op([b"5M"], "M"), lambda: duckhts_amd.is_paired([1]),
                     lambda: duckhts_amd.seq_kmers([b"ACGT"], 3)):
            with pytest.raises(duckhts_amd.DhtsError, match="no CPU fallback"):
                call()
