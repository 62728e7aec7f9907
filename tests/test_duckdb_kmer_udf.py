"""The k-mer family through its DuckDB surface (register_kmer_udf_functions, csrc/duckdb_udf.inc) on a ctypes host (tests/scalarhost.py):
every scalar function on chunks of 2048 rows and of one row, list and struct outputs, seq_kmers across the 2048-row chunk boundary.
Exact comparisons against tests/kmer_udf_ref.py; DOUBLE by bits."""
import json
import os
import struct

import pytest

import kmer_udf_cases as cases
import kmer_udf_ref as ref
import scalarhost
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
STATEMENTS = json.load(open(os.path.join(GOLDEN, "kmer_udf_statements.json")))
SCALARS = [r for r in ref.REGISTERED if r[0] != "seq_kmers"]


@pytest.fixture(scope="module")
def host():
    return scalarhost.load({"DHTS_KMER_FUNCTIONS": "1"})


def _eq(g, e):
    if isinstance(e, float):
        return isinstance(g, float) and struct.pack("<d", g) == struct.pack("<d", e)
    return g == e and isinstance(g, bool) == isinstance(e, bool)


def same(got, exp):
    return len(got) == len(exp) and all(_eq(g, e) for g, e in zip(got, exp))


def as_bytes(x):
    return x.encode() if isinstance(x, str) else x


def column(ptype, n, salt):
    """n rows of a parameter type, NULLs among them; short enough that a 2048-row chunk stays small"""
    if ptype == "VARCHAR":
        src = [s for s in cases.seq_column() if s is None or len(s) <= 257] + cases.cigar_column()
    elif ptype == "UTINYINT[]":
        src = [r for r in cases.code_column() if r is None or len(r) <= 257]
    else:
        src = [v for v in cases.flag_column() if v is None or (0 <= v <= 65535 if ptype == "USMALLINT" else True)]
    return [src[(salt + 7 * i) % len(src)] for i in range(n)]


def test_reference_statements(host):
    for st in STATEMENTS["literals"]:
        got = host.call(st["fn"], *[[as_bytes(a)] for a in st["args"]])[0]
        if st.get("format"):
            assert st["format"] % got == st["expect"], st
        else:
            assert _eq(got, as_bytes(st["expect"])), (st, got)
    for st in STATEMENTS["seq_kmers"]:
        r = host.table_function("seq_kmers", st["seq"], st["k"], **({"canonical": True} if st["canonical"] else {}))
        assert r["columns"] == [("pos", "BIGINT"), ("kmer", "VARCHAR")] and r["max_threads"] == 1
        assert r["rows"] == [(i + 1, e.encode()) for i, e in enumerate(st["expect"])], (st, r)
        assert r["cardinality"] == (len(st["expect"]), True)


@pytest.mark.parametrize("n", [2048, 1])
@pytest.mark.parametrize("fn", [r[0] for r in SCALARS])
def test_every_scalar_function_on_a_chunk(host, fn, n):
    _, params, _ = next(r for r in SCALARS if r[0] == fn)
    cols = [column(p, n, 11 + 1000 * k) for k, p in enumerate(params)]
    if fn == "cigar_has_op":
        cols[1] = [[b"M", b"S", b"s", b"I", None, b"B", b"MM", b"="][i % 8] for i in range(n)]
        cols[0] = [cases.cigar_column()[(3 + 5 * i) % 3000] for i in range(n)]
    got = host.call(fn, *cols)
    exp = [ref.call(fn, *args) for args in zip(*cols)]
    assert same(got, exp), (fn, next((i, g, e) for i, (g, e) in enumerate(zip(got, exp)) if not _eq(g, e)))
    if n > 1:
        assert any(e is None for e in exp) and any(e is not None for e in exp)
    assert host.call(fn, *[[None] for _ in params]) == [None]


def test_seq_encode_4bit_appends_behind_children_the_vector_holds(host):
    f = host.function("seq_encode_4bit")
    out = scalarhost.Vec(f.ret)
    out.fill([[9, 9, 9], [7]])                                       # four children are there already
    assert out.list_size == 4
    rows = [b"ACGT", b"AC-T", None, b"", b"acgtn" * 500, b"N"]
    got = host.call("seq_encode_4bit", rows, output=out)
    assert got == [ref.seq_encode_4bit(r) for r in rows]
    assert out.list_size == 4 + 4 + 0 + 0 + 0 + 2500 + 1
    entries = [(int.from_bytes(bytes(out.buf[16 * i:16 * i + 8]), "little"), int.from_bytes(bytes(out.buf[16 * i + 8:16 * i + 16]), "little")) for i in range(6)]
    assert entries == [(4, 4), (8, 0), (8, 0), (8, 0), (8, 2500), (2508, 1)]              # :435-478: a NULL row keeps the running offset and no children
    assert list(out.child.buf[:4]) == [9, 9, 9, 7]


def test_sam_flag_bits_children_and_their_validity(host):
    flags = [1 | 16 | 128, None, 4095, 0, 65535]
    got = host.call("sam_flag_bits", flags)
    assert got == [ref.sam_flag_bits(v) for v in flags]
    out = host.last_output
    assert len(out.children) == 12 and [n for n, _ in out.t.fields] == ref.FLAG_FIELDS
    for k, ch in enumerate(out.children):
        assert ch.read(5) == [bool(v >> k & 1) if v is not None else None for v in flags]       # :670-676: a NULL row is NULL in every child
    assert not out.is_valid(1) and out.is_valid(0)


def test_seq_kmers_across_the_chunk_boundary(host):
    seq = "".join("ACGTNacgtX"[(i * 7 + i // 13) % 10] for i in range(5000))
    for canonical in (False, True):
        r = host.table_function("seq_kmers", seq, 3, canonical=canonical)
        assert r["chunks"] == [2048, 2048, 902] and r["cardinality"] == (4998, True)
        assert r["rows"] == ref.seq_kmers(seq.encode(), 3, canonical)
    assert host.table_function("seq_kmers", "AC", 3)["rows"] == []
    assert host.table_function("seq_kmers", "ACGTA", 5)["rows"] == [(1, b"ACGTA")]
