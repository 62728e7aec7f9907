"""fasta_nuc through the DuckDB surface (tests/minihost, DHTS_NUC_FUNCTIONS=1): the reference's own statements (test/sql/duckhts.test:
286-317) on the heads of its ce.fa with its targets.bed, the schema, chunking, projection, and every error string at its stage
(src/interval_udf.c:475-627)."""
import os
import shutil
import struct
import subprocess

import pytest

import fasta_index_ref as F
import fasta_nuc_ref as M
from conftest import GOLDEN, read_golden
from test_duckdb_surface import HOST, parse_chunks, run_host

ON = {"DHTS_NUC_FUNCTIONS": "1"}
BIGINT, DOUBLE, VARCHAR = 5, 11, 17
TYPES = [VARCHAR, BIGINT, BIGINT, DOUBLE, DOUBLE] + [BIGINT] * 7 + [VARCHAR]


def nuc(path, named=(), proj=None):
    return run_host(path, named=named, proj=proj, fn="fasta_nuc", env=ON)


def columns(dump):
    """-> (schema, chunk sizes, per projected column the values: bytes / None, ints, and for DOUBLE the 64 bits as an int)"""
    schema, chunks = parse_chunks(dump)
    ncol = len(chunks[0][1]) if chunks else 0
    cols = [[] for _ in range(ncol)]
    for n, cc in chunks:
        for k, (_t, valid, vals) in enumerate(cc):
            for r in range(n):
                ok = (int(valid[r >> 6]) >> (r & 63)) & 1
                cols[k].append((vals[r] if isinstance(vals[r], (bytes, type(None))) else int(vals[r])) if ok else None)
    return schema, [n for n, _ in chunks], cols


def as_dumped(exp, names):
    """the model's columns the way `columns` shows them"""
    def bits(x):
        return struct.unpack("<q", struct.pack("<d", x))[0]
    return [[bits(v) for v in exp[k]] if k in ("pct_at", "pct_gc") else exp[k] for k in names]


@pytest.fixture()
def ce(tmp_path):
    d = str(tmp_path)
    fa, bed = os.path.join(d, "ce_heads.fa"), os.path.join(d, "targets.bed")
    shutil.copy(os.path.join(GOLDEN, "ce_heads.fa"), fa)
    shutil.copy(os.path.join(GOLDEN, "targets.bed"), bed)
    return {"dir": d, "fa": fa, "bed": bed, "text": read_golden("ce_heads.fa"), "bed_text": read_golden("targets.bed")}


@pytest.mark.gpu
def test_reference_statements(ce):
    rc, out, _ = nuc(ce["fa"], named=[("bin_width", "10")])
    assert rc == 3 and out == "ERROR bind: fasta_nuc: failed to open FASTA index"                       # a missing .fai is never built
    rc, out, _ = run_host(ce["fa"], fn="fasta_index", env={"DHTS_SEQ_FUNCTIONS": "1"})
    assert rc == 0, out
    fai = ce["fa"] + ".fai"
    if not os.path.exists(fai):                                                                        # fasta_index returns the rows; the file is the caller's
        open(fai, "wb").write(F.save(F.build(ce["text"])))
    fai_bytes = open(fai, "rb").read()
    assert fai_bytes == F.save(F.build(ce["text"]))
    rc, out, dump = nuc(ce["fa"], named=[("bed_path", ce["bed"])])
    assert rc == 0 and "rows=4 " in out, out
    schema, sizes, cols = columns(dump)
    assert schema == list(zip(M.COLUMNS[:12], TYPES[:12]))                                             # interval_udf.c:451-473
    exp = M.fasta_nuc(ce["text"], fai_bytes, bed_text=ce["bed_text"])
    assert cols == as_dumped(exp, M.COLUMNS[:12])
    i = [k for k in range(4) if cols[0][k] == b"CHROMOSOME_I" and cols[1][k] == 0][0]                  # duckhts.test:286-295
    assert [cols[k][i] for k in range(5, 12)] == [2, 4, 2, 2, 0, 0, 10]
    assert [struct.unpack("<d", struct.pack("<q", cols[k][i]))[0] for k in (3, 4)] == [0.4, 0.6]
    rc, out, dump = nuc(ce["fa"], named=[("bin_width", "10"), ("region", "CHROMOSOME_I:1-20")])         # :297-305
    assert rc == 0 and "rows=2 " in out, out
    _, _, cols = columns(dump)
    assert sum(cols[11]) == 20 and cols[1] == [0, 10] and cols[2] == [10, 20]
    rc, out, dump = nuc(ce["fa"], named=[("bed_path", ce["bed"]), ("include_seq", "true")])             # :307-317
    assert rc == 0 and "rows=4 " in out, out
    schema, _, cols = columns(dump)
    assert schema == list(zip(M.COLUMNS, TYPES)) and cols[12][i] == b"GCCTAAGCCT"
    assert cols == as_dumped(M.fasta_nuc(ce["text"], fai_bytes, bed_text=ce["bed_text"], include_seq=True), M.COLUMNS)
    # the BED's own region: with a tabix index made by tabix_index, without one (silent), and a sequence the index does not know
    gz, tbi = os.path.join(ce["dir"], "t.bed.gz"), os.path.join(ce["dir"], "elsewhere.tbi")
    rc, out, _ = run_host(ce["bed"], named=[("output_path", gz), ("keep", "true"), ("overwrite", "true")], fn="bgzip")
    assert rc == 0, out
    rc, out, dump = nuc(ce["fa"], named=[("bed_path", gz), ("region", "CHROMOSOME_I:1-15")])
    assert rc == 0 and "rows=2 " in out, out
    rc, out, _ = run_host(gz, named=[("preset", "bed"), ("index_path", tbi), ("threads", "1")], fn="tabix_index")
    assert rc == 0, out
    rc, out, dump2 = nuc(ce["fa"], named=[("bed_path", gz), ("region", "CHROMOSOME_I:1-15"), ("bed_index_path", tbi)])
    assert rc == 0 and "rows=2 " in out and columns(dump2)[2] == columns(dump)[2], out
    rc, out, _ = nuc(ce["fa"], named=[("bed_path", gz), ("region", "CHROMOSOME_V"), ("bed_index_path", tbi)])
    assert rc != 0 and out == "ERROR init: fasta_nuc: failed to create BED region iterator", out        # interval_udf.c:600-605
    rc, out, _ = nuc(ce["fa"], named=[("bed_path", gz), ("region", "CHROMOSOME_V")])
    assert rc == 0 and "rows=0 " in out, out
    # init errors
    for region in ("nope", "CHROMOSOME_I:1-101", "CHROMOSOME_I:102"):
        rc, out, _ = nuc(ce["fa"], named=[("bin_width", "10"), ("region", region)])
        assert rc != 0 and out == "ERROR init: fasta_nuc: invalid FASTA region", out                    # :584-588
    rc, out, _ = nuc(ce["fa"], named=[("bed_path", "/no/such.bed")])
    assert rc != 0 and out == "ERROR init: fasta_nuc: failed to open BED file", out                     # :591-596
    bad = os.path.join(ce["dir"], "bad.fai")
    open(bad, "wb").write(b"CHROMOSOME_I\tnot\tnumbers\n")
    rc, out, _ = nuc(ce["fa"], named=[("bin_width", "10"), ("index_path", bad)])
    assert rc != 0 and out == "ERROR init: fasta_nuc: failed to load FASTA index", out                  # :578-583
    other = os.path.join(ce["dir"], "other.fai")
    shutil.copy(fai, other)
    os.remove(fai)
    rc, out, _ = nuc(ce["fa"], named=[("bin_width", "50"), ("index_path", other)])
    assert rc == 0 and "rows=14 " in out, out


@pytest.mark.gpu
def test_chunks_and_projection(tmp_path):
    import random
    rng = random.Random(3)
    seq = bytes(rng.choice(b"ACGTNacgtnRY") for _ in range(4996))
    text = b">a\n" + b"\n".join(seq[i:i + 60] for i in range(0, len(seq), 60)) + b"\n>b\nACGT\n"
    fa = os.path.join(str(tmp_path), "five.fa")
    open(fa, "wb").write(text)
    fai = F.save(F.build(text))
    open(fa + ".fai", "wb").write(fai)
    exp = M.fasta_nuc(text, fai, bin_width=1, include_seq=True)
    assert exp["n_rows"] == 5000
    rc, out, dump = nuc(fa, named=[("bin_width", "1"), ("include_seq", "true")], proj=[12, 10, 0, 4, 2])   # projection ids out of order
    assert rc == 0 and "rows=5000 " in out, out
    _, sizes, cols = columns(dump)
    assert sizes == [2048, 2048, 904]
    assert cols == as_dumped(exp, ["seq", "num_other", "chrom", "pct_gc", "end"])
    rc, out, dump = nuc(fa, named=[("bin_width", "1")], proj=[11])
    assert rc == 0 and columns(dump)[2] == [[1] * 5000]


def test_bind_errors_without_a_device(tmp_path):
    rc, out, _ = nuc("")
    assert rc == 3 and out == "ERROR bind: fasta_nuc requires a FASTA path"
    rc, out, _ = nuc("x.fa")
    assert rc == 3 and out == "ERROR bind: fasta_nuc requires exactly one of bed_path or bin_width"
    rc, out, _ = nuc("x.fa", named=[("bed_path", "x.bed"), ("bin_width", "5")])
    assert rc == 3 and out == "ERROR bind: fasta_nuc requires exactly one of bed_path or bin_width"
    for w in ("0", "-4"):
        rc, out, _ = nuc("x.fa", named=[("bin_width", w)])
        assert rc == 3 and out == "ERROR bind: fasta_nuc bin_width must be > 0"
    rc, out, _ = nuc("/no/such.fa", named=[("bin_width", "5")])
    assert rc == 3 and out == "ERROR bind: fasta_nuc: failed to open FASTA index"
    fa = os.path.join(str(tmp_path), "no_index.fa")
    open(fa, "wb").write(b">a\nACGT\n")
    rc, out, _ = nuc(fa, named=[("bin_width", "5")])
    assert rc == 3 and out == "ERROR bind: fasta_nuc: failed to open FASTA index" and not os.path.exists(fa + ".fai")
    rc, out, _ = nuc("x.fa", named=[("bogus", "1")])
    assert rc == 3 and "unknown named parameter" in out
    for k in ("bed_path", "bin_width", "region", "index_path", "bed_index_path", "include_seq"):
        rc, out, _ = nuc("/no/such.fa", named=[(k, "1")])
        assert "unknown named parameter" not in out


def test_registered_only_with_the_variable():
    import duckhts_amd
    others = ("DHTS_INTERVAL_FUNCTIONS", "DHTS_SEQ_FUNCTIONS", "DHTS_TABIX_FUNCTIONS")
    env = {k: v for k, v in os.environ.items() if k not in others + ("DHTS_NUC_FUNCTIONS",)}

    def catalog(**kw):
        return subprocess.run([HOST, duckhts_amd.LIB_PATH, "--catalog", "-"], capture_output=True, text=True, env=dict(env, **kw)).stdout.splitlines()

    r = subprocess.run([HOST, duckhts_amd.LIB_PATH, "fasta_nuc", ""], capture_output=True, text=True, env=env)
    assert r.returncode == 3 and r.stdout.strip() == "ERROR catalog: table function fasta_nuc not registered"
    default = catalog()
    assert [ln.split()[1] for ln in default] == ["read_bcf", "read_bam", "bgzip", "bgunzip", "bam_index", "bcf_index", "tabix_index"]
    three = catalog(**{k: "1" for k in others})
    assert [ln.split()[1] for ln in three][len(default):] == ["read_fasta", "read_fastq", "fasta_index", "read_bed", "read_tabix", "read_gtf", "read_gff"]
    for k in others:                                                        # none of the existing variables registers it
        assert not any("fasta_nuc" in ln for ln in catalog(**{k: "1"}))
    on = catalog(**ON)
    assert on[:len(default)] == default
    assert on[len(default):] == ["TF fasta_nuc pushdown=1 bind=1 init=1 local_init=0 func=1 named=bed_path:17,bin_width:5,region:17,index_path:17,bed_index_path:17,include_seq:1"]   # interval_udf.c:854-876
    four = catalog(DHTS_NUC_FUNCTIONS="1", **{k: "1" for k in others})
    assert [ln.split()[1] for ln in four][len(default):] == ["read_fasta", "read_fastq", "fasta_index", "read_bed", "fasta_nuc", "read_tabix", "read_gtf", "read_gff"]   # src/duckhts.c:56-69
    assert [ln for ln in four if "fasta_nuc" not in ln] == three
