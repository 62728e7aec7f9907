"""read_tabix / read_gtf / read_gff through the DuckDB surface (tests/minihost, DHTS_TABIX_FUNCTIONS=1): the reference's statements of
test/sql/duckhts.test:406-519 that need no LIST parameter, the schemas with their MAP and DOUBLE columns, chunking and projection, and,
without a device, the bind / init errors and the registered sets."""
import os
import subprocess

import pytest

import read_tabix_ref as M
from conftest import GOLDEN
from test_duckdb_surface import HOST, parse_chunks, run_host

ON = {"DHTS_TABIX_FUNCTIONS": "1"}
INTEGER, BIGINT, DOUBLE, VARCHAR, MAP = 4, 5, 11, 17, 26
GFF = os.path.join(GOLDEN, "gff_file.gff.gz")
GXF_SCHEMA = [(n, t) for n, t in zip(M.GXF_NAMES, M.GXF_TYPES)]


def tf(fn, path, named=(), proj=None):
    return run_host(path, named=named, proj=proj, fn=fn, env=ON)


def columns(dump):
    """-> (schema, chunk sizes, per projected column the values: bytes, int, ("d", bits) for DOUBLE, [(key, value), ...] for MAP, None)"""
    schema, chunks = parse_chunks(dump)
    ncol = len(chunks[0][1]) if chunks else 0
    cols = [[] for _ in range(ncol)]
    for n, cc in chunks:
        for k, (t, valid, vals) in enumerate(cc):
            for r in range(n):
                if not (int(valid[r >> 6]) >> (r & 63)) & 1:
                    cols[k].append(None)
                elif t == MAP:
                    ent, kk, vv = vals
                    o, ln = int(ent[r][0]), int(ent[r][1])
                    cols[k].append(list(zip(kk[o:o + ln], vv[o:o + ln])))
                elif t == DOUBLE:
                    cols[k].append(("d", int(vals[r]) & 0xffffffffffffffff))      # the dump holds the 8 bytes
                else:
                    cols[k].append(vals[r] if isinstance(vals[r], bytes) else int(vals[r]))
    return schema, [n for n, _ in chunks], cols


def norm(v):
    return ("d", M.dbl_bits(v)) if isinstance(v, float) else v


def model_cols(rows, ids):
    return [[norm(r[i]) for r in rows] for i in ids]


@pytest.mark.gpu
def test_reference_statements():
    import collections
    import gzip
    text = gzip.decompress(open(GFF, "rb").read())
    exp = M.scan(text, M.GFF)
    rc, out, dump = tf("read_gff", GFF)
    assert rc == 0 and "rows=62 " in out, out                                                           # duckhts.test:410-413
    schema, sizes, cols = columns(dump)
    assert schema == GXF_SCHEMA and sizes == [62]
    assert [c[0] for c in cols[:5]] == [b"X", b"Vega", b"exon", 2934816, 2935190]                       # :416-419
    assert cols == model_cols(exp, range(9))
    assert collections.Counter(cols[2]) == {b"exon": 23, b"intron": 19, b"CDS": 15, b"transcript": 4, b"gene": 1}      # :462-469
    rc, out, dump = tf("read_gff", GFF, proj=[2])                                                       # :456-459
    assert rc == 0 and columns(dump)[2][0][0] == b"exon"
    rc, out, _ = tf("read_gff", GFF, named=[("region", "X:2934816-2935190")])                           # :472-475
    assert rc == 0 and "rows=4 " in out, out
    rc, out, dump = tf("read_gff", GFF, named=[("attributes_map", "true")])                             # :478-481
    schema, _, cols = columns(dump)
    assert rc == 0 and schema == GXF_SCHEMA + [("attributes_map", MAP)]
    assert sum(m is not None for m in cols[9]) == 62 and cols[9] == [r[9] for r in exp]
    rc, out, dump = tf("read_tabix", GFF)                                                               # :488-491
    assert rc == 0 and "rows=62 " in out, out
    schema, _, cols = columns(dump)
    assert schema == [("column%d" % i, VARCHAR) for i in range(9)]
    rc, out, dump = tf("read_tabix", GFF, proj=[0, 2])                                                  # :494-498
    assert [c[:2] for c in columns(dump)[2]] == [[b"X", b"X"], [b"exon", b"gene"]]
    counts = []
    for region in ("X:2934816-2935190", "X:2937010-2937500", "X:2934816-2935190,X:2937010-2937500"):    # :501-519
        rc, out, _ = tf("read_tabix", GFF, named=[("region", region)])
        assert rc == 0, out
        counts.append(int(out.split("rows=")[1].split()[0]))
    assert counts == [4, 3, 7]
    rc, out, _ = tf("read_tabix", GFF, named=[("region", "nosuch:1-5")])
    assert rc == 0 and "rows=0 " in out, out                                                            # an empty result, no error (tabix_reader.c:821-824)
    rc, out, dump = tf("read_gtf", GFF, named=[("attributes_map", "true")], proj=[9])
    assert rc == 0 and columns(dump)[2][0] == [r[9] for r in M.scan(text, M.GTF)]


@pytest.mark.gpu
def test_meta_and_header_fixtures():
    meta, hdr = os.path.join(GOLDEN, "meta_tabix.tsv.gz"), os.path.join(GOLDEN, "header_tabix.tsv.gz")
    rc, out, dump = tf("read_tabix", meta)                                                              # :426-429
    schema, _, cols = columns(dump)
    assert rc == 0 and schema[:2] == [("column0", VARCHAR), ("column1", VARCHAR)] and (cols[0][0], cols[1][0]) == (b"chr1", b"1")
    rc, out, dump = tf("read_tabix", hdr, named=[("header", "true")])                                   # :432-435
    schema, _, cols = columns(dump)
    assert rc == 0 and [n for n, _ in schema] == ["chrom", "pos", "value"] and (cols[0][0], cols[1][0]) == (b"chr1", b"1")
    rc, out, dump = tf("read_tabix", meta, named=[("auto_detect", "true")])                             # :444-447
    schema, _, cols = columns(dump)
    assert rc == 0 and schema[1] == ("column1", BIGINT) and cols[1][0] == 1


@pytest.mark.gpu
def test_chunks_projection_and_a_double_column(tmp_path):
    L = [b"chr%d\t%d\t%d.25\tn%d\t%s" % (i // 2000, i * 7, i, i, b"." if i % 5 == 0 else b"1e-3") for i in range(5000)]
    fn = os.path.join(str(tmp_path), "five.tsv")
    text = b"#five thousand rows\n" + b"\n".join(L) + b"\n"
    open(fn, "wb").write(text)
    b = M.bind(text, auto_detect=True)
    assert b["types"] == [VARCHAR, BIGINT, DOUBLE, VARCHAR, DOUBLE]
    exp = M.scan(text, M.GENERIC, b["types"])
    rc, out, dump = tf("read_tabix", fn, named=[("auto_detect", "true")], proj=[4, 1, 3, 2])           # projection ids out of order
    assert rc == 0 and "rows=5000 " in out, out
    schema, sizes, cols = columns(dump)
    assert schema == [("column%d" % i, t) for i, t in enumerate(b["types"])]
    assert sizes == [2048, 2048, 904]
    assert cols == model_cols(exp, [4, 1, 3, 2])
    assert cols[0][0] is None and cols[0][1] == ("d", M.dbl_bits(1e-3))


def test_errors_without_a_device(tmp_path):
    for fn in ("read_tabix", "read_gtf", "read_gff"):
        rc, out, _ = tf(fn, "")
        assert rc == 3 and out == "ERROR bind: %s requires a file path" % fn                            # tabix_reader.c:520-527
        rc, out, _ = tf(fn, "x.gz", named=[("bogus", "1")])
        assert rc == 3 and "unknown named parameter" in out
    rc, out, _ = tf("read_tabix", "/no/such/file.tsv.gz")
    assert rc == 3 and out == "ERROR bind: Cannot open file"                                            # :636-641
    for fn in ("read_gtf", "read_gff"):                                                                 # GTF / GFF open the file at init (:794-801)
        rc, out, _ = tf(fn, "/no/such/file.gff.gz")
        assert rc != 0 and out == "ERROR init: Cannot open file: /no/such/file.gff.gz", out
        rc, out, _ = tf(fn, __file__, named=[("region", "x:1-2")])
        assert rc != 0 and out == "ERROR init: Region query requested but no tabix index found for: " + __file__, out     # :806-816
        rc, out, _ = tf(fn, __file__, named=[("region", "x"), ("index_path", os.path.join(str(tmp_path), "missing.tbi"))])
        assert rc != 0 and out == "ERROR init: Region query requested but no tabix index found for: " + __file__, out


def test_registered_only_with_the_variable():
    import duckhts_amd
    env = {k: v for k, v in os.environ.items() if k not in ("DHTS_TABIX_FUNCTIONS", "DHTS_SEQ_FUNCTIONS", "DHTS_INTERVAL_FUNCTIONS")}

    def catalog(**kw):
        return subprocess.run([HOST, duckhts_amd.LIB_PATH, "--catalog", "-"], capture_output=True, text=True, env=dict(env, **kw)).stdout.splitlines()
    for fn in ("read_tabix", "read_gtf", "read_gff"):
        r = subprocess.run([HOST, duckhts_amd.LIB_PATH, fn, ""], capture_output=True, text=True, env=env)
        assert r.returncode == 3 and r.stdout.strip() == "ERROR catalog: table function %s not registered" % fn
    default = catalog()
    assert [ln.split()[1] for ln in default] == ["read_bcf", "read_bam", "bgzip", "bgunzip", "bam_index", "bcf_index", "tabix_index"]
    named = "named=region:17,index_path:17,attributes_map:1,header:1,header_names:24,auto_detect:1,column_types:24"     # create_tabix_tf, tabix_reader.c:1043-1071
    on = catalog(**ON)
    assert on[:len(default)] == default
    assert on[len(default):] == ["TF %s pushdown=1 bind=1 init=1 local_init=0 func=1 %s" % (fn, named) for fn in ("read_tabix", "read_gtf", "read_gff")]     # src/duckhts.c:67-69
    seq, itv = catalog(DHTS_SEQ_FUNCTIONS="1"), catalog(DHTS_INTERVAL_FUNCTIONS="1")
    assert [ln.split()[1] for ln in seq][len(default):] == ["read_fasta", "read_fastq", "fasta_index"]
    assert [ln.split()[1] for ln in itv][len(default):] == ["read_bed"]
    every = catalog(DHTS_SEQ_FUNCTIONS="1", DHTS_INTERVAL_FUNCTIONS="1", **ON)
    assert [ln.split()[1] for ln in every][len(default):] == ["read_fasta", "read_fastq", "fasta_index", "read_bed", "read_tabix", "read_gtf", "read_gff"]
