"""bam_bedgraph_export through the DuckDB surface (tests/minihost, DHTS_EXPORT_FUNCTIONS=1): the six columns and their types, the single row,
index_path NULL for 'none', every named parameter reaching the count (the file's text against the CPU model), the refusals in the order bind
checks them, and the registration behind a variable of its own."""
import gzip
import os
import shutil
import subprocess

import pytest

import bam_bedgraph_export_ref as X
import bam_bedgraph_ref as M
from conftest import GOLDEN, read_golden
from test_duckdb_fasta_nuc import columns
from test_duckdb_surface import HOST, run_host

ON = {"DHTS_EXPORT_FUNCTIONS": "1"}
BOOLEAN, BIGINT, VARCHAR = 1, 5, 17
SCHEMA = [("success", BOOLEAN), ("output_path", VARCHAR), ("index_path", VARCHAR), ("n_rows", BIGINT), ("bytes_text", BIGINT), ("bytes_out", BIGINT)]
OWN = ["out_path", "index", "level", "overwrite"]
NAMED = OWN + ["zero_runs", "breaks", "bed_path", "region", "index_path", "min_read_len", "min_mapq", "min_baseq", "include_deletions", "include_flags", "require_flags", "exclude_flags"]
BOOLEANS = ("overwrite", "zero_runs", "include_deletions")


def export(path, named=(), env=None):
    return run_host(path, named=list(named), fn="bam_bedgraph_export", env=dict(ON, **(env or {})))


@pytest.fixture()
def rng(tmp_path):
    fn = os.path.join(str(tmp_path), "range.bam")
    shutil.copy(os.path.join(GOLDEN, "range.bam"), fn)
    shutil.copy(os.path.join(GOLDEN, "range.bam.bai"), fn + ".bai")
    return fn, read_golden("range.bam"), str(tmp_path)


def model_text(data, **kw):
    kw.setdefault("exclude_flags", M.DEFAULT_EXCLUDE)                     # the table function's default
    refs, reads = M.reads_from_bam(data)
    return X.export(reads, refs, **kw)


@pytest.mark.gpu
def test_schema_the_single_row_and_the_named_parameters(rng):
    fn, data, d = rng
    out = os.path.join(d, "o.bed.gz")
    rc, msg, dump = export(fn, named=[("out_path", out)])
    assert rc == 0 and "rows=1 " in msg, msg
    schema, sizes, cols = columns(dump)
    text, res = model_text(data)
    z = open(out, "rb").read()
    assert schema == SCHEMA and sizes == [1]
    assert [c[0] for c in cols] == [1, out.encode(), (out + ".tbi").encode(), res["n_rows"], len(text), len(z)] and res["n_rows"] > 0
    assert gzip.decompress(z) == text and os.path.getsize(out + ".tbi") > 28
    # an existing output is refused until overwrite is set
    rc, msg, _ = export(fn, named=[("out_path", out)])
    assert rc != 0 and X.err_exists(out) in msg and open(out, "rb").read() == z
    # index := 'none': index_path is NULL and no index is written; 'csi' names the other file
    none = os.path.join(d, "n.bed.gz")
    rc, msg, dump = export(fn, named=[("out_path", none), ("index", "none"), ("level", "0")])
    cols = columns(dump)[2]
    assert rc == 0 and cols[2] == [None] and cols[1] == [none.encode()] and sorted(os.listdir(d)) == ["n.bed.gz", "o.bed.gz", "o.bed.gz.tbi", "range.bam", "range.bam.bai"]
    assert gzip.decompress(open(none, "rb").read()) == text and cols[5] == [os.path.getsize(none)] and cols[5][0] > len(text)      # level 0 stores
    # every named parameter of bam_bedgraph reaches the count: two sets
    for named, kw, kind in (([("zero_runs", "true"), ("breaks", "1,5,150"), ("min_baseq", "25"), ("include_deletions", "true"), ("index", "csi")],
                             dict(zero_runs=1, breaks="1,5,150", min_baseq=25, include_deletions=1), "csi"),
                            ([("min_read_len", "100"), ("require_flags", "64"), ("include_flags", "48"), ("min_mapq", "1"), ("exclude_flags", "16"), ("overwrite", "true")],
                             dict(min_read_len=100, require_flags=64, include_flags=48, min_mapq=1, exclude_flags=16), "tbi")):
        rc, msg, dump = export(fn, named=[("out_path", out), ("overwrite", "true")] + [kv for kv in named if kv[0] != "overwrite"])
        assert rc == 0, msg
        text, res = model_text(data, **kw)
        cols = columns(dump)[2]
        assert gzip.decompress(open(out, "rb").read()) == text and cols[3] == [res["n_rows"]] and cols[4] == [len(text)] and cols[2] == [(out + "." + kind).encode()]
        assert os.path.exists(out + "." + kind)
    # a region through the BAM's index, in file order
    region = "CHROMOSOME_I:901-1000,CHROMOSOME_I:1001-1100"
    import duckhts_amd
    scanned = duckhts_amd.read_bam(data, region=region, index=read_golden("range.bam.bai"))
    refs, _ = M.reads_from_bam(data)
    text, res = X.export(M.reads_from_cols(scanned), refs, rows=[(0, 900, 1000), (0, 1000, 1100)], exclude_flags=M.DEFAULT_EXCLUDE, zero_runs=1)
    rc, msg, dump = export(fn, named=[("out_path", out), ("overwrite", "true"), ("region", region), ("zero_runs", "true")])
    assert rc == 0 and gzip.decompress(open(out, "rb").read()) == text and columns(dump)[2][3] == [res["n_rows"]], msg
    rc, msg, _ = export(fn, named=[("out_path", os.path.join(d, "r.bed.gz")), ("region", "CHROMOSOME_I:1001-1100,CHROMOSOME_I:901-1000")])
    assert rc != 0 and X.ERR_ORDER in msg and not os.path.exists(os.path.join(d, "r.bed.gz"))


def test_refusals_in_the_order_bind_checks_them():
    o = ("out_path", "/tmp/never-written.bed.gz")
    rc, out, _ = export("")                                                   # out_path is asked for first
    assert rc == 3 and out == "ERROR bind: " + X.ERR_NO_OUT_PATH
    rc, out, _ = export("/no/such/file.bam", named=[("out_path", "")])
    assert rc == 3 and out == "ERROR bind: " + X.ERR_NO_OUT_PATH
    rc, out, _ = export("/no/such/file.bam", named=[("min_mapq", "256")])
    assert rc == 3 and out == "ERROR bind: " + X.ERR_NO_OUT_PATH
    rc, out, _ = export("", named=[o])
    assert rc == 3 and out == "ERROR bind: " + X.ERR_NO_PATH
    rc, out, _ = export("/no/such/file.bam", named=[o])
    assert rc == 3 and out == "ERROR bind: Failed to open SAM/BAM/CRAM file: /no/such/file.bam"     # read_bam's own (bam_reader.c:446)
    rc, out, _ = export("x.bam", named=[o, ("bogus", "1")])
    assert rc == 3 and "unknown named parameter" in out
    for k in NAMED[1:]:
        rc, out, _ = export("/no/such/file.bam", named=[o, (k, "false" if k in BOOLEANS else "1")])
        assert "unknown named parameter" not in out
    many = ",".join(str(i) for i in range(1, 18))
    E = X.as_export
    # bam_bedgraph's checks in bam_bedgraph's order with this function's prefix, then the kind of the index, all in front of the file
    for named, msg in (([("min_mapq", "256")], E(M.err_range("min_mapq"))), ([("min_baseq", "-1")], E(M.err_range("min_baseq"))), ([("include_flags", "65536")], E(M.err_range("include_flags"))),
                       ([("require_flags", "-1")], E(M.err_range("require_flags"))), ([("exclude_flags", "65536")], E(M.err_range("exclude_flags"))), ([("min_read_len", "-1")], E(M.ERR_READ_LEN)),
                       ([("breaks", many)], E(M.ERR_MANY_BREAKS)), ([("breaks", "0,5")], E(M.ERR_BREAKS)), ([("breaks", "5,2")], E(M.ERR_BREAKS)), ([("breaks", "2,,4")], E(M.ERR_BREAKS)),
                       ([("breaks", "1,2147483648")], E(M.ERR_BREAKS)), ([("bed_path", "/no/such.bed"), ("region", "c1:1-5")], E(M.ERR_BED_AND_REGION)),
                       ([("index", "bai")], X.ERR_INDEX_KIND), ([("index", "")], X.ERR_INDEX_KIND),
                       # wrong in two ways: the first in the order of the checks is reported
                       ([("min_read_len", "-1"), ("min_mapq", "256")], E(M.ERR_READ_LEN)), ([("breaks", "0"), ("exclude_flags", "70000")], E(M.err_range("exclude_flags"))),
                       ([("breaks", "4,2"), ("bed_path", "/no/such.bed"), ("region", "c1:1-5")], E(M.ERR_BREAKS)), ([("index", "bai"), ("breaks", "0")], E(M.ERR_BREAKS)),
                       ([("index", "bai"), ("bed_path", "/no/such.bed"), ("region", "c1:1-5")], E(M.ERR_BED_AND_REGION))):
        rc, out, _ = export("/no/such/file.bam", named=[o] + named)
        assert rc == 3 and out == "ERROR bind: " + msg, (named, out)
    assert not os.path.exists(o[1])


def test_absent_without_its_variable_and_registered_last():
    import duckhts_amd

    def catalog(**kv):
        env = {k: x for k, x in os.environ.items() if not (k.startswith("DHTS_") and k.endswith("_FUNCTIONS"))}
        env.update(kv)
        return subprocess.run([HOST, duckhts_amd.LIB_PATH, "--catalog", "-"], capture_output=True, text=True, env=env).stdout.splitlines()

    default = catalog()
    assert default and not any("bam_bedgraph_export" in ln for ln in default)
    existing = ("DHTS_SEQ_FUNCTIONS", "DHTS_INTERVAL_FUNCTIONS", "DHTS_NUC_FUNCTIONS", "DHTS_KMER_FUNCTIONS", "DHTS_TABIX_FUNCTIONS", "DHTS_COVERAGE_FUNCTIONS", "DHTS_DEPTH_FUNCTIONS",
                "DHTS_PERBASE_FUNCTIONS", "DHTS_PILEUP_FUNCTIONS", "DHTS_BEDGRAPH_FUNCTIONS", "DHTS_HIST_FUNCTIONS")
    for var in existing:
        for v in ("0", "1", "2", "3"):
            assert not any("bam_bedgraph_export" in ln for ln in catalog(**{var: v})), (var, v)
    for v in ("0", "2", "true"):
        assert catalog(DHTS_EXPORT_FUNCTIONS=v) == default
    line = ("TF bam_bedgraph_export pushdown=0 bind=1 init=1 local_init=0 func=1 named=out_path:17,index:17,level:5,overwrite:1,zero_runs:1,breaks:17,bed_path:17,region:17,"
            "index_path:17,min_read_len:5,min_mapq:5,min_baseq:5,include_deletions:1,include_flags:5,require_flags:5,exclude_flags:5")
    assert catalog(DHTS_EXPORT_FUNCTIONS="1") == default + [line]
    others = dict(DHTS_HIST_FUNCTIONS="1", DHTS_BEDGRAPH_FUNCTIONS="1", DHTS_PILEUP_FUNCTIONS="1", DHTS_COVERAGE_FUNCTIONS="2", DHTS_TABIX_FUNCTIONS="1")
    both = catalog(DHTS_EXPORT_FUNCTIONS="1", **others)
    assert both[-1] == line and both[:-1] == catalog(**others) and both[-2].startswith("TF bam_depth_hist ")
    # the function cannot be called without the variable
    rc, out, _ = run_host("/no/such/file.bam", named=[("out_path", "/tmp/never-written.bed.gz")], fn="bam_bedgraph_export", env={"DHTS_EXPORT_FUNCTIONS": "0"})
    assert rc != 0 and "never-written" not in out
