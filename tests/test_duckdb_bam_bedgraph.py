"""bam_bedgraph through the DuckDB surface (tests/minihost, DHTS_BEDGRAPH_FUNCTIONS=1): the four columns and their types, the defaults and every
named parameter against the CPU model, a BED, a region with an index, projection pushdown, pages of 1 and 7 rows, the refusals in the order bind
checks them, and the registration."""
import os
import shutil
import subprocess

import pytest

import bam_bedgraph_cases as G
import bam_bedgraph_ref as M
import bam_depth_cases as D
from conftest import GOLDEN, read_golden
from test_duckdb_fasta_nuc import columns
from test_duckdb_surface import HOST, run_host

ON = {"DHTS_BEDGRAPH_FUNCTIONS": "1"}
BIGINT, VARCHAR = 5, 17
SCHEMA = [("chrom", VARCHAR), ("start", BIGINT), ("end", BIGINT), ("depth", BIGINT)]
NAMED = ["zero_runs", "breaks", "bed_path", "region", "index_path", "min_read_len", "min_mapq", "min_baseq", "include_deletions", "include_flags", "require_flags", "exclude_flags"]
BOOLEANS = ("zero_runs", "include_deletions")


def bedgraph(path, named=(), proj=None, env=None):
    return run_host(path, named=list(named), proj=proj, fn="bam_bedgraph", env=dict(ON, **(env or {})))


def as_dumped(exp, refs, names=("chrom", "start", "end", "depth")):
    cols = {"chrom": [refs[t][0] for t in exp["tid"]], "start": exp["start"].tolist(), "end": exp["end"].tolist(), "depth": exp["depth"].tolist()}
    return [cols[k] for k in names]


def model(data, rows=None, **kw):
    kw.setdefault("exclude_flags", M.DEFAULT_EXCLUDE)                     # the table function's default
    refs, reads = M.reads_from_bam(data)
    return M.bedgraph(reads, refs, rows=rows, **kw), refs


def write(tmp_path, name, data):
    fn = os.path.join(str(tmp_path), name)
    open(fn, "wb").write(data)
    return fn


@pytest.fixture()
def rng(tmp_path):
    fn = os.path.join(str(tmp_path), "range.bam")
    shutil.copy(os.path.join(GOLDEN, "range.bam"), fn)
    shutil.copy(os.path.join(GOLDEN, "range.bam.bai"), fn + ".bai")
    return fn, read_golden("range.bam")


@pytest.mark.gpu
def test_schema_defaults_and_every_named_parameter(rng):
    fn, data = rng
    rc, out, dump = bedgraph(fn)
    assert rc == 0 and "max_threads=1" in out, out
    schema, sizes, cols = columns(dump)
    assert schema == SCHEMA
    exp, refs = model(data)
    assert cols == as_dumped(exp, refs) and f"rows={exp['n_rows']} " in out and exp["n_rows"] > 0
    assert all(v is not None for c in cols for v in c)                                        # no column is ever NULL
    for named, kw in (([("zero_runs", "true")], dict(zero_runs=1)),
                      ([("zero_runs", "false"), ("breaks", "2,4")], dict(breaks="2,4")),
                      ([("zero_runs", "true"), ("breaks", "1,5,150")], dict(zero_runs=1, breaks="1,5,150")),
                      ([("min_mapq", "1"), ("exclude_flags", "16")], dict(min_mapq=1, exclude_flags=16)),
                      ([("min_baseq", "30"), ("zero_runs", "true")], dict(min_baseq=30, zero_runs=1)),
                      ([("include_deletions", "true"), ("min_baseq", "25")], dict(include_deletions=1, min_baseq=25)),
                      ([("min_read_len", "100"), ("require_flags", "64"), ("include_flags", "48")], dict(min_read_len=100, require_flags=64, include_flags=48))):
        rc, out, dump = bedgraph(fn, named=named)
        assert rc == 0, out
        assert columns(dump)[2] == as_dumped(*model(data, **kw)), named


@pytest.mark.gpu
def test_projection_and_pages(tmp_path):
    data = G.bam(*G.many_runs())
    fn = write(tmp_path, "many.bam", data)
    exp, refs = model(data, zero_runs=1)
    assert exp["n_rows"] > 2048
    rc, out, dump = bedgraph(fn, named=[("zero_runs", "true")])
    schema, sizes, cols = columns(dump)
    assert rc == 0 and cols == as_dumped(exp, refs) and sizes[:-1] == [2048] * (len(sizes) - 1) and len(sizes) > 1          # longer than one chunk
    for proj, names in (([3], ["depth"]), ([2, 0], ["end", "chrom"]), ([1], ["start"])):
        rc, out, dump = bedgraph(fn, named=[("zero_runs", "true")], proj=proj)
        assert rc == 0 and columns(dump)[2] == as_dumped(exp, refs, names)
    # pages of 1 and of 7 rows: the chunks stay full and the rows the same
    small, _ = model(data, breaks="2,4")
    for page in ("1", "7"):
        rc, out, dump = bedgraph(fn, named=[("breaks", "2,4")], env={"DHTS_BEDGRAPH_PAGE_ROWS": page})
        assert rc == 0 and columns(dump)[2] == as_dumped(small, refs) and small["n_rows"] > 200
    rc, out, dump = bedgraph(fn, named=[("zero_runs", "true")], env={"DHTS_BEDGRAPH_PAGE_ROWS": "7"})
    schema, sizes, cols = columns(dump)
    assert rc == 0 and cols == as_dumped(exp, refs) and sizes[:-1] == [2048] * (len(sizes) - 1)


@pytest.mark.gpu
def test_bed_path_and_region(rng, tmp_path):
    import duckhts_amd
    data = G.bam(G.TOUCH_REFS, G.TOUCH_READS)
    fn, bed = write(tmp_path, "t.bam", data), write(tmp_path, "t.bed", D.bed_text(G.TOUCH_BED))
    refs, _ = M.reads_from_bam(data)
    rows, _ = M.merge_bed(G.TOUCH_BED, refs)
    for named, kw in (([], dict()), ([("zero_runs", "true"), ("breaks", "2")], dict(zero_runs=1, breaks="2"))):
        rc, out, dump = bedgraph(fn, named=[("bed_path", bed)] + named)
        assert rc == 0, out
        assert columns(dump)[2] == as_dumped(*model(data, rows=rows, **kw))
    fn, data = rng
    region = "CHROMOSOME_I:1001-1100,CHROMOSOME_I:901-1000"
    scanned = duckhts_amd.read_bam(data, region=region, index=read_golden("range.bam.bai"))
    refs, _ = M.reads_from_bam(data)
    for named, kw in (([], dict()), ([("zero_runs", "true")], dict(zero_runs=1))):
        exp = M.bedgraph(M.reads_from_cols(scanned), refs, rows=[(0, 1000, 1100), (0, 900, 1000)], exclude_flags=M.DEFAULT_EXCLUDE, **kw)
        rc, out, dump = bedgraph(fn, named=[("region", region)] + named)
        assert rc == 0 and f"rows={exp['n_rows']} " in out, out
        assert columns(dump)[2] == as_dumped(exp, refs)
    rc, out, _ = bedgraph(fn, named=[("region", "CHROMOSOME_I:1-1000,CHROMOSOME_I:900-1100")])
    assert rc != 0 and M.err_overlap("CHROMOSOME_I:1-1000", "CHROMOSOME_I:900-1100") in out, out


def test_refusals_in_the_order_bind_checks_them():
    rc, out, _ = bedgraph("")
    assert rc == 3 and out == "ERROR bind: bam_bedgraph requires a file path"
    rc, out, _ = bedgraph("/no/such/file.bam")
    assert rc == 3 and out == "ERROR bind: Failed to open SAM/BAM/CRAM file: /no/such/file.bam"     # read_bam's own (bam_reader.c:446)
    rc, out, _ = bedgraph("x.bam", named=[("bogus", "1")])
    assert rc == 3 and "unknown named parameter" in out
    for k in NAMED:
        rc, out, _ = bedgraph("/no/such/file.bam", named=[(k, "false" if k in BOOLEANS else "1")])
        assert "unknown named parameter" not in out
    many = ",".join(str(i) for i in range(1, 18))
    # the parameters are checked in front of the file: the filter, the breaks, then a BED beside a region
    for named, msg in (([("min_mapq", "256")], M.err_range("min_mapq")), ([("min_mapq", "-1")], M.err_range("min_mapq")), ([("min_baseq", "256")], M.err_range("min_baseq")),
                       ([("min_baseq", "-1")], M.err_range("min_baseq")), ([("include_flags", "65536")], M.err_range("include_flags")), ([("require_flags", "-1")], M.err_range("require_flags")),
                       ([("exclude_flags", "65536")], M.err_range("exclude_flags")), ([("min_read_len", "-1")], M.ERR_READ_LEN),
                       ([("breaks", many)], M.ERR_MANY_BREAKS), ([("breaks", "0,5")], M.ERR_BREAKS), ([("breaks", "3,3")], M.ERR_BREAKS), ([("breaks", "5,2")], M.ERR_BREAKS),
                       ([("breaks", "2,,4")], M.ERR_BREAKS), ([("breaks", "2,4,")], M.ERR_BREAKS), ([("breaks", "a")], M.ERR_BREAKS), ([("breaks", "-4")], M.ERR_BREAKS),
                       ([("breaks", "1, 5")], M.ERR_BREAKS), ([("breaks", "1,2147483648")], M.ERR_BREAKS), ([("breaks", "1,99999999999")], M.ERR_BREAKS),
                       ([("bed_path", "/no/such.bed"), ("region", "c1:1-5")], M.ERR_BED_AND_REGION),
                       # wrong in two ways: the first in the order of the checks is reported
                       ([("min_read_len", "-1"), ("min_mapq", "256")], M.ERR_READ_LEN), ([("breaks", "0"), ("exclude_flags", "70000")], M.err_range("exclude_flags")),
                       ([("breaks", many + ",x")], M.ERR_MANY_BREAKS), ([("breaks", "4,2"), ("bed_path", "/no/such.bed"), ("region", "c1:1-5")], M.ERR_BREAKS)):
        rc, out, _ = bedgraph("/no/such/file.bam", named=named)
        assert rc == 3 and out == "ERROR bind: " + msg, (named, out)
    rc, out, _ = bedgraph("/no/such/file.bam", named=[("breaks", "1,2147483647")])             # the largest break is taken: the file is what fails
    assert rc == 3 and out == "ERROR bind: Failed to open SAM/BAM/CRAM file: /no/such/file.bam"


@pytest.mark.gpu
def test_file_region_and_bed_errors_are_the_readers_own(rng, tmp_path):
    fn, data = rng
    rc, out, _ = bedgraph(write(tmp_path, "bad.bam", b"not a bam file at all"))
    assert rc == 3 and out == "ERROR bind: Failed to read SAM/BAM/CRAM header"
    rc, out, _ = bedgraph(fn, named=[("region", "nosuch:1-5")])
    assert rc == 3 and out == "ERROR bind: No reads found for region(s): nosuch:1-5"
    noidx = os.path.join(str(tmp_path), "noindex.bam")
    shutil.copy(fn, noidx)
    rc, out, _ = bedgraph(noidx, named=[("region", "CHROMOSOME_I:1-1000")])
    assert rc == 3 and out == "ERROR bind: Region query requires an index (.bai/.csi/.crai)"
    rc, out, _ = bedgraph(fn, named=[("bed_path", "/no/such.bed")])
    assert rc == 3 and out == "ERROR bind: read_bed: failed to open file: /no/such.bed"           # as bam_bedcov binds


def test_registered_last_under_a_variable_of_its_own():
    import duckhts_amd

    def catalog(**kv):
        env = {k: x for k, x in os.environ.items() if not (k.startswith("DHTS_") and k.endswith("_FUNCTIONS"))}
        env.update(kv)
        return subprocess.run([HOST, duckhts_amd.LIB_PATH, "--catalog", "-"], capture_output=True, text=True, env=env).stdout.splitlines()

    default = catalog()
    assert default and not any("bam_bedgraph" in ln for ln in default)
    # absent under every value of every existing variable, whose sets are what they were
    existing = ("DHTS_SEQ_FUNCTIONS", "DHTS_INTERVAL_FUNCTIONS", "DHTS_NUC_FUNCTIONS", "DHTS_KMER_FUNCTIONS", "DHTS_TABIX_FUNCTIONS", "DHTS_COVERAGE_FUNCTIONS", "DHTS_DEPTH_FUNCTIONS",
                "DHTS_PERBASE_FUNCTIONS", "DHTS_PILEUP_FUNCTIONS")
    for var in existing:
        for v in ("0", "1", "2", "3"):
            assert not any("bam_bedgraph" in ln for ln in catalog(**{var: v})), (var, v)
    assert catalog(DHTS_PILEUP_FUNCTIONS="1")[:-1] == default and catalog(DHTS_PILEUP_FUNCTIONS="1")[-1].startswith("TF bam_pileup ")
    for v in ("0", "2", "true"):
        assert catalog(DHTS_BEDGRAPH_FUNCTIONS=v) == default
    line = ("TF bam_bedgraph pushdown=1 bind=1 init=1 local_init=0 func=1 named=zero_runs:1,breaks:17,bed_path:17,region:17,index_path:17,min_read_len:5,min_mapq:5,"
            "min_baseq:5,include_deletions:1,include_flags:5,require_flags:5,exclude_flags:5")
    assert catalog(DHTS_BEDGRAPH_FUNCTIONS="1") == default + [line]
    others = dict(DHTS_PILEUP_FUNCTIONS="1", DHTS_PERBASE_FUNCTIONS="1", DHTS_DEPTH_FUNCTIONS="1", DHTS_COVERAGE_FUNCTIONS="2", DHTS_TABIX_FUNCTIONS="1", DHTS_KMER_FUNCTIONS="1")
    both = catalog(DHTS_BEDGRAPH_FUNCTIONS="1", **others)
    assert both[-1] == line and both[:-1] == catalog(**others) and both[-2].startswith("TF bam_pileup ")
