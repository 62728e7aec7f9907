"""bam_coverage through the DuckDB surface (tests/minihost, DHTS_DEPTH_FUNCTIONS=1): the nine columns and their types, the defaults against
the CPU model, named parameters, projection pushdown, a region, every error string at bind, and the registration."""
import os
import shutil
import struct
import subprocess

import pytest

import bam_coverage_cases as K
import bam_coverage_ref as M
from conftest import GOLDEN, read_golden
from test_duckdb_fasta_nuc import columns
from test_duckdb_surface import HOST, run_host

ON = {"DHTS_DEPTH_FUNCTIONS": "1"}
BIGINT, DOUBLE, VARCHAR = 5, 11, 17
SCHEMA = list(zip(M.COLUMNS, [VARCHAR, BIGINT, BIGINT, BIGINT, BIGINT, DOUBLE, DOUBLE, DOUBLE, DOUBLE]))


def coverage(path, named=(), proj=None):
    return run_host(path, named=list(named), proj=proj, fn="bam_coverage", env=ON)


def as_dumped(exp, names=M.COLUMNS):
    """the model's columns the way `columns` shows them: a DOUBLE as its 64 bits"""
    def bits(x):
        return struct.unpack("<q", struct.pack("<d", x))[0]
    return [[bits(v) for v in exp[k]] if k in M.COLUMNS[5:] else exp[k] for k in names]


def model(data, **kw):
    kw.setdefault("exclude_flags", M.DEFAULT_EXCLUDE)                     # the table function's default
    refs, reads = M.reads_from_bam(data)
    return M.coverage(reads, refs, **kw)


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
def test_schema_and_values(rng):
    fn, data = rng
    rc, out, dump = coverage(fn)
    assert rc == 0 and "max_threads=1" in out, out
    schema, sizes, cols = columns(dump)
    assert schema == SCHEMA
    exp = model(data)
    assert cols == as_dumped(exp) and f"rows={exp['n_rows']} " in out and sum(exp["numreads"]) > 0
    for named, kw in (([("min_mapq", "1"), ("exclude_flags", "16")], dict(min_mapq=1, exclude_flags=16)),
                      ([("min_baseq", "30"), ("min_depth", "2")], dict(min_baseq=30, min_depth=2)),
                      ([("min_read_len", "100"), ("require_flags", "64"), ("include_flags", "48")], dict(min_read_len=100, require_flags=64, include_flags=48))):
        rc, out, dump = coverage(fn, named=named)
        assert rc == 0, out
        assert columns(dump)[2] == as_dumped(model(data, **kw))
    rc, out, dump = coverage(fn, proj=[7, 0, 4])
    assert rc == 0 and columns(dump)[2] == as_dumped(exp, ["meanbaseq", "chrom", "covbases"])


@pytest.mark.gpu
def test_the_hand_written_table(tmp_path):
    fn = write(tmp_path, "hand.bam", K.bam(K.HAND_REFS, K.HAND_READS))
    rc, out, dump = coverage(fn, named=[("min_mapq", "10"), ("min_baseq", "20"), ("min_read_len", "4"), ("min_depth", "2")])
    assert rc == 0, out
    exp = {k: [row[i] for row in K.HAND_EXPECTED] for i, k in enumerate(M.COLUMNS)}
    assert columns(dump)[2] == as_dumped(exp)


@pytest.mark.gpu
def test_region(rng):
    import duckhts_amd
    fn, data = rng
    region = "CHROMOSOME_I:1001-1100,CHROMOSOME_I:901-1000"
    rows = duckhts_amd.read_bam(data, region=region, index=read_golden("range.bam.bai"))
    refs, _ = M.reads_from_bam(data)
    exp = M.coverage(M.reads_from_cols(rows), refs, rows=[(0, 1000, 1100), (0, 900, 1000)], exclude_flags=M.DEFAULT_EXCLUDE)
    rc, out, dump = coverage(fn, named=[("region", region)])
    assert rc == 0 and "rows=2 " in out, out
    assert columns(dump)[2] == as_dumped(exp)
    rc, out, _ = coverage(fn, named=[("region", "CHROMOSOME_I:1-1000,CHROMOSOME_I:900-1100")])
    assert rc != 0 and M.err_overlap("CHROMOSOME_I:1-1000", "CHROMOSOME_I:900-1100") in out, out


def test_bind_errors_without_a_device():
    rc, out, _ = coverage("")
    assert rc == 3 and out == "ERROR bind: " + M.ERR_PATH
    rc, out, _ = coverage("/no/such/file.bam")
    assert rc == 3 and out == "ERROR bind: Failed to open SAM/BAM/CRAM file: /no/such/file.bam"     # read_bam's own (bam_reader.c:446)
    rc, out, _ = coverage("x.bam", named=[("bogus", "1")])
    assert rc == 3 and "unknown named parameter" in out
    for k in ("region", "index_path", "min_read_len", "min_mapq", "min_baseq", "include_flags", "require_flags", "exclude_flags", "min_depth"):
        rc, out, _ = coverage("/no/such/file.bam", named=[(k, "1")])
        assert "unknown named parameter" not in out
    # the parameters are checked in front of the file
    for named, msg in (([("min_mapq", "256")], M.err_range("min_mapq")), ([("min_mapq", "-1")], M.err_range("min_mapq")), ([("min_baseq", "256")], M.err_range("min_baseq")),
                       ([("include_flags", "65536")], M.err_range("include_flags")), ([("require_flags", "-1")], M.err_range("require_flags")),
                       ([("exclude_flags", "65536")], M.err_range("exclude_flags")), ([("min_read_len", "-1")], M.ERR_READ_LEN), ([("min_depth", "0")], M.ERR_DEPTH),
                       # wrong in two ways: the first in the order of the checks is reported
                       ([("min_read_len", "-1"), ("min_mapq", "256")], M.ERR_READ_LEN), ([("min_baseq", "-1"), ("include_flags", "65536")], M.err_range("min_baseq")),
                       ([("require_flags", "-1"), ("exclude_flags", "70000")], M.err_range("require_flags")), ([("min_depth", "0"), ("exclude_flags", "70000")], M.err_range("exclude_flags"))):
        rc, out, _ = coverage("/no/such/file.bam", named=named)
        assert rc == 3 and out == "ERROR bind: " + msg, out


@pytest.mark.gpu
def test_region_and_index_errors_are_read_bams_own(rng, tmp_path):
    fn, data = rng
    rc, out, _ = coverage(write(tmp_path, "bad.bam", b"not a bam file at all"))
    assert rc == 3 and out == "ERROR bind: Failed to read SAM/BAM/CRAM header"
    rc, out, _ = coverage(fn, named=[("region", "nosuch:1-5")])
    assert rc == 3 and out == "ERROR bind: No reads found for region(s): nosuch:1-5"
    noidx = os.path.join(str(tmp_path), "noindex.bam")
    shutil.copy(fn, noidx)
    rc, out, _ = coverage(noidx, named=[("region", "CHROMOSOME_I:1-1000")])
    assert rc == 3 and out == "ERROR bind: Region query requires an index (.bai/.csi/.crai)"
    rc, out, _ = coverage(noidx, named=[("region", "CHROMOSOME_I:1-1000"), ("index_path", fn + ".bai")])
    assert rc == 0 and "rows=1 " in out, out


def test_registered_last_under_a_variable_of_its_own():
    import duckhts_amd

    def catalog(**kv):
        env = {k: x for k, x in os.environ.items() if not (k.startswith("DHTS_") and k.endswith("_FUNCTIONS"))}
        env.update(kv)
        return subprocess.run([HOST, duckhts_amd.LIB_PATH, "--catalog", "-"], capture_output=True, text=True, env=env).stdout.splitlines()

    default = catalog()
    assert default and not any("bam_coverage" in ln for ln in default)
    # absent under every existing variable, whose sets are what they were
    sets = {v: catalog(DHTS_COVERAGE_FUNCTIONS=v) for v in ("1", "2", "3")}
    assert sets["3"] == default and sets["2"][:len(sets["1"])] == sets["1"] and sets["1"][-1].startswith("TF bam_bin_counts ") and sets["2"][-1].startswith("TF bam_bedcov ")
    for lines in list(sets.values()) + [catalog(DHTS_KMER_FUNCTIONS="1"), catalog(DHTS_TABIX_FUNCTIONS="1"), catalog(DHTS_DEPTH_FUNCTIONS="2"), catalog(DHTS_DEPTH_FUNCTIONS="0")]:
        assert not any("bam_coverage" in ln for ln in lines)
    line = ("TF bam_coverage pushdown=1 bind=1 init=1 local_init=0 func=1 named=region:17,index_path:17,min_read_len:5,min_mapq:5,min_baseq:5,include_flags:5,require_flags:5,"
            "exclude_flags:5,min_depth:5")
    assert catalog(DHTS_DEPTH_FUNCTIONS="1") == default + [line]
    both = catalog(DHTS_DEPTH_FUNCTIONS="1", DHTS_COVERAGE_FUNCTIONS="2", DHTS_TABIX_FUNCTIONS="1", DHTS_KMER_FUNCTIONS="1")
    assert both[-1] == line and both[:-1] == catalog(DHTS_COVERAGE_FUNCTIONS="2", DHTS_TABIX_FUNCTIONS="1", DHTS_KMER_FUNCTIONS="1")
