"""bam_bin_counts through the DuckDB surface (tests/minihost, DHTS_COVERAGE_FUNCTIONS=1): the schema, the values against the CPU model, the
2048-row chunks, projection pushdown, every error string at bind, read_bam's own errors, and the opt-in registration."""
import os
import shutil
import subprocess

import pytest

import bam_bins_cases as K
import bam_bins_ref as M
import orc
from conftest import GOLDEN, read_golden
from duckhts_amd import synth
from test_duckdb_fasta_nuc import columns
from test_duckdb_surface import HOST, run_host

ON = {"DHTS_COVERAGE_FUNCTIONS": "1"}
BIGINT, VARCHAR = 5, 17
SCHEMA = list(zip(M.COLUMNS, [VARCHAR] + [BIGINT] * 6))


def bins(path, named=(), proj=None):
    return run_host(path, named=named, proj=proj, fn="bam_bin_counts", env=ON)


def model_cols(data, names=M.COLUMNS, **kw):
    c = orc.bam_read(data)
    exp = M.bin_counts(c, c["ref_names"], c["ref_len"], **kw)
    return exp, [exp[k] for k in names]


@pytest.fixture()
def rng(tmp_path):
    fn = os.path.join(str(tmp_path), "range.bam")
    shutil.copy(os.path.join(GOLDEN, "range.bam"), fn)
    shutil.copy(os.path.join(GOLDEN, "range.bam.bai"), fn + ".bai")
    return fn, read_golden("range.bam")


@pytest.mark.gpu
def test_schema_and_values(rng):
    fn, data = rng
    rc, out, dump = bins(fn)
    assert rc == 0 and "max_threads=1" in out, out
    schema, sizes, cols = columns(dump)
    assert schema == SCHEMA
    exp, want = model_cols(data, bin_width=5000)                                              # the default bin_width
    assert cols == want and f"rows={exp['n_rows']} " in out
    for named, kw in (([("bin_width", "1000")], dict(bin_width=1000)),
                      ([("bin_width", "100"), ("min_mapq", "1"), ("require_flags", "2"), ("exclude_flags", "1024"), ("include_flags", "192"), ("dedup", "adjacent")],
                       dict(bin_width=100, min_mapq=1, require_flags=2, exclude_flags=1024, include_flags=192, dedup="adjacent")),
                      ([("bin_width", "250000"), ("emit_zero_bins", "true")], dict(bin_width=250000, emit_zero_bins=True))):
        rc, out, dump = bins(fn, named=named)
        assert rc == 0, out
        exp, want = model_cols(data, **kw)
        assert columns(dump)[2] == want and f"rows={exp['n_rows']} " in out
    assert model_cols(data, bin_width=1000)[0]["n_rows"] == 10


@pytest.mark.gpu
def test_region(rng):
    import duckhts_amd
    fn, data = rng
    region = "CHROMOSOME_I:1-1000"
    rows = duckhts_amd.read_bam(data, region=region, index=read_golden("range.bam.bai"))
    hdr = rows["header"]
    for zero in (False, True):
        exp = M.bin_counts(rows, hdr["ref_names"], hdr["ref_len"], bin_width=100, emit_zero_bins=zero, named_tids={0})
        rc, out, dump = bins(fn, named=[("bin_width", "100"), ("region", region)] + ([("emit_zero_bins", "true")] if zero else []))
        assert rc == 0 and f"rows={exp['n_rows']} " in out, out
        assert columns(dump)[2] == [exp[k] for k in M.COLUMNS]


@pytest.mark.gpu
def test_chunks_and_projection(tmp_path):
    data = synth.bam_file(30000, seed=42)
    fn = os.path.join(str(tmp_path), "synth.bam")
    open(fn, "wb").write(data)
    exp, want = model_cols(data, bin_width=5000)
    assert exp["n_rows"] == 29990
    rc, out, dump = bins(fn, named=[("bin_width", "5000")])
    assert rc == 0 and "rows=29990 " in out, out
    schema, sizes, cols = columns(dump)
    assert sizes == [2048] * 14 + [29990 - 14 * 2048] and cols == want
    rc, out, dump = bins(fn, named=[("bin_width", "5000")], proj=[0, 4])
    assert rc == 0 and columns(dump)[2] == [exp["chrom"], exp["count_total"]]
    rc, out, dump = bins(fn, named=[("bin_width", "5000")], proj=[6])
    assert rc == 0 and columns(dump)[2] == [exp["count_rev"]]
    rc, out, dump = bins(fn, named=[("bin_width", "5000")], proj=[5, 1, 2])
    assert rc == 0 and columns(dump)[2] == [exp["count_fwd"], exp["start"], exp["end"]]


def test_path_error_without_a_device(tmp_path):
    import duckhts_amd
    if duckhts_amd.lib().dhts_device_count() == 0:                          # no device here: the file is there, the bind says what is missing
        fn = os.path.join(str(tmp_path), "range.bam")
        shutil.copy(os.path.join(GOLDEN, "range.bam"), fn)
        rc, out, _ = bins(fn)
        assert rc == 3 and out == "ERROR bind: bam_bin_counts: no MI355X (gfx950) device available; this build has no CPU fallback"
    rc, out, _ = bins("")
    assert rc == 3 and out == "ERROR bind: " + M.ERR_PATH
    rc, out, _ = bins("/no/such/file.bam")
    assert rc == 3 and out == "ERROR bind: Failed to open SAM/BAM/CRAM file: /no/such/file.bam"     # read_bam's own (bam_reader.c:446)
    rc, out, _ = bins("x.bam", named=[("bogus", "1")])
    assert rc == 3 and "unknown named parameter" in out
    for k in ("bin_width", "min_mapq", "include_flags", "require_flags", "exclude_flags", "dedup", "region", "index_path", "emit_zero_bins"):
        rc, out, _ = bins("/no/such/file.bam", named=[(k, "1")])
        assert "unknown named parameter" not in out
    # the parameters are checked in front of the file
    for named, msg in (([("bin_width", "0")], M.ERR_BIN_WIDTH), ([("bin_width", "-5")], M.ERR_BIN_WIDTH), ([("min_mapq", "256")], M.ERR_MAPQ), ([("min_mapq", "-1")], M.ERR_MAPQ),
                       ([("include_flags", "65536")], M.err_flags("include")), ([("require_flags", "-1")], M.err_flags("require")), ([("exclude_flags", "65536")], M.err_flags("exclude")),
                       ([("dedup", "optical")], M.ERR_DEDUP),
                       # wrong in two ways: the first in the order of the checks is reported
                       ([("bin_width", "0"), ("min_mapq", "256")], M.ERR_BIN_WIDTH), ([("min_mapq", "256"), ("include_flags", "65536")], M.ERR_MAPQ),
                       ([("require_flags", "-1"), ("exclude_flags", "70000")], M.err_flags("require")), ([("dedup", "optical"), ("exclude_flags", "70000")], M.err_flags("exclude"))):
        rc, out, _ = bins("/no/such/file.bam", named=named)
        assert rc == 3 and out == "ERROR bind: " + msg, out


@pytest.mark.gpu
def test_bind_errors_on_the_device(rng, tmp_path):
    fn, data = rng
    for named, msg in (([("bin_width", "0")], M.ERR_BIN_WIDTH), ([("min_mapq", "256")], M.ERR_MAPQ), ([("include_flags", "65536")], M.err_flags("include")),
                       ([("require_flags", "65536")], M.err_flags("require")), ([("exclude_flags", "-1")], M.err_flags("exclude")), ([("dedup", "ADJACENT")], M.ERR_DEDUP)):
        rc, out, _ = bins(fn, named=named)
        assert rc == 3 and out == "ERROR bind: " + msg, out
    # the bin-count limit states the count
    big = os.path.join(str(tmp_path), "big.bam")
    open(big, "wb").write(K.bam([("big", 2 ** 31 - 1), ("small", 10)], [(0, 0, 5, 30, -1)]))
    rc, out, _ = bins(big, named=[("bin_width", "1")])
    assert rc == 3 and out.startswith("ERROR bind: bam_bin_counts: ") and str(2 ** 31 - 1 + 10) in out and "bins" in out, out
    rc, out, dump = bins(big, named=[("bin_width", "16")])
    assert rc == 0 and "rows=1 " in out and columns(dump)[2] == [[b"big"], [0], [16], [0], [1], [1], [0]], out
    # read_bam's own errors, verbatim
    bad = os.path.join(str(tmp_path), "bad.bam")
    open(bad, "wb").write(b"not a bam file at all")
    rc, out, _ = bins(bad)
    assert rc == 3 and out == "ERROR bind: Failed to read SAM/BAM/CRAM header"                # bam_reader.c:461
    rc, out, _ = bins(fn, named=[("region", "nosuch:1-5")])
    assert rc == 3 and out == "ERROR bind: No reads found for region(s): nosuch:1-5"         # bam_reader.c:662-667
    noidx = os.path.join(str(tmp_path), "noindex.bam")
    shutil.copy(fn, noidx)
    rc, out, _ = bins(noidx, named=[("region", "CHROMOSOME_I:1-1000")])
    assert rc == 3 and out == "ERROR bind: Region query requires an index (.bai/.csi/.crai)"  # bam_reader.c:647-648
    rc, out, _ = bins(noidx, named=[("region", "CHROMOSOME_I:1-1000"), ("index_path", fn + ".bai")])
    assert rc == 0, out


def test_registered_only_with_the_variable():
    import duckhts_amd
    others = ("DHTS_INTERVAL_FUNCTIONS", "DHTS_SEQ_FUNCTIONS", "DHTS_TABIX_FUNCTIONS", "DHTS_NUC_FUNCTIONS", "DHTS_KMER_FUNCTIONS")
    env = {k: v for k, v in os.environ.items() if k not in others + ("DHTS_COVERAGE_FUNCTIONS",)}

    def catalog(**kw):
        return subprocess.run([HOST, duckhts_amd.LIB_PATH, "--catalog", "-"], capture_output=True, text=True, env=dict(env, **kw)).stdout.splitlines()

    r = subprocess.run([HOST, duckhts_amd.LIB_PATH, "bam_bin_counts", ""], capture_output=True, text=True, env=env)
    assert r.returncode == 3 and r.stdout.strip() == "ERROR catalog: table function bam_bin_counts not registered"
    default = catalog()
    assert not any("bam_bin_counts" in ln for ln in default)
    for k in others:                                                        # none of the existing variables registers it
        assert not any("bam_bin_counts" in ln for ln in catalog(**{k: "1"}))
    on = catalog(**ON)
    assert on[:len(default)] == default
    assert on[len(default):] == ["TF bam_bin_counts pushdown=1 bind=1 init=1 local_init=0 func=1 named=bin_width:5,min_mapq:5,include_flags:5,require_flags:5,exclude_flags:5,"
                                 "dedup:17,region:17,index_path:17,emit_zero_bins:1"]
    everything = catalog(DHTS_COVERAGE_FUNCTIONS="1", **{k: "1" for k in others})
    assert everything[-1] == on[-1] and everything[:-1] == catalog(**{k: "1" for k in others})     # last, and the other sets as they were
    assert "".join(ln + "\n" for ln in everything[:-1]) == open(os.path.join(GOLDEN, "surface_catalog.txt")).read()
