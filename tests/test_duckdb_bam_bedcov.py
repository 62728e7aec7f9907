"""bam_bedcov through the DuckDB surface (tests/minihost, DHTS_COVERAGE_FUNCTIONS=2): the eight columns and their types, the defaults against
the CPU model, projection pushdown, a BED longer than one 2048-row chunk, every error string at bind, and the registration."""
import os
import shutil
import subprocess

import pytest

import bam_bedcov_cases as K
import bam_bedcov_ref as M
import orc
from conftest import GOLDEN, read_golden
from test_duckdb_fasta_nuc import columns
from test_duckdb_surface import HOST, run_host

ON = {"DHTS_COVERAGE_FUNCTIONS": "2"}
BIGINT, VARCHAR = 5, 17
SCHEMA = list(zip(M.COLUMNS, [VARCHAR, BIGINT, BIGINT, VARCHAR, VARCHAR, VARCHAR, BIGINT, BIGINT]))


def bedcov(path, bed=None, named=(), proj=None):
    return run_host(path, named=([("bed_path", bed)] if bed is not None else []) + list(named), proj=proj, fn="bam_bedcov", env=ON)


def model_cols(data, bed_text, names=M.COLUMNS, **kw):
    kw.setdefault("exclude_flags", M.DEFAULT_EXCLUDE)                     # the table function's default
    c = orc.bam_read(data)
    exp = M.bedcov(c, c["ref_names"], bed_text, **kw)
    return exp, [exp[k] for k in names]


def write(tmp_path, name, data):
    fn = os.path.join(str(tmp_path), name)
    open(fn, "wb").write(data)
    return fn


@pytest.fixture()
def rng(tmp_path):
    fn = os.path.join(str(tmp_path), "range.bam")
    shutil.copy(os.path.join(GOLDEN, "range.bam"), fn)
    shutil.copy(os.path.join(GOLDEN, "range.bam.bai"), fn + ".bai")
    return fn, read_golden("range.bam"), write(tmp_path, "golden.bed", K.GOLDEN_BED)


@pytest.mark.gpu
def test_schema_and_values(rng):
    fn, data, bed = rng
    rc, out, dump = bedcov(fn, bed)
    assert rc == 0 and "max_threads=1" in out, out
    schema, sizes, cols = columns(dump)
    assert schema == SCHEMA
    exp, want = model_cols(data, K.GOLDEN_BED)
    assert cols == want and f"rows={exp['n_rows']} " in out and exp["n_rows"] == 14
    for named, kw in (([("min_mapq", "1"), ("exclude_flags", "16")], dict(min_mapq=1, exclude_flags=16)),
                      ([("count_deletions", "false")], dict(count_deletions=False)),
                      ([("count_deletions", "false"), ("count_ref_skips", "false"), ("require_flags", "64"), ("include_flags", "48")],
                       dict(count_deletions=False, count_ref_skips=False, require_flags=64, include_flags=48))):
        rc, out, dump = bedcov(fn, bed, named=named)
        assert rc == 0, out
        assert columns(dump)[2] == model_cols(data, K.GOLDEN_BED, **kw)[1]


@pytest.mark.gpu
def test_defaults_exclude_duplicates(tmp_path):
    # exclude_flags defaults to 0x704: the duplicate-flagged read, the secondary one and the QC failure count only when the mask is cleared
    rows = [(0, 0, 100, 30, "10M"), (0x400, 0, 100, 30, "10M"), (0x100, 0, 100, 30, "10M"), (0x200, 0, 100, 30, "10M"), (0x800, 0, 100, 30, "5M3D5M")]
    data = K.bam(K.REFS, rows)
    fn, bed = write(tmp_path, "dup.bam", data), write(tmp_path, "one.bed", b"c1\t100\t120\tx\n")
    rc, out, dump = bedcov(fn, bed)
    assert rc == 0 and columns(dump)[2][6:] == [[23], [2]], out                    # the supplementary read is not in samtools' default mask
    rc, out, dump = bedcov(fn, bed, named=[("exclude_flags", "0")])
    assert rc == 0 and columns(dump)[2][6:] == [[53], [5]], out
    rc, out, dump = bedcov(fn, bed, named=[("exclude_flags", "0"), ("count_deletions", "false")])
    assert rc == 0 and columns(dump)[2][6:] == [[50], [5]], out
    assert model_cols(data, b"c1\t100\t120\tx\n")[1][6:] == [[23], [2]]


@pytest.mark.gpu
def test_region(rng):
    import duckhts_amd
    fn, data, bed = rng
    region = "CHROMOSOME_I:1-1000"
    rows = duckhts_amd.read_bam(data, region=region, index=read_golden("range.bam.bai"))
    exp = M.bedcov(rows, rows["header"]["ref_names"], K.GOLDEN_BED, exclude_flags=M.DEFAULT_EXCLUDE)
    rc, out, dump = bedcov(fn, bed, named=[("region", region)])
    assert rc == 0 and "rows=14 " in out, out
    assert columns(dump)[2] == [exp[k] for k in M.COLUMNS]


@pytest.mark.gpu
def test_chunks_and_projection(tmp_path):
    text = K.bed([("c1" if i < 2600 else "c2", 20 * (i % 2600), 20 * (i % 2600) + 13, f"t{i}") for i in range(5000)])
    data = K.bam(K.REFS, [(0, i % 2, (i * 331) % 52000, 30, ("30M", "10M5D10M", "4S26M")[i % 3]) for i in range(300)])
    fn, bed = write(tmp_path, "reads.bam", data), write(tmp_path, "long.bed", text)
    exp, want = model_cols(data, text)
    rc, out, dump = bedcov(fn, bed)
    assert rc == 0 and "rows=5000 " in out, out
    schema, sizes, cols = columns(dump)
    assert sizes == [2048, 2048, 904] and cols == want
    rc, out, dump = bedcov(fn, bed, proj=[0, 6])
    assert rc == 0 and columns(dump)[2] == [exp["chrom"], exp["bases_covered"]]
    rc, out, dump = bedcov(fn, bed, proj=[7])
    assert rc == 0 and columns(dump)[2] == [exp["read_count"]]
    rc, out, dump = bedcov(fn, bed, proj=[3, 7, 1, 2])
    assert rc == 0 and columns(dump)[2] == [exp["name"], exp["read_count"], exp["start"], exp["end"]]


def test_bind_errors_without_a_device(tmp_path):
    rc, out, _ = bedcov("", "x.bed")
    assert rc == 3 and out == "ERROR bind: " + M.ERR_PATH
    rc, out, _ = bedcov("/no/such/file.bam")
    assert rc == 3 and out == "ERROR bind: " + M.ERR_BED_PATH                       # in front of the file
    rc, out, _ = bedcov("/no/such/file.bam", "")
    assert rc == 3 and out == "ERROR bind: " + M.ERR_BED_PATH
    rc, out, _ = bedcov("/no/such/file.bam", "x.bed")
    assert rc == 3 and out == "ERROR bind: Failed to open SAM/BAM/CRAM file: /no/such/file.bam"     # read_bam's own (bam_reader.c:446)
    rc, out, _ = bedcov("x.bam", "x.bed", named=[("bogus", "1")])
    assert rc == 3 and "unknown named parameter" in out
    for k in ("min_mapq", "include_flags", "require_flags", "exclude_flags", "count_deletions", "count_ref_skips", "region", "index_path"):
        rc, out, _ = bedcov("/no/such/file.bam", "x.bed", named=[(k, "1")])
        assert "unknown named parameter" not in out
    # the parameters are checked in front of the file
    for named, msg in (([("min_mapq", "256")], M.ERR_MAPQ), ([("min_mapq", "-1")], M.ERR_MAPQ), ([("include_flags", "65536")], M.err_flags("include")),
                       ([("require_flags", "-1")], M.err_flags("require")), ([("exclude_flags", "65536")], M.err_flags("exclude")),
                       # wrong in two ways: the first in the order of the checks is reported
                       ([("min_mapq", "256"), ("include_flags", "65536")], M.ERR_MAPQ), ([("require_flags", "-1"), ("exclude_flags", "70000")], M.err_flags("require"))):
        rc, out, _ = bedcov("/no/such/file.bam", "x.bed", named=named)
        assert rc == 3 and out == "ERROR bind: " + msg, out


@pytest.mark.gpu
def test_bind_and_init_errors_on_the_device(rng, tmp_path):
    fn, data, bed = rng
    rc, out, _ = bedcov(fn)
    assert rc == 3 and out == "ERROR bind: " + M.ERR_BED_PATH
    rc, out, _ = bedcov(fn, "/no/such/file.bed")
    assert rc == 3 and out == "ERROR bind: read_bed: failed to open file: /no/such/file.bed"         # read_bed's own
    # read_bam's own errors, verbatim
    rc, out, _ = bedcov(write(tmp_path, "bad.bam", b"not a bam file at all"), bed)
    assert rc == 3 and out == "ERROR bind: Failed to read SAM/BAM/CRAM header"
    rc, out, _ = bedcov(fn, bed, named=[("region", "nosuch:1-5")])
    assert rc == 3 and out == "ERROR bind: No reads found for region(s): nosuch:1-5"
    noidx = os.path.join(str(tmp_path), "noindex.bam")
    shutil.copy(fn, noidx)
    rc, out, _ = bedcov(noidx, bed, named=[("region", "CHROMOSOME_I:1-1000")])
    assert rc == 3 and out == "ERROR bind: Region query requires an index (.bai/.csi/.crai)"
    rc, out, _ = bedcov(noidx, bed, named=[("region", "CHROMOSOME_I:1-1000"), ("index_path", fn + ".bai")])
    assert rc == 0, out
    # a BED line with fewer than three fields: read_bed's error, with the line number
    rc, out, _ = bedcov(fn, write(tmp_path, "short.bed", b"CHROMOSOME_I\t1\t2\nCHROMOSOME_I\t5\n"))
    assert rc != 0 and "read_bed: BED line has fewer than 3 tab-delimited fields (line 2)" in out, out
    # an empty BED is an empty result
    rc, out, _ = bedcov(fn, write(tmp_path, "empty.bed", b""))
    assert rc == 0 and "rows=0 " in out, out


def test_registered_behind_bam_bin_counts():
    import duckhts_amd

    def catalog(v):
        env = {k: x for k, x in os.environ.items() if not (k.startswith("DHTS_") and k.endswith("_FUNCTIONS"))}
        if v is not None:
            env["DHTS_COVERAGE_FUNCTIONS"] = v
        return subprocess.run([HOST, duckhts_amd.LIB_PATH, "--catalog", "-"], capture_output=True, text=True, env=env).stdout.splitlines()

    default, one, two = catalog(None), catalog("1"), catalog("2")
    assert not any("bam_bedcov" in ln for ln in default + one)                        # the set under 1 is what it was
    assert two[:len(one)] == one and one[-1].startswith("TF bam_bin_counts ")
    assert two[len(one):] == ["TF bam_bedcov pushdown=1 bind=1 init=1 local_init=0 func=1 named=bed_path:17,min_mapq:5,include_flags:5,require_flags:5,exclude_flags:5,"
                              "count_deletions:1,count_ref_skips:1,region:17,index_path:17"]
    assert catalog("3") == default
