"""bam_depth_hist through the DuckDB surface (tests/minihost, DHTS_HIST_FUNCTIONS=1) against the Python function: the eight columns and their types,
fraction_at_least as the IEEE quotient of the two integers, the defaults and every named parameter, a BED, regions, projection pushdown, pages
of 1 and 7 rows, and the refusals in the order bind checks them.  (The registration is test_bam_depth_hist_surface's.)"""
import os
import shutil

import numpy as np
import pytest

import bam_depth_cases as D
import bam_depth_hist_cases as H
import bam_depth_hist_ref as M
import duckhts_amd
from conftest import GOLDEN, read_golden
from test_duckdb_fasta_nuc import columns
from test_duckdb_surface import run_host

ON = {"DHTS_HIST_FUNCTIONS": "1"}
BIGINT, DOUBLE, VARCHAR = 5, 11, 17
NAMES = ["chrom", "start", "end", "depth", "n_positions", "n_at_least", "length", "fraction_at_least"]
SCHEMA = [(n, VARCHAR if n == "chrom" else DOUBLE if n == "fraction_at_least" else BIGINT) for n in NAMES]
NAMED = ["depth_cap", "per", "bed_path", "region", "index_path", "min_read_len", "min_mapq", "min_baseq", "include_deletions", "include_flags", "require_flags", "exclude_flags"]


def hist(path, named=(), proj=None, env=None):
    return run_host(path, named=list(named), proj=proj, fn="bam_depth_hist", env=dict(ON, **(env or {})))


def as_dumped(got, names=NAMES):
    """the Python function's result the way `columns` shows the table function's: names for ids, and of the quotient its 64 bits"""
    cols = {k: got[k].tolist() for k in duckhts_amd.DEPTH_HIST_COLUMNS}
    cols["chrom"] = [got["contigs"][t] for t in got["tid"]]
    cols["fraction_at_least"] = (got["n_at_least"] / got["length"]).view(np.int64).tolist()      # numpy's true division of two int64: the same IEEE division
    return [cols[k] for k in names]


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
    rc, out, dump = hist(fn)
    assert rc == 0 and "max_threads=1" in out, out
    schema, sizes, cols = columns(dump)
    assert schema == SCHEMA
    got = duckhts_amd.bam_depth_hist(data)
    assert cols == as_dumped(got) and f"rows={got['n_rows']} " in out and got["n_rows"] > 6
    assert all(v is not None for c in cols for v in c)                                        # no column is ever NULL
    assert cols[7][0] == np.float64(1.0).view(np.int64) and cols[5][0] == cols[6][0]          # a group's lowest bin: everything is at least that deep
    for named, kw in (([("depth_cap", "3")], dict(depth_cap=3)),
                      ([("per", "contig"), ("depth_cap", "1")], dict(per="contig", depth_cap=1)),
                      ([("per", "row"), ("min_mapq", "1"), ("exclude_flags", "16")], dict(min_mapq=1, exclude_flags=16)),
                      ([("min_baseq", "30"), ("depth_cap", "1048575")], dict(min_baseq=30, depth_cap=1048575)),
                      ([("include_deletions", "true"), ("min_baseq", "25")], dict(include_deletions=1, min_baseq=25)),
                      ([("min_read_len", "100"), ("require_flags", "64"), ("include_flags", "48")], dict(min_read_len=100, require_flags=64, include_flags=48))):
        rc, out, dump = hist(fn, named=named)
        assert rc == 0, out
        assert columns(dump)[2] == as_dumped(duckhts_amd.bam_depth_hist(data, **kw)), named


@pytest.mark.gpu
def test_projection_and_pages(tmp_path):
    case = H.stack()
    data = H.bam(case["refs"], case["reads"] + [H.R(0, 0, 10 + i, 30, f"{5 + i}M", 30) for i in range(24)])
    fn = write(tmp_path, "stack.bam", data)
    got = duckhts_amd.bam_depth_hist(data, depth_cap=5000)
    assert got["n_rows"] > 14
    named = [("depth_cap", "5000")]
    rc, out, dump = hist(fn, named=named)
    assert rc == 0 and columns(dump)[2] == as_dumped(got)
    # fraction_at_least alone needs its two integers on the host and shows neither
    for proj, names in (([7], ["fraction_at_least"]), ([3], ["depth"]), ([5, 0], ["n_at_least", "chrom"]), ([7, 4], ["fraction_at_least", "n_positions"]), ([6], ["length"])):
        rc, out, dump = hist(fn, named=named, proj=proj)
        assert rc == 0 and columns(dump)[2] == as_dumped(got, names), proj
    for page in ("1", "7"):                                                   # a page seam inside a group: the rows stay the same
        rc, out, dump = hist(fn, named=named, env={"DHTS_DEPTH_HIST_PAGE_ROWS": page})
        assert rc == 0 and columns(dump)[2] == as_dumped(got)
        rc, out, dump = hist(fn, named=named, proj=[7], env={"DHTS_DEPTH_HIST_PAGE_ROWS": page})
        assert rc == 0 and columns(dump)[2] == as_dumped(got, ["fraction_at_least"])


@pytest.mark.gpu
def test_bed_path_and_region(rng, tmp_path):
    case = H.bed()
    data = H.bam(case["refs"], case["reads"])
    fn, bed = write(tmp_path, "t.bam", data), write(tmp_path, "t.bed", D.bed_text(case["bed"]))
    for named, kw in (([], dict()), ([("per", "contig"), ("depth_cap", "2")], dict(per="contig", depth_cap=2))):
        rc, out, dump = hist(fn, named=[("bed_path", bed)] + named)
        assert rc == 0, out
        assert columns(dump)[2] == as_dumped(duckhts_amd.bam_depth_hist(data, bed=D.bed_text(case["bed"]), **kw))
    fn, data = rng
    region = "CHROMOSOME_I:1001-1100,CHROMOSOME_I:901-1000"
    for named, kw in (([], dict()), ([("per", "contig")], dict(per="contig"))):
        got = duckhts_amd.bam_depth_hist(data, region=region, index=read_golden("range.bam.bai"), **kw)
        rc, out, dump = hist(fn, named=[("region", region)] + named)
        assert rc == 0 and f"rows={got['n_rows']} " in out, out
        assert columns(dump)[2] == as_dumped(got)
    rc, out, _ = hist(fn, named=[("region", "CHROMOSOME_I:1-1000,CHROMOSOME_I:900-1100")])
    assert rc != 0 and M.err_overlap("CHROMOSOME_I:1-1000", "CHROMOSOME_I:900-1100") in out, out


def test_refusals_in_the_order_bind_checks_them():
    rc, out, _ = hist("")
    assert rc == 3 and out == "ERROR bind: bam_depth_hist requires a file path"
    rc, out, _ = hist("/no/such/file.bam")
    assert rc == 3 and out == "ERROR bind: Failed to open SAM/BAM/CRAM file: /no/such/file.bam"     # read_bam's own
    rc, out, _ = hist("x.bam", named=[("bogus", "1")])
    assert rc == 3 and "unknown named parameter" in out
    for k in NAMED:
        rc, out, _ = hist("/no/such/file.bam", named=[(k, "false" if k == "include_deletions" else "row" if k == "per" else "1")])
        assert "unknown named parameter" not in out
    # the parameters are checked in front of the file: the filter, depth_cap, per, then a BED beside a region
    for named, msg in (([("min_mapq", "256")], M.err_range("min_mapq")), ([("min_mapq", "-1")], M.err_range("min_mapq")), ([("min_baseq", "256")], M.err_range("min_baseq")),
                       ([("min_baseq", "-1")], M.err_range("min_baseq")), ([("include_flags", "65536")], M.err_range("include_flags")), ([("require_flags", "-1")], M.err_range("require_flags")),
                       ([("exclude_flags", "65536")], M.err_range("exclude_flags")), ([("min_read_len", "-1")], M.ERR_READ_LEN),
                       ([("depth_cap", "0")], M.ERR_DEPTH_CAP), ([("depth_cap", "-1")], M.ERR_DEPTH_CAP), ([("depth_cap", "1048576")], M.ERR_DEPTH_CAP), ([("depth_cap", "99999999999")], M.ERR_DEPTH_CAP),
                       ([("per", "total")], M.ERR_PER), ([("per", "ROW")], M.ERR_PER), ([("per", "")], M.ERR_PER), ([("per", "contig ")], M.ERR_PER),
                       ([("bed_path", "/no/such.bed"), ("region", "c1:1-5")], M.ERR_BED_AND_REGION),
                       # wrong in two ways: the first in the order of the checks is reported
                       ([("min_read_len", "-1"), ("min_mapq", "256")], M.ERR_READ_LEN), ([("depth_cap", "0"), ("exclude_flags", "70000")], M.err_range("exclude_flags")),
                       ([("per", "total"), ("depth_cap", "0")], M.ERR_DEPTH_CAP), ([("per", "total"), ("bed_path", "/no/such.bed"), ("region", "c1:1-5")], M.ERR_PER)):
        rc, out, _ = hist("/no/such/file.bam", named=named)
        assert rc == 3 and out == "ERROR bind: " + msg, (named, out)
    rc, out, _ = hist("/no/such/file.bam", named=[("depth_cap", "1048575"), ("per", "contig")])   # the largest cap is taken: the file is what fails
    assert rc == 3 and out == "ERROR bind: Failed to open SAM/BAM/CRAM file: /no/such/file.bam"


@pytest.mark.gpu
def test_file_region_bed_and_cap_errors(rng, tmp_path):
    fn, data = rng
    rc, out, _ = hist(write(tmp_path, "bad.bam", b"not a bam file at all"))
    assert rc == 3 and out == "ERROR bind: Failed to read SAM/BAM/CRAM header"
    rc, out, _ = hist(fn, named=[("region", "nosuch:1-5")])
    assert rc == 3 and out == "ERROR bind: No reads found for region(s): nosuch:1-5"
    rc, out, _ = hist(fn, named=[("bed_path", "/no/such.bed")])
    assert rc == 3 and out == "ERROR bind: read_bed: failed to open file: /no/such.bed"           # as bam_bedcov binds
    # the histogram's 1 GiB: 129 target rows of 1,048,576 bins are 8 MiB more, and per := 'contig' stays under it
    bed = write(tmp_path, "many.bed", D.bed_text([(b"CHROMOSOME_I", 20 * i, 20 * i + 10) for i in range(129)]))
    rc, out, _ = hist(fn, named=[("bed_path", bed), ("depth_cap", "1048575")])
    assert rc != 0 and M.err_hist(129 * 1048576 * 8, 1 << 30) in out, out
    rc, out, dump = hist(fn, named=[("bed_path", bed), ("depth_cap", "1048575"), ("per", "contig")])
    assert rc == 0 and columns(dump)[2][6] == [1290] * len(columns(dump)[2][6]), out
