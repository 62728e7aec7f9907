"""interval_nearest through the DuckDB surface (tests/minihost, DHTS_NEAREST_FUNCTIONS=1): the columns and their types, results equal to the
model across the 2,048-row chunk edge and under small pages, projections, every bind error by its text and order, empty files and the registration."""
import os
import subprocess

import pytest

import interval_nearest_ref as N
import interval_ref as R
from bamwriter import bgzf_file
from test_duckdb_fasta_nuc import columns
from test_duckdb_surface import HOST, run_host

ON = {"DHTS_NEAREST_FUNCTIONS": "1"}
BIGINT, VARCHAR = 5, 17
SCHEMA = list(zip(N.NEAREST_COLUMNS, [VARCHAR] + [BIGINT] * 8))
CATALOG_LINE = "TF interval_nearest pushdown=1 bind=1 init=1 local_init=0 func=1 named=right_path:17,k:5,max_distance:5,ties:17"


def nearest(path, right=None, named=(), proj=None, env=None):
    return run_host(path, named=([("right_path", right)] if right is not None else []) + list(named), proj=proj, fn="interval_nearest", env=dict(ON, **(env or {})))


def write(tmp_path, name, data):
    fn = os.path.join(str(tmp_path), name)
    open(fn, "wb").write(data)
    return fn


def cols_of(rows, ncols=9):
    return [[r[k] for r in rows] for k in range(ncols)]


@pytest.fixture()
def files(tmp_path):
    """a left file whose result with the right file at k = 4 is more than one 2,048-row chunk"""
    left = R.seeded_bed(51, 900, n_chroms=3, span=3000)
    right = [(b"chr%d" % (1 + i % 4), 3 * i, 3 * i + 1 + i % 2) for i in range(6000)] + R.seeded_bed(52, 300, n_chroms=2, span=3000)
    ltext, rtext = R.bed_text(left), R.bed_text(right)
    return write(tmp_path, "left.bed", ltext), write(tmp_path, "right.bed.gz", bgzf_file(rtext)), ltext, rtext


@pytest.mark.gpu
def test_schema_values_chunks_and_pages(files):
    lp, rp, ltext, rtext = files
    rc, out, dump = nearest(lp, rp, named=[("k", "4")])
    assert rc == 0 and "max_threads=1" in out, out
    schema, sizes, cols = columns(dump)
    exp = N.nearest(ltext, rtext, 4)
    assert schema == SCHEMA and len(exp) > 2048 and sizes[0] == 2048 and sum(sizes) == len(exp) and f"rows={len(exp)} " in out
    assert cols == cols_of(exp)
    rc, out, dump = nearest(lp, rp, named=[("k", "4")], env={"DHTS_INTERVAL_PAGE_ROWS": "100", "DHTS_BATCH_BLOCKS": "1"})      # pages that end inside a chunk
    assert rc == 0 and columns(dump)[2] == cols_of(exp), out
    rc, out, dump = nearest(lp, rp, named=[("k", "4"), ("ties", "first"), ("max_distance", "2")])
    exp = N.nearest(ltext, rtext, 4, 2, "first")
    assert rc == 0 and 0 < len(exp) and columns(dump)[2] == cols_of(exp), out
    rc, out, dump = nearest(lp, rp)                                              # the defaults: k 1, no max_distance, 'all'
    assert rc == 0 and columns(dump)[2] == cols_of(N.nearest(ltext, rtext)), out


@pytest.mark.gpu
def test_projection(files):
    lp, rp, ltext, rtext = files
    exp = cols_of(N.nearest(ltext, rtext, 2))
    for proj in ([8], [0], [6, 3], [1, 8, 5, 0]):
        rc, out, dump = nearest(lp, rp, named=[("k", "2")], proj=proj)
        assert rc == 0 and columns(dump)[2] == [exp[k] for k in proj], (proj, out)


def test_bind_errors_without_a_device(tmp_path):
    here = write(tmp_path, "a.bed", b"c\t0\t1\n")
    bad_k, bad_md, bad_ties = ("k", "0"), ("max_distance", "-1"), ("ties", "any")
    rc, out, _ = nearest("", "", named=[bad_k, bad_md, bad_ties])
    assert rc == 3 and out == "ERROR bind: " + N.ERR_NEAREST_PATH
    for right in (None, ""):
        rc, out, _ = nearest(here, right, named=[bad_k, bad_md, bad_ties])
        assert rc == 3 and out == "ERROR bind: " + N.ERR_RIGHT_PATH
    # the parameters are checked in their order, in front of the files
    rc, out, _ = nearest("/no/such/left.bed", "/no/such/right.bed", named=[bad_k, bad_md, bad_ties])
    assert rc == 3 and out == "ERROR bind: " + N.ERR_K
    for bad in ("0", "-3", str((1 << 20) + 1)):
        rc, out, _ = nearest(here, here, named=[("k", bad)])
        assert rc == 3 and out == "ERROR bind: " + N.ERR_K, out
    rc, out, _ = nearest("/no/such/left.bed", "/no/such/right.bed", named=[bad_md, bad_ties])
    assert rc == 3 and out == "ERROR bind: " + N.ERR_MAX_DISTANCE
    for bad in ("first ", "FIRST", "", "any"):
        rc, out, _ = nearest("/no/such/left.bed", here, named=[("ties", bad), ("k", str(1 << 20)), ("max_distance", "0")])
        assert rc == 3 and out == "ERROR bind: " + N.ERR_TIES, out
    rc, out, _ = nearest("/no/such/left.bed", "/no/such/right.bed")
    assert rc == 3 and out == "ERROR bind: " + N.ERR_OPEN + "/no/such/left.bed"
    rc, out, _ = nearest(here, "/no/such/right.bed", named=[("ties", "first")])
    assert rc == 3 and out == "ERROR bind: " + N.ERR_OPEN + "/no/such/right.bed"
    rc, out, _ = nearest(here, here, named=[("mode", "any")])
    assert rc == 3 and "unknown named parameter" in out


@pytest.mark.gpu
def test_read_errors_and_empty_files(tmp_path):
    good, short = write(tmp_path, "a.bed", b"c\t0\t10\nc\t25\t30\n"), write(tmp_path, "short.bed", b"c\t1\t2\n#x\nc\t5\n")
    rc, out, _ = nearest(good, short)
    assert rc != 0 and "read_bed: BED line has fewer than 3 tab-delimited fields (line 3)" in out, out
    empty = write(tmp_path, "empty.bed", b"")
    for l, r in ((good, empty), (empty, good), (empty, empty)):
        rc, out, _ = nearest(l, r)
        assert rc == 0 and "rows=0 " in out, out
    rc, out, dump = nearest(good, good, named=[("k", "2"), ("ties", "first")])
    assert rc == 0 and columns(dump)[2] == cols_of(N.nearest(b"c\t0\t10\nc\t25\t30\n", b"c\t0\t10\nc\t25\t30\n", 2, None, "first"))


def test_registered_behind_interval_overlap_only_with_the_variable():
    import duckhts_amd

    def catalog(**on):
        env = {k: x for k, x in os.environ.items() if not (k.startswith("DHTS_") and k.endswith("_FUNCTIONS"))}
        env.update(on)
        return subprocess.run([HOST, duckhts_amd.LIB_PATH, "--catalog", "-"], capture_output=True, text=True, env=env).stdout.splitlines()

    default = catalog()
    assert not any("interval_" in ln for ln in default) and catalog(DHTS_NEAREST_FUNCTIONS="2") == default
    assert catalog(DHTS_NEAREST_FUNCTIONS="1") == default + [CATALOG_LINE]
    both = catalog(DHTS_ALGEBRA_FUNCTIONS="1", DHTS_NEAREST_FUNCTIONS="1")
    assert both == catalog(DHTS_ALGEBRA_FUNCTIONS="1") + [CATALOG_LINE] and both[-2].split()[1] == "interval_overlap"
