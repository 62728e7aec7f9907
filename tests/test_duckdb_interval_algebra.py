"""interval_merge and interval_overlap through the DuckDB surface (tests/minihost, DHTS_ALGEBRA_FUNCTIONS=1): the columns and their types, results
equal to the model across the 2,048-row chunk edge, projection of a single column, every bind error by its text, and the registration."""
import os
import subprocess

import pytest

import interval_ref as R
from bamwriter import bgzf_file
from test_duckdb_fasta_nuc import columns
from test_duckdb_surface import HOST, run_host

ON = {"DHTS_ALGEBRA_FUNCTIONS": "1"}
BIGINT, VARCHAR = 5, 17
MERGE_SCHEMA = list(zip(R.MERGE_COLUMNS, [VARCHAR, BIGINT, BIGINT, BIGINT]))
OVERLAP_SCHEMA = list(zip(R.OVERLAP_COLUMNS, [VARCHAR] + [BIGINT] * 7))


def merge(path, named=(), proj=None, env=None):
    return run_host(path, named=list(named), proj=proj, fn="interval_merge", env=dict(ON, **(env or {})))


def overlap(path, right=None, named=(), proj=None, env=None):
    return run_host(path, named=([("right_path", right)] if right is not None else []) + list(named), proj=proj, fn="interval_overlap", env=dict(ON, **(env or {})))


def write(tmp_path, name, data):
    fn = os.path.join(str(tmp_path), name)
    open(fn, "wb").write(data)
    return fn


def cols_of(rows, ncols):
    return [[r[k] for r in rows] for k in range(ncols)]


@pytest.fixture()
def files(tmp_path):
    """a left file whose pairs with the right file, and a right file whose runs, are more than one 2,048-row chunk"""
    left = R.seeded_bed(51, 900, n_chroms=3, span=3000)
    right = [(b"chr%d" % (1 + i % 4), 3 * i, 3 * i + 1 + i % 2) for i in range(6000)] + R.seeded_bed(52, 300, n_chroms=2, span=3000)
    ltext, rtext = R.bed_text(left), R.bed_text(right)
    return write(tmp_path, "left.bed", ltext), write(tmp_path, "right.bed.gz", bgzf_file(rtext)), ltext, rtext


@pytest.mark.gpu
def test_schemas_values_and_chunks(files):
    lp, rp, ltext, rtext = files
    rc, out, dump = merge(rp)
    assert rc == 0 and "max_threads=1" in out, out
    schema, sizes, cols = columns(dump)
    exp = R.merge(rtext)
    assert schema == MERGE_SCHEMA and len(exp) > 2048 and sizes[0] == 2048 and sum(sizes) == len(exp) and f"rows={len(exp)} " in out
    assert cols == cols_of(exp, 4)
    rc, out, dump = merge(rp, named=[("max_gap", "2")], env={"DHTS_INTERVAL_PAGE_ROWS": "1000"})        # pages that end inside a chunk
    exp = R.merge(rtext, 2)
    assert rc == 0 and columns(dump)[2] == cols_of(exp, 4) and 0 < len(exp) < len(R.merge(rtext)), out
    for mode in R.MODES:
        rc, out, dump = overlap(lp, rp, named=[("mode", mode)])
        assert rc == 0, out
        schema, sizes, cols = columns(dump)
        exp = R.overlap(ltext, rtext, mode)
        assert schema == OVERLAP_SCHEMA and sum(sizes) == len(exp) and cols == cols_of(exp, 8), mode
        assert mode != "any" or (len(exp) > 2048 and sizes[0] == 2048)
    rc, out, dump = overlap(lp, rp, env={"DHTS_INTERVAL_PAGE_ROWS": "100", "DHTS_BATCH_BLOCKS": "1"})  # the default mode is 'any'
    assert rc == 0 and columns(dump)[2] == cols_of(R.overlap(ltext, rtext, "any"), 8), out


@pytest.mark.gpu
def test_projection(files):
    lp, rp, ltext, rtext = files
    exp = cols_of(R.overlap(ltext, rtext, "any"), 8)
    for proj in ([7], [0], [6, 3], [1, 5, 0]):
        rc, out, dump = overlap(lp, rp, proj=proj)
        assert rc == 0 and columns(dump)[2] == [exp[k] for k in proj], (proj, out)
    expm = cols_of(R.merge(ltext), 4)
    for proj in ([3], [0], [2, 1]):
        rc, out, dump = merge(lp, proj=proj)
        assert rc == 0 and columns(dump)[2] == [expm[k] for k in proj], (proj, out)


def test_bind_errors_without_a_device(tmp_path):
    here = write(tmp_path, "a.bed", b"c\t0\t1\n")
    rc, out, _ = merge("")
    assert rc == 3 and out == "ERROR bind: " + R.ERR_MERGE_PATH
    rc, out, _ = overlap("", here)
    assert rc == 3 and out == "ERROR bind: " + R.ERR_OVERLAP_PATH
    rc, out, _ = overlap(here)
    assert rc == 3 and out == "ERROR bind: " + R.ERR_RIGHT_PATH
    rc, out, _ = overlap(here, "")
    assert rc == 3 and out == "ERROR bind: " + R.ERR_RIGHT_PATH
    for bad in ("touch", "ANY", ""):
        rc, out, _ = overlap(here, here, named=[("mode", bad)])
        assert rc == 3 and out == "ERROR bind: " + R.ERR_MODE, out
    for bad in ("-1", str((1 << 40) + 1)):
        rc, out, _ = merge(here, named=[("max_gap", bad)])
        assert rc == 3 and out == "ERROR bind: " + R.ERR_MAX_GAP, out
    # the parameters are checked in front of the files
    rc, out, _ = merge("/no/such/file.bed", named=[("max_gap", "-1")])
    assert rc == 3 and out == "ERROR bind: " + R.ERR_MAX_GAP
    rc, out, _ = merge("/no/such/file.bed")
    assert rc == 3 and out == "ERROR bind: " + R.ERR_OPEN + "/no/such/file.bed"
    rc, out, _ = overlap("/no/such/left.bed", here)
    assert rc == 3 and out == "ERROR bind: " + R.ERR_OPEN + "/no/such/left.bed"
    rc, out, _ = overlap(here, "/no/such/right.bed")
    assert rc == 3 and out == "ERROR bind: " + R.ERR_OPEN + "/no/such/right.bed"
    rc, out, _ = merge(here, named=[("bogus", "1")])
    assert rc == 3 and "unknown named parameter" in out
    rc, out, _ = overlap(here, here, named=[("max_gap", "1")])
    assert rc == 3 and "unknown named parameter" in out


@pytest.mark.gpu
def test_read_errors_and_empty_files(tmp_path):
    good, short = write(tmp_path, "a.bed", b"c\t0\t10\nc\t5\t20\n"), write(tmp_path, "short.bed", b"c\t1\t2\n#x\nc\t5\n")
    rc, out, _ = merge(short)
    assert rc != 0 and "read_bed: BED line has fewer than 3 tab-delimited fields (line 3)" in out, out
    rc, out, _ = overlap(good, short)
    assert rc != 0 and "read_bed: BED line has fewer than 3 tab-delimited fields (line 3)" in out, out
    empty = write(tmp_path, "empty.bed", b"")
    rc, out, _ = merge(empty)
    assert rc == 0 and "rows=0 " in out, out
    rc, out, _ = overlap(good, empty)
    assert rc == 0 and "rows=0 " in out, out
    rc, out, dump = overlap(good, good, named=[("mode", "within")])
    assert rc == 0 and columns(dump)[2] == cols_of(R.overlap(b"c\t0\t10\nc\t5\t20\n", b"c\t0\t10\nc\t5\t20\n", "within"), 8)


def test_registered_behind_fasta_nuc_only_with_the_variable():
    import duckhts_amd

    def catalog(**on):
        env = {k: x for k, x in os.environ.items() if not (k.startswith("DHTS_") and k.endswith("_FUNCTIONS"))}
        env.update(on)
        return subprocess.run([HOST, duckhts_amd.LIB_PATH, "--catalog", "-"], capture_output=True, text=True, env=env).stdout.splitlines()

    default = catalog()
    assert not any("interval_" in ln for ln in default) and catalog(DHTS_ALGEBRA_FUNCTIONS="2") == default
    alone = catalog(DHTS_ALGEBRA_FUNCTIONS="1")
    assert alone == default + ["TF interval_merge pushdown=1 bind=1 init=1 local_init=0 func=1 named=max_gap:5",
                               "TF interval_overlap pushdown=1 bind=1 init=1 local_init=0 func=1 named=right_path:17,mode:17"]
    # (the mini host holds 16 table functions and leaves the scalar-function slots empty, so the k-mer family is seq_kmers alone)
    every = dict(DHTS_INTERVAL_FUNCTIONS="1", DHTS_NUC_FUNCTIONS="1", DHTS_KMER_FUNCTIONS="1", DHTS_TABIX_FUNCTIONS="1")
    before, after = catalog(**every), catalog(DHTS_ALGEBRA_FUNCTIONS="1", **every)
    names = [ln.split()[1] for ln in after]
    at = names.index("interval_merge")
    assert names[at - 1] == "fasta_nuc" and names[at + 1] == "interval_overlap" and names[at + 2] == "seq_kmers" and len(before) == 13
    assert after[:at] + after[at + 2:] == before                                   # the registered set is otherwise what it was
