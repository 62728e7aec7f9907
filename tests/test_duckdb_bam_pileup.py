"""bam_pileup through the DuckDB surface (tests/minihost, DHTS_PILEUP_FUNCTIONS=1): the five columns and their types, the defaults and every
named parameter against the CPU model, a region with an index, projection pushdown of each column alone, a result longer than one chunk and
than one page, every error string at bind, and the registration."""
import os
import shutil
import subprocess

import pytest

import bam_pileup_cases as P
import bam_pileup_ref as M
from conftest import GOLDEN, read_golden
from test_duckdb_fasta_nuc import columns
from test_duckdb_surface import HOST, run_host

ON = {"DHTS_PILEUP_FUNCTIONS": "1"}
BIGINT, VARCHAR = 5, 17
NAMES = ["chrom", "pos", "strand", "nucleotide", "count"]
SCHEMA = list(zip(NAMES, [VARCHAR, BIGINT, VARCHAR, VARCHAR, BIGINT]))
NAMED = ["region", "index_path", "min_read_len", "min_mapq", "min_baseq", "include_flags", "require_flags", "exclude_flags", "include_deletions", "include_insertions",
         "distinguish_strands", "min_nucleotide_depth"]
BOOLS = ("include_deletions", "include_insertions", "distinguish_strands")


def pileup(path, named=(), proj=None, env=None):
    return run_host(path, named=list(named), proj=proj, fn="bam_pileup", env=dict(ON, **(env or {})))


def as_dumped(exp, refs, names=NAMES):
    cols = {"chrom": [refs[t][0] for t in exp["tid"]], "pos": exp["pos"], "strand": [s.encode() for s in exp["strand"]], "nucleotide": [n.encode() for n in exp["nucleotide"]],
            "count": exp["count"]}
    return [cols[k] for k in names]


def model(data, rows=None, **kw):
    refs, reads = M.reads_from_bam(data)
    return M.pileup(reads, refs, rows=rows, **{**M.DEFAULTS, **kw}), refs                    # the table function's defaults


@pytest.fixture()
def rng(tmp_path):
    fn = os.path.join(str(tmp_path), "range.bam")
    shutil.copy(os.path.join(GOLDEN, "range.bam"), fn)
    shutil.copy(os.path.join(GOLDEN, "range.bam.bai"), fn + ".bai")
    return fn, read_golden("range.bam")


@pytest.mark.gpu
def test_schema_and_defaults(rng):
    fn, data = rng
    rc, out, dump = pileup(fn)
    assert rc == 0 and "max_threads=1" in out, out
    schema, sizes, cols = columns(dump)
    assert schema == SCHEMA
    exp, refs = model(data)
    assert cols == as_dumped(exp, refs) and f"rows={exp['n_rows']} " in out and exp["n_rows"] > 2048
    assert sizes[:-1] == [2048] * (len(sizes) - 1) and len(sizes) > 1                     # longer than one chunk


@pytest.mark.gpu
@pytest.mark.parametrize("named,kw", [([("min_mapq", "1"), ("exclude_flags", "16")], dict(min_mapq=1, exclude_flags=16)),
                                      ([("min_baseq", "30"), ("include_insertions", "true")], dict(min_baseq=30, include_insertions=1)),
                                      ([("include_deletions", "false"), ("distinguish_strands", "false"), ("min_nucleotide_depth", "2")],
                                       dict(include_deletions=0, distinguish_strands=0, min_nucleotide_depth=2)),
                                      ([("min_read_len", "100"), ("require_flags", "64"), ("include_flags", "48")], dict(min_read_len=100, require_flags=64, include_flags=48))],
                         ids=["mapq_exclude", "baseq_insertions", "switches_depth", "len_require_include"])
def test_every_named_parameter(rng, named, kw):
    fn, data = rng
    rc, out, dump = pileup(fn, named=named)
    assert rc == 0, out
    assert columns(dump)[2] == as_dumped(*model(data, **kw))


@pytest.mark.gpu
def test_the_hand_written_table(tmp_path):
    fn = os.path.join(str(tmp_path), "hand.bam")
    open(fn, "wb").write(P.hand_bam())
    names = [n.encode() for n, _ in P.HAND_REFS]
    base = [("min_mapq", "10"), ("min_read_len", "4")]
    for extra, rows in P.HAND_SETS:
        named = base + [(k, ("true" if v else "false") if k in BOOLS else str(v)) for k, v in extra.items()]
        rc, out, dump = pileup(fn, named=named)
        assert rc == 0, out
        assert columns(dump)[2] == [[names[t] for t, *_ in rows], [r[1] for r in rows], [r[2].encode() for r in rows], [r[3].encode() for r in rows], [r[4] for r in rows]]


@pytest.mark.gpu
@pytest.mark.parametrize("proj", [[0], [1], [2], [3], [4], [4, 0]], ids=str)
def test_projection(rng, proj):
    fn, data = rng
    exp, refs = model(data)
    rc, out, dump = pileup(fn, proj=proj)
    assert rc == 0 and columns(dump)[2] == as_dumped(exp, refs, [NAMES[i] for i in proj]), proj


@pytest.mark.gpu
def test_pages(rng):
    fn, data = rng
    exp, refs = model(data)
    # pages shorter than a chunk, and pages that are no multiple of it: the chunks stay full and the rows the same
    for page in ("1000", "3000"):
        rc, out, dump = pileup(fn, env={"DHTS_PILEUP_PAGE_ROWS": page})
        schema, sizes, cols = columns(dump)
        assert rc == 0 and cols == as_dumped(exp, refs) and sizes[:-1] == [2048] * (len(sizes) - 1) and exp["n_rows"] > 3000


@pytest.mark.gpu
def test_region(rng):
    import duckhts_amd
    fn, data = rng
    region = "CHROMOSOME_I:1001-1100,CHROMOSOME_I:901-1000"
    scanned = duckhts_amd.read_bam(data, region=region, index=read_golden("range.bam.bai"))
    refs, _ = M.reads_from_bam(data)
    for named, kw in (([], dict()), ([("include_insertions", "true"), ("distinguish_strands", "false")], dict(include_insertions=1, distinguish_strands=0))):
        exp = M.pileup(M.reads_from_cols(scanned), refs, rows=[(0, 1000, 1100), (0, 900, 1000)], **{**M.DEFAULTS, **kw})
        rc, out, dump = pileup(fn, named=[("region", region)] + named)
        assert rc == 0 and f"rows={exp['n_rows']} " in out, out
        assert columns(dump)[2] == as_dumped(exp, refs)
    rc, out, _ = pileup(fn, named=[("region", "CHROMOSOME_I:1-1000,CHROMOSOME_I:900-1100")])
    assert rc != 0 and M.err_overlap("CHROMOSOME_I:1-1000", "CHROMOSOME_I:900-1100") in out, out


def test_bind_errors_without_a_device():
    rc, out, _ = pileup("")
    assert rc == 3 and out == "ERROR bind: " + M.ERR_PATH
    rc, out, _ = pileup("/no/such/file.bam")
    assert rc == 3 and out == "ERROR bind: Failed to open SAM/BAM/CRAM file: /no/such/file.bam"     # read_bam's own (bam_reader.c:446)
    rc, out, _ = pileup("x.bam", named=[("bogus", "1")])
    assert rc == 3 and "unknown named parameter" in out
    for k in NAMED:
        rc, out, _ = pileup("/no/such/file.bam", named=[(k, "false" if k in BOOLS else "1")])
        assert "unknown named parameter" not in out
    # the parameters are checked in front of the file
    for named, msg in (([("min_mapq", "256")], M.err_range("min_mapq")), ([("min_mapq", "-1")], M.err_range("min_mapq")), ([("min_baseq", "256")], M.err_range("min_baseq")),
                       ([("min_baseq", "-1")], M.err_range("min_baseq")), ([("include_flags", "65536")], M.err_range("include_flags")), ([("require_flags", "-1")], M.err_range("require_flags")),
                       ([("exclude_flags", "65536")], M.err_range("exclude_flags")), ([("min_read_len", "-1")], M.ERR_READ_LEN), ([("min_nucleotide_depth", "0")], M.ERR_MIN_DEPTH),
                       # wrong in two ways: the first in the order of the checks is reported
                       ([("min_read_len", "-1"), ("min_mapq", "256")], M.ERR_READ_LEN), ([("min_baseq", "-1"), ("include_flags", "65536")], M.err_range("min_baseq")),
                       ([("require_flags", "-1"), ("exclude_flags", "70000")], M.err_range("require_flags")),
                       ([("min_nucleotide_depth", "0"), ("exclude_flags", "70000")], M.err_range("exclude_flags"))):
        rc, out, _ = pileup("/no/such/file.bam", named=named)
        assert rc == 3 and out == "ERROR bind: " + msg, out


@pytest.mark.gpu
def test_file_and_region_errors_are_read_bams_own(rng, tmp_path):
    fn, data = rng
    bad = os.path.join(str(tmp_path), "bad.bam")
    open(bad, "wb").write(b"not a bam file at all")
    rc, out, _ = pileup(bad)
    assert rc == 3 and out == "ERROR bind: Failed to read SAM/BAM/CRAM header"
    rc, out, _ = pileup(fn, named=[("region", "nosuch:1-5")])
    assert rc == 3 and out == "ERROR bind: No reads found for region(s): nosuch:1-5"
    noidx = os.path.join(str(tmp_path), "noindex.bam")
    shutil.copy(fn, noidx)
    rc, out, _ = pileup(noidx, named=[("region", "CHROMOSOME_I:1-1000")])
    assert rc == 3 and out == "ERROR bind: Region query requires an index (.bai/.csi/.crai)"
    rc, out, _ = pileup(noidx, named=[("region", "CHROMOSOME_I:1-1000"), ("index_path", fn + ".bai")])
    assert rc == 0 and "rows=" in out, out


def test_registered_last_under_a_variable_of_its_own():
    import duckhts_amd

    def catalog(**kv):
        env = {k: x for k, x in os.environ.items() if not (k.startswith("DHTS_") and k.endswith("_FUNCTIONS"))}
        env.update(kv)
        return subprocess.run([HOST, duckhts_amd.LIB_PATH, "--catalog", "-"], capture_output=True, text=True, env=env).stdout.splitlines()

    default = catalog()
    assert default and not any("bam_pileup" in ln for ln in default)
    # absent under every value of every existing variable
    existing = ("DHTS_SEQ_FUNCTIONS", "DHTS_INTERVAL_FUNCTIONS", "DHTS_NUC_FUNCTIONS", "DHTS_KMER_FUNCTIONS", "DHTS_TABIX_FUNCTIONS", "DHTS_COVERAGE_FUNCTIONS", "DHTS_DEPTH_FUNCTIONS",
                "DHTS_PERBASE_FUNCTIONS")
    for var in existing:
        for v in ("0", "1", "2", "3"):
            assert not any("bam_pileup" in ln for ln in catalog(**{var: v})), (var, v)
    for v in ("0", "2", "true"):
        assert catalog(DHTS_PILEUP_FUNCTIONS=v) == default
    line = ("TF bam_pileup pushdown=1 bind=1 init=1 local_init=0 func=1 named=region:17,index_path:17,min_read_len:5,min_mapq:5,min_baseq:5,include_flags:5,require_flags:5,"
            "exclude_flags:5,include_deletions:1,include_insertions:1,distinguish_strands:1,min_nucleotide_depth:5")
    assert catalog(DHTS_PILEUP_FUNCTIONS="1") == default + [line]
    others = dict(DHTS_PERBASE_FUNCTIONS="1", DHTS_DEPTH_FUNCTIONS="1", DHTS_COVERAGE_FUNCTIONS="2", DHTS_TABIX_FUNCTIONS="1", DHTS_KMER_FUNCTIONS="1")
    both = catalog(DHTS_PILEUP_FUNCTIONS="1", **others)
    assert both[-1] == line and both[:-1] == catalog(**others) and both[-2].startswith("TF bam_depth ")          # bam_depth still last but one
