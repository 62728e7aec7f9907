"""read_fasta and fasta_index through the DuckDB surface (tests/minihost, DHTS_SEQ_FUNCTIONS=1): the reference's own statements on a file
of the shape of its test/data/ce.fa (test/sql/duckhts.test:198-235) and its error strings (src/seq_reader.c)."""
import os
import subprocess

import pytest

import bamwriter as W
import fasta_index_ref as R
from test_duckdb_surface import HOST, parse_chunks, run_host

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "htslib_faidx")
ON = {"DHTS_SEQ_FUNCTIONS": "1"}
NAME, DESCRIPTION, SEQUENCE = range(3)


@pytest.fixture(scope="module")
def ce_text():
    return R.ce_shaped()


def _ce(tmp_path, text, name="ce.fa"):
    fn = os.path.join(str(tmp_path), name)
    open(fn, "wb").write(text)
    return fn


def _col(chunks, k):
    return [x for _n, cols in chunks for x in cols[k][2]]


def _rows(dump):
    schema, chunks = parse_chunks(dump)
    return schema, chunks, sum(n for n, _ in chunks)


@pytest.mark.gpu
def test_read_fasta_whole_file(tmp_path, ce_text):
    fa = _ce(tmp_path, ce_text)
    rc, out, dump = run_host(fa, fn="read_fasta", env=ON)
    assert rc == 0, out
    schema, chunks, n = _rows(dump)
    assert [s[0] for s in schema] == ["NAME", "DESCRIPTION", "SEQUENCE"] and n == 7                       # duckhts.test:198-201
    assert _col(chunks, NAME)[0] == b"CHROMOSOME_I"                                                      # duckhts.test:204-207
    assert [(nm, len(s)) for nm, s in zip(_col(chunks, NAME), _col(chunks, SEQUENCE))][:3] == \
        [(b"CHROMOSOME_I", 1009800), (b"CHROMOSOME_II", 5000), (b"CHROMOSOME_III", 5000)]                # duckhts.test:210-215
    assert _col(chunks, SEQUENCE)[1] == ce_text[1030025:1030025 + 5100].replace(b"\n", b"")
    assert _col(chunks, DESCRIPTION) == [None] * 7


@pytest.mark.gpu
def test_fasta_index_then_regions(tmp_path, ce_text):
    fa = _ce(tmp_path, ce_text)
    # a region query without a .fai: the reference's error, and no index is built on the side
    rc, out, _ = run_host(fa, named=[("region", "CHROMOSOME_I:1-10")], fn="read_fasta", env=ON)
    assert rc != 0 and "read_fasta: region query requires a FASTA index (.fai); run fasta_index(path) first" in out, out
    assert not os.path.exists(fa + ".fai")
    rc, out, dump = run_host(fa, fn="fasta_index", env=ON)                                              # duckhts.test:232-235
    assert rc == 0, out
    schema, chunks, n = _rows(dump)
    assert [s[0] for s in schema] == ["success", "index_path"] and n == 1
    assert int(_col(chunks, 0)[0]) == 1 and _col(chunks, 1) == [b""]
    assert open(fa + ".fai", "rb").read() == open(os.path.join(GOLD, "ce.fa.fai"), "rb").read()
    assert not os.path.exists(fa + ".gzi") and sorted(os.listdir(str(tmp_path))) == ["ce.fa", "ce.fa.fai"]
    rc, out, dump = run_host(fa, named=[("region", "CHROMOSOME_I:1-10")], fn="read_fasta", env=ON)      # duckhts.test:218-222
    assert rc == 0, out
    _, chunks, n = _rows(dump)
    assert n == 1 and _col(chunks, NAME) == [b"CHROMOSOME_I"] and _col(chunks, SEQUENCE) == [ce_text[14:24]] and _col(chunks, DESCRIPTION) == [None]
    rc, out, dump = run_host(fa, named=[("region", "CHROMOSOME_I:1-10,CHROMOSOME_II:1-5")], fn="read_fasta", env=ON)   # duckhts.test:225-229
    assert rc == 0, out
    _, chunks, n = _rows(dump)
    assert n == 2 and _col(chunks, SEQUENCE) == [ce_text[14:24], ce_text[1030025:1030030]]
    rc, out, _ = run_host(fa, named=[("region", "CHROMOSOME_I:1-10,nope:1-5")], fn="read_fasta", env=ON)
    assert rc != 0 and "read_fasta: invalid or missing region 'nope:1-5'" in out, out


@pytest.mark.gpu
def test_index_path_projection_and_bgzf(tmp_path, ce_text):
    fa = _ce(tmp_path, W.bgzf_file(ce_text), "ce.fa.gz")
    idx = os.path.join(str(tmp_path), "elsewhere.fai")
    rc, out, dump = run_host(fa, named=[("index_path", idx)], fn="fasta_index", env=ON)
    assert rc == 0, out
    _, chunks, _n = _rows(dump)
    assert _col(chunks, 1) == [idx.encode()]
    assert open(idx, "rb").read() == open(os.path.join(GOLD, "ce.fa.fai"), "rb").read() and not os.path.exists(fa + ".fai")
    assert open(fa + ".gzi", "rb").read() == R.gzi(*R.bgzf_blocks(open(fa, "rb").read()))
    rc, out, _ = run_host(fa, named=[("region", "CHROMOSOME_V:11-20")], fn="read_fasta", env=ON)         # <path>.fai is not there
    assert rc != 0 and "read_fasta: region query requires a FASTA index (.fai)" in out, out
    rc, out, dump = run_host(fa, named=[("region", " CHROMOSOME_V:11-20 ,, CHROMOSOME_X"), ("index_path", idx)], proj=[SEQUENCE], fn="read_fasta", env=ON)
    assert rc == 0, out
    _, chunks, n = _rows(dump)
    _, tab = R.read(open(idx, "rb").read())
    assert n == 2 and _col(chunks, 0) == [R.fetch(ce_text, tab, b"CHROMOSOME_V:11-20"), R.fetch(ce_text, tab, b"CHROMOSOME_X")]
    rc, out, dump = run_host(fa, proj=[SEQUENCE], fn="read_fasta", env=ON)                              # SEQUENCE alone, whole file
    assert rc == 0, out
    _, chunks, n = _rows(dump)
    assert n == 7 and [len(s) for s in _col(chunks, 0)] == [ln for _nm, ln in R.CE_NAMES]


@pytest.mark.gpu
def test_header_comment_and_failed_index(tmp_path):
    """DESCRIPTION is the CO tag of the record, which htslib's FASTA reader makes only under its fastq_aux option; the reference never
    sets it, so a header comment leaves DESCRIPTION NULL and NAME without the comment"""
    fa = _ce(tmp_path, b">one first sequence\nACGTAC\nAC\n>three x=1\nGG\n", "c.fa")
    rc, out, dump = run_host(fa, fn="read_fasta", env=ON)
    assert rc == 0, out
    _, chunks, n = _rows(dump)
    assert n == 2 and _col(chunks, NAME) == [b"one", b"three"] and _col(chunks, SEQUENCE) == [b"ACGTACAC", b"GG"]
    assert _col(chunks, DESCRIPTION) == [None] * 2
    bad = _ce(tmp_path, b">a\nACGT\nACGTAA\n", "bad.fa")
    rc, out, _ = run_host(bad, fn="fasta_index", env=ON)
    assert rc != 0 and "fasta_index: failed to build index for " + bad in out, out
    assert sorted(os.listdir(str(tmp_path))) == ["bad.fa", "c.fa"]                                     # no partial file behind the error


def test_bind_errors_without_a_device():
    rc, out, _ = run_host("", fn="read_fasta", env=ON)
    assert rc == 3 and out == "ERROR bind: read_fasta requires a file path"
    rc, out, _ = run_host("", fn="fasta_index", env=ON)
    assert rc == 3 and out == "ERROR bind: fasta_index requires a file path"
    rc, out, _ = run_host("/no/such/file.fa", fn="read_fasta", env=ON)
    assert rc == 3 and out == "ERROR bind: Failed to open file: /no/such/file.fa"


@pytest.mark.parametrize("fn", ["read_fasta", "fasta_index"])
def test_not_registered_by_default(fn):
    import duckhts_amd
    env = {k: v for k, v in os.environ.items() if k != "DHTS_SEQ_FUNCTIONS"}
    r = subprocess.run([HOST, duckhts_amd.LIB_PATH, fn, ""], capture_output=True, text=True, env=env)
    assert r.returncode != 0 and "requires a file path" not in r.stdout, r.stdout
