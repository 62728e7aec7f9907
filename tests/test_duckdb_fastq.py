"""FASTQ through the DuckDB surface (tests/minihost): read_bam on a FASTQ file, and the opt-in read_fastq table function against the
reference's own expectations (test/sql/duckhts.test:320-387) and error strings (src/seq_reader.c)."""
import os
import shutil

import pytest

from test_duckdb_surface import parse_chunks, run_host

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "htslib_fastq")
ON = {"DHTS_SEQ_FUNCTIONS": "1"}
NAME, DESCRIPTION, SEQUENCE, QUALITY, MATE, PAIR_ID = range(6)


def _fq(tmp_path, name):
    fn = os.path.join(str(tmp_path), name)
    shutil.copy(os.path.join(GOLD, name), fn)
    return fn


def _col(chunks, k):
    return [x for _n, cols in chunks for x in cols[k][2]]


def _rows(dump):
    schema, chunks = parse_chunks(dump)
    return schema, chunks, sum(n for n, _ in chunks)


@pytest.mark.gpu
def test_read_bam_on_r1_fq(tmp_path):
    rc, out, dump = run_host(_fq(tmp_path, "r1.fq"), proj=[0, 1, 2, 3, 5, 9, 10])
    assert rc == 0, out
    _, chunks, n = _rows(dump)
    exp = [l.split("\t") for l in open(os.path.join(GOLD, "r1.sam")).read().split("\n") if l and not l.startswith("@")]
    assert n == 5
    assert [x.decode() for x in _col(chunks, 0)] == [e[0] for e in exp] and [int(x) for x in _col(chunks, 1)] == [int(e[1]) for e in exp]
    assert _col(chunks, 2) == [b"*"] * 5 and [int(x) for x in _col(chunks, 3)] == [0] * 5 and _col(chunks, 4) == [b"*"] * 5
    assert [x.decode() for x in _col(chunks, 5)] == [e[9] for e in exp] and [x.decode() for x in _col(chunks, 6)] == [e[10] for e in exp]


@pytest.mark.gpu
def test_read_fastq_counts_and_first_row(tmp_path):
    r1 = _fq(tmp_path, "r1.fq")
    rc, out, dump = run_host(r1, fn="read_fastq", env=ON)
    assert rc == 0, out
    schema, chunks, n = _rows(dump)
    assert [s[0] for s in schema] == ["NAME", "DESCRIPTION", "SEQUENCE", "QUALITY"] and n == 5          # duckhts.test:325-328
    assert _col(chunks, NAME)[0] == b"HS25_09827:2:1201:1505:59795#49"                                  # duckhts.test:330-334
    assert len(_col(chunks, SEQUENCE)[0]) == 100 and len(_col(chunks, QUALITY)[0]) == 100
    assert _col(chunks, DESCRIPTION) == [None] * 5


@pytest.mark.gpu
def test_read_fastq_mate_path(tmp_path):
    r1, r2 = _fq(tmp_path, "r1.fq"), _fq(tmp_path, "r2.fq")
    rc, out, dump = run_host(r1, named=[("mate_path", r2)], fn="read_fastq", env=ON)
    assert rc == 0, out
    schema, chunks, n = _rows(dump)
    assert [s[0] for s in schema] == ["NAME", "DESCRIPTION", "SEQUENCE", "QUALITY", "MATE", "PAIR_ID"] and n == 10   # duckhts.test:337-340
    mate = [int(x) for x in _col(chunks, MATE)]
    assert mate.count(1) == 5 and mate.count(2) == 5 and mate == [1, 2] * 5                             # duckhts.test:342-350
    assert len(set(_col(chunks, PAIR_ID))) == 5                                                         # duckhts.test:352-355


@pytest.mark.gpu
def test_read_fastq_interleaved(tmp_path):
    rc, out, dump = run_host(_fq(tmp_path, "interleaved.fq"), named=[("interleaved", "true")], fn="read_fastq", env=ON)
    assert rc == 0, out
    _, chunks, n = _rows(dump)
    mate = [int(x) for x in _col(chunks, MATE)]
    assert n == 10 and mate.count(1) == 5 and mate.count(2) == 5 and len(set(_col(chunks, PAIR_ID))) == 5   # duckhts.test:364-382


@pytest.mark.gpu
def test_read_fastq_error_strings(tmp_path):
    m1, m2, odd = _fq(tmp_path, "mate_mismatch_r1.fq"), _fq(tmp_path, "mate_mismatch_r2.fq"), _fq(tmp_path, "odd_interleaved.fq")
    rc, out, _ = run_host(m1, named=[("mate_path", m2)], fn="read_fastq", env=ON)
    assert rc != 0 and "read_fastq: mate files out of sync (QNAME mismatch: 'readA' vs 'readB')" in out, out   # duckhts.test:358-361
    rc, out, _ = run_host(m1, named=[("mate_path", m2)], proj=[SEQUENCE], fn="read_fastq", env=ON)      # NAME is not projected
    assert rc != 0 and "read_fastq: mate files out of sync (QNAME mismatch: 'readA' vs 'readB')" in out, out
    rc, out, _ = run_host(odd, named=[("interleaved", "true")], fn="read_fastq", env=ON)
    assert rc != 0 and "read_fastq: interleaved file has an unpaired record" in out, out                # duckhts.test:385-388
    short = os.path.join(str(tmp_path), "r1_short.fq")                                                  # the first two of r1's five records
    open(short, "wb").write(b"".join(open(os.path.join(GOLD, "r1.fq"), "rb").read().splitlines(True)[:8]))
    rc, out, _ = run_host(_fq(tmp_path, "r1.fq"), named=[("mate_path", short)], fn="read_fastq", env=ON)
    assert rc != 0 and "read_fastq: mate files have different record counts" in out, out
    rc, out, _ = run_host(m1, named=[("mate_path", m2), ("interleaved", "true")], fn="read_fastq", env=ON)
    assert rc != 0 and "read_fastq: use mate_path or interleaved, not both" in out, out


def test_read_fastq_bind_errors_without_a_device():
    rc, out, _ = run_host("", fn="read_fastq", env=ON)
    assert rc == 3 and out == "ERROR bind: read_fastq requires a file path"
    rc, out, _ = run_host("/no/such/file.fq", fn="read_fastq", env=ON)
    assert rc == 3 and out == "ERROR bind: Failed to open file: /no/such/file.fq"


def test_read_fastq_is_not_registered_by_default():
    env = {k: v for k, v in os.environ.items() if k != "DHTS_SEQ_FUNCTIONS"}
    import subprocess
    import duckhts_amd
    from test_duckdb_surface import HOST
    r = subprocess.run([HOST, duckhts_amd.LIB_PATH, "read_fastq", "/no/such/file.fq"], capture_output=True, text=True, env=env)
    assert r.returncode != 0 and "Failed to open file" not in r.stdout and "read_fastq requires" not in r.stdout, r.stdout
