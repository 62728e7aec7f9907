"""register_kmer_udf_functions as a DuckDB host sees it (tests/scalarhost.py, tests/minihost): what is registered, with which types, in
which order, only behind DHTS_KMER_FUNCTIONS=1; and the error of a call without a device.  No GPU needed."""
import os
import subprocess

import pytest

import duckhts_amd
import kmer_udf_ref as ref
import scalarhost
from conftest import ROOT

MINIHOST = os.path.join(ROOT, "tests", "minihost", "minihost")
DEFAULT = ["read_bcf", "read_bam", "bgzip", "bgunzip", "bam_index", "bcf_index", "tabix_index"]
NO_DEVICE = "{}: no MI355X (gfx950) device available; this build has no CPU fallback"


@pytest.fixture(scope="module")
def host():
    return scalarhost.load({"DHTS_KMER_FUNCTIONS": "1"})


def test_names_types_and_order_are_the_reference_registrations(host):
    """src/kmer_udf.c:1224-1253: 29 scalar functions and the table function seq_kmers, 30 registrations"""
    cat = host.catalog()
    assert [c[0] for c in cat[:len(DEFAULT)]] == DEFAULT and not host.unimplemented
    got = cat[len(DEFAULT):]
    assert len(got) == len(ref.REGISTERED) == 30
    for (name, params, ret), (rname, rparams, rret) in zip(got, ref.REGISTERED):
        assert name == rname and params == rparams, (name, params, rname, rparams)
        if name == "seq_kmers":
            assert ret == {"canonical": "BOOLEAN"} and host.function(name).kind == "table"
        else:
            assert ret == rret and host.function(name).kind == "scalar", (name, ret, rret)
    assert got[15][2] == "STRUCT(" + ", ".join(f + " BOOLEAN" for f in ref.FLAG_FIELDS) + ")"


def test_nothing_new_is_registered_without_the_variable():
    assert [c[0] for c in scalarhost.load().catalog()] == DEFAULT
    for other in ("DHTS_SEQ_FUNCTIONS", "DHTS_INTERVAL_FUNCTIONS", "DHTS_NUC_FUNCTIONS", "DHTS_TABIX_FUNCTIONS"):
        names = [c[0] for c in scalarhost.load({other: "1"}).catalog()]
        assert "seq_kmers" not in names and "seq_revcomp" not in names, other
    both = [c[0] for c in scalarhost.load({"DHTS_KMER_FUNCTIONS": "1", "DHTS_TABIX_FUNCTIONS": "1", "DHTS_NUC_FUNCTIONS": "1"}).catalog()]
    assert both[len(DEFAULT)] == "fasta_nuc" and both[len(DEFAULT) + 1] == "seq_revcomp" and both[-3:] == ["read_tabix", "read_gtf", "read_gff"]      # src/duckhts.c:60-69


def test_a_host_without_scalar_slots_gets_seq_kmers_only():
    """tests/minihost leaves the scalar-function slots NULL: the scalar functions are skipped, seq_kmers is listed, the process exits cleanly"""
    env = {k: v for k, v in os.environ.items() if not (k.startswith("DHTS_") and k.endswith("_FUNCTIONS"))}
    off = subprocess.run([MINIHOST, duckhts_amd.LIB_PATH, "--catalog", "-"], capture_output=True, text=True, env=env)
    on = subprocess.run([MINIHOST, duckhts_amd.LIB_PATH, "--catalog", "-"], capture_output=True, text=True, env=dict(env, DHTS_KMER_FUNCTIONS="1"))
    assert off.returncode == 0 and on.returncode == 0, (on.stderr, off.stderr)
    assert [ln.split()[1] for ln in off.stdout.splitlines()] == DEFAULT
    lines = on.stdout.splitlines()
    assert lines[:len(DEFAULT)] == off.stdout.splitlines()
    assert lines[len(DEFAULT):] == ["TF seq_kmers pushdown=0 bind=1 init=1 local_init=0 func=1 named=canonical:1"]


def test_seq_kmers_bind_errors_are_the_reference_strings(host):
    for params, msg in (((None, 3), "seq_kmers: sequence must not be NULL"), (("ACGT", None), "seq_kmers: k must not be NULL"),
                        (("ACGT", 0), "seq_kmers: k must be > 0"), (("ACGT", -1), "seq_kmers: k must be > 0")):
        with pytest.raises(scalarhost.HostError) as e:
            host.table_function("seq_kmers", *params)
        assert str(e.value) == msg


def test_without_a_device_every_call_fails_with_the_no_device_error(host):
    if duckhts_amd.lib().dhts_device_count() != 0:
        return                                                    # (with a device the calls succeed: tests/test_duckdb_kmer_udf.py)
    samples = {"VARCHAR": "ACGT", "UTINYINT[]": [1, 2], "USMALLINT": 1, "BIGINT": 1}
    for name, params, _ in ref.REGISTERED:
        if name == "seq_kmers":
            continue
        with pytest.raises(scalarhost.HostError) as e:
            host.call(name, *[[samples[p], None] for p in params])
        assert str(e.value) == NO_DEVICE.format(name)
    with pytest.raises(scalarhost.HostError) as e:
        host.table_function("seq_kmers", "ACGTA", 3)
    assert str(e.value) == NO_DEVICE.format("seq_kmers")
