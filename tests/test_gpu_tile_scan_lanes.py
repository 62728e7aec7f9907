"""bam_tile_scan_lanes (one lane per tile, straight from HBM) against bam_tile_scan (one wave per tile out of LDS) and against the oracle.

(a) dhts_debug_tile_scan runs each kernel alone over the inflated batch: first, end_next, count, err, recs_first and the record list
    must be equal for every tile t >= 1 (tile 0 is the wave kernel's in both runs).  Over the whole file as one batch, and over the
    file's first batch of two BGZF blocks: not the last one, it ends inside a record.
(b) read_bam under DHTS_TILE_SCAN=lanes equals the oracle in all 13 columns and in status, as one batch and with max_blocks 1 and 3,
    and its repair / retry counters (dhts_debug_tile_stats) equal those of a DHTS_TILE_SCAN=wave run: the two kernels hand the repair
    rounds the same table.

Streams: tile_scan_cases.py (the smallest at which the lane kernel can still go wrong), the decoy files of decoy_cases.TILE_CASES and
3,000 synthetic records of 150 bases."""
import functools
import os

import numpy as np
import pytest

import decoy_cases as D
import duckhts_amd
import orc
import tile_scan_cases as T
from duckhts_amd import synth

pytestmark = pytest.mark.gpu

COLS = duckhts_amd.BAM_COLUMNS
CAP = 8 << 20                    # more than any stream here inflates to
TABLES = ("first", "end_next", "count", "err", "recs_first")


@functools.lru_cache(maxsize=None)
def _file(name):
    if name == "synth3000":
        data = synth.bam_file(3000, seed=7)
    elif name.startswith("decoy_"):
        data = D.case("bam", name[6:])["data"]
    else:
        data = T.bam(name)
    return data, orc.bam_read(data)


class _mode:
    """DHTS_TILE_SCAN for the reads inside the block (the library reads it per batch)"""

    def __init__(self, m):
        self.m = m

    def __enter__(self):
        self.old = os.environ.get("DHTS_TILE_SCAN")
        os.environ["DHTS_TILE_SCAN"] = self.m

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("DHTS_TILE_SCAN", None)
        else:
            os.environ["DHTS_TILE_SCAN"] = self.old


def _same(got, exp, ctx):
    assert got["n_rows"] == exp["n_rows"], f"{ctx}: rows {got['n_rows']} != {exp['n_rows']}"
    assert (got["status"] < 0) == (exp["status"] < 0), f"{ctx}: status {got['status']} vs {exp['status']}"
    for k in COLS:
        a, b = got[k], exp[k]
        if isinstance(b, np.ndarray):
            assert np.array_equal(np.asarray(a), b), f"{ctx}: column {k} differs"
        else:
            assert list(a) == list(b), f"{ctx}: column {k} differs"


def _tables(name, max_blocks):
    """both kernels alone over the file's first batch of max_blocks blocks (0: the whole file)"""
    data, _ = _file(name)
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(data); ctx.bgzf_index(); ctx.bam_open()
        ctx.next_batch(max_blocks)                            # the context now holds the batch's inflated stream, whatever the batch's status
        return ctx.debug_tile_scan("wave", CAP), ctx.debug_tile_scan("lanes", CAP)
    finally:
        ctx.close()


def _equal_tables(name, w, l):
    nt = len(w["first"])
    assert len(l["first"]) == nt
    for k in TABLES:
        d = np.nonzero(w[k][1:] != l[k][1:])[0]
        assert d.size == 0, f"{name}: {k} differs at tile {int(d[0]) + 1}: wave {w[k][1 + int(d[0])]} lanes {l[k][1 + int(d[0])]}"
    d = np.nonzero((w["recs"][1:] != l["recs"][1:]).any(axis=1))[0]
    assert d.size == 0, f"{name}: the record list differs at tile {int(d[0]) + 1}"
    return nt


NONFINAL_SEEN = set()


def _check(name):
    w, l = _tables(name, 0)
    nt = _equal_tables(name, w, l)
    # a non-final batch: the first two blocks of a file that has more (18,000 bytes, three tiles, the last record incomplete; the synthetic
    # and the decoy files have blocks of 65,280 bytes and many of them)
    if name in T.names() and len(T.stream(name)) <= 2 * T.PAYLOAD:
        pass                                                  # (the streams of one tile or two: two blocks are the whole file)
    else:
        assert _equal_tables(name + " (first two blocks)", *_tables(name, 2)) >= 3
        NONFINAL_SEEN.add(name)
    _, exp = _file(name)
    stats = {}
    for mode in ("wave", "lanes"):
        with _mode(mode):
            for mb in (0, 1, 3):
                st = {}
                _same(duckhts_amd.read_bam(_file(name)[0], max_blocks=mb, stats=st), exp, f"{name}/{mode}/max_blocks {mb}")
                stats[(mode, mb)] = st
    for mb in (0, 1, 3):
        assert stats[("lanes", mb)] == stats[("wave", mb)], (name, mb, stats[("lanes", mb)], stats[("wave", mb)])
    return w, nt


def test_synthetic_records():
    w, nt = _check("synth3000")
    assert nt >= 100 and int(w["count"][1:].sum()) > 2500


@pytest.mark.parametrize("name", D.TILE_CASES)
def test_decoy_files(name):
    w, nt = _check("decoy_" + name)
    if name.startswith("every_tile"):
        c = D.case("bam", name)
        true = set(c["starts"])
        assert sum(1 for t in range(1, nt) if int(w["first"][t]) not in true) >= 1            # the files do mis-speculate, in both kernels alike


def test_long_records_and_a_block_size_word_across_a_tile_boundary():
    w, nt = _check("long40k")
    assert int((w["first"][1:] == np.uint64(0xffffffffffffffff)).sum()) >= 4              # tiles inside the long record
    for k in range(4):
        w, nt = _check("straddle%d" % k)
        if k:                                                                              # the straddling record starts in tile 1: its last one
            assert int(w["recs"][1][int(w["count"][1]) - 1]) == T.TILE - k
        else:
            assert int(w["end_next"][1]) == 2 * T.TILE


def test_shortest_records():
    w, nt = _check("dense")
    assert all(int(c) > 200 for c in w["count"][1:nt - 1])
    w, nt = _check("dense_and_one")
    assert int(w["count"][1]) > 64 and int(w["count"][2]) == 1


@pytest.mark.parametrize("j", (1, 2, 3))
def test_stream_ends_next_to_a_tile_boundary(j):
    for d in T.END_D:
        _check("end_%d_%d" % (j, d))


@pytest.mark.parametrize("j", (1, 2, 3))
def test_truncated_files_of_the_same_lengths(j):
    for d in T.END_D:
        name = "cut_%d_%d" % (j, d)
        assert _file(name)[1]["status"] < 0
        _check(name)


@pytest.mark.parametrize("name", ("bs31", "bs_minus1", "runs_past"))
def test_damaged_block_size(name):
    assert _file(name)[1]["status"] < 0
    w, nt = _check(name)
    assert int(w["err"][1:].sum()) >= 1
    assert name in NONFINAL_SEEN


def test_a_block_size_that_runs_past_the_stream_in_a_non_final_batch():
    """the damaged record (it claims a megabyte) cut by the end of a batch that is not the file's last: incomplete, not an error, in both kernels"""
    data, _ = _file("runs_past")
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(data); ctx.bgzf_index(); ctx.bam_open()
        b = ctx.next_batch(3)                                 # 27,000 of the stream's 27,170 bytes: the damaged last record begins inside
        assert b.status == 0
        w, l = ctx.debug_tile_scan("wave", CAP), ctx.debug_tile_scan("lanes", CAP)
    finally:
        ctx.close()
    assert _equal_tables("runs_past, three blocks", w, l) == 4
    assert int(l["err"][1:].sum()) == 0 and int(l["end_next"][3]) == sum(len(r) for r in T.case("runs_past")["recs"][:-1])


@pytest.mark.parametrize("name", ("near_nul", "near_aux"))
def test_candidates_that_pass_the_prefilter_and_fail_one_later_test(name):
    w, nt = _check(name)
    starts, o = set(), 0
    for r in T.case(name)["recs"]:
        starts.add(o); o += len(r)
    assert int(w["first"][1]) in starts and int(w["first"][1]) > T.TILE + 845           # behind the candidate, which lies at 8,192 + 845
