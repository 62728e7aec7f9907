"""The record stage on files built to mis-speculate (decoy_cases.py): every column against the oracle, and -- through dhts_debug_tile_stats --
proof that the repair rounds, the sequential fallback, the retries of a speculated shard start and the validate-rows pass were taken.

The files are valid; the model (tile_spec_ref.py, pinned by test_tile_spec_ref.py) says which tiles the scan guesses wrong."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import decoy_cases as D
import duckhts_amd
import orc
import tile_spec_ref as M
from conftest import ROOT

pytestmark = pytest.mark.gpu

KINDS = ("bam", "bcf")
COLS = duckhts_amd.BAM_COLUMNS
ZERO = {k: 0 for k in duckhts_amd.Context.TILE_STATS}


@functools.lru_cache(maxsize=None)
def _exp(kind, name):
    c = D.case(kind, name)
    exp = orc.bam_read(c["data"]) if kind == "bam" else orc.bcf_read(c["data"])
    assert exp["n_rows"] == len(c["starts"]) and (exp["status"] >= 0 if kind == "bam" else exp["status"] == 0)
    return exp


@functools.lru_cache(maxsize=None)
def _mis(kind, name):
    c = D.case(kind, name)
    return M.mis_count(M.tile_table(c["rule"], c["stream"], 0, c["starts"], start0=c["first"]))


def assert_same(got, exp, ctx=""):
    assert got["n_rows"] == exp["n_rows"], f"{ctx}: rows {got['n_rows']} != {exp['n_rows']}"
    assert (got["status"] < 0) == (exp["status"] < 0), f"{ctx}: status {got['status']} vs {exp['status']}"
    for k in COLS:
        a, b = got[k], exp[k]
        if isinstance(b, np.ndarray):
            assert np.array_equal(np.asarray(a), b), f"{ctx}: column {k} differs"
        elif list(a) != list(b):
            for i, (x, y) in enumerate(zip(a, b)):
                assert x == y, f"{ctx}: column {k} row {i}: {x!r} != {y!r}"
            raise AssertionError(f"{ctx}: column {k} length differs")


def _read(kind, name, ctx="", **kw):
    """one scan of the case with the given options, compared with the oracle; returns the hook's counters"""
    data, exp, stats = D.case(kind, name)["data"], _exp(kind, name), {}
    if kind == "bam":
        assert_same(duckhts_amd.read_bam(data, stats=stats, **kw), exp, f"{name}/{ctx}")
    else:
        got = duckhts_amd.read_bcf(data, stats=stats, **kw)
        d = orc.bcf_cols_diff(exp, got)
        assert d is None, (name, ctx, d)
        assert got["status"] == 1, (name, ctx, got["status"])
    return stats


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", D.TILE_CASES)
def test_tile_cases(kind, name):
    """whole file in one batch (tiles count from the stream's first byte, as in the model), then in batches of 1 and 3 blocks"""
    st = _read(kind, name, "one batch")
    mis = _mis(kind, name)
    print(f"{kind}/{name}: model mis-speculated {mis}; one batch {st}")
    assert st["repaired_tiles"] >= mis
    assert st["spec_retries"] == st["validate_rejections"] == st["gave_up"] == 0          # (no shard starts mid-stream here)
    if name == "control":
        assert st == ZERO
    else:
        assert st["repair_rounds"] >= 1
    if name.startswith("every_tile"):
        assert st["repair_rounds"] > 256 and st["fallback_batches"] >= 1
    for mb in (1, 3):
        st = _read(kind, name, f"mb{mb}", max_blocks=mb)
        print(f"{kind}/{name}: max_blocks {mb} {st}")         # (a batch's short last tile may hold no record start: a repair round marks it "inside a record")


NO_STRINGS = {"FLAG": 1, "POS": 3, "MAPQ": 4, "PNEXT": 7, "TLEN": 8}


@pytest.mark.parametrize("name", D.TILE_CASES)
def test_bam_tile_cases_projected_without_the_string_columns(name):
    """a projection without QNAME / CIGAR / SEQ / QUAL / READ_GROUP_ID skips the string pass; the repaired tile table must serve the rest alike"""
    data, exp = D.case("bam", name)["data"], _exp("bam", name)
    mask = sum(1 << b for b in NO_STRINGS.values())
    for mb in (0, 3):
        ctx = duckhts_amd.Context(0)
        try:
            ctx.open(data); ctx.bgzf_index(); ctx.bam_open()
            row = 0
            while True:
                b = ctx.next_batch(mb, colmask=mask)
                n = int(b.n_rows)
                if n:
                    for c, (ptr, dt) in {"FLAG": (b.flag, np.uint16), "POS": (b.pos, np.int64), "MAPQ": (b.mapq, np.int32), "PNEXT": (b.pnext, np.int64),
                                         "TLEN": (b.tlen, np.int64)}.items():
                        assert ctx.d2h(ptr, n, dt).tolist() == [int(x) for x in exp[c][row:row + n]], (name, mb, c, row)
                row += n
                if b.status != 0:
                    assert b.status == 1
                    break
            assert row == exp["n_rows"]
            if mb == 0 and name != "control":
                assert ctx.debug_tile_stats()["repaired_tiles"] >= _mis("bam", name)
        finally:
            ctx.close()


def test_bam_cases_with_the_fused_row_pass_in_a_child_process():
    """DHTS_ROWS=fused is read once per process: a child reads every BAM decoy file with bam_tile_rows (its "re-walked by a repair round" branch)"""
    code = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import duckhts_amd, orc
import decoy_cases as D
for name in D.TILE_CASES:
    d = D.case("bam", name)["data"]
    exp = orc.bam_read(d)
    for mb in (0, 3):
        st = {}
        got = duckhts_amd.read_bam(d, max_blocks=mb, stats=st)
        assert got["n_rows"] == exp["n_rows"] and got["status"] == 1, (name, mb, got["n_rows"], exp["n_rows"], got["status"])
        for k in duckhts_amd.BAM_COLUMNS:
            assert list(got[k]) == list(exp[k]), (name, mb, k)
        print(name, mb, st)
        assert (st["repaired_tiles"] > 0) == (name != "control"), (name, st)
print("fused decoys ok")
""" % (ROOT, ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, DHTS_ROWS="fused"), timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "fused decoys ok" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])


def _two_shards(kind, name):
    """shard 0 = blocks [0, b) from the known first record, shard 1 = [b, end) with a speculated start; returns the parts and shard 1's counters"""
    c = D.case(kind, name)
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(c["data"])
        nb = ctx.bgzf_index()
    finally:
        ctx.close()
    b, st = c["block"], {}
    read = duckhts_amd.read_bam if kind == "bam" else duckhts_amd.read_bcf
    p0 = read(c["data"], block_range=(0, b, False))
    p1 = read(c["data"], block_range=(b, nb, True), stats=st)
    return c, p0, p1, st


def _check_shards(kind, name, p0, p1):
    c, exp = D.case(kind, name), _exp(kind, name)
    assert p0["status"] == 1 and p1["status"] == 1, (p0["status"], p1["status"])
    assert p0["n_rows"] == D.SHARD_AT + 1 and p0["n_rows"] + p1["n_rows"] == exp["n_rows"], (p0["n_rows"], p1["n_rows"], exp["n_rows"])
    assert p0["end_uoff"] == p1["first_rec_uoff"] == c["starts"][D.SHARD_AT + 1], (p0["end_uoff"], p1["first_rec_uoff"])
    if kind == "bam":
        cat = {"n_rows": p0["n_rows"] + p1["n_rows"], "status": 1}
        for k in COLS:
            cat[k] = np.concatenate([p0[k], p1[k]]) if isinstance(exp[k], np.ndarray) else list(p0[k]) + list(p1[k])
        assert_same(cat, exp, name)
    else:
        for part, rows in ((p0, range(0, p0["n_rows"])), (p1, range(p0["n_rows"], exp["n_rows"]))):
            d = orc.bcf_cols_diff(orc.bcf_take_rows(exp, list(rows)), part)
            assert d is None, (name, d)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", D.SHARD_KS)
def test_shard_start_behind_k_decoy_chains(kind, k):
    """a valid file reads like the oracle however many decoys precede the shard's first record: one retry per chain, never a give-up"""
    name = "shard_start_%d" % k
    c, p0, p1, st = _two_shards(kind, name)
    print(f"{kind}/{name}: {st}")
    _check_shards(kind, name, p0, p1)
    assert st["spec_retries"] == k and st["gave_up"] == 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name, chains", [("shard_start_links4", 1), ("shard_start_links20", 1), ("shard_start_2x_links20", 2)])
def test_shard_start_behind_long_decoy_chains(kind, name, chains):
    """chains of 4 and of 20 decoys: several offsets of one chain pass the filter and break at the same stop word.  The retries pass over
    the members of a failed chain, so a chain costs one retry however long it is, and the search never gives up on a valid file"""
    c, p0, p1, st = _two_shards(kind, name)
    print(f"{kind}/{name}: {st}")
    _check_shards(kind, name, p0, p1)
    cands, _ = M.shard_candidates(c["rule"], c["stream"], c["cut"], c["starts"])
    assert st["spec_retries"] == len(cands) == chains and st["gave_up"] == 0


@pytest.mark.parametrize("kind", KINDS)
def test_shard_start_behind_a_rejoining_decoy(kind):
    """the fake record ends exactly where the cut record ends: its chain holds to the end of the batch and only the full validation of its
    "records" (bam_validate_rows / bcf_rec_check) can refuse it"""
    c, p0, p1, st = _two_shards(kind, "shard_start_rejoin")
    print(f"{kind}/shard_start_rejoin: {st}")
    _check_shards(kind, "shard_start_rejoin", p0, p1)
    assert st["validate_rejections"] >= 1 and st["spec_retries"] == 1 and st["gave_up"] == 0


@pytest.mark.parametrize("kind", KINDS)
def test_shard_start_with_the_candidates_behind_the_first_tile(kind):
    """the record cut by the shard boundary runs across the batch's first tile: tile 0 holds no record, and its candidates (two decoy chains,
    then the true record) lie in the second tile"""
    c, p0, p1, st = _two_shards(kind, "shard_start_far")
    print(f"{kind}/shard_start_far: {st}")
    _check_shards(kind, "shard_start_far", p0, p1)
    assert st["spec_retries"] == 2 and st["gave_up"] == 0


def test_damaged_speculative_shard_gives_up_after_few_retries():
    """the input of test_damaged_block_in_the_first_batch_of_a_speculative_shard (test_gpu_bam.py): a really damaged shard must not retry once
    per record -- every candidate on its true chain breaks at the damage, so the search stops when two in a row break at the same place"""
    data = bytearray(cases.case_basic(payload=777, n=3000, seed=12))
    p, blocks = 0, []
    while p + 18 <= len(data):
        bl = (data[p + 16] | (data[p + 17] << 8)) + 1
        blocks.append((p, bl)); p += bl
    nb = len(blocks)
    for k in (nb * 5 // 8, nb // 2 + 1):
        d = bytearray(data)
        o, bl = blocks[k]
        d[o + 18 + (bl - 26) // 2] ^= 0x55
        d = bytes(d)
        exp = orc.bam_read(d)
        st = {}
        p0 = duckhts_amd.read_bam(d, block_range=(0, nb // 2, False))
        p1 = duckhts_amd.read_bam(d, block_range=(nb // 2, nb, True), stats=st)
        print(f"damaged block {k}: {st}")
        assert p0["status"] == 1 and p1["status"] < 0
        assert list(p0["QNAME"]) + list(p1["QNAME"]) == list(exp["QNAME"])
        assert st["spec_retries"] <= 17 and st["gave_up"] == 1
