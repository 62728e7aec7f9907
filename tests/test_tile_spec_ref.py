"""The speculation model (tile_spec_ref.py) on the decoy files (decoy_cases.py): every file is valid for the oracle, and the model confirms
that it mis-speculates where its case says.  These are conditions on the INPUTS; what the device makes of them is test_gpu_record_decoys.py."""
import pytest

import decoy_cases as D
import orc
import tile_spec_ref as M
from tile_spec_ref import TILE

KINDS = ("bam", "bcf")


def _table(c):
    return M.tile_table(c["rule"], c["stream"], 0, c["starts"], start0=c["first"])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", D.TILE_CASES + D.SHARD_CASES)
def test_every_decoy_file_is_valid_for_the_oracle(kind, name):
    c = D.case(kind, name)
    assert len(c["stream"]) <= 2_500_000
    if kind == "bam":
        exp = orc.bam_read(c["data"])
        assert exp["status"] >= 0 and exp["n_rows"] == len(c["starts"])
        assert [bytes(q) for q in exp["QNAME"][:3]] == [b"0000000", b"0000001", b"0000002"]
    else:
        exp = orc.bcf_read(c["data"])
        assert exp["status"] == 0 and exp["n_rows"] == len(c["starts"])
    z = orc.bgzf_inflate_all(c["data"])
    assert z["data"] == c["stream"]
    assert int(z["ulen"][0]) > c["first"]          # the first record lies in block 0: a whole-file batch has its origin at byte 0 of the stream


def test_the_filter_on_single_records():
    """the decoys pass the filter, a true record passes it, the stop word and plain bytes do not"""
    for kind in KINDS:
        c = D.case(kind, "control")
        rule, u = c["rule"], c["stream"]
        assert rule.filter(u, c["starts"][0]) == (M.OK, 1024) and rule.filter(u, c["starts"][5]) == (M.OK, 1024)
        assert rule.filter(u, c["starts"][0] + 4)[0] == M.INVALID
        assert rule.filter(u, len(u) - 3)[0] == M.INCOMPLETE
        assert rule.filter(u, c["starts"][-1] + 1)[0] != M.OK
    b = D.bam_decoy() * 2 + D.BAM_STOP + bytes(64)
    assert M.BamRule(1).filter(b, 0) == (M.OK, 52) and M.BamRule(1).filter(b, 52) == (M.OK, 52) and M.BamRule(1).filter(b, 104)[0] == M.INVALID
    assert M.BamRule(0).filter(b, 0)[0] == M.INVALID                                  # refID 0 of a header without references
    assert M.BamRule(1).filter(D.bam_decoy(block_len=70000) + bytes(70000), 0)[0] == M.INVALID      # body - core > 8 * core + 65536
    assert M.BamRule(1).filter(D.bam_decoy(block_len=70000, l_seq=20000) + bytes(70000), 0) == (M.OK, 70004)
    v = D.bcf_decoy() * 2 + D.BCF_STOP + bytes(64)
    assert M.BcfRule(2, 0).filter(v, 0) == (M.OK, 32) and M.BcfRule(2, 0).filter(v, 64)[0] == M.INVALID
    assert M.BcfRule(0, 0).filter(v, 0)[0] == M.INVALID


@pytest.mark.parametrize("kind", KINDS)
def test_control_file_speculates_every_tile_correctly(kind):
    t = _table(D.case(kind, "control"))
    assert len(t) == 51 and M.mis_count(t) == 0
    assert [e["spec"] for e in t[:3]] == [960, TILE + 960, 2 * TILE + 960]
    assert all(e["err"] == 0 for e in t)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["every_tile_chain3", "every_tile_rejoin"])
def test_every_tile_behind_the_first_is_mis_speculated(kind, name):
    t = _table(D.case(kind, name))
    assert len(t) == 301 and not t[0]["mis"]
    assert M.mis_count(t) == 300 and M.longest_mis_run(t) == 300 >= 257
    assert all(e["spec"] == e["t"] * TILE + D.AT for e in t[1:])
    if name == "every_tile_chain3":       # three decoys, then the walk stops on the stop word
        assert all((e["count"], e["err"], e["end_next"]) == (3, 1, e["spec"] + 3 * (52 if kind == "bam" else 32)) for e in t[1:])
    else:                                 # the fake record ends on the tile's first true record: right exit, one record too many
        assert all(e["err"] == 0 and e["count"] == 9 and e["end_next"] == (e["t"] + 1) * TILE + 960 for e in t[1:-1])


@pytest.mark.parametrize("kind", KINDS)
def test_sparse(kind):
    t = _table(D.case(kind, "sparse"))
    assert M.mis_count(t) >= 5 and M.correct_behind_mis(t) >= 5, (M.mis_count(t), M.correct_behind_mis(t))


@pytest.mark.parametrize("kind", KINDS)
def test_leap(kind):
    t = _table(D.case(kind, "leap"))
    far = [e["t"] for e in t if e["mis"] and e["end_next"] >= (e["t"] + 4) * TILE]
    assert far == [3, 10, 11, 20, 21, 22, 30]
    assert all(t[k]["end_next"] == (k + 4) * TILE + 960 and t[k]["count"] == 1 and t[k]["err"] == 0 for k in far)
    assert M.mis_count(t) == len(far)                  # the tiles in between speculate correctly and are claimed to lie "inside a record"


@pytest.mark.parametrize("kind", KINDS)
def test_window_edge(kind):
    c = D.case(kind, "window_edge")
    t = _table(c)
    rule = c["rule"]
    # (a) the candidate's first follow-up lies inside the staged window but too close to its end for the LDS form of the filter
    e = t[5]
    o2 = e["spec"] + rule.filter(c["stream"], e["spec"])[1]
    assert e["mis"] and e["paths"][0] == "lds" and e["paths"][1] == "global"
    assert TILE + M.HALO - rule.need < o2 - 5 * TILE < TILE + M.HALO          # it begins inside the window, too close to its end
    # (b) the candidate straddles the end of a tile that lies inside one long record
    e = t[26]
    assert e["true"] is None and e["mis"] and e["spec"] < 27 * TILE < e["spec"] + (52 if kind == "bam" else 32)
    assert not t[27]["mis"] and t[27]["spec"] == c["starts"][D.LONG_AT + 1]
    if kind == "bam":
        # (c) the candidate of the last tile: fewer than 300 bytes of the stream behind it
        e = t[-1]
        assert e["mis"] and e["paths"][0] == "global" and len(c["stream"]) - e["spec"] < 300
        assert M.mis_count(t) == 4                     # tiles 5, 6 (the chain tile 5 hops into), 26 and the last
    else:
        assert M.mis_count(t) == 2


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", D.SHARD_KS)
def test_shard_start_goes_through_k_candidates(kind, k):
    c = D.case(kind, "shard_start_%d" % k)
    z = orc.bgzf_inflate_all(c["data"])
    assert int(z["ulen"][:c["block"]].sum()) == c["cut"]           # the block boundary falls where the case says
    assert c["starts"][D.SHARD_AT] < c["cut"] < c["starts"][D.SHARD_AT + 1]
    cands, settled = M.shard_candidates(c["rule"], c["stream"], c["cut"], c["starts"])
    assert len(cands) == k and settled == c["starts"][D.SHARD_AT + 1]
    assert all(kind_ == "breaks" for _, kind_, _ in cands)
    breaks = [b for _, _, b in cands]
    assert breaks == sorted(breaks) and len(set(breaks)) == k      # (three links per chain: one candidate and one break per chain)
    assert cands[-1][0] - c["cut"] < TILE                          # all inside the first tile of the shard's batch


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name, chains, links", [("shard_start_links4", 1, 4), ("shard_start_links20", 1, 20), ("shard_start_2x_links20", 2, 20)])
def test_shard_start_behind_long_chains_whose_candidates_break_at_one_place(kind, name, chains, links):
    """a chain of L > 3 decoys holds L - 2 offsets that pass the three-deep filter, and all of them break at the chain's stop word: successive
    candidates with the SAME break in a valid file.  The driver passes over the members of a failed chain, so each chain costs one candidate."""
    c = D.case(kind, name)
    plain, settled = M.shard_candidates(c["rule"], c["stream"], c["cut"], c["starts"], skip_members=False)
    assert len(plain) == chains * (links - 2) and settled == c["starts"][D.SHARD_AT + 1]
    assert len(set(b for _, _, b in plain)) == chains                  # breaks coincide
    cands, settled = M.shard_candidates(c["rule"], c["stream"], c["cut"], c["starts"])
    assert len(cands) == chains and settled == c["starts"][D.SHARD_AT + 1]


@pytest.mark.parametrize("kind", KINDS)
def test_shard_start_rejoin_and_far(kind):
    c = D.case(kind, "shard_start_rejoin")
    cands, settled = M.shard_candidates(c["rule"], c["stream"], c["cut"], c["starts"])
    assert [x[1] for x in cands] == ["holds"] and settled == c["starts"][D.SHARD_AT + 1]       # only the full validation can refuse it
    c = D.case(kind, "shard_start_far")
    cands, settled = M.shard_candidates(c["rule"], c["stream"], c["cut"], c["starts"])
    assert [x[1] for x in cands] == ["breaks", "breaks"] and settled == c["starts"][D.SHARD_AT + 1]
    assert cands[0][0] - c["cut"] >= TILE                                                      # the candidates lie behind the batch's first tile
