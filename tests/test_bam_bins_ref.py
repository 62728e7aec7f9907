"""The CPU model of bam_bin_counts (bam_bins_ref.py) against an independent group-by on the golden file, against a table written out by hand
for the duplicate rule, and against fasta_nuc's bins for the clipping and the zero bins.  No device."""
import collections

import numpy as np
import pytest

import bam_bins_cases as K
import bam_bins_ref as M
import fasta_nuc_ref as N
import orc
from conftest import read_golden


@pytest.fixture(scope="module")
def rng_bam():
    return orc.bam_read(read_golden("range.bam"))


def test_the_golden_file_is_what_the_tests_assume(rng_bam):
    c = rng_bam
    assert c["n_rows"] == 112
    assert (c["tid"] >= 0).all() and (c["POS"] >= 1).all() and all(int(c["POS"][i]) - 1 < int(c["ref_len"][c["tid"][i]]) for i in range(112))
    key = c["tid"].astype(np.int64) << 32 | c["POS"]
    assert (np.diff(key) >= 0).all()                                                  # coordinate-sorted
    assert int(((c["FLAG"] & 0x10) != 0).sum()) == 56 and int((c["MAPQ"] == 0).sum()) == 17
    assert int(((c["FLAG"] & 0x2) != 0).sum()) == 109 and int(c["MAPQ"].max()) == 60
    # no adjacent duplicates: rows that share their start with the row before are paired and have another PNEXT
    same = [i for i in range(1, 112) if c["tid"][i] == c["tid"][i - 1] and c["POS"][i] == c["POS"][i - 1]]
    assert all(c["FLAG"][i] & 1 and c["PNEXT"][i] != c["PNEXT"][i - 1] for i in same)


@pytest.mark.parametrize("bin_width,n_bins,largest", [(1000, 10, 23), (100, 55, None), (37, 85, None)])
def test_defaults_against_a_group_by(rng_bam, bin_width, n_bins, largest):
    c = rng_bam
    got = M.bin_counts(c, c["ref_names"], c["ref_len"], bin_width=bin_width)
    fwd = collections.Counter((int(t), (int(p) - 1) // bin_width) for t, p, f in zip(c["tid"], c["POS"], c["FLAG"]) if not f & 0x10)
    rev = collections.Counter((int(t), (int(p) - 1) // bin_width) for t, p, f in zip(c["tid"], c["POS"], c["FLAG"]) if f & 0x10)
    keys = sorted(set(fwd) | set(rev))
    assert len(keys) == n_bins == got["n_rows"]
    names = [bytes(n) if not isinstance(n, str) else n.encode() for n in c["ref_names"]]
    assert got["chrom"] == [names[t] for t, _ in keys] and got["bin_id"] == [b for _, b in keys]
    assert got["count_fwd"] == [fwd[k] for k in keys] and got["count_rev"] == [rev[k] for k in keys]
    assert got["count_total"] == [fwd[k] + rev[k] for k in keys] and sum(got["count_total"]) == 112
    assert got["start"] == [b * bin_width for _, b in keys]
    assert got["end"] == [min(b * bin_width + bin_width, int(c["ref_len"][t])) for t, b in keys]
    if largest is not None:
        assert max(got["count_total"]) == largest
    assert got["stats"] == {"n_rows": 112, "n_flag_filtered": 0, "n_unplaced": 0, "n_out_of_range": 0, "n_duplicate": 0, "n_low_mapq": 0, "n_counted": 112}
    # the same table by numpy
    ids, cnt = np.unique(c["tid"].astype(np.int64) * (1 << 32) + (c["POS"] - 1) // bin_width, return_counts=True)
    assert [int(x) for x in cnt] == got["count_total"] and [int(x) & 0xffffffff for x in ids] == got["bin_id"]


def test_filters_on_the_golden_file(rng_bam):
    c = rng_bam
    base = dict(cols=c, ref_names=c["ref_names"], ref_len=c["ref_len"], bin_width=1000)
    st = M.bin_counts(min_mapq=1, **base)["stats"]
    assert st["n_counted"] == 95 and st["n_low_mapq"] == 17
    st = M.bin_counts(require_flags=0x2, **base)["stats"]
    assert st["n_counted"] == 109 and st["n_flag_filtered"] == 3
    st = M.bin_counts(exclude_flags=0x10, **base)["stats"]
    assert st["n_counted"] == 56 and st["n_flag_filtered"] == 56
    st = M.bin_counts(include_flags=0x10 | 0x2, **base)["stats"]
    assert st["n_counted"] == int(((c["FLAG"] & 0x12) != 0).sum())
    st = M.bin_counts(dedup="adjacent", **base)["stats"]
    assert st["n_duplicate"] == 0 and st["n_counted"] == 112


def test_the_duplicate_rule_on_a_hand_written_file():
    c = orc.bam_read(K.bam(K.DEDUP_REFS, K.DEDUP_ROWS))
    assert c["n_rows"] == len(K.DEDUP_ROWS)
    got = M.bin_counts(c, c["ref_names"], c["ref_len"], **K.DEDUP_PARAMS)
    assert got["stats"] == K.DEDUP_STATS
    assert K.table_rows(got) == K.DEDUP_TABLE
    got = M.bin_counts(c, c["ref_names"], c["ref_len"], **dict(K.DEDUP_PARAMS, dedup="none"))
    assert got["stats"] == K.NODEDUP_STATS
    assert K.table_rows(got) == K.NODEDUP_TABLE
    for res in (K.DEDUP_TABLE, K.NODEDUP_TABLE):
        assert all(r[4] == r[5] + r[6] for r in res)


@pytest.mark.parametrize("bin_width", [1, 37, 100, 999, 1000, 1001, 5000])
def test_clipping_and_zero_bins_are_fasta_nucs(bin_width):
    refs = [("a", 1000), ("empty", 0), ("b", 37), ("c", 1)]
    c = orc.bam_read(K.bam(refs, [(0, 0, 999, 30, -1), (0x10, 2, 36, 30, -1), (0, 3, 0, 30, -1)]))
    names = [n for n, _ in refs]
    tab = {n: (ln,) for n, ln in refs}
    want = [(n.encode(), s, e) for n, s, e in N.bin_intervals(names, tab, bin_width, None)]
    got = M.bin_counts(c, c["ref_names"], c["ref_len"], bin_width=bin_width, emit_zero_bins=True)
    assert list(zip(got["chrom"], got["start"], got["end"])) == want and got["n_rows"] == M.total_bins([ln for _, ln in refs], bin_width)
    assert sum(got["count_total"]) == 3
    some = M.bin_counts(c, c["ref_names"], c["ref_len"], bin_width=bin_width)
    assert some["n_rows"] == 3 and set(zip(some["chrom"], some["start"], some["end"])) <= set(want)
    assert some["end"][0] == 1000 and some["end"][1] == 37 and some["end"][2] == 1
    # a region query names contigs: zero bins only there
    named = M.bin_counts(c, c["ref_names"], c["ref_len"], bin_width=bin_width, emit_zero_bins=True, named_tids={2})
    assert [r for r in zip(named["chrom"], named["start"], named["end"]) if r[0] == b"b"] == [r for r in want if r[0] == b"b"]
    assert sorted(set(named["chrom"])) == [b"a", b"b", b"c"] and named["n_rows"] == 2 + (37 + bin_width - 1) // bin_width


def test_parameter_errors():
    for kw, msg in ((dict(bin_width=0), M.ERR_BIN_WIDTH), (dict(bin_width=-5), M.ERR_BIN_WIDTH), (dict(min_mapq=-1), M.ERR_MAPQ), (dict(min_mapq=256), M.ERR_MAPQ),
                    (dict(include_flags=65536), M.err_flags("include")), (dict(require_flags=-1), M.err_flags("require")), (dict(exclude_flags=1 << 20), M.err_flags("exclude")),
                    (dict(dedup="optical"), M.ERR_DEDUP)):
        with pytest.raises(M.BinsError) as e:
            M.check_params(**kw)
        assert str(e.value) == msg
