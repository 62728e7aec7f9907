"""bam_bin_counts on the device (dhts_bam_bins_*, csrc/bam_bins.hip) against the CPU model bam_bins_ref, bit for bit: the golden file, the
shapes a wave of the add kernel can meet, placement, the filters, the duplicate rule across batches, many batches, and the ABI's states."""
import numpy as np
import pytest

import bam_bins_cases as K
import bam_bins_ref as M
import duckhts_amd
import orc
from conftest import read_golden
from duckhts_amd import synth

pytestmark = pytest.mark.gpu


def model(data, named_tids=None, **kw):
    c = orc.bam_read(data)
    return M.bin_counts(c, c["ref_names"], c["ref_len"], named_tids=named_tids, **kw)


def same(got, exp):
    assert got["stats"] == exp["stats"]
    assert got["n_rows"] == exp["n_rows"]
    assert list(got["chrom"]) == exp["chrom"]
    for k in M.COLUMNS[1:]:
        assert got[k].dtype == np.int64 and got[k].tolist() == exp[k], k
    assert (got["count_total"] == got["count_fwd"] + got["count_rev"]).all()
    assert int(got["count_total"].sum()) == got["stats"]["n_counted"]
    assert sum(v for k, v in got["stats"].items() if k != "n_rows") == got["stats"]["n_rows"]


def check(data, **kw):
    got = duckhts_amd.bam_bin_counts(data, **kw)
    kw.pop("max_blocks", None), kw.pop("max_rows", None)
    exp = model(data, **kw)
    same(got, exp)
    assert got["status"] == 1
    return got


# ---- the golden file ----
@pytest.fixture(scope="module")
def rng():
    return read_golden("range.bam")


@pytest.mark.parametrize("emit_zero_bins", [False, True])
@pytest.mark.parametrize("bin_width,n_bins", [(1000, 10), (100, 55), (37, 85), (1 << 31, 4)])
def test_golden_file(rng, bin_width, n_bins, emit_zero_bins):
    got = check(rng, bin_width=bin_width, emit_zero_bins=emit_zero_bins)
    assert int((got["count_total"] > 0).sum()) == n_bins and got["stats"]["n_counted"] == 112
    if bin_width == 1 << 31:
        assert got["bin_id"].tolist() == [0] * got["n_rows"] and (got["start"] == 0).all()


@pytest.mark.parametrize("emit_zero_bins", [False, True])
def test_golden_file_region(rng, emit_zero_bins):
    bai = read_golden("range.bam.bai")
    region = "CHROMOSOME_I:1-1000"
    rows = duckhts_amd.read_bam(rng, region=region, index=bai)
    assert 0 < rows["n_rows"] < 112
    hdr = rows["header"]
    exp = M.bin_counts(rows, hdr["ref_names"], hdr["ref_len"], bin_width=100, emit_zero_bins=emit_zero_bins, named_tids={0})
    got = duckhts_amd.bam_bin_counts(rng, bin_width=100, region=region, index=bai, emit_zero_bins=emit_zero_bins)
    same(got, exp)
    assert got["stats"]["n_rows"] == rows["n_rows"]
    if emit_zero_bins:
        assert got["n_rows"] == (hdr["ref_len"][0] + 99) // 100 and set(got["chrom"]) == {b"CHROMOSOME_I"}
    without_index = duckhts_amd.bam_bin_counts(rng, bin_width=100, region=region, emit_zero_bins=emit_zero_bins)
    same(without_index, exp)


# ---- what a wave of the add kernel can meet ----
REFS2 = [("c1", 100000), ("c2", 100000)]


def fwd(tid, pos0):
    return (0, tid, pos0, 30, -1)


def rev(tid, pos0):
    return (0x10, tid, pos0, 30, -1)


WAVES = {
    "1_row": [fwd(0, 5)],
    "63_rows_one_bin": [fwd(0, 5 + i) for i in range(63)],
    "64_rows_one_bin": [fwd(0, 5 + i) for i in range(64)],
    "65_rows_one_bin": [fwd(0, 5 + i) for i in range(65)],
    "129_rows_one_bin": [fwd(0, 5 + i) for i in range(129)],
    "every_lane_a_head": [(rev if i & 1 else fwd)(0, 5 + i) for i in range(64)],
    "a_word_comes_back": [fwd(0, 5000 * (i & 1) + i) for i in range(100)],
    "run_across_two_waves": [fwd(0, 10 + i) for i in range(40)] + [fwd(0, 2000 + i) for i in range(50)] + [rev(0, 2000 + i) for i in range(80)],
    "bin_0_of_two_contigs": [fwd(0, i) for i in range(30)] + [fwd(1, i) for i in range(30)],
    "uncounted_rows_inside_a_run": [((0x200 if i % 5 == 2 else 0), 0, 7, (0 if i % 7 == 3 else 30), -1) for i in range(200)],
}


@pytest.mark.parametrize("name", sorted(WAVES))
def test_wave_shapes(name):
    data = K.bam(REFS2, WAVES[name])
    got = check(data, bin_width=1000, min_mapq=1, exclude_flags=0x200)
    assert got["stats"]["n_rows"] == len(WAVES[name])
    if name.endswith("rows_one_bin"):
        assert got["n_rows"] == 1 and got["count_fwd"].tolist() == [len(WAVES[name])]
    if name == "bin_0_of_two_contigs":
        assert got["chrom"] == [b"c1", b"c2"] and got["count_total"].tolist() == [30, 30] and got["bin_id"].tolist() == [0, 0]
    if name == "a_word_comes_back":
        assert got["count_total"].tolist() == [50, 50]


# ---- placement ----
def test_placement():
    refs = [("a", 1000), ("z", 0), ("b", 50)]
    rows = [fwd(0, 999), fwd(0, 1000), fwd(0, 1100), rev(2, 49), fwd(2, 50), fwd(1, 0), (4, -1, -1, 0, -1), (4, -1, 7, 0, -1), (0, 0, -1, 30, -1), fwd(0, 0)]
    data = K.bam(refs, rows)
    got = check(data, bin_width=100)
    assert got["stats"] == {"n_rows": 10, "n_flag_filtered": 0, "n_unplaced": 3, "n_out_of_range": 4, "n_duplicate": 0, "n_low_mapq": 0, "n_counted": 3}
    assert K.table_rows(got) == [(b"a", 0, 100, 0, 1, 1, 0), (b"a", 900, 1000, 9, 1, 1, 0), (b"b", 0, 50, 0, 1, 0, 1)]
    zero = check(data, bin_width=100, emit_zero_bins=True)
    assert zero["n_rows"] == 11 and b"z" not in zero["chrom"]                     # a contig of length 0 has no bins
    for bw in (1, 7, 10 ** 6, 1 << 31, 1 << 40):
        check(data, bin_width=bw)
        check(data, bin_width=bw, emit_zero_bins=True)
    one = check(data, bin_width=1, emit_zero_bins=True)
    assert one["n_rows"] == 1050 and one["end"].tolist() == [s + 1 for s in one["start"].tolist()]


def test_header_without_references():
    data = K.bam([], [(4, -1, -1, 0, -1)] * 3)
    for zero in (False, True):
        got = check(data, bin_width=100, emit_zero_bins=zero)
        assert got["n_rows"] == 0 and got["stats"]["n_unplaced"] == 3


# ---- filters ----
@pytest.mark.parametrize("kw", [dict(require_flags=0x2), dict(exclude_flags=0x10), dict(include_flags=0x40 | 0x10), dict(require_flags=0x1, exclude_flags=0x20, include_flags=0x80 | 0x10),
                                dict(min_mapq=0), dict(min_mapq=1), dict(min_mapq=255), dict(require_flags=0x2, min_mapq=30, dedup="adjacent"), dict(require_flags=0xffff), dict(exclude_flags=0xffff)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_filters(rng, kw):
    got = check(rng, bin_width=1000, **kw)
    if kw == dict(require_flags=0x2):
        assert got["stats"]["n_counted"] == 109
    if kw == dict(min_mapq=1):
        assert got["stats"]["n_counted"] == 95
    if kw == dict(min_mapq=255):
        assert got["stats"]["n_low_mapq"] == 112 and got["n_rows"] == 0


# ---- the duplicate rule across batches ----
@pytest.mark.parametrize("dedup", ["adjacent", "none"])
def test_duplicates_across_batches(dedup):
    # every record in a BGZF block of its own: a scan of one block per batch parts every pair of neighbours, a flag-filtered or unplaced
    # row is the last row of its batch, and two or three blocks per batch shift the cuts
    data = K.bam(K.DEDUP_REFS, K.DEDUP_ROWS, one_record_per_block=True)
    assert orc.bam_read(data)["n_rows"] == len(K.DEDUP_ROWS)
    kw = dict(K.DEDUP_PARAMS, dedup=dedup)
    exp = model(data, **kw)
    assert K.table_rows(exp) == (K.DEDUP_TABLE if dedup == "adjacent" else K.NODEDUP_TABLE)
    for max_blocks in (1, 2, 3, 0):
        got = duckhts_amd.bam_bin_counts(data, max_blocks=max_blocks, **kw)
        same(got, exp)
        assert got["stats"] == (K.DEDUP_STATS if dedup == "adjacent" else K.NODEDUP_STATS)
    same(duckhts_amd.bam_bin_counts(K.bam(K.DEDUP_REFS, K.DEDUP_ROWS), **kw), exp)          # and in one block


def open_ctx(data):
    ctx = duckhts_amd.Context(0)
    ctx.open(data)
    ctx.bgzf_index()
    return ctx, ctx.bam_open()


def drain(ctx, max_rows=0):
    parts = []
    while True:
        cols, st = ctx.bam_bins_next(max_rows)
        assert cols["n_rows"] <= (max_rows or 1 << 20)
        parts.append(cols)
        if st:
            return {k: np.concatenate([p[k] for p in parts]) for k in duckhts_amd.BINS_COLUMNS}


def test_accumulate_fed_by_the_callers_own_loop():
    data = K.bam(K.DEDUP_REFS, K.DEDUP_ROWS, one_record_per_block=True)
    ctx, _ = open_ctx(data)
    try:
        ctx.bam_bins_open(**K.DEDUP_PARAMS)
        sizes = []
        while True:
            b = ctx.next_batch(1, duckhts_amd.BINS_COLMASK)
            sizes.append(int(b.n_rows))
            ctx.bam_bins_accumulate(b)
            if b.status:
                break
        assert sum(sizes) == len(K.DEDUP_ROWS) and max(sizes) == 1                  # the duplicate pairs did fall into different batches
        st = ctx.bam_bins_stats()
        assert {k: v for k, v in st.items() if k.startswith("n_")} == K.DEDUP_STATS and st["status"] == 1 and st["total_bins"] == 20
        own = drain(ctx)
    finally:
        ctx.close()
    exp = duckhts_amd.bam_bin_counts(data, **K.DEDUP_PARAMS)
    for k in duckhts_amd.BINS_COLUMNS[1:]:
        assert own[k].tolist() == exp[k].tolist()
    assert own["chrom"].tolist() == [0, 0, 0, 1, 1]


# ---- many batches ----
@pytest.fixture(scope="module")
def many():
    data = synth.bam_file(30000, seed=42)
    c = orc.bam_read(data)
    assert c["n_rows"] == 30000 and c["n_ref"] == 25 and int(((c["FLAG"] & 0x10) != 0).sum()) == 15000 and int((c["MAPQ"] == 0).sum()) == 571
    return data, c


@pytest.mark.parametrize("max_blocks", [7, 0])
@pytest.mark.parametrize("bin_width", [5000000, 5000])
def test_many_batches(many, bin_width, max_blocks):
    data, c = many
    for kw in (dict(), dict(min_mapq=1, exclude_flags=0x400), dict(min_mapq=1, exclude_flags=0x400, dedup="adjacent")):
        exp = M.bin_counts(c, c["ref_names"], c["ref_len"], bin_width=bin_width, **kw)
        got = duckhts_amd.bam_bin_counts(data, bin_width=bin_width, max_blocks=max_blocks, **kw)
        same(got, exp)
        assert got["stats"]["n_rows"] == 30000
        if not kw and bin_width == 5000:
            assert got["n_rows"] == 29990


# ---- the ABI's states ----
def test_calls_in_the_wrong_state(rng):
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(rng)
        ctx.bgzf_index()
        with pytest.raises(duckhts_amd.DhtsError, match="dhts_bam_open not called"):
            ctx.bam_bins_open()
        ctx.bam_open()
        b = ctx.next_batch(0, duckhts_amd.BINS_COLMASK)
        for call in (lambda: ctx.bam_bins_accumulate(b), ctx.bam_bins_scan, ctx.bam_bins_stats, ctx.bam_bins_next):
            with pytest.raises(duckhts_amd.DhtsError, match="dhts_bam_bins_open not called"):
                call()
        for kw, msg in ((dict(bin_width=0), M.ERR_BIN_WIDTH), (dict(min_mapq=256), M.ERR_MAPQ), (dict(include_flags=65536), M.err_flags("include")),
                        (dict(require_flags=-1), M.err_flags("require")), (dict(exclude_flags=70000), M.err_flags("exclude")), (dict(dedup="optical"), M.ERR_DEDUP),
                        # wrong in two ways: the first in the order of the checks is reported
                        (dict(bin_width=0, min_mapq=256), M.ERR_BIN_WIDTH), (dict(min_mapq=256, include_flags=65536), M.ERR_MAPQ),
                        (dict(require_flags=-1, exclude_flags=70000), M.err_flags("require"))):
            with pytest.raises(duckhts_amd.DhtsError) as e:
                ctx.bam_bins_open(**kw)
            assert str(e.value) == msg
    finally:
        ctx.close()


def test_bin_count_limit_and_shards(many):
    data, c = many
    ctx, hdr = open_ctx(data)
    try:
        total = M.total_bins(hdr["ref_len"], 1)
        assert total > M.MAX_BINS
        with pytest.raises(duckhts_amd.DhtsError) as e:
            ctx.bam_bins_open(bin_width=1)
        assert str(total) in str(e.value) and "bins" in str(e.value)
        assert M.total_bins(hdr["ref_len"], 12) <= M.MAX_BINS < M.total_bins(hdr["ref_len"], 11)
        with pytest.raises(duckhts_amd.DhtsError, match=str(M.total_bins(hdr["ref_len"], 11))):
            ctx.bam_bins_open(bin_width=11)
        ctx.set_shard(0, 2)
        with pytest.raises(duckhts_amd.DhtsError, match="shard or block range"):
            ctx.bam_bins_open()
        ctx.set_shard(0, 1)
        ctx.bam_bins_open()
        ctx.set_block_range(3, 9, 1)
        with pytest.raises(duckhts_amd.DhtsError, match="shard or block range"):
            ctx.bam_bins_scan()
    finally:
        ctx.close()


@pytest.mark.parametrize("max_rows", [1, 3])
def test_paging(rng, max_rows):
    one = duckhts_amd.bam_bin_counts(rng, bin_width=1000)
    paged = duckhts_amd.bam_bin_counts(rng, bin_width=1000, max_rows=max_rows)
    assert one["n_rows"] == 10
    same(paged, {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in one.items()})
    ctx, _ = open_ctx(rng)
    try:
        ctx.bam_bins_open(bin_width=1000)
        assert ctx.bam_bins_scan() == 1
        a = drain(ctx, max_rows)
        assert a["count_total"].tolist() == one["count_total"].tolist()
        cols, st = ctx.bam_bins_next(max_rows)                                       # behind the last batch: nothing, and still the end
        assert cols["n_rows"] == 0 and st == 1
    finally:
        ctx.close()
