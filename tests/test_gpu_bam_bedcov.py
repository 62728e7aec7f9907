"""bam_bedcov on the device (dhts_bam_bedcov_*, csrc/bam_bedcov.hip) against the CPU model bam_bedcov_ref, bit for bit: the shapes a wave
of the add kernel can meet, rounds over several segments, every kind of CIGAR under the four option combinations, interval edges, contigs,
positions at the end of a 2^31 - 1 contig, a breakpoint table of several scan tiles, many batches, the golden file, and the ABI's states."""
import ctypes as C

import numpy as np
import pytest

import bam_bedcov_cases as K
import bam_bedcov_ref as M
import duckhts_amd
import orc
from conftest import read_golden

pytestmark = pytest.mark.gpu
WHOLE = 1 << 31


def model_params(kw):
    p = {k: v for k, v in kw.items() if k in ("min_mapq", "include_flags", "require_flags", "exclude_flags", "count_deletions", "count_ref_skips")}
    p.setdefault("exclude_flags", M.DEFAULT_EXCLUDE)                     # the Python function's default
    return p


def same(got, exp):
    assert {k: got["stats"][k] for k in M.COUNTERS} == exp["stats"]
    assert got["n_rows"] == exp["n_rows"] == got["stats"]["n_bed_rows"]
    for k in M.COLUMNS[:6]:
        assert list(got[k]) == exp[k], k
    for k in M.COLUMNS[6:]:
        assert got[k].dtype == np.int64 and got[k].tolist() == exp[k], k
    assert sum(got["stats"][k] for k in M.COUNTERS[1:]) == got["stats"]["n_rows"]


def whole_contig_invariant(data, c, **kw):
    """a BED of one interval [0, 2^31) per contig: bases_covered = the model's total segment length on the contig, read_count = its counted reads"""
    names = [bytes(n) for n in c["ref_names"]]
    if not names:
        return
    st, reads = M.counted_reads(c, len(names), **model_params(kw))
    got = duckhts_amd.bam_bedcov(data, K.bed([(n.decode(), 0, WHOLE) for n in names]), **kw)
    for t in range(len(names)):
        mine = [r for r in reads if r[0] == t]
        assert int(got["read_count"][t]) == len(mine), t
        assert int(got["bases_covered"][t]) == sum(max(0, min(b, WHOLE) - a) for _, _, segs in mine for a, b in segs), t
    assert {k: got["stats"][k] for k in M.COUNTERS} == st


def check(data, bed_text, **kw):
    got = duckhts_amd.bam_bedcov(data, bed_text, **kw)
    c = orc.bam_read(data)
    exp = M.bedcov(c, c["ref_names"], bed_text, **model_params(kw))
    same(got, exp)
    assert got["status"] == 1
    whole_contig_invariant(data, c, **{k: v for k, v in kw.items() if k not in ("max_blocks", "bed_max_blocks")})
    return got


def r10(tid, pos0, cigar="10M", flag=0, mapq=30):
    return (flag, tid, pos0, mapq, cigar)


# ---- what a wave of the add kernel can meet ----
TWO = K.bed([("c1", 1000, 2000), ("c1", 5000, 6000), ("c2", 1000, 2000)])
WAVES = {
    "1_read": [r10(0, 1100)],
    "63_reads_between_two_breakpoints": [r10(0, 1100 + i) for i in range(63)],
    "64_reads_between_two_breakpoints": [r10(0, 1100 + i) for i in range(64)],
    "65_reads_between_two_breakpoints": [r10(0, 1100 + i) for i in range(65)],
    "129_reads_between_two_breakpoints": [r10(0, 1100 + i) for i in range(129)],
    "a_counter_comes_back": [r10(0, 1100 + 4000 * (i & 1) + i) for i in range(100)],
    "run_across_two_waves": [r10(0, 1100 + i) for i in range(40)] + [r10(0, 5100 + i) for i in range(50)] + [r10(1, 1100 + i) for i in range(80)],
    "uncounted_rows_inside_a_run": [r10(0, 1100 + i, flag=(0x200 if i % 5 == 2 else 0), mapq=(0 if i % 7 == 3 else 30)) for i in range(200)],
    "runs_that_straddle_a_breakpoint": [r10(0, 1985 + (i // 4)) for i in range(100)],
}


@pytest.mark.parametrize("name", sorted(WAVES))
def test_wave_shapes(name):
    got = check(K.bam(K.REFS, WAVES[name]), TWO, min_mapq=1)
    n = len(WAVES[name])
    assert got["stats"]["n_rows"] == n
    if name.endswith("between_two_breakpoints"):
        assert K.pairs(got) == [(10 * n, n), (0, 0), (0, 0)]
    if name == "a_counter_comes_back":
        assert K.pairs(got) == [(500, 50), (500, 50), (0, 0)]
    if name == "uncounted_rows_inside_a_run":
        assert got["stats"]["n_flag_filtered"] == 40 and got["stats"]["n_low_mapq"] == 23 and got["stats"]["n_counted"] == 137


def test_every_lane_on_a_different_counter():
    # 64 one-base intervals with one read start in each: no two neighbouring lanes share a counter index
    bed = K.bed([("c1", 1000 + 2 * i, 1001 + 2 * i) for i in range(64)])
    got = check(K.bam(K.REFS, [r10(0, 1000 + 2 * i, "1M") for i in range(64)]), bed)
    assert K.pairs(got) == [(1, 1)] * 64 and got["stats"]["n_breakpoints"] == 128
    # and out of order: nothing depends on the order of the rows
    rows = [r10(0, 1000 + 2 * ((i * 37) % 64), "1M") for i in range(64)]
    assert K.pairs(check(K.bam(K.REFS, rows), bed)) == [(1, 1)] * 64


# ---- rounds ----
FIVE = "5M2D5M2D5M2D5M2D5M"
ROUNDS_BED = K.bed([("c1", 1000, 1100), ("c1", 1030, 1033), ("c1", 1035, 1037), ("c1", 1037, 1042), ("c1", 1049, 1051), ("c1", 1063, 1200), ("c1", 0, 100000)])


@pytest.mark.parametrize("count_deletions,count_ref_skips", K.OPTIONS)
@pytest.mark.parametrize("lane", [0, 31, 63])
def test_one_lane_with_five_segments(lane, count_deletions, count_ref_skips):
    rows = [r10(0, 1000 + i, "20M") for i in range(63)]
    rows.insert(lane, r10(0, 1030, FIVE))
    got = check(K.bam(K.REFS, rows), ROUNDS_BED, count_deletions=count_deletions, count_ref_skips=count_ref_skips)
    assert int(got["bases_covered"][6]) == 63 * 20 + (33 if count_deletions else 25) and int(got["read_count"][6]) == 64


@pytest.mark.parametrize("count_deletions,count_ref_skips", K.OPTIONS)
def test_a_wave_without_a_segment(count_deletions, count_ref_skips):
    # the first wave has 64 mapped reads without a depth operation (no CIGAR, clips only, a deletion that does not count); the second has segments
    rows = [r10(0, 1000 + i, ("*", "4S", "3D")[i % 3] if not count_deletions else ("*", "4S")[i % 2]) for i in range(64)] + [r10(0, 1010 + i) for i in range(6)]
    got = check(K.bam(K.REFS, rows), ROUNDS_BED, count_deletions=count_deletions, count_ref_skips=count_ref_skips)
    assert K.pairs(got)[6] == (60, 70)
    only = check(K.bam(K.REFS, rows[:64]), ROUNDS_BED, count_deletions=count_deletions, count_ref_skips=count_ref_skips)
    assert K.pairs(only)[6] == (0, 64) and K.pairs(only)[0] == (0, 64)


# ---- CIGAR ----
CIGARS = ["*", "4S", "3S4M2I4M3S", "5M3D5M", "5M100N5M", "4=1X4=", "2H5M1P5M", "3D", "0M", "5M0D5M", "2D5M", "5M3D2N5M", "3M1D1N1D3M"]
CIGAR_BED = K.bed([("c1", 0, 100000), ("c1", 1000, 1001), ("c1", 1005, 1008), ("c1", 1004, 1012), ("c1", 1010, 1110), ("c1", 990, 1000), ("c1", 1000, 1000),
                   ("c1", 1001, 1002), ("c1", 1105, 1200), ("c2", 0, 100000)])


@pytest.mark.parametrize("count_deletions,count_ref_skips", K.OPTIONS)
@pytest.mark.parametrize("cigar", CIGARS)
def test_cigars(cigar, count_deletions, count_ref_skips):
    got = check(K.bam(K.REFS, [r10(0, 1000, cigar)]), CIGAR_BED, count_deletions=count_deletions, count_ref_skips=count_ref_skips)
    assert got["stats"]["n_counted"] == 1 and K.pairs(got)[9] == (0, 0)
    if cigar in ("*", "4S", "0M"):
        # a mapped read with rlen 0: read_count 1 on an interval at its position, depth 0
        assert K.pairs(got)[:2] == [(0, 1), (0, 1)] and K.pairs(got)[7] == (0, 0)
    if cigar == "5M100N5M":
        assert K.pairs(got)[0] == ((110 if count_ref_skips else 10), 1) and K.pairs(got)[8] == (5, 1)
    if cigar == "5M3D5M":
        assert K.pairs(got)[2] == ((3 if count_deletions else 0), 1)


@pytest.mark.parametrize("count_deletions,count_ref_skips", K.OPTIONS)
def test_unmapped_flag_with_a_position(count_deletions, count_ref_skips):
    rows = [r10(0, 1000, "10M", flag=4), r10(0, 1001, "*", flag=4), r10(0, 1005, "10M")]
    got = check(K.bam(K.REFS, rows), CIGAR_BED, exclude_flags=0, count_deletions=count_deletions, count_ref_skips=count_ref_skips)
    assert got["stats"]["n_counted"] == 3
    assert K.pairs(got)[:4] == [(10, 3), (0, 1), (3, 1), (7, 1)] and K.pairs(got)[7] == (0, 1)
    dflt = check(K.bam(K.REFS, rows), CIGAR_BED, count_deletions=count_deletions, count_ref_skips=count_ref_skips)          # 0x704 drops the two
    assert dflt["stats"]["n_flag_filtered"] == 2 and K.pairs(dflt)[0] == (10, 1)


# ---- edges ----
EDGE_ROWS = [r10(0, 1000), r10(0, 2000, "5M3D5M"), r10(0, 3000, "5M100N5M"), r10(0, 99995), r10(1, 1000), r10(0, 1000, flag=16)]
EDGE_BED = (K.bed([("c1", 1000, 1020, "starts_at_s"), ("c1", 1010, 1020, "ends_at_s"), ("c1", 990, 1000, "starts_at_e"), ("c1", 990, 1010, "ends_at_e"),
                   ("c1", 1009, 1020, "one_base_left"), ("c1", 990, 1001, "one_base_right"), ("c1", 1003, 1006, "inside_a_read", 7, "+"), ("c1", 2005, 2008, "the_deletion"),
                   ("c1", 2006, 2007, "inside_the_deletion"), ("c1", 3010, 3050, "inside_the_ref_skip"), ("c1", 900, 1100, "read_inside"),
                   ("c1", 900, 1100, "read_inside"), ("c1", 950, 1005, "overlapping"), ("c1", 1000, 1010, "nested"), ("c1", 1002, 1003, "nested"),
                   ("c1", 1500, 1500, "empty"), ("c1", 1010, 1000, "inverted"), ("c1", -5, 1005, "negative_start"), ("c1", 99990, 200000, "past_ref_len"),
                   ("c1", 100000, 100005, "behind_ref_len"), ("c1", "x", 1005, "null_start"), ("c1", 1000, "1e3", "null_end"), ("c9", 1000, 1010, "no_such_chrom"),
                   ("c2", 1000, 1010), ("c3", 1000, 1010)]) + b"c1\t1000\t1010\t\t\t\n" + b"#c1\t1\t2\n\nc1\t1004\t1005")


@pytest.mark.parametrize("count_deletions,count_ref_skips", K.OPTIONS)
def test_edges(count_deletions, count_ref_skips):
    got = check(K.bam(K.REFS, EDGE_ROWS), EDGE_BED, count_deletions=count_deletions, count_ref_skips=count_ref_skips)
    by = dict(zip(got["name"], K.pairs(got)))
    assert by[b"starts_at_s"] == (20, 2) and by[b"ends_at_s"] == (0, 0) and by[b"starts_at_e"] == (0, 0) and by[b"ends_at_e"] == (20, 2)
    assert by[b"one_base_left"] == (2, 2) and by[b"one_base_right"] == (2, 2) and by[b"inside_a_read"] == (6, 2)
    assert by[b"the_deletion"] == ((3 if count_deletions else 0), 1) and by[b"inside_the_ref_skip"] == ((40 if count_ref_skips else 0), 1)
    assert by[b"empty"] == by[b"inverted"] == by[b"null_start"] == by[b"null_end"] == by[b"no_such_chrom"] == (0, 0)
    assert by[b"negative_start"] == (10, 2) and by[b"past_ref_len"] == (10, 1) and by[b"behind_ref_len"] == (5, 1)          # the read runs past ref_len: positions are not compared with it
    assert got["n_rows"] == 27 and got["name"][-2:] == [None, None] and got["start"][20] is None and got["end"][21] is None
    assert K.pairs(got)[-1] == (2, 2) and got["score"][6] == b"7" and got["strand"][6] == b"+"


# ---- contigs ----
def test_nothing_carries_over_between_contigs():
    rows = [r10(0, 1000 + i) for i in range(70)] + [r10(1, 1005 + i, "5M2D5M") for i in range(30)]
    bed = K.bed([(c, s, e) for c in ("c1", "c2", "c3") for s, e in ((1000, 1010), (1005, 1200), (0, 900))])
    for cd in (True, False):
        got = check(K.bam(K.REFS, rows), bed, count_deletions=cd)
        assert K.pairs(got)[6:] == [(0, 0)] * 3 and K.pairs(got)[2] == K.pairs(got)[5] == (0, 0)
        assert K.pairs(got)[0] == (55, 10) and int(got["read_count"][3]) == 5


def test_a_contig_with_reads_and_no_intervals():
    rows = [r10(0, 1000 + i) for i in range(20)] + [r10(1, 1000 + i) for i in range(50)] + [r10(2, 1000 + i) for i in range(20)]
    got = check(K.bam(K.REFS, rows), K.bed([("c1", 1000, 1005), ("c3", 1000, 1005), ("c3", 1001, 1030)]))
    assert K.pairs(got) == [(15, 5), (15, 5), (sum(min(1030, 1010 + i) - max(1001, 1000 + i) for i in range(20)), 20)]
    assert got["stats"]["n_counted"] == 90 and got["stats"]["n_breakpoints"] == 6


def test_header_without_references():
    data = K.bam([], [(4, -1, -1, 0, "*")] * 3)
    got = check(data, K.bed([("c1", 0, 100)]), exclude_flags=0)
    assert K.pairs(got) == [(0, 0)] and got["stats"]["n_unplaced"] == 3 and got["stats"]["n_breakpoints"] == 0


@pytest.mark.parametrize("bed", [b"", b"\n", b"#only a comment\n"], ids=["empty", "newline", "comment"])
def test_empty_bed(bed):
    got = check(K.bam(K.REFS, [r10(0, 1000), r10(1, 5)]), bed)
    assert got["n_rows"] == 0 and got["stats"]["n_counted"] == 2 and len(got["bases_covered"]) == 0


# ---- large positions: the wrapping sums ----
@pytest.mark.parametrize("count_deletions", [True, False])
def test_last_kilobase_of_a_long_contig(count_deletions):
    n = (1 << 31) - 1
    refs = [("small", 5000), ("long", n)]
    rows = [r10(0, 100 + i) for i in range(10)] + [r10(1, n - 1000 + 7 * i, "20M3D20M") for i in range(130)] + [r10(1, n - 2, "10M")]
    bed = K.bed([("small", 0, 5000), ("long", n - 1000, n - 900), ("long", n - 500, n), ("long", n - 1, n), ("long", n - 100, n + 50), ("long", 0, n), ("long", n, n + 100),
                 ("long", n - 640, n - 630), ("long", 0, WHOLE)])
    got = check(K.bam(refs, rows), bed, count_deletions=count_deletions)
    assert K.pairs(got)[3] == (1, 1) and K.pairs(got)[6] == (8, 1) and int(got["read_count"][8]) == 131
    assert int(got["bases_covered"][8]) == 130 * (43 if count_deletions else 40) + 3         # [0, 2^31) takes three bases of the last read


# ---- the 64-bit scan: a breakpoint table of several tiles ----
@pytest.fixture(scope="module")
def big_bed():
    rows = [("c1" if i < 2600 else "c2", 20 * (i % 2600), 20 * (i % 2600) + 13) for i in range(5000)]
    text = K.bed(rows)
    assert len(text) > 65280                                                # more than one piece of BED text
    return text


@pytest.fixture(scope="module")
def big_bam():
    rows = [r10(i % 2, (i * 331) % 52000, ("30M", "10M5D10M", "4S26M")[i % 3]) for i in range(300)]
    return K.bam(K.REFS, rows)


@pytest.mark.parametrize("bed_max_blocks", [0, 1])
def test_breakpoints_over_several_scan_tiles(big_bed, big_bam, bed_max_blocks):
    got = check(big_bam, big_bed, bed_max_blocks=bed_max_blocks)
    # 10,000 breakpoints and the slot behind them: nine full tiles of 1,024 and one that ends inside
    assert got["stats"]["n_breakpoints"] == 10000 and got["n_rows"] == 5000
    assert int((got["read_count"] > 0).sum()) > 500 and int(got["read_count"][2400:2600].sum()) > 0 and int(got["read_count"][2600:].sum()) > 0
    cd = check(big_bam, big_bed, bed_max_blocks=bed_max_blocks, count_deletions=False)
    assert int(cd["bases_covered"].sum()) < int(got["bases_covered"].sum())


def test_result_paged_on_the_bed_side(big_bed, big_bam):
    ctx, bctx = contexts(big_bam, big_bed)
    try:
        ctx.bam_bedcov_open(bctx, exclude_flags=0x704)
        assert ctx.bam_bedcov_scan() == 1
        sizes = []
        while True:
            cols, st = ctx.bam_bedcov_next(bctx, 1)
            sizes.append(cols["n_rows"])
            if st:
                break
        assert len(sizes) >= 2 and sum(sizes) == 5000 and all(sizes[:-1])
        cols, st = ctx.bam_bedcov_next(bctx, 1)                             # behind the last batch: nothing, and still the end
        assert cols["n_rows"] == 0 and st == 1
    finally:
        bctx.close()
        ctx.close()


# ---- batches ----
@pytest.mark.parametrize("k", range(4))
def test_one_record_per_block(k):
    cd, cs = K.OPTIONS[k]
    data = K.bam(K.REFS, K.HAND_ROWS, one_record_per_block=True)
    one = K.bam(K.REFS, K.HAND_ROWS)
    kw = dict(K.HAND_PARAMS, count_deletions=cd, count_ref_skips=cs)
    exp = duckhts_amd.bam_bedcov(one, K.HAND_BED, **kw)
    assert K.pairs(exp) == [row[k] for row in K.HAND_EXPECTED] and {c: exp["stats"][c] for c in M.COUNTERS} == K.HAND_STATS
    for max_blocks in (1, 2, 3, 0):
        got = check(data, K.HAND_BED, max_blocks=max_blocks, **kw)
        assert K.pairs(got) == K.pairs(exp) and got["stats"] == exp["stats"]


def test_151_blocks():
    rows = [r10(i % 3, 1000 + 13 * i, ("10M", "5M2D5M", "3S7M", "5M20N5M")[i % 4], flag=(0x400 if i % 11 == 0 else 0)) for i in range(151)]
    data = K.bam(K.REFS, rows, one_record_per_block=True)
    bed = K.bed([(c, s, s + 150) for c in ("c1", "c2", "c3") for s in range(900, 3100, 100)])
    one = check(data, bed, count_ref_skips=False)
    many = check(data, bed, count_ref_skips=False, max_blocks=1)
    assert K.pairs(one) == K.pairs(many) and one["stats"] == many["stats"] and one["stats"]["n_rows"] == 151


# ---- the golden file ----
@pytest.fixture(scope="module")
def rng():
    return read_golden("range.bam")


@pytest.mark.parametrize("kw", [dict(), dict(exclude_flags=0x10, min_mapq=1), dict(count_deletions=False), dict(require_flags=0x40, include_flags=0x30)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()) or "defaults")
def test_golden_file(rng, kw):
    got = check(rng, K.GOLDEN_BED, **kw)
    assert got["n_rows"] == 14
    if not kw:
        assert got["stats"]["n_counted"] == 112 and got["chrom"][0] == b"CHROMOSOME_I" and got["name"][:3] == [b"first", None, b"wide"]


def test_golden_file_region(rng):
    bai = read_golden("range.bam.bai")
    region = "CHROMOSOME_I:1-1000"
    rows = duckhts_amd.read_bam(rng, region=region, index=bai)
    assert 0 < rows["n_rows"] < 112
    exp = M.bedcov(rows, rows["header"]["ref_names"], K.GOLDEN_BED, exclude_flags=M.DEFAULT_EXCLUDE)
    got = duckhts_amd.bam_bedcov(rng, K.GOLDEN_BED, region=region, index=bai)
    same(got, exp)
    assert got["stats"]["n_rows"] == rows["n_rows"]
    same(duckhts_amd.bam_bedcov(rng, K.GOLDEN_BED, region=region), exp)     # without the index: the whole file is scanned and filtered
    assert sum(got["read_count"][5:]) == 0 and got["read_count"][0] > 0


# ---- the ABI's states ----
def contexts(data, bed_text):
    ctx = duckhts_amd.Context(0)
    ctx.open(data)
    ctx.bgzf_index()
    ctx.bam_open()
    bctx = duckhts_amd.Context(0)
    bctx.open(bed_text)
    bctx.L.dhts_bgzf_index(bctx.h)
    bctx._chk(bctx.L.dhts_bed_open(bctx.h))
    return ctx, bctx


def drain(ctx, bctx):
    out = []
    while True:
        cols, st = ctx.bam_bedcov_next(bctx)
        out += K.pairs(cols)
        if st:
            return out


def test_calls_in_the_wrong_state(rng):
    ctx, bctx = duckhts_amd.Context(0), duckhts_amd.Context(0)
    try:
        ctx.open(rng)
        ctx.bgzf_index()
        bctx.open(K.GOLDEN_BED)
        bctx.L.dhts_bgzf_index(bctx.h)
        with pytest.raises(duckhts_amd.DhtsError, match="dhts_bam_open not called"):
            ctx.bam_bedcov_open(bctx)
        ctx.bam_open()
        with pytest.raises(duckhts_amd.DhtsError, match="the BED context is not open"):
            ctx.bam_bedcov_open(bctx)
        with pytest.raises(duckhts_amd.DhtsError, match="the BED context is not open"):
            ctx.bam_bedcov_open(None)
        bctx._chk(bctx.L.dhts_bed_open(bctx.h))
        with pytest.raises(duckhts_amd.DhtsError, match="a second context"):
            ctx.bam_bedcov_open(ctx)
        b = ctx.next_batch(0, duckhts_amd.BEDCOV_COLMASK)
        for call in (lambda: ctx.bam_bedcov_accumulate(b), ctx.bam_bedcov_scan, ctx.bam_bedcov_stats, lambda: ctx.bam_bedcov_next(bctx)):
            with pytest.raises(duckhts_amd.DhtsError, match="dhts_bam_bedcov_open not called"):
                call()
        for kw, msg in ((dict(min_mapq=256), M.ERR_MAPQ), (dict(min_mapq=-1), M.ERR_MAPQ), (dict(include_flags=65536), M.err_flags("include")),
                        (dict(require_flags=-1), M.err_flags("require")), (dict(exclude_flags=70000), M.err_flags("exclude")),
                        # wrong in two ways: the first in the order of the checks is reported
                        (dict(min_mapq=256, include_flags=65536), M.ERR_MAPQ), (dict(require_flags=-1, exclude_flags=70000), M.err_flags("require")),
                        (dict(count_deletions=2, exclude_flags=70000), M.err_flags("exclude"))):
            with pytest.raises(duckhts_amd.DhtsError) as e:
                ctx.bam_bedcov_open(bctx, **kw)
            assert str(e.value) == msg
        with pytest.raises(duckhts_amd.DhtsError, match="dhts_bam_bedcov_open not called"):      # an open that failed leaves nothing open
            ctx.bam_bedcov_stats()
    finally:
        bctx.close()
        ctx.close()


def test_second_open_and_accumulate_after_the_result_has_started():
    data = K.bam(K.REFS, K.HAND_ROWS, one_record_per_block=True)
    want = [row[0] for row in K.HAND_EXPECTED]
    ctx, bctx = contexts(data, K.HAND_BED)
    try:
        ctx.bam_bedcov_open(bctx, **K.HAND_PARAMS)
        assert ctx.bam_bedcov_scan(1) == 1
        assert drain(ctx, bctx) == want
        # a second open zeroes the counters and the steps: the same scan gives the same result, not twice the counts
        ctx.bam_bedcov_open(bctx, **K.HAND_PARAMS)
        st = ctx.bam_bedcov_stats()
        assert st["n_rows"] == 0 and st["status"] == 0 and st["n_bed_rows"] == 10
        assert drain(ctx, bctx) == [(0, 0)] * 10
        ctx.rewind()
        # the caller's own loop; the result is started after three batches and starts over with the next accumulate
        sizes, stale = [], None
        while True:
            b = ctx.next_batch(1, duckhts_amd.BEDCOV_COLMASK)
            if stale is not None and b.n_rows:
                with pytest.raises(duckhts_amd.DhtsError, match="not the one dhts_bam_next_batch returned last"):
                    ctx.bam_bedcov_accumulate(stale)
                stale = None
            sizes.append(int(b.n_rows))
            ctx.bam_bedcov_accumulate(b)
            if len(sizes) == 1:
                stale = duckhts_amd.BamBatch()
                C.memmove(C.byref(stale), C.byref(b), C.sizeof(b))
            if len(sizes) == 3:
                cols, st = ctx.bam_bedcov_next(bctx)
                assert K.pairs(cols)[2] == (133, 3) and st == 1           # the first three reads of c1, so far
            if b.status:
                break
        assert sum(sizes) == len(K.HAND_ROWS) and max(sizes) == 1
        assert drain(ctx, bctx) == want
        st = ctx.bam_bedcov_stats()
        assert {k: st[k] for k in M.COUNTERS} == K.HAND_STATS and st["status"] == 1
    finally:
        bctx.close()
        ctx.close()


def test_limits_and_refusals(rng):
    ctx, bctx = contexts(rng, K.GOLDEN_BED)
    L = ctx.L
    try:
        # more BED rows than the limit: the error states the count (the limit itself is 2^27; the test lowers it for the process)
        L.dhts_debug_bedcov_max_rows(13)
        with pytest.raises(duckhts_amd.DhtsError) as e:
            ctx.bam_bedcov_open(bctx)
        assert str(e.value) == "bam_bedcov: the BED file has 14 rows; at most 13 are supported"
        L.dhts_debug_bedcov_max_rows(14)
        ctx.bam_bedcov_open(bctx)
        L.dhts_debug_bedcov_max_rows(0)
        assert M.MAX_BED_ROWS == 1 << 27
        # a shard or a block range of the file, in bam_bin_counts' words
        ctx.set_shard(0, 2)
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_SHARD):
            ctx.bam_bedcov_open(bctx)
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_SHARD):
            ctx.bam_bins_open()
        ctx.set_shard(0, 1)
        ctx.bam_bedcov_open(bctx)
        ctx.set_block_range(0, 1, 1)
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_SHARD):
            ctx.bam_bedcov_scan()
    finally:
        L.dhts_debug_bedcov_max_rows(0)
        bctx.close()
        ctx.close()
    # read_bed's error for a short line, with its line number
    ctx, bctx = contexts(rng, b"CHROMOSOME_I\t1\t2\n#c\nCHROMOSOME_I\t5\n")
    try:
        with pytest.raises(duckhts_amd.DhtsError) as e:
            ctx.bam_bedcov_open(bctx)
        assert str(e.value) == "read_bed: BED line has fewer than 3 tab-delimited fields (line 3)"
    finally:
        bctx.close()
        ctx.close()
    with pytest.raises(duckhts_amd.DhtsError, match="fewer than 3 tab-delimited fields"):
        duckhts_amd.bam_bedcov(rng, b"CHROMOSOME_I\t1\n")
