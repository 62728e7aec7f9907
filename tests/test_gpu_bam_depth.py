"""bam_depth on the device (dhts_bam_depth_*, csrc/bam_depth.hip) against the CPU model bam_depth_ref, row for row: tid, pos, depth, the
counters and the stats.  Contig lengths around the tile, pages of every size with their edges inside runs and at row edges, the three modes,
deletions at run, row and tile edges, the add pass's shapes on the instantiations without words, the cross-check against bam_coverage on the
device, regions, BED targets, the projection, batches, a result taken twice, the table cap and the ABI's states."""
import ctypes as C

import numpy as np
import pytest

import bam_coverage_cases as K
import bam_depth_cases as D
import bam_depth_ref as M
import duckhts_amd
from conftest import read_golden
from test_gpu_bam_coverage import CIGARS, LENGTHS, low_at, parse_rows, ramp

pytestmark = pytest.mark.gpu
R = K.read
FILTERS = ("min_read_len", "min_mapq", "min_baseq", "include_flags", "require_flags", "exclude_flags", "include_deletions", "all_positions")


def model_params(kw):
    p = {k: v for k, v in kw.items() if k in FILTERS}
    p.setdefault("exclude_flags", M.DEFAULT_EXCLUDE)                     # the Python function's default
    return p


def same(got, exp, rows=None, refs=None):
    assert {k: got["stats"][k] for k in M.COUNTERS} == exp["stats"]
    assert sum(got["stats"][k] for k in M.COUNTERS[1:]) == got["stats"]["n_rows"]
    assert got["n_rows"] == exp["n_rows"] == got["stats"]["n_positions"] == sum(got["pages"])
    for k, dt in (("tid", np.int32), ("pos", np.int64), ("depth", np.int32)):
        assert got[k].dtype == dt and len(got[k]) == exp["n_rows"]
        assert np.array_equal(got[k], np.array(exp[k], dt)), (k, got[k].tolist()[:40], exp[k][:40])
    if rows is not None:
        assert got["stats"]["n_target_rows"] == len(rows) and got["stats"]["table_bytes"] == M.table_bytes(rows)


def check(data, **kw):
    got = duckhts_amd.bam_depth(data, **kw)
    refs, reads = M.reads_from_bam(data)
    same(got, M.depth(reads, refs, **model_params(kw)), rows=[(t, 0, l) for t, (_, l) in enumerate(refs)])
    assert got["status"] == 1 and got["contigs"] == [n for n, _ in refs]
    return got


def check_region(data, region, index=None, **kw):
    """the model's reads are the rows of read_bam's own region query"""
    scanned = duckhts_amd.read_bam(data, region=region, index=index)
    refs, _ = M.reads_from_bam(data)
    rows = parse_rows(refs, region)
    got = duckhts_amd.bam_depth(data, region=region, index=index, **kw)
    same(got, M.depth(M.reads_from_cols(scanned), refs, rows=rows, **model_params(kw)), rows=rows)
    assert got["stats"]["n_rows"] == scanned["n_rows"]
    return got


def check_bed(data, bed_rows, **kw):
    refs, reads = M.reads_from_bam(data)
    rows, skipped = M.merge_bed(bed_rows, refs)
    got = duckhts_amd.bam_depth(data, bed=D.bed_text(bed_rows), **kw)
    same(got, M.depth(reads, refs, rows=rows, **model_params(kw)), rows=rows)
    assert got["stats"]["n_bed_skipped"] == skipped
    return got


def open_ctx(data):
    ctx = duckhts_amd.Context(0)
    ctx.open(data)
    ctx.bgzf_index()
    ctx.bam_open()
    return ctx


def drain(ctx, max_rows=0, columns=None):
    parts = []
    while True:
        cols, st = ctx.bam_depth_next(max_rows, columns)
        parts.append(cols)
        if st:
            return {k: None if parts[0][k] is None else np.concatenate([p[k] for p in parts]) for k in duckhts_amd.DEPTH_COLUMNS}, [p["n_rows"] for p in parts]


# ---- emit and pages ----
TILE_REFS = [("zero", 0), ("one", 1), ("t1023", 1023), ("t1024", 1024), ("t1025", 1025), ("t3073", 3 * 1024 + 1)]
TILE_READS = [R(0, 1, 0, 30, "1M", ramp), R(0, 1, 0, 30, "5M", ramp),                                           # the one-base contig, a read that hangs over it
              R(0, 2, 0, 30, "10M", ramp), R(0, 2, 1000, 30, "30M", ramp), R(0, 2, 1022, 30, "1M", ramp),        # the ends of a contig one short of the tile
              R(0, 3, 1000, 30, "24M", ramp), R(0, 3, 1023, 30, "5M", ramp), R(0, 3, 500, 30, "10M5D10M", ramp),  # ... of the tile's length: a run to its last slot
              R(0, 4, 1000, 30, "25M", ramp), R(0, 4, 1020, 30, "10M", ramp), R(0, 4, 1024, 30, "1M", ramp),     # a run over the tile's edge into one position
              R(0, 5, 1000, 30, "60M", ramp), R(0, 5, 1010, 30, "30M", ramp), R(0, 5, 1023, 30, "2M", ramp),     # runs over the first edge; the second tile is empty behind them;
              R(0, 5, 3060, 30, "20M", ramp), R(0, 5, 3072, 30, "1M", ramp), R(0, 5, 5, 30, "3M", ramp)]         # the third is reached again, and the one-position tile
PAGE_SIZES = [1, 2, 255, 256, 257, 1024, 1025, 0]


@pytest.fixture(scope="module")
def tile_file():
    data = K.bam(TILE_REFS, TILE_READS)
    refs, reads = M.reads_from_bam(data)
    return data, {mode: M.depth(reads, refs, exclude_flags=M.DEFAULT_EXCLUDE, all_positions=mode) for mode in (0, 2)}


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("max_rows", PAGE_SIZES)
def test_pages_of_every_size(tile_file, max_rows, mode):
    data, exp = tile_file
    got = duckhts_amd.bam_depth(data, max_rows=max_rows, all_positions=mode)
    same(got, exp[mode])
    n = exp[mode]["n_rows"]
    assert n == (sum(l for _, l in TILE_REFS) if mode == 2 else n) and n > 150
    if max_rows:
        assert got["pages"][:-1] == [max_rows] * ((n - 1) // max_rows) and 0 <= got["pages"][-1] <= max_rows
    else:
        assert got["pages"] == [n]


def test_page_edges_inside_a_run_and_at_a_row_edge(tile_file):
    data, exp = tile_file
    e = exp[2]
    # mode 2: contig "one" ends at result index 1, t1023 at 1024: pages of 1024 cut at the row edge, and inside t1024's run of depth at 1000..
    got = duckhts_amd.bam_depth(data, max_rows=1024, all_positions=2)
    same(got, e)
    assert got["tid"][1023] == 2 and got["tid"][1024] == 3 and got["pos"][1024] == 1
    # mode 0: a page that ends inside the run 1001..1030 of t1023 (its first 13 rows: "one" 1, t1023 10, then the run)
    got = duckhts_amd.bam_depth(data, max_rows=13)
    same(got, exp[0])
    assert got["pos"][12] == 1002 and got["pos"][13] == 1003 and got["tid"][12] == got["tid"][13] == 2


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_a_file_without_a_counted_read(mode):
    reads = [R(0x400, 0, 10, 30, "10M", 30), R(0, 1, 10, 3, "10M", 30), R(4, -1, -1, 0, "*", 30)]
    got = check(K.bam([("a", 1500), ("b", 7)], reads), min_mapq=10, all_positions=mode)
    assert got["n_rows"] == (1507 if mode == 2 else 0) and got["stats"]["n_counted"] == 0


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_header_without_references(mode):
    got = check(K.bam([], [R(4, -1, -1, 0, "*", 30)] * 3), exclude_flags=0, all_positions=mode)
    assert got["n_rows"] == 0 and got["stats"]["n_unplaced"] == 3 and got["pages"] == [0]


# ---- modes ----
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_modes_with_untouched_contigs(mode):
    refs = [("a", 1500), ("b", 1100), ("c", 30), ("d", 2049), ("e", 1024)]
    reads = [R(0, 0, 1000, 30, "50M", ramp), R(0, 2, 5, 30, "10M", ramp), R(0, 4, 1000, 30, "24M", ramp), R(0, 4, 0, 30, "1M", ramp), R(0x400, 1, 10, 30, "10M", ramp)]
    got = check(K.bam(refs, reads), all_positions=mode)
    assert got["n_rows"] == {0: 50 + 10 + 25, 1: 1500 + 30 + 1024, 2: 1500 + 1100 + 30 + 2049 + 1024}[mode]
    assert sorted(set(got["tid"].tolist())) == ([0, 2, 4] if mode < 2 else [0, 1, 2, 3, 4])


def test_mode_1_on_a_contig_touched_by_an_unmapped_flag_read_only():
    refs = [("a", 1030), ("b", 40)]
    reads = [R(0, 0, 1000, 30, "10M", ramp), R(4, 1, 5, 30, "10M", ramp)]
    got = check(K.bam(refs, reads), exclude_flags=0, all_positions=1)
    assert got["n_rows"] == 1070 and got["depth"][1030:].tolist() == [0] * 40 and got["stats"]["n_counted"] == 2
    assert check(K.bam(refs, reads), all_positions=1)["n_rows"] == 1030                  # with the default mask the read is filtered and b stays untouched


# ---- deletions ----
@pytest.mark.parametrize("min_baseq", [0, 20])
@pytest.mark.parametrize("include_deletions", [0, 1])
def test_every_cigar_operation(include_deletions, min_baseq):
    reads = [R(0, i % 2, 1000 + 40 * i, 30, cg, lambda k: 12 + (k * 5) % 17) for i, cg in enumerate(CIGARS)]
    reads.append(R(0, 2, 500, 30, "1S1N", cg="30M5D2I30M10N17M", qual=ramp))              # the real CIGAR in the CG tag
    reads.append(R(0, 2, 900, 30, "6M", 30))
    got = check(K.bam(K.REFS, reads), min_baseq=min_baseq, include_deletions=include_deletions)
    assert got["stats"]["n_counted"] == len(reads)
    if not min_baseq:
        assert int(got["depth"][got["tid"] == 2].sum()) == 77 + 6 + 5 * include_deletions


@pytest.mark.parametrize("min_baseq", [0, 20])
@pytest.mark.parametrize("include_deletions", [0, 1])
def test_deletions_at_run_row_and_tile_edges(include_deletions, min_baseq):
    refs = [("a", 1000), ("b", 3000)]
    reads = [R(0, 1, 100, 30, "20M3D20M", low_at(40, {19})), R(0, 1, 200, 30, "20M3D20M", low_at(40, {20})), R(0, 1, 300, 30, "20M3D20M", low_at(40, {19, 20})),
             R(0, 1, 400, 30, "20M3D20M", 30), R(0, 1, 500, 30, "20M3D20M", 3),
             R(0, 0, 990, 30, "8M6D8M", ramp), R(0, 0, 995, 30, "5M10D5M", ramp), R(0, 0, 997, 30, "3D5M", ramp),          # a D over, up to and from the row's end
             R(0, 1, 1015, 30, "8M6D8M", ramp), R(0, 1, 1019, 30, "5M5D5M", ramp), R(0, 1, 1014, 30, "10M4D4M", ramp),     # ... over, from and up to the tile's edge at 1024
             R(0, 1, 2040, 30, "3D", ramp), R(0, 1, 2046, 30, "4D", ramp), R(0, 1, 2100, 30, "2D5M", ramp), R(0, 1, 2200, 30, "5M3D2N5M", ramp),
             R(0, 1, 2300, 30, "5M2N3D5M", ramp), R(0, 1, 2400, 30, "5M3D", ramp), R(0, 1, 2500, 30, "5M2D3I2D5M", ramp), R(0, 1, 2600, 30, "4M1D1P1D4M", ramp)]
    got = check(K.bam(refs, reads), min_baseq=min_baseq, include_deletions=include_deletions)
    on_b = got["pos"][got["tid"] == 1]
    for p0 in (120, 220, 320, 420, 520):                                                   # the D of 20M3D20M counts whatever lies around it
        assert bool(np.isin([p0 + 1, p0 + 2, p0 + 3], on_b).all()) == bool(include_deletions)
    assert bool(np.isin([2041, 2042, 2043, 2047, 2050, 2101, 2102], on_b).all()) == bool(include_deletions)
    assert not np.isin([2209, 2210, 2306, 2307], on_b).any()                                # N never counts


# ---- the add pass's shapes on the instantiations without words ----
@pytest.mark.parametrize("min_baseq", [0, 20])
@pytest.mark.parametrize("include_deletions", [0, 1])
def test_read_lengths(include_deletions, min_baseq):
    reads = [R(0, 0, 1000 + 3 * i, 30, f"{n}M", ramp) for i, n in enumerate(LENGTHS)] + [R(0, 1, 1000 + 3 * i, 30, f"{n}M2D{n}M", ramp) for i, n in enumerate(LENGTHS)]
    got = check(K.bam(K.REFS, reads), min_baseq=min_baseq, include_deletions=include_deletions)
    assert min_baseq or int(got["depth"].sum()) == 3 * sum(LENGTHS) + 2 * len(LENGTHS) * include_deletions


@pytest.mark.parametrize("min_baseq", [0, 20])
@pytest.mark.parametrize("include_deletions", [0, 1])
def test_qual_at_every_offset_mod_16(include_deletions, min_baseq):
    reads = [R(0, 0, 1000 + i, 30, f"{n}M", lambda k: 5 + (k * 11) % 40, qname="q" * (1 + (i * 5) % 23)) for i in range(32) for n in (37, 38)]
    offs, p = set(), 0
    for i, r in enumerate(reads):
        offs.add((p + 36 + len(r["qname"]) + 1 + 4 + (K.qlen_of(r["cigar"]) + 1) // 2) % 16)
        p += len(K.record(i, r))
    assert offs == set(range(16))
    check(K.bam(K.REFS, reads), min_baseq=min_baseq, include_deletions=include_deletions)


@pytest.mark.parametrize("min_baseq", [0, 20])
@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_reads_around_a_wave(n, min_baseq):
    reads = [R(0, i % 3, 1000 + i, 30, "10M2D10M", ramp) for i in range(n)]
    for include_deletions in (0, 1):
        got = check(K.bam(K.REFS, reads), min_baseq=min_baseq, include_deletions=include_deletions)
        assert got["stats"]["n_counted"] == n


@pytest.mark.parametrize("include_deletions", [0, 1])
def test_5000_reads_at_one_position(include_deletions):
    data = K.bam(K.REFS, [R(0, 0, 777, 30, "1M1D2M", [30, 10, 30])] * 5000)
    got = check(data, min_baseq=20, include_deletions=include_deletions)
    exp = [(778, 5000), (779, 5000), (781, 5000)] if include_deletions else [(778, 5000), (781, 5000)]
    assert list(zip(got["pos"].tolist(), got["depth"].tolist())) == exp


@pytest.mark.parametrize("include_deletions", [0, 1])
@pytest.mark.parametrize("min_baseq", [1, 20, 31, 255])
def test_low_bases(min_baseq, include_deletions):
    reads = [R(0, 0, 1000, 30, "40M", low_at(40, {0})), R(0, 0, 1100, 30, "40M", low_at(40, {39})), R(0, 0, 1200, 30, "40M", low_at(40, {0, 39})),
             R(0, 0, 1300, 30, "40M", 3), R(0, 0, 1400, 30, "41M", low_at(41, set(range(0, 41, 2)))), R(0, 0, 1500, 30, "41M", low_at(41, set(range(1, 41, 2)))),
             R(0, 0, 1600, 30, "20M3D20M", low_at(40, {19, 20})), R(0, 0, 1700, 30, "20M3I20M", low_at(43, {19, 23})), R(0, 0, 1800, 30, "20M3I20M", low_at(43, {20, 21, 22}))]
    # a low base on either side of every 16-byte boundary of QUAL, whatever QUAL's own offset is
    reads += [R(0, 1, 2000 + 100 * j, 30, "64M", low_at(64, {j, j + 16, j + 32}), qname="n" * (1 + j % 5)) for j in range(16)]
    reads += [R(0, 1, 5000 + 100 * j, 30, "32M1D32M", low_at(64, set(range(64)) - {j, j + 17, j + 40})) for j in range(16)]
    check(K.bam(K.REFS, reads), min_baseq=min_baseq, include_deletions=include_deletions)


def test_the_hand_written_table():
    data = D.bam(D.HAND_REFS, D.HAND_READS)
    for kw, exp in ((dict(), D.HAND_ROWS), (dict(include_deletions=1), D.HAND_ROWS_DEL), (dict(all_positions=1), D.hand_rows_all(1)), (dict(all_positions=2), D.hand_rows_all(2))):
        got = check(data, **D.HAND_PARAMS, **kw)
        assert list(zip(got["tid"].tolist(), got["pos"].tolist(), got["depth"].tolist())) == exp
        assert {k: got["stats"][k] for k in M.COUNTERS} == D.HAND_STATS


# ---- the cross-check on the device: bam_coverage's sums of the same table ----
@pytest.fixture(scope="module")
def rng():
    return read_golden("range.bam")


def cross_check(data, **kw):
    cov = duckhts_amd.bam_coverage(data, min_depth=1, **kw)
    got = check(data, **kw)
    n_ref = len(got["contigs"])
    assert np.bincount(got["tid"], weights=got["depth"], minlength=n_ref).astype(np.int64).tolist() == cov["sum_depth"].tolist()
    assert np.bincount(got["tid"], minlength=n_ref).tolist() == cov["covbases"].tolist()
    assert {k: got["stats"][k] for k in M.COUNTERS} == {k: cov["stats"][k] for k in M.COUNTERS}


@pytest.mark.parametrize("min_baseq", [0, 25])
def test_sums_equal_bam_coverages_on_the_golden_file(rng, min_baseq):
    cross_check(rng, min_baseq=min_baseq)


def test_sums_equal_bam_coverages_on_twenty_contigs():
    refs = [(f"k{t}", 700 + 211 * t) for t in range(20)]
    reads = [R(0, (i * 7) % 20, (i * 131) % 900, 30, ("30M", "10M5D10M", "4S26M", "12M3N12M")[i % 4], ramp) for i in range(400)]
    cross_check(K.bam(refs, reads), min_baseq=12)


# ---- regions ----
def test_regions_on_the_golden_file(rng):
    bai = read_golden("range.bam.bai")
    region = "CHROMOSOME_I:1001-1100,CHROMOSOME_I:901-1000,CHROMOSOME_II:1-5000,CHROMOSOME_I:1101-1150,CHROMOSOME_I:1151-1151"
    got = check_region(rng, region, index=bai, all_positions=2)
    assert got["n_rows"] == sum(e - b for _, b, e in parse_rows(M.reads_from_bam(rng)[0], region)) and got["pos"][:100].tolist() == list(range(1001, 1101)) and got["pos"][100] == 901
    got = check_region(rng, region, min_baseq=25, max_rows=77)                           # without the index: the whole file is scanned and filtered
    assert got["n_rows"] > 0
    check_region(rng, region, index=bai, include_deletions=1, all_positions=1)
    check_region(rng, "CHROMOSOME_I")


@pytest.mark.parametrize("include_deletions", [0, 1])
def test_reads_across_several_regions(include_deletions):
    reads = [R(0, 0, 85, 30, "60M", ramp), R(0, 0, 95, 30, "10M", ramp), R(0, 0, 99, 30, "1M", ramp), R(0, 0, 100, 30, "1M", ramp), R(0, 0, 90, 30, "8M6D8M", ramp),
             R(0, 0, 104, 30, "5M20N5M", ramp), R(0, 0, 60, 30, "20M", ramp), R(0, 1, 95, 30, "30M", ramp), R(0, 0, 140, 30, "3S10M", ramp)]
    region = "c1:121-130,c1:91-100,c2:100-100,c1:101-110,c1:141-141"
    for mode, max_rows in ((0, 0), (2, 7)):
        got = check_region(K.bam(K.REFS, reads), region, min_baseq=15, include_deletions=include_deletions, all_positions=mode, max_rows=max_rows)
        if mode == 2:
            assert got["pos"].tolist() == list(range(121, 131)) + list(range(91, 101)) + [100] + list(range(101, 111)) + [141] and got["tid"][20] == 1


def test_last_kilobase_of_a_long_contig():
    n = (1 << 31) - 1
    refs = [("small", 5000), ("long", n)]
    reads = [R(0, 0, 100 + i, 30, "10M", ramp) for i in range(10)] + [R(0, 1, n - 1000 + 7 * i, 30, "20M3D20M", ramp) for i in range(130)] + [R(0, 1, n - 2, 30, "10M", ramp)]
    got = check_region(K.bam(refs, reads), f"long:{n - 999}-{n}", min_baseq=15, include_deletions=1, all_positions=2)
    assert got["n_rows"] == 1000 and int(got["pos"][-1]) == n and int(got["pos"][0]) == n - 999 and got["depth"][-1] > 0


def test_overlapping_regions_are_refused(rng):
    with pytest.raises(duckhts_amd.DhtsError) as e:
        duckhts_amd.bam_depth(rng, region="CHROMOSOME_I:1-1000,CHROMOSOME_II:1-10,CHROMOSOME_I:1000-1200")
    assert str(e.value) == M.err_overlap("CHROMOSOME_I:1-1000", "CHROMOSOME_I:1000-1200")
    with pytest.raises(duckhts_amd.DhtsError) as e:
        duckhts_amd.bam_depth(rng, region="CHROMOSOME_I:500-600,CHROMOSOME_I")
    assert str(e.value) == M.err_overlap("CHROMOSOME_I:500-600", "CHROMOSOME_I")
    duckhts_amd.bam_depth(rng, region="CHROMOSOME_I:1-1000,CHROMOSOME_I:1001-1200")       # adjacent


# ---- BED targets ----
@pytest.mark.parametrize("mode", [0, 2])
def test_the_bed_merge_on_the_device(mode):
    reads = [R(0, 0, (i * 37) % 990, 30, ("30M", "10M5D10M", "4S26M", "12M3N12M")[i % 4], ramp) for i in range(120)] + [R(0, 1, (i * 29) % 490, 30, "25M", ramp) for i in range(40)]
    got = check_bed(K.bam(D.BED_REFS, reads), D.BED_ROWS, all_positions=mode, include_deletions=1, max_rows=100)
    assert got["stats"]["n_target_rows"] == len(D.BED_MERGED) and got["stats"]["n_bed_skipped"] == D.BED_SKIPPED
    if mode == 2:
        assert got["n_rows"] == sum(e - b for _, b, e in D.BED_MERGED)


def test_300_one_base_intervals():
    refs = [("a", 2000)]
    reads = [R(0, 0, 3 * i, 30, "10M", ramp) for i in range(500)]
    bed_rows = [(b"a", 5 * i, 5 * i + 1) for i in range(300)]
    got = check_bed(K.bam(refs, reads), bed_rows, all_positions=2)
    assert got["n_rows"] == 300 and got["stats"]["table_bytes"] == 300 * 4096 and got["pos"].tolist() == [5 * i + 1 for i in range(300)]


def test_a_bed_and_a_region_are_refused(rng):
    with pytest.raises(duckhts_amd.DhtsError) as e:
        duckhts_amd.bam_depth(rng, region="CHROMOSOME_I:1-1000", bed=b"CHROMOSOME_I\t0\t10\n")
    assert str(e.value) == M.ERR_BED_AND_REGION


# ---- projection ----
def test_projection(rng):
    full = duckhts_amd.bam_depth(rng, max_rows=300)
    for cols in (["depth"], ["pos"], ["pos", "tid"]):
        got = duckhts_amd.bam_depth(rng, max_rows=300, columns=cols)
        assert got["n_rows"] == full["n_rows"] and got["pages"] == full["pages"]
        for k in duckhts_amd.DEPTH_COLUMNS:
            assert (got[k] is None) if k not in cols else np.array_equal(got[k], full[k]), k
    # the batch itself: null pointers for the columns that were left out, and 4 bytes per row for depth alone
    ctx = open_ctx(rng)
    try:
        ctx.bam_depth_open(exclude_flags=0x704)
        ctx.bam_depth_scan()
        b = duckhts_amd.BedBatch()
        ctx._chk(ctx.L.dhts_bam_depth_next(ctx.h, 100, 1 << duckhts_amd.DEPTH_COLUMNS.index("depth"), C.byref(b)))
        assert b.n_rows == 100 and b.n_cols == 3 and not b.cols[0].fixed and not b.cols[1].fixed and b.cols[2].fixed and not b.cols[2].valid
        assert ctx.L.dhts_bam_depth_batch_host_bytes(C.byref(b)) == 400
    finally:
        ctx.close()


# ---- batches, pages, a result taken twice ----
def test_one_record_per_block_and_many_blocks():
    reads = [R((0x400 if i % 11 == 0 else 0), i % 3, 1000 + 13 * i, 30, ("10M", "5M2D5M", "3S7M", "5M20N5M")[i % 4], ramp) for i in range(151)]
    data = K.bam(K.REFS, reads, one_record_per_block=True)
    one = check(data, min_baseq=14, include_deletions=1)
    for max_blocks in (1, 3):
        many = check(data, min_baseq=14, include_deletions=1, max_blocks=max_blocks)
        assert many["stats"] == one["stats"]


def test_accumulate_after_a_page_was_taken():
    reads = [R(0, i % 3, 100 + 5 * i, 30, "10M", ramp) for i in range(12)]
    data = K.bam(K.REFS, reads, one_record_per_block=True)
    refs, mreads = M.reads_from_bam(data)
    ctx = open_ctx(data)
    try:
        ctx.bam_depth_open(min_baseq=15)
        assert ctx.bam_depth_stats()["n_positions"] == 0
        seen, stale = 0, None
        while True:
            b = ctx.next_batch(1, duckhts_amd.DEPTH_COLMASK)
            if stale is not None and b.n_rows:
                with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_STALE):
                    ctx.bam_depth_accumulate(stale)
                stale = None
            ctx.bam_depth_accumulate(b)
            seen += int(b.n_rows)
            if seen == 1 and stale is None:
                stale = duckhts_amd.BamBatch()
                C.memmove(C.byref(stale), C.byref(b), C.sizeof(b))
            if seen == 5:                                                  # a whole result in the middle: the reads so far; the table and the counters stay intact
                exp = M.depth(mreads[:seen], refs, min_baseq=15)
                cols, sizes = drain(ctx, 7)
                assert sum(sizes) == exp["n_rows"] and cols["pos"].tolist() == exp["pos"] and cols["depth"].tolist() == exp["depth"] and cols["tid"].tolist() == exp["tid"]
                assert ctx.bam_depth_stats()["n_positions"] == exp["n_rows"]
            if seen == 9:                                                  # one page of a result taken: the next accumulate starts the result over
                exp = M.depth(mreads[:seen], refs, min_baseq=15)
                cols, st = ctx.bam_depth_next(4)
                assert cols["n_rows"] == 4 and st == 0 and cols["pos"].tolist() == exp["pos"][:4] and cols["depth"].tolist() == exp["depth"][:4]
            if b.status:
                break
        exp = M.depth(mreads, refs, min_baseq=15)
        assert ctx.bam_depth_stats()["n_positions"] == 0                   # (no result of the table as it is now was taken)
        cols, sizes = drain(ctx)
        assert sizes == [exp["n_rows"]] and cols["pos"].tolist() == exp["pos"] and cols["depth"].tolist() == exp["depth"]
        st = ctx.bam_depth_stats()
        assert {k: st[k] for k in M.COUNTERS} == exp["stats"] and st["n_positions"] == exp["n_rows"] and st["status"] == 1
        cols, st = ctx.bam_depth_next()                                     # behind the last page: nothing, and still the end
        assert cols["n_rows"] == 0 and st == 1
        # a result taken twice: a second open zeroes everything
        ctx.bam_depth_open(all_positions=2)
        st = ctx.bam_depth_stats()
        assert st["n_rows"] == 0 and st["status"] == 0 and st["n_target_rows"] == 3 and st["n_positions"] == 0 and st["table_bytes"] == M.table_bytes([(t, 0, l) for t, (_, l) in enumerate(refs)])
        cols, sizes = drain(ctx, 100000)
        assert sum(sizes) == 300000 and not cols["depth"].any() and cols["pos"][99999] == 100000 and cols["pos"][100000] == 1
    finally:
        ctx.close()


def test_a_cigar_longer_than_l_seq_ends_the_stream():
    reads = [R(0, 0, 1000, 30, "20M", 30), R(0, 0, 1100, 30, "20M", [30] * 10, seq="A" * 10, l_seq=10), R(0, 0, 1200, 30, "20M", 30)]
    data = K.bam(K.REFS, reads)
    got = duckhts_amd.bam_depth(data)
    scanned = duckhts_amd.read_bam(data)
    refs, mreads = M.reads_from_bam(data)
    assert got["status"] < 0 and got["status"] == scanned["status"] and scanned["n_rows"] < 3
    same(got, M.depth(mreads[:scanned["n_rows"]], refs, exclude_flags=M.DEFAULT_EXCLUDE))
    reads[1] = R(4, 0, 1100, 30, "20M", [30] * 10, seq="A" * 10)                          # with FLAG & 4 the record is taken, and such a read has no counted base
    got = check(K.bam(K.REFS, reads), exclude_flags=0)
    assert got["n_rows"] == 40 and got["stats"]["n_counted"] == 3


# ---- limits and states ----
def test_the_table_cap(rng):
    refs, _ = M.reads_from_bam(rng)
    need = M.table_bytes([(t, 0, l) for t, (_, l) in enumerate(refs)])
    ctx = open_ctx(rng)
    L = ctx.L
    try:
        L.dhts_debug_coverage_max_table_bytes(need - 1)
        with pytest.raises(duckhts_amd.DhtsError) as e:
            ctx.bam_depth_open()
        assert str(e.value) == M.err_table(need, need - 1)
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_NOT_OPEN):    # an open that failed leaves nothing open
            ctx.bam_depth_stats()
        L.dhts_debug_coverage_max_table_bytes(need)
        ctx.bam_depth_open()
        assert ctx.bam_depth_stats()["table_bytes"] == need
    finally:
        L.dhts_debug_coverage_max_table_bytes(0)
        ctx.close()


def test_calls_in_the_wrong_state_and_refusals(rng):
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(rng)
        ctx.bgzf_index()
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_BAM_NOT_OPEN):
            ctx.bam_depth_open()
        ctx.bam_open()
        b = ctx.next_batch(0, duckhts_amd.DEPTH_COLMASK)
        for call in (lambda: ctx.bam_depth_accumulate(b), ctx.bam_depth_scan, ctx.bam_depth_stats, ctx.bam_depth_next):
            with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_NOT_OPEN):
                call()
        for kw, msg in ((dict(min_mapq=256), M.err_range("min_mapq")), (dict(min_mapq=-1), M.err_range("min_mapq")), (dict(min_baseq=256), M.err_range("min_baseq")),
                        (dict(min_baseq=-1), M.err_range("min_baseq")), (dict(include_flags=65536), M.err_range("include_flags")), (dict(require_flags=-1), M.err_range("require_flags")),
                        (dict(exclude_flags=70000), M.err_range("exclude_flags")), (dict(min_read_len=-1), M.ERR_READ_LEN), (dict(include_deletions=2), M.ERR_DELETIONS),
                        (dict(include_deletions=-1), M.ERR_DELETIONS), (dict(all_positions=3), M.ERR_ALL), (dict(all_positions=-1), M.ERR_ALL),
                        # wrong in two ways: the first in the order of the checks is reported
                        (dict(min_read_len=-1, min_mapq=256), M.ERR_READ_LEN), (dict(min_baseq=-1, include_flags=65536), M.err_range("min_baseq")),
                        (dict(require_flags=-1, exclude_flags=70000), M.err_range("require_flags")), (dict(include_deletions=2, exclude_flags=70000), M.err_range("exclude_flags")),
                        (dict(include_deletions=2, all_positions=3), M.ERR_DELETIONS)):
            with pytest.raises(duckhts_amd.DhtsError) as e:
                ctx.bam_depth_open(**kw)
            assert str(e.value) == msg
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_NOT_OPEN):
            ctx.bam_depth_stats()
        with pytest.raises(duckhts_amd.DhtsError, match="the BED context has to be a second context"):
            ctx.bam_depth_open(bed_ctx=ctx)
        other = duckhts_amd.Context(0)
        try:
            other.open(b"c\t0\t1\n")
            with pytest.raises(duckhts_amd.DhtsError, match="the BED context is not open"):
                ctx.bam_depth_open(bed_ctx=other)
        finally:
            other.close()
        # a shard or a block range of the file
        ctx.set_shard(0, 2)
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_SHARD):
            ctx.bam_depth_open()
        ctx.set_shard(0, 1)
        ctx.bam_depth_open()
        ctx.set_block_range(0, 1, 1)
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_SHARD):
            ctx.bam_depth_scan()
    finally:
        ctx.close()
