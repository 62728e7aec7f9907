"""bam_coverage on the device (dhts_bam_coverage_*, csrc/bam_coverage.hip) against the CPU model bam_coverage_ref, bit for bit: the counters,
the nine columns and the three sums.  Read lengths and QUAL alignments around the 16-byte pieces, reads per wave, every CIGAR operation,
quality thresholds at run and piece boundaries, odd quality fields, the parameters, row edges, contigs and tiles, regions, batches, a result
taken twice, the table cap and the ABI's states."""
import ctypes as C

import numpy as np
import pytest

import bam_coverage_cases as K
import bam_coverage_ref as M
import duckhts_amd
from conftest import read_golden

pytestmark = pytest.mark.gpu
R = K.read


def model_params(kw):
    p = {k: v for k, v in kw.items() if k in ("min_read_len", "min_mapq", "min_baseq", "include_flags", "require_flags", "exclude_flags", "min_depth")}
    p.setdefault("exclude_flags", M.DEFAULT_EXCLUDE)                     # the Python function's default
    return p


def same(got, exp):
    assert {k: got["stats"][k] for k in M.COUNTERS} == exp["stats"]
    assert sum(got["stats"][k] for k in M.COUNTERS[1:]) == got["stats"]["n_rows"]
    assert got["n_rows"] == exp["n_rows"]
    assert list(got["chrom"]) == exp["chrom"]
    for k in M.COLUMNS[1:5] + M.SUMS:
        assert got[k].dtype == np.int64 and got[k].tolist() == exp[k], k
    for k in M.COLUMNS[5:]:
        assert got[k].dtype == np.float64 and got[k].tobytes() == np.array(exp[k], np.float64).tobytes(), (k, got[k].tolist(), exp[k])
    # the invariant: sum_depth is the model's number of counted bases on the row, and covbases fits the row
    for r in range(exp["n_rows"]):
        assert int(got["sum_depth"][r]) == sum(exp["depth"][r].values()) and 0 <= int(got["covbases"][r]) <= int(got["end"][r]) - int(got["start"][r])


def check(data, **kw):
    got = duckhts_amd.bam_coverage(data, **kw)
    refs, reads = M.reads_from_bam(data)
    same(got, M.coverage(reads, refs, **model_params(kw)))
    assert got["status"] == 1
    return got


def parse_rows(refs, region):
    """(tid, beg, end) per region token 'name' or 'name:a-b' (1-based, closed), clipped to the contig"""
    names = [n for n, _ in refs]
    rows = []
    for tok in region.split(","):
        name, _, span = tok.partition(":")
        t = names.index(name.encode())
        b, e = (0, refs[t][1]) if not span else (int(span.split("-")[0].replace(",", "")) - 1, int(span.split("-")[1].replace(",", "")))
        rows.append((t, min(b, refs[t][1]), min(e, refs[t][1])))
    return rows


def check_region(data, region, index=None, **kw):
    """the model's reads are the rows of read_bam's own region query"""
    scanned = duckhts_amd.read_bam(data, region=region, index=index)
    refs, _ = M.reads_from_bam(data)
    exp = M.coverage(M.reads_from_cols(scanned), refs, rows=parse_rows(refs, region), **model_params(kw))
    got = duckhts_amd.bam_coverage(data, region=region, index=index, **kw)
    same(got, exp)
    assert got["stats"]["n_rows"] == scanned["n_rows"]
    return got


def ramp(k):
    return 10 + (k * 7) % 31


BQ = [0, 20]

# ---- read lengths around the 16-byte pieces, and QUAL at every offset mod 16 ----
LENGTHS = [1, 15, 16, 17, 31, 33, 63, 64, 65, 150, 300]


@pytest.mark.parametrize("min_baseq", BQ)
def test_read_lengths(min_baseq):
    reads = [R(0, 0, 1000 + 3 * i, 30, f"{n}M", ramp) for i, n in enumerate(LENGTHS)]
    got = check(K.bam(K.REFS, reads), min_baseq=min_baseq)
    assert int(got["numreads"][0]) == len(LENGTHS) and (min_baseq or int(got["sum_depth"][0]) == sum(LENGTHS))


@pytest.mark.parametrize("min_baseq", BQ)
def test_qual_at_every_offset_mod_16(min_baseq):
    # the qname's length moves CIGAR, SEQ and QUAL by a byte each; odd and even l_seq move QUAL by (l_seq + 1) / 2
    reads = [R(0, 0, 1000 + i, 30, f"{n}M", lambda k: 5 + (k * 11) % 40, qname="q" * (1 + (i * 5) % 23)) for i in range(32) for n in (37, 38)]
    offs = set()
    p = 0
    for i, r in enumerate(reads):
        rec = K.record(i, r)
        n = K.qlen_of(r["cigar"])
        offs.add((p + 36 + len(r["qname"]) + 1 + 4 + (n + 1) // 2) % 16)
        p += len(rec)
    assert offs == set(range(16))
    check(K.bam(K.REFS, reads), min_baseq=min_baseq)


# ---- what a wave of the add kernel can meet ----
@pytest.mark.parametrize("min_baseq", BQ)
@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_reads_around_a_wave(n, min_baseq):
    reads = [R(0, i % 3, 1000 + i, 30, "20M", ramp) for i in range(n)]
    got = check(K.bam(K.REFS, reads), min_baseq=min_baseq)
    assert got["stats"]["n_counted"] == n


@pytest.mark.parametrize("min_depth", [1, 2, 1000, 5001])
def test_5000_reads_at_one_position(min_depth):
    data = K.bam(K.REFS, [R(0, 0, 777, 30, "3M", [30, 10, 30])] * 5000)
    got = check(data, min_depth=min_depth, min_baseq=20)
    assert int(got["covbases"][0]) == (2 if min_depth <= 5000 else 0) and int(got["sum_depth"][0]) == 10000 and int(got["numreads"][0]) == 5000


def test_uncounted_rows_inside_runs():
    reads = [R((0x200 if i % 5 == 2 else 0), 0, 1100 + i, (0 if i % 7 == 3 else 30), "12M" if i % 11 else "3M", ramp) for i in range(200)]
    got = check(K.bam(K.REFS, reads), min_mapq=1, min_read_len=4, min_baseq=15)
    st = got["stats"]
    assert st["n_flag_filtered"] == 40 and st["n_short"] > 0 and st["n_low_mapq"] > 0 and st["n_counted"] < 160


# ---- CIGAR ----
CIGARS = ["*", "4S", "3S4M2I4M3S", "5M3D5M", "5M100N5M", "4=1X4=", "2H5M1P5M2H", "3D", "0M", "5M0D5M", "2D5M", "5M3D2N5M", "3M1D1N1D3M", "2H3S20M1I20M2D17M4S1H",
          "5M0I5M0N0D5M", "1M1I1M1D1M1N1M1P1M"]


@pytest.mark.parametrize("min_baseq", BQ)
def test_every_cigar_operation(min_baseq):
    reads = [R(0, i % 2, 1000 + 40 * i, 30, cg, lambda k: 12 + (k * 5) % 17) for i, cg in enumerate(CIGARS)]
    reads.append(R(0, 2, 500, 30, "1S1N", cg="30M5D2I30M10N17M", qual=ramp))              # the real CIGAR in the CG tag
    reads.append(R(0, 2, 900, 30, "6M", 30))
    got = check(K.bam(K.REFS, reads), min_baseq=min_baseq)
    assert got["stats"]["n_counted"] == len(reads) and int(got["numreads"][2]) == 2
    if not min_baseq:
        assert int(got["sum_depth"][2]) == 77 + 6


# ---- qualities against min_baseq ----
def low_at(n, low, hi=30, lo=3):
    return [lo if k in low else hi for k in range(n)]


@pytest.mark.parametrize("min_baseq", [1, 20, 31, 255])
def test_low_bases(min_baseq):
    reads = [R(0, 0, 1000, 30, "40M", low_at(40, {0})), R(0, 0, 1100, 30, "40M", low_at(40, {39})), R(0, 0, 1200, 30, "40M", low_at(40, {0, 39})),
             R(0, 0, 1300, 30, "40M", 3), R(0, 0, 1400, 30, "41M", low_at(41, set(range(0, 41, 2)))), R(0, 0, 1500, 30, "41M", low_at(41, set(range(1, 41, 2)))),
             R(0, 0, 1600, 30, "20M3D20M", low_at(40, {19, 20})), R(0, 0, 1700, 30, "20M3I20M", low_at(43, {19, 23})), R(0, 0, 1800, 30, "20M3I20M", low_at(43, {20, 21, 22}))]
    # a low base on either side of every 16-byte boundary of QUAL, whatever QUAL's own offset is
    reads += [R(0, 1, 2000 + 100 * j, 30, "64M", low_at(64, {j, j + 16, j + 32}), qname="n" * (1 + j % 5)) for j in range(16)]
    reads += [R(0, 1, 5000 + 100 * j, 30, "64M", low_at(64, set(range(64)) - {j, j + 17, j + 40})) for j in range(16)]
    check(K.bam(K.REFS, reads), min_baseq=min_baseq)


@pytest.mark.parametrize("min_baseq", [0, 1, 255])
def test_odd_quality_fields(min_baseq):
    reads = [R(0, 0, 1000, 30, "20M", 0, raw_qual=b"\xff" * 20),                        # QUAL all 0xff: 255 each, as samtools takes it
             R(0, 0, 1100, 30, "20M", [0] * 20),
             R(0, 0, 1200, 30, "10M2D10M", [], seq="*"),                                # l_seq = 0 with a CIGAR: every base counts and adds 0
             R(0, 1, 1300, 30, "300M", [], seq="*")]
    got = check(K.bam(K.REFS, reads), min_baseq=min_baseq)
    assert int(got["sum_depth"][1]) == 300 and int(got["sum_baseq"][1]) == 0
    assert int(got["sum_baseq"][0]) == 20 * 255


def test_a_cigar_longer_than_l_seq_ends_the_stream():
    """a record whose CIGAR does not fit its l_seq > 0 is one the scan refuses (bam_read1's check): the stream ends there on an error, the
    reads in front of it are counted, and the result carries the status"""
    reads = [R(0, 0, 1000, 30, "20M", 30), R(0, 0, 1100, 30, "20M", [30] * 10, seq="A" * 10, l_seq=10), R(0, 0, 1200, 30, "20M", 30)]
    data = K.bam(K.REFS, reads)
    got = duckhts_amd.bam_coverage(data)
    scanned = duckhts_amd.read_bam(data)
    refs, mreads = M.reads_from_bam(data)
    assert got["status"] < 0 and got["status"] == scanned["status"] and scanned["n_rows"] < 3
    same(got, M.coverage(mreads[:scanned["n_rows"]], refs, exclude_flags=M.DEFAULT_EXCLUDE))
    # with FLAG & 4 the record is taken, and such a read has no counted base
    reads[1] = R(4, 0, 1100, 30, "20M", [30] * 10, seq="A" * 10)
    got = check(K.bam(K.REFS, reads), exclude_flags=0)
    assert int(got["numreads"][0]) == 3 and int(got["sum_depth"][0]) == 40


# ---- parameters ----
PARAM_READS = [R(0, 0, 100, 30, "50M", ramp), R(16, 0, 120, 3, "30M", ramp), R(0x40, 0, 130, 60, "8M", ramp), R(0x80 | 16, 1, 100, 20, "50M", ramp), R(4, 1, 150, 0, "20M", ramp),
               R(4, -1, -1, 0, "*", 30), R(0x400, 0, 100, 30, "50M", ramp), R(0x100, 1, 100, 30, "50M", ramp), R(0x200, 2, 100, 30, "50M", ramp), R(0, 2, 10, 255, "1M", 255)]


@pytest.mark.parametrize("kw", [dict(), dict(min_read_len=9), dict(min_read_len=51), dict(min_mapq=4), dict(min_mapq=255), dict(min_depth=2), dict(min_depth=1000),
                                dict(exclude_flags=0), dict(exclude_flags=0, min_baseq=25), dict(require_flags=0x10), dict(include_flags=0xc0), dict(exclude_flags=0x10, include_flags=0x40),
                                dict(min_read_len=9, min_mapq=4, min_baseq=20, min_depth=2)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()) or "defaults")
def test_parameters(kw):
    got = check(K.bam(K.REFS, PARAM_READS), **kw)
    if kw == dict(exclude_flags=0):
        # FLAG & 4 on a placed read: counted for numreads and MAPQ, no base
        assert int(got["numreads"][1]) == 3 and int(got["sum_depth"][1]) == 100 and got["stats"]["n_unplaced"] == 1


def test_the_hand_written_table():
    data = K.bam(K.HAND_REFS, K.HAND_READS)
    got = check(data, **K.HAND_PARAMS)
    for r, exp in enumerate(K.HAND_EXPECTED):
        assert (got["chrom"][r],) + tuple(got[k][r].item() for k in M.COLUMNS[1:] + M.SUMS) == exp
    assert {k: got["stats"][k] for k in M.COUNTERS} == K.HAND_STATS


# ---- row edges, contigs, tiles ----
@pytest.mark.parametrize("min_baseq", BQ)
def test_row_edges(min_baseq):
    refs = [("a", 1000), ("empty", 0), ("one", 1), ("b", 3 * 1024 + 1)]
    reads = [R(0, 0, 990, 30, "20M", ramp), R(0, 0, 999, 30, "1M", ramp), R(0, 0, 1000, 30, "5M", ramp), R(0, 0, 2000, 30, "5M", ramp), R(0, 0, 980, 30, "10M5D10M", ramp),
             R(0, 0, 985, 30, "15M10I5M", ramp), R(0, 2, 0, 30, "10M", ramp), R(0, 2, 0, 30, "1M", ramp), R(0, 2, 1, 30, "1M", ramp), R(0, 1, 0, 30, "5M", ramp),
             R(0, 3, 0, 30, "5M", ramp), R(0, 3, 1020, 30, "10M", ramp), R(0, 3, 2040, 30, "20M", ramp), R(0, 3, 3065, 30, "20M", ramp), R(0, 3, 3072, 30, "1M", ramp), R(0, 3, 3073, 30, "1M", ramp)]
    got = check(K.bam(refs, reads), min_baseq=min_baseq)
    assert got["end"].tolist() == [1000, 0, 1, 3073] and got["stats"]["n_outside"] == 5
    assert got["coverage"][1] == 0.0 and int(got["numreads"][2]) == 2 and (min_baseq or int(got["covbases"][2]) == 1)


def test_header_without_references():
    got = check(K.bam([], [R(4, -1, -1, 0, "*", 30)] * 3), exclude_flags=0)
    assert got["n_rows"] == 0 and got["stats"]["n_unplaced"] == 3 and len(got["coverage"]) == 0


def test_twenty_contigs_that_are_no_multiple_of_the_tile():
    refs = [(f"k{t}", 700 + 211 * t) for t in range(20)]
    reads = [R(0, (i * 7) % 20, (i * 131) % 900, 30, ("30M", "10M5D10M", "4S26M", "12M3N12M")[i % 4], ramp) for i in range(400)]
    got = check(K.bam(refs, reads), min_baseq=12)
    assert got["n_rows"] == 20 and int((got["numreads"] > 0).sum()) == 20


# ---- regions ----
@pytest.fixture(scope="module")
def rng():
    return read_golden("range.bam")


def test_regions_on_the_golden_file(rng):
    bai = read_golden("range.bam.bai")
    # two regions on one contig with reads across both, out of order, adjacent ones, and another contig
    region = "CHROMOSOME_I:1001-1100,CHROMOSOME_I:901-1000,CHROMOSOME_II:1-5000,CHROMOSOME_I:1101-1150"
    got = check_region(rng, region, index=bai)
    assert got["start"].tolist() == [1000, 900, 0, 1100] and int(got["numreads"][0]) > 0 and int(got["numreads"][1]) > 0
    check_region(rng, region, min_baseq=25, min_depth=2)                                 # without the index: the whole file is scanned and filtered
    whole = check_region(rng, "CHROMOSOME_I")
    assert whole["end"].tolist() == [M.reads_from_bam(rng)[0][0][1]]


@pytest.mark.parametrize("min_baseq", BQ)
def test_reads_across_several_regions(min_baseq):
    # adjacent regions, one behind a gap, one of a single base, given out of order; reads that cover one, two and all of them, and a deletion over an edge
    reads = [R(0, 0, 85, 30, "60M", ramp), R(0, 0, 95, 30, "10M", ramp), R(0, 0, 99, 30, "1M", ramp), R(0, 0, 100, 30, "1M", ramp), R(0, 0, 90, 30, "8M6D8M", ramp),
             R(0, 0, 104, 30, "5M20N5M", ramp), R(0, 0, 60, 30, "20M", ramp), R(0, 1, 95, 30, "30M", ramp), R(0, 0, 140, 30, "3S10M", ramp)]
    got = check_region(K.bam(K.REFS, reads), "c1:121-130,c1:91-100,c2:100-100,c1:101-110,c1:141-141", min_baseq=min_baseq)
    assert got["start"].tolist() == [120, 90, 99, 100, 140] and got["numreads"].tolist() == [2, 4, 1, 5, 2]


def test_defaults_on_the_golden_file(rng):
    got = check(rng)
    assert got["n_rows"] == len(M.reads_from_bam(rng)[0]) and got["stats"]["n_rows"] == 112 and got["chrom"][0] == b"CHROMOSOME_I"
    check(rng, min_baseq=30, min_mapq=1, exclude_flags=0x10)


def test_last_kilobase_of_a_long_contig():
    n = (1 << 31) - 1
    refs = [("small", 5000), ("long", n)]
    reads = [R(0, 0, 100 + i, 30, "10M", ramp) for i in range(10)] + [R(0, 1, n - 1000 + 7 * i, 30, "20M3D20M", ramp) for i in range(130)] + [R(0, 1, n - 2, 30, "10M", ramp)]
    data = K.bam(refs, reads)
    got = check_region(data, f"long:{n - 999}-{n}", min_baseq=15)
    assert got["start"].tolist() == [n - 1000] and got["end"].tolist() == [n] and int(got["numreads"][0]) == 131


def test_overlapping_regions_are_refused(rng):
    with pytest.raises(duckhts_amd.DhtsError) as e:
        duckhts_amd.bam_coverage(rng, region="CHROMOSOME_I:1-1000,CHROMOSOME_II:1-10,CHROMOSOME_I:1000-1200")
    assert str(e.value) == M.err_overlap("CHROMOSOME_I:1-1000", "CHROMOSOME_I:1000-1200")
    with pytest.raises(duckhts_amd.DhtsError) as e:
        duckhts_amd.bam_coverage(rng, region="CHROMOSOME_I:500-600,CHROMOSOME_I")
    assert str(e.value) == M.err_overlap("CHROMOSOME_I:500-600", "CHROMOSOME_I")
    duckhts_amd.bam_coverage(rng, region="CHROMOSOME_I:1-1000,CHROMOSOME_I:1001-1200")     # adjacent


# ---- batches, pages, a result taken twice ----
def test_one_record_per_block_and_many_blocks():
    reads = [R((0x400 if i % 11 == 0 else 0), i % 3, 1000 + 13 * i, 30, ("10M", "5M2D5M", "3S7M", "5M20N5M")[i % 4], ramp) for i in range(151)]
    data = K.bam(K.REFS, reads, one_record_per_block=True)
    one = check(data, min_baseq=14)
    for max_blocks in (1, 3):
        many = check(data, min_baseq=14, max_blocks=max_blocks)
        assert many["stats"] == one["stats"] and many["sum_baseq"].tolist() == one["sum_baseq"].tolist()
    paged = check(data, min_baseq=14, max_rows=2)
    assert paged["n_rows"] == 3


def open_ctx(data):
    ctx = duckhts_amd.Context(0)
    ctx.open(data)
    ctx.bgzf_index()
    ctx.bam_open()
    return ctx


def drain(ctx, max_rows=0):
    parts = []
    while True:
        cols, st = ctx.bam_coverage_next(max_rows)
        parts.append(cols)
        if st:
            return {k: np.concatenate([p[k] for p in parts]) for k in duckhts_amd.COVERAGE_COLUMNS}, [p["n_rows"] for p in parts]


def test_accumulate_after_a_result_was_started():
    reads = [R(0, i % 3, 100 + 5 * i, 30, "10M", ramp) for i in range(12)]
    data = K.bam(K.REFS, reads, one_record_per_block=True)
    refs, mreads = M.reads_from_bam(data)
    ctx = open_ctx(data)
    try:
        ctx.bam_coverage_open(min_baseq=15)
        seen, stale = 0, None
        while True:
            b = ctx.next_batch(1, duckhts_amd.COVERAGE_COLMASK)
            if stale is not None and b.n_rows:
                with pytest.raises(duckhts_amd.DhtsError, match="not the one dhts_bam_next_batch returned last"):
                    ctx.bam_coverage_accumulate(stale)
                stale = None
            ctx.bam_coverage_accumulate(b)
            seen += int(b.n_rows)
            if seen == 1 and stale is None:
                stale = duckhts_amd.BamBatch()
                C.memmove(C.byref(stale), C.byref(b), C.sizeof(b))
            if seen == 5:                                                  # a whole result in the middle: the reads so far; the table and the counters stay intact
                exp = M.coverage(mreads[:seen], refs, min_baseq=15)
                cols, sizes = drain(ctx, 2)
                assert sizes == [2, 1] and cols["sum_depth"].tolist() == exp["sum_depth"] and cols["sum_baseq"].tolist() == exp["sum_baseq"] and cols["numreads"].tolist() == exp["numreads"]
            if seen == 9:                                                  # one page of a result taken: the next accumulate starts the result over
                exp = M.coverage(mreads[:seen], refs, min_baseq=15)
                cols, st = ctx.bam_coverage_next(2)
                assert cols["n_rows"] == 2 and st == 0 and cols["sum_depth"].tolist() == exp["sum_depth"][:2] and cols["covbases"].tolist() == exp["covbases"][:2]
            if b.status:
                break
        exp = M.coverage(mreads, refs, min_baseq=15)
        cols, sizes = drain(ctx)
        assert sizes == [3] and cols["sum_depth"].tolist() == exp["sum_depth"] and cols["covbases"].tolist() == exp["covbases"]
        cols, st = ctx.bam_coverage_next()                                  # behind the last page: nothing, and still the end
        assert cols["n_rows"] == 0 and st == 1
        # a second open zeroes everything
        ctx.bam_coverage_open()
        st = ctx.bam_coverage_stats()
        assert st["n_rows"] == 0 and st["status"] == 0 and st["n_target_rows"] == 3 and st["table_bytes"] == M.table_bytes([(t, 0, l) for t, (_, l) in enumerate(refs)])
        assert drain(ctx)[0]["sum_depth"].tolist() == [0, 0, 0]
    finally:
        ctx.close()


# ---- limits and states ----
def test_the_table_cap(rng):
    refs, _ = M.reads_from_bam(rng)
    need = M.table_bytes([(t, 0, l) for t, (_, l) in enumerate(refs)])
    ctx = open_ctx(rng)
    L = ctx.L
    try:
        L.dhts_debug_coverage_max_table_bytes(need - 1)
        with pytest.raises(duckhts_amd.DhtsError) as e:
            ctx.bam_coverage_open()
        assert str(e.value) == M.err_table(need, need - 1)
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_NOT_OPEN):    # an open that failed leaves nothing open
            ctx.bam_coverage_stats()
        L.dhts_debug_coverage_max_table_bytes(need)
        ctx.bam_coverage_open()
        assert ctx.bam_coverage_stats()["table_bytes"] == need
        L.dhts_debug_coverage_max_table_bytes(0)
        assert M.DEFAULT_CAP == 16 << 30
    finally:
        L.dhts_debug_coverage_max_table_bytes(0)
        ctx.close()


def test_calls_in_the_wrong_state_and_refusals(rng):
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(rng)
        ctx.bgzf_index()
        with pytest.raises(duckhts_amd.DhtsError, match="dhts_bam_open not called"):
            ctx.bam_coverage_open()
        ctx.bam_open()
        b = ctx.next_batch(0, duckhts_amd.COVERAGE_COLMASK)
        for call in (lambda: ctx.bam_coverage_accumulate(b), ctx.bam_coverage_scan, ctx.bam_coverage_stats, ctx.bam_coverage_next):
            with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_NOT_OPEN):
                call()
        for kw, msg in ((dict(min_mapq=256), M.err_range("min_mapq")), (dict(min_mapq=-1), M.err_range("min_mapq")), (dict(min_baseq=256), M.err_range("min_baseq")),
                        (dict(min_baseq=-1), M.err_range("min_baseq")), (dict(include_flags=65536), M.err_range("include_flags")), (dict(require_flags=-1), M.err_range("require_flags")),
                        (dict(exclude_flags=70000), M.err_range("exclude_flags")), (dict(min_read_len=-1), M.ERR_READ_LEN), (dict(min_depth=0), M.ERR_DEPTH),
                        # wrong in two ways: the first in the order of the checks is reported
                        (dict(min_read_len=-1, min_mapq=256), M.ERR_READ_LEN), (dict(min_baseq=-1, include_flags=65536), M.err_range("min_baseq")),
                        (dict(require_flags=-1, exclude_flags=70000), M.err_range("require_flags")), (dict(min_depth=0, exclude_flags=70000), M.err_range("exclude_flags"))):
            with pytest.raises(duckhts_amd.DhtsError) as e:
                ctx.bam_coverage_open(**kw)
            assert str(e.value) == msg
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_NOT_OPEN):
            ctx.bam_coverage_stats()
        # a shard or a block range of the file
        ctx.set_shard(0, 2)
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_SHARD):
            ctx.bam_coverage_open()
        ctx.set_shard(0, 1)
        ctx.bam_coverage_open()
        ctx.set_block_range(0, 1, 1)
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_SHARD):
            ctx.bam_coverage_scan()
    finally:
        ctx.close()
