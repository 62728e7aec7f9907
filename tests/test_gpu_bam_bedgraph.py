"""bam_bedgraph on the device (dhts_bam_bedgraph_*, csrc/bam_bedgraph.hip) against the CPU model bam_bedgraph_ref, row for row: tid, start, end,
depth, the counters and the stats.  Runs at, over and far behind tile edges, rows around the tile's length, regions and their seams, a BED,
classes, pages of every size, rows of more than 4,096 tiles, the cross-check against bam_depth on the device, the projection, a result taken
after a page, the table cap, the ABI's states and every refusal."""
import ctypes as C

import numpy as np
import pytest

import bam_bedgraph_cases as G
import bam_bedgraph_ref as M
import bam_depth_cases as D
import duckhts_amd
from conftest import read_golden
from test_gpu_bam_coverage import CIGARS, parse_rows, ramp

pytestmark = pytest.mark.gpu
R = G.R
DTYPES = (("tid", np.int32), ("start", np.int64), ("end", np.int64), ("depth", np.int32))


def model_params(kw):
    p = {k: v for k, v in kw.items() if k in M.FILTERS + ("zero_runs", "breaks")}
    p.setdefault("exclude_flags", M.DEFAULT_EXCLUDE)                     # the Python function's default
    return p


def same(got, exp, rows=None):
    assert {k: got["stats"][k] for k in M.COUNTERS} == exp["stats"]
    assert got["n_rows"] == exp["n_rows"] == got["stats"]["n_runs"] == sum(got["pages"])
    for k, dt in DTYPES:
        assert got[k].dtype == dt and len(got[k]) == exp["n_rows"]
        bad = np.flatnonzero(got[k] != exp[k])
        assert not len(bad), (k, bad[:5].tolist(), got[k][bad[:5]].tolist(), exp[k][bad[:5]].tolist())
    if rows is not None:
        assert got["stats"]["n_target_rows"] == len(rows) and got["stats"]["table_bytes"] == M.table_bytes(rows)


def check(data, **kw):
    got = duckhts_amd.bam_bedgraph(data, **kw)
    refs, reads = M.reads_from_bam(data)
    same(got, M.bedgraph(reads, refs, **model_params(kw)), rows=[(t, 0, l) for t, (_, l) in enumerate(refs)])
    assert got["status"] == 1 and got["contigs"] == [n for n, _ in refs]
    return got


def check_region(data, region, **kw):
    """the model's reads are the rows of read_bam's own region query"""
    scanned = duckhts_amd.read_bam(data, region=region)
    refs, _ = M.reads_from_bam(data)
    rows = parse_rows(refs, region)
    got = duckhts_amd.bam_bedgraph(data, region=region, **kw)
    same(got, M.bedgraph(M.reads_from_cols(scanned), refs, rows=rows, **model_params(kw)), rows=rows)
    return got


def check_bed(data, bed_rows, **kw):
    refs, reads = M.reads_from_bam(data)
    rows, skipped = M.merge_bed(bed_rows, refs)
    got = duckhts_amd.bam_bedgraph(data, bed=D.bed_text(bed_rows), **kw)
    same(got, M.bedgraph(reads, refs, rows=rows, **model_params(kw)), rows=rows)
    assert got["stats"]["n_bed_skipped"] == skipped
    return got


def rows_of(got):
    return list(zip(got["tid"].tolist(), got["start"].tolist(), got["end"].tolist(), got["depth"].tolist()))


def open_ctx(data):
    ctx = duckhts_amd.Context(0)
    ctx.open(data)
    ctx.bgzf_index()
    ctx.bam_open()
    return ctx


def drain(ctx, max_rows=0, columns=None):
    parts = []
    while True:
        cols, st = ctx.bam_bedgraph_next(max_rows, columns)
        parts.append(cols)
        if st:
            return {k: None if parts[0][k] is None else np.concatenate([p[k] for p in parts]) for k in duckhts_amd.BEDGRAPH_COLUMNS}, [p["n_rows"] for p in parts]


# ---- runs and tile edges ----
@pytest.mark.parametrize("zero_runs,breaks", G.COMBOS)
def test_runs_at_over_and_far_behind_tile_edges(zero_runs, breaks):
    got = check(G.bam(*G.tile_edges()), zero_runs=zero_runs, breaks=breaks)
    if not zero_runs and breaks is None:
        rows = rows_of(got)
        assert (0, 1000, 1024, 1) in rows and (0, 1024, 1041, 2) in rows            # one ends on slot 1023, the next starts on slot 0
        assert (1, 1010, 1101, 1) in rows and (2, 2000, 4150, 1) in rows            # over one edge; over three tiles, no boundary in the middle one


@pytest.mark.parametrize("zero_runs,breaks", G.COMBOS)
def test_rows_around_the_tile(zero_runs, breaks):
    got = check(G.bam(*G.row_lengths()), zero_runs=zero_runs, breaks=breaks)
    if zero_runs and breaks is None:
        rows = rows_of(got)
        assert rows[0] == (0, 0, 1, 1) and (2, 1023, 1024, 4) in rows and (3, 1024, 1025, 5) in rows and rows[-1] == (5, 0, 1024, 0)
        assert got["stats"]["table_bytes"] == 4 * 1024 * (1 + 1 + 2 + 2 + 0 + 2)      # at 1,024 the closing slot opens a tile of its own


@pytest.mark.parametrize("zero_runs,breaks", G.COMBOS)
def test_adjacent_regions_with_equal_depth_across_the_seam(zero_runs, breaks):
    data = G.bam(G.REFS, G.SEAM_READS)
    two = check_region(data, G.SEAM_TWO, zero_runs=zero_runs, breaks=breaks)
    one = check_region(data, G.SEAM_ONE, zero_runs=zero_runs, breaks=breaks)
    rev = check_region(data, G.SEAM_REVERSED, zero_runs=zero_runs, breaks=breaks)
    assert rows_of(two) == [(0, 90, 100, 2), (0, 100, 110, 2)] and rows_of(one) == [(0, 90, 110, 2)] and rows_of(rev) == rows_of(two)[::-1]


@pytest.mark.parametrize("zero_runs,breaks", G.COMBOS)
def test_bed_intervals_that_touch_are_one_row(zero_runs, breaks):
    got = check_bed(G.bam(G.TOUCH_REFS, G.TOUCH_READS), G.TOUCH_BED, zero_runs=zero_runs, breaks=breaks)
    assert got["stats"]["n_target_rows"] == 2
    if breaks is None:
        assert (0, 150, 250, 3) in rows_of(got) and (0, 1500, 2600, 1) in rows_of(got)    # one run through the seam at 200; one over two tile edges


@pytest.mark.parametrize("zero_runs,breaks", G.COMBOS)
def test_classes(zero_runs, breaks):
    got = check(G.bam(G.CLASS_REFS, G.CLASS_READS), zero_runs=zero_runs, breaks=breaks)
    assert rows_of(got) == G.CLASS_ROWS[(zero_runs, breaks)]
    if breaks:
        assert rows_of(check(G.bam(G.CLASS_REFS, G.CLASS_READS), zero_runs=zero_runs, breaks=[2, 4])) == rows_of(got)


def test_sixteen_breaks_and_the_largest():
    breaks = list(range(1, 16)) + [2**31 - 1]
    reads = [r for i in range(18) for r in G.at(0, 100 + 10 * i, 10 * (18 - i))]     # depth 1 .. 18 in steps of ten positions
    got = check(G.bam(G.CLASS_REFS, reads), breaks=breaks)
    assert rows_of(got) == [(0, 100 + 10 * i, 110 + 10 * i, i + 1) for i in range(14)] + [(0, 240, 280, 15)]


@pytest.mark.parametrize("zero_runs,breaks", G.COMBOS)
def test_an_omitted_zero_run_between_two_emitted_runs(zero_runs, breaks):
    got = check(G.bam(G.GAP_REFS, G.GAP_READS), zero_runs=zero_runs, breaks=breaks)
    if not zero_runs:
        assert rows_of(got) == [(0, 1000, 1020, 2), (0, 2100, 2120, 2)]              # the first ends where the zero run starts


# ---- pages ----
@pytest.fixture(scope="module")
def many():
    data = G.bam(*G.many_runs())
    refs, reads = M.reads_from_bam(data)
    return data, {c: M.bedgraph(reads, refs, exclude_flags=M.DEFAULT_EXCLUDE, zero_runs=c[0], breaks=c[1]) for c in G.COMBOS}


@pytest.mark.parametrize("zero_runs,breaks", G.COMBOS)
@pytest.mark.parametrize("max_rows", [1, 2, 7, 255, 256, 257, 1025, 0])
def test_pages_of_every_size(many, max_rows, zero_runs, breaks):
    data, exp = many
    e = exp[(zero_runs, breaks)]
    got = duckhts_amd.bam_bedgraph(data, max_rows=max_rows, zero_runs=zero_runs, breaks=breaks)
    same(got, e)
    n = e["n_rows"]
    assert n > (200 if breaks else 1500 + 1500 * zero_runs)
    if max_rows:
        assert got["pages"][:-1] == [max_rows] * ((n - 1) // max_rows) and 0 <= got["pages"][-1] <= max_rows
    else:
        assert got["pages"] == [n]
    if zero_runs and breaks is None:                                           # the zero run that ends nineteen tiles behind the tile it starts in
        assert (1, 15, 19990, 0) in rows_of(got)


# ---- rows of more than 4,096 tiles ----
@pytest.fixture(scope="module")
def long_ends():
    return G.bam(G.LONG_REFS, G.LONG_ENDS)


@pytest.mark.parametrize("breaks", [None, "2,4"])
def test_a_zero_run_over_more_than_4096_tiles(long_ends, breaks):
    got = check(long_ends, zero_runs=1, breaks=breaks, max_rows=2)
    assert got["stats"]["table_bytes"] > 4096 * 4096
    assert rows_of(got) == ([(0, 0, 10, 1), (0, 10, G.LONG - 10, 0), (0, G.LONG - 10, G.LONG, 1)] if breaks is None else [(0, 0, G.LONG, 0)])
    assert check(long_ends, breaks=breaks)["n_rows"] == (2 if breaks is None else 0)


@pytest.mark.parametrize("zero_runs", [0, 1])
def test_a_deletion_over_more_than_4096_tiles(zero_runs):
    data = G.bam(G.LONG_REFS, G.LONG_DELETION)
    got = check(data, include_deletions=1, zero_runs=zero_runs)
    assert [r for r in rows_of(got) if r[3]] == [(0, 20000, 4270020, 1)]
    got = check(data, zero_runs=zero_runs)
    assert [r for r in rows_of(got) if r[3]] == [(0, 20000, 20010, 1), (0, 4270010, 4270020, 1)]


# ---- nothing to count ----
@pytest.mark.parametrize("zero_runs,breaks", G.COMBOS)
def test_untouched_contigs_no_references_no_counted_read(zero_runs, breaks):
    got = check(G.bam([("a", 1500), ("b", 7), ("c", 0)], G.at(0, 100, 10, 3)), zero_runs=zero_runs, breaks=breaks)
    if zero_runs:
        assert rows_of(got)[-1] == (1, 0, 7, 0)                                 # an untouched contig is one row
    got = check(G.bam([], [R(4, -1, -1, 0, "*", 30)] * 3), exclude_flags=0, zero_runs=zero_runs, breaks=breaks)
    assert got["n_rows"] == 0 and got["stats"]["n_unplaced"] == 3 and got["pages"] == [0]
    reads = [R(0x400, 0, 10, 30, "10M", 30), R(0, 1, 10, 3, "10M", 30), R(4, -1, -1, 0, "*", 30)]
    got = check(G.bam([("a", 1500), ("b", 7)], reads), min_mapq=10, zero_runs=zero_runs, breaks=breaks)
    assert rows_of(got) == ([(0, 0, 1500, 0), (1, 0, 7, 0)] if zero_runs else []) and got["stats"]["n_counted"] == 0


# ---- the filter and the counted bases ----
@pytest.mark.parametrize("min_baseq", [0, 20])
@pytest.mark.parametrize("include_deletions", [0, 1])
def test_every_cigar_operation(include_deletions, min_baseq):
    reads = [R(0, i % 2, 1000 + 40 * i, 30, cg, lambda k: 12 + (k * 5) % 17) for i, cg in enumerate(CIGARS)]
    reads.append(R(0, 2, 500, 30, "1S1N", cg="30M5D2I30M10N17M", qual=ramp))              # the real CIGAR in the CG tag
    reads.append(R(0, 2, 900, 30, "6M", 30))
    for zero_runs, breaks in G.COMBOS:
        got = check(G.bam(G.REFS, reads), min_baseq=min_baseq, include_deletions=include_deletions, zero_runs=zero_runs, breaks=breaks)
        assert got["stats"]["n_counted"] == len(reads)


def test_the_hand_written_table_of_bam_depth():
    data = D.bam(D.HAND_REFS, D.HAND_READS)
    for kw, exp in ((dict(), D.HAND_ROWS), (dict(include_deletions=1), D.HAND_ROWS_DEL), (dict(zero_runs=1), D.hand_rows_all(2))):
        got = check(data, **D.HAND_PARAMS, **kw)
        tid, pos, depth = M.expand(got)
        assert list(zip(tid.tolist(), pos.tolist(), depth.tolist())) == exp
        assert {k: got["stats"][k] for k in M.COUNTERS} == D.HAND_STATS


# ---- the identity, on the device: expanded, bam_bedgraph is bam_depth ----
def expanded_is_bam_depth(data, **kw):
    for zero_runs, mode in ((1, 2), (0, 0)):
        got = check(data, zero_runs=zero_runs, max_rows=1000, **kw)
        dep = duckhts_amd.bam_depth(data, all_positions=mode, **kw)
        tid, pos, depth = M.expand(got)
        assert np.array_equal(tid, dep["tid"]) and np.array_equal(pos, dep["pos"]) and np.array_equal(depth, dep["depth"])
        assert {k: got["stats"][k] for k in M.COUNTERS} == {k: dep["stats"][k] for k in M.COUNTERS}


@pytest.fixture(scope="module")
def rng():
    return read_golden("range.bam")


@pytest.mark.parametrize("min_baseq", [0, 25])
def test_expanded_equals_bam_depth_on_the_golden_file(rng, min_baseq):
    expanded_is_bam_depth(rng, min_baseq=min_baseq)
    check(rng, min_baseq=min_baseq, breaks="2,4", zero_runs=1)


def test_expanded_equals_bam_depth_on_twenty_contigs():
    refs = [(f"k{t}", 700 + 211 * t) for t in range(20)]
    reads = [R(0, (i * 7) % 20, (i * 131) % 900, 30, ("30M", "10M5D10M", "4S26M", "12M3N12M")[i % 4], ramp) for i in range(400)]
    expanded_is_bam_depth(G.bam(refs, reads), min_baseq=12, include_deletions=1)
    check(G.bam(refs, reads), min_baseq=12, breaks="2,4")


# ---- a result taken after a page, projection ----
def test_accumulate_after_a_page_was_taken():
    reads = [R(0, i % 3, 100 + 5 * i, 30, "10M", ramp) for i in range(12)]
    data = G.bam(G.REFS, reads, one_record_per_block=True)
    refs, mreads = M.reads_from_bam(data)
    ctx = open_ctx(data)
    try:
        ctx.bam_bedgraph_open(min_baseq=15, zero_runs=1)
        assert ctx.bam_bedgraph_stats()["n_runs"] == 0
        seen, stale = 0, None
        while True:
            b = ctx.next_batch(1, duckhts_amd.BEDGRAPH_COLMASK)
            if stale is not None and b.n_rows:
                with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_STALE):
                    ctx.bam_bedgraph_accumulate(stale)
                stale = None
            ctx.bam_bedgraph_accumulate(b)
            seen += int(b.n_rows)
            if seen == 1 and stale is None:
                stale = duckhts_amd.BamBatch()
                C.memmove(C.byref(stale), C.byref(b), C.sizeof(b))
            if seen == 5:                                                  # a whole result in the middle: the reads so far; the table and the counters stay intact
                exp = M.bedgraph(mreads[:seen], refs, min_baseq=15, zero_runs=1)
                cols, sizes = drain(ctx, 3)
                assert sum(sizes) == exp["n_rows"] and all(np.array_equal(cols[k], exp[k]) for k in duckhts_amd.BEDGRAPH_COLUMNS)
                assert ctx.bam_bedgraph_stats()["n_runs"] == exp["n_rows"]
            if seen == 9:                                                  # one page of a result taken: the next accumulate starts the result over
                exp = M.bedgraph(mreads[:seen], refs, min_baseq=15, zero_runs=1)
                cols, st = ctx.bam_bedgraph_next(4)
                assert cols["n_rows"] == 4 and st == 0 and cols["start"].tolist() == exp["start"][:4].tolist() and cols["end"].tolist() == exp["end"][:4].tolist()
            if b.status:
                break
        exp = M.bedgraph(mreads, refs, min_baseq=15, zero_runs=1)
        assert ctx.bam_bedgraph_stats()["n_runs"] == 0                     # (no result of the table as it is now was taken)
        cols, sizes = drain(ctx)
        assert sizes == [exp["n_rows"]] and all(np.array_equal(cols[k], exp[k]) for k in duckhts_amd.BEDGRAPH_COLUMNS)
        st = ctx.bam_bedgraph_stats()
        assert {k: st[k] for k in M.COUNTERS} == exp["stats"] and st["n_runs"] == exp["n_rows"] and st["status"] == 1
        cols, st = ctx.bam_bedgraph_next()                                  # behind the last page: nothing, and still the end
        assert cols["n_rows"] == 0 and st == 1
        ctx.bam_bedgraph_open(zero_runs=1)                                  # a second open zeroes everything
        st = ctx.bam_bedgraph_stats()
        assert st["n_rows"] == 0 and st["status"] == 0 and st["n_target_rows"] == 3 and st["n_runs"] == 0
        cols, sizes = drain(ctx, 2)
        assert sizes == [2, 1] and cols["end"].tolist() == [100000] * 3 and not cols["depth"].any()
    finally:
        ctx.close()


def test_projection_of_each_single_column(rng):
    full = duckhts_amd.bam_bedgraph(rng, max_rows=300, zero_runs=1)
    for cols in (["tid"], ["start"], ["end"], ["depth"], ["end", "tid"]):
        got = duckhts_amd.bam_bedgraph(rng, max_rows=300, zero_runs=1, columns=cols)
        assert got["n_rows"] == full["n_rows"] and got["pages"] == full["pages"]
        for k in duckhts_amd.BEDGRAPH_COLUMNS:
            assert (got[k] is None) if k not in cols else np.array_equal(got[k], full[k]), k
    # the batch itself: null pointers for the columns that were left out, and 8 bytes per row for end alone
    ctx = open_ctx(rng)
    try:
        ctx.bam_bedgraph_open(exclude_flags=0x704)
        ctx.bam_bedgraph_scan()
        b = duckhts_amd.BedBatch()
        ctx._chk(ctx.L.dhts_bam_bedgraph_next(ctx.h, 10, 1 << duckhts_amd.BEDGRAPH_COLUMNS.index("end"), C.byref(b)))
        assert b.n_rows == 10 and b.n_cols == 4 and not b.cols[0].fixed and not b.cols[1].fixed and b.cols[2].fixed and not b.cols[3].fixed and not b.cols[2].valid
        assert ctx.L.dhts_bam_bedgraph_batch_host_bytes(C.byref(b)) == 80
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
            ctx.bam_bedgraph_open()
        assert str(e.value) == M.err_table(need, need - 1)
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_NOT_OPEN):    # an open that failed leaves nothing open
            ctx.bam_bedgraph_stats()
        L.dhts_debug_coverage_max_table_bytes(need)
        ctx.bam_bedgraph_open()
        assert ctx.bam_bedgraph_stats()["table_bytes"] == need
    finally:
        L.dhts_debug_coverage_max_table_bytes(0)
        ctx.close()


def test_calls_in_the_wrong_state_and_every_refusal(rng):
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(rng)
        ctx.bgzf_index()
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_BAM_NOT_OPEN):
            ctx.bam_bedgraph_open()
        ctx.bam_open()
        b = ctx.next_batch(0, duckhts_amd.BEDGRAPH_COLMASK)
        for call in (lambda: ctx.bam_bedgraph_accumulate(b), ctx.bam_bedgraph_scan, ctx.bam_bedgraph_stats, ctx.bam_bedgraph_next):
            with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_NOT_OPEN):
                call()
        for kw, msg in ((dict(min_mapq=256), M.err_range("min_mapq")), (dict(min_mapq=-1), M.err_range("min_mapq")), (dict(min_baseq=256), M.err_range("min_baseq")),
                        (dict(min_baseq=-1), M.err_range("min_baseq")), (dict(include_flags=65536), M.err_range("include_flags")), (dict(require_flags=-1), M.err_range("require_flags")),
                        (dict(exclude_flags=70000), M.err_range("exclude_flags")), (dict(min_read_len=-1), M.ERR_READ_LEN), (dict(zero_runs=2), M.ERR_ZERO_RUNS),
                        (dict(zero_runs=-1), M.ERR_ZERO_RUNS), (dict(include_deletions=2), M.ERR_DELETIONS), (dict(include_deletions=-1), M.ERR_DELETIONS),
                        (dict(breaks=list(range(1, 18))), M.ERR_MANY_BREAKS), (dict(breaks=[0, 5]), M.ERR_BREAKS), (dict(breaks=[3, 3]), M.ERR_BREAKS), (dict(breaks=[5, 2]), M.ERR_BREAKS),
                        (dict(breaks=[-4]), M.ERR_BREAKS), (dict(breaks=[1, 2**31]), M.ERR_BREAKS),
                        # wrong in two ways: the first in the order of the checks is reported
                        (dict(min_read_len=-1, min_mapq=256), M.ERR_READ_LEN), (dict(zero_runs=2, exclude_flags=70000), M.err_range("exclude_flags")),
                        (dict(zero_runs=2, include_deletions=2), M.ERR_ZERO_RUNS), (dict(include_deletions=2, breaks=[0]), M.ERR_DELETIONS),
                        (dict(breaks=[0] * 17), M.ERR_MANY_BREAKS)):
            with pytest.raises(duckhts_amd.DhtsError) as e:
                ctx.bam_bedgraph_open(**kw)
            assert str(e.value) == msg
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_NOT_OPEN):
            ctx.bam_bedgraph_stats()
        with pytest.raises(duckhts_amd.DhtsError, match="bam_bedgraph: the BED context has to be a second context"):
            ctx.bam_bedgraph_open(bed_ctx=ctx)
        other = duckhts_amd.Context(0)
        try:
            other.open(b"c\t0\t1\n")
            with pytest.raises(duckhts_amd.DhtsError, match="bam_bedgraph: the BED context is not open"):
                ctx.bam_bedgraph_open(bed_ctx=other)
        finally:
            other.close()
        ctx.set_shard(0, 2)                                                # a shard or a block range of the file
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_SHARD):
            ctx.bam_bedgraph_open()
        ctx.set_shard(0, 1)
        ctx.bam_bedgraph_open()
        ctx.set_block_range(0, 1, 1)
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_SHARD):
            ctx.bam_bedgraph_scan()
    finally:
        ctx.close()
    with pytest.raises(duckhts_amd.DhtsError) as e:
        duckhts_amd.bam_bedgraph(rng, region="CHROMOSOME_I:1-1000", bed=b"CHROMOSOME_I\t0\t10\n")
    assert str(e.value) == M.ERR_BED_AND_REGION
    with pytest.raises(duckhts_amd.DhtsError) as e:
        duckhts_amd.bam_bedgraph(rng, region="CHROMOSOME_I:1-1000,CHROMOSOME_II:1-10,CHROMOSOME_I:1000-1200")
    assert str(e.value) == M.err_overlap("CHROMOSOME_I:1-1000", "CHROMOSOME_I:1000-1200")
    for text in ("2,,4", "a", "", "2;4", "4,2"):
        with pytest.raises(duckhts_amd.DhtsError) as e:
            duckhts_amd.bam_bedgraph(rng, breaks=text)
        assert str(e.value) == M.ERR_BREAKS
