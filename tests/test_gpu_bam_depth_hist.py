"""bam_depth_hist on the device (dhts_bam_hist_*, csrc/bam_depth_hist.hip) against the CPU model bam_depth_hist_ref, row for row: the seven columns,
the counters, the stats and the page sizes.  Rows around the tile's length, spans of tiles that meet inside a row, groups and their seams, bins
on both sides of the LDS limit, a flat tile, the filter's dispatch, a BED, the device's own bam_depth and bam_bedgraph, pages and projection, a
result taken after a page, both table caps, the ABI's states and every refusal."""
import ctypes as C

import numpy as np
import pytest

import bam_depth_cases as D
import bam_depth_hist_cases as H
import bam_depth_hist_ref as M
import duckhts_amd
from conftest import read_golden
from test_gpu_bam_coverage import CIGARS, ramp

pytestmark = pytest.mark.gpu
R = H.R
DTYPES = tuple(zip(duckhts_amd.DEPTH_HIST_COLUMNS, duckhts_amd.DEPTH_HIST_DTYPES))


def model_params(kw):
    p = {k: v for k, v in kw.items() if k in M.FILTERS + ("depth_cap", "per")}
    p.setdefault("exclude_flags", M.DEFAULT_EXCLUDE)                     # the Python function's default
    return p


def same(got, exp, rows=None, cap=1000, per="row", max_rows=0):
    assert {k: got["stats"][k] for k in M.COUNTERS} == exp["stats"]
    assert got["n_rows"] == exp["n_rows"] == got["stats"]["n_result_rows"] == sum(got["pages"])
    for k, dt in DTYPES:
        assert got[k].dtype == dt and len(got[k]) == exp["n_rows"]
        bad = np.flatnonzero(got[k] != exp[k])
        assert not len(bad), (k, bad[:5].tolist(), got[k][bad[:5]].tolist(), exp[k][bad[:5]].tolist())
    n = exp["n_rows"]
    assert got["pages"] == (([max_rows] * (n // max_rows) + [n % max_rows] * (n % max_rows > 0) or [0]) if max_rows else [n])      # full pages, then the rest: no empty last page
    if rows is not None:
        st = got["stats"]
        assert st["n_target_rows"] == len(rows) and st["table_bytes"] == M.table_bytes(rows) and st["n_groups"] == exp["n_groups"] and st["hist_bytes"] == M.hist_bytes(rows, cap, per)


def check_case(case, **kw):
    """a case of bam_depth_hist_cases on the device against the model; with regions the model's reads are the rows of read_bam's own region query"""
    data = H.bam(case["refs"], case["reads"])
    refs, reads = M.reads_from_bam(data)
    args = dict(case.get("kw", {}), **kw)
    skipped = 0
    if "region" in case:
        rows = H.rows_of_region(refs, case["region"])
        reads = M.reads_from_cols(duckhts_amd.read_bam(data, region=case["region"]))
        got = duckhts_amd.bam_depth_hist(data, region=case["region"], **args)
    elif "bed" in case:
        rows, skipped = M.merge_bed(case["bed"], refs)
        got = duckhts_amd.bam_depth_hist(data, bed=D.bed_text(case["bed"]), **args)
    else:
        rows = [(t, 0, l) for t, (_, l) in enumerate(refs)]
        got = duckhts_amd.bam_depth_hist(data, **args)
    exp = M.hist(reads, refs, rows=rows, **model_params(args))
    same(got, exp, rows=rows, cap=args.get("depth_cap", 1000), per=args.get("per", "row"), max_rows=args.get("max_rows", 0))
    assert got["status"] == 1 and got["contigs"] == [n for n, _ in refs] and got["stats"]["n_bed_skipped"] == skipped
    return got


def rows_of(got):
    return list(zip(*(got[k].tolist() for k in duckhts_amd.DEPTH_HIST_COLUMNS)))


def open_ctx(data):
    ctx = duckhts_amd.Context(0)
    ctx.open(data)
    ctx.bgzf_index()
    ctx.bam_open()
    return ctx


def drain(ctx, max_rows=0, columns=None):
    parts = []
    while True:
        cols, st = ctx.bam_depth_hist_next(max_rows, columns)
        parts.append(cols)
        if st:
            return {k: None if parts[0][k] is None else np.concatenate([p[k] for p in parts]) for k in duckhts_amd.DEPTH_HIST_COLUMNS}, [p["n_rows"] for p in parts]


# ---- tile and span edges ----
@pytest.mark.parametrize("per", H.PERS)
def test_rows_of_length_1_1023_1024_1025(per):
    got = check_case(H.row_lengths(), per=per)
    assert got["stats"]["table_bytes"] == 4 * 1024 * (1 + 1 + 2 + 2)              # 1,023 fills a tile with its closing slot, 1,024 spills
    if per == "row":
        assert rows_of(got)[0] == (0, 0, 1, 1, 1, 1, 1)
        assert sorted(set(got["length"].tolist())) == [1, 1023, 1024, 1025]
    else:
        assert set(got["length"].tolist()) == {1 + 1023 + 1024 + 1025} and set(got["start"].tolist()) == {0} and set(got["end"].tolist()) == {6025}
    check_case(H.contig_lengths(), per=per)


@pytest.mark.parametrize("per", H.PERS)
def test_spans_of_several_tiles_that_meet_inside_a_row(per):
    case = H.spans()
    ntiles = sum((l + 1 + 1023) // 1024 for _, l in case["refs"])
    span = duckhts_amd.depth_hist_span_tiles(ntiles)                              # read from the module, not assumed
    assert 1 < span and 2 * span < ntiles
    got = check_case(case, per=per)
    assert got["stats"]["table_bytes"] == ntiles * 4096


# ---- group seams ----
@pytest.mark.parametrize("per", H.PERS)
def test_regions_out_of_order_one_clipped_to_empty(per):
    got = check_case(H.seams(), per=per)
    st = got["stats"]
    assert st["n_target_rows"] == 5 and st["n_groups"] == (4 if per == "row" else 2)
    key = list(dict.fromkeys(zip(got["tid"].tolist(), got["start"].tolist(), got["end"].tolist(), got["length"].tolist())))
    assert key == ([(0, 300, 400, 100), (0, 90, 100, 10), (1, 0, 200, 200), (0, 5000, 5050, 50)] if per == "row" else [(0, 90, 5050, 160), (1, 0, 200, 200)])


@pytest.mark.parametrize("per", H.PERS)
def test_adjacent_contigs_in_one_span_and_an_untouched_contig(per):
    got = check_case(H.adjacent_contigs(), per=per)
    assert (2, 0, 7, 0, 7, 7, 7) in rows_of(got) and got["stats"]["n_groups"] == 4      # the untouched contig's single row; the empty contig has no group
    assert duckhts_amd.depth_hist_span_tiles(2 + 2 + 1 + 2) >= 7                  # (all tiles lie in one span: every group but the last is flushed at a seam)


# ---- bins ----
@pytest.fixture(scope="module")
def stacked():
    case = H.stack()
    data = H.bam(case["refs"], case["reads"])
    refs, reads = M.reads_from_bam(data)
    return data, refs, reads


@pytest.mark.parametrize("cap", H.CAPS + (1,))
def test_a_stack_on_one_position_around_the_lds_limit(stacked, cap):
    data, refs, reads = stacked
    rows = [(t, 0, l) for t, (_, l) in enumerate(refs)]
    for per in H.PERS:
        got = duckhts_amd.bam_depth_hist(data, depth_cap=cap, per=per)
        same(got, M.hist(reads, refs, depth_cap=cap, per=per, exclude_flags=M.DEFAULT_EXCLUDE), rows=rows, cap=cap, per=per)
    k = got["tid"] == 0
    assert got["depth"][k].max() == min(cap, H.STACK + 1) and got["n_at_least"][k][0] == 3000
    if cap == 5000:
        assert got["depth"][k].tolist()[-3:] == [H.LDS, H.LDS + 1, H.STACK + 1]   # unclamped, at and above the LDS limit: straight to the table
    if cap == H.LDS:
        assert got["n_positions"][k][-1] == 6                                     # 4,096, 4,097 and 4,201 clamped into the first bin the LDS does not hold


@pytest.mark.parametrize("name", ["flat", "flat_but_one"])
def test_one_depth_across_a_whole_tile(name):
    got = check_case(H.ALL[name](), per="row")
    assert got["n_positions"][got["depth"] == 3].tolist() == [1024 + 8 - (name == "flat_but_one")]


# ---- the filter's dispatch ----
@pytest.mark.parametrize("min_baseq,include_deletions", [(0, 0), (20, 0), (0, 1), (20, 1)])
def test_every_cigar_operation(min_baseq, include_deletions):
    reads = [R(0, i % 2, 1000 + 40 * i, 30, cg, lambda k: 12 + (k * 5) % 17) for i, cg in enumerate(CIGARS)]
    reads.append(R(0, 2, 500, 30, "1S1N", cg="30M5D2I30M10N17M", qual=ramp))              # the real CIGAR in the CG tag
    got = check_case(dict(refs=H.REFS, reads=reads), min_baseq=min_baseq, include_deletions=include_deletions, depth_cap=3)
    assert got["stats"]["n_counted"] == len(reads)


# ---- BED ----
@pytest.mark.parametrize("per", H.PERS)
def test_bed_rows_that_merge_and_an_unknown_contig(per):
    got = check_case(H.bed(), per=per)
    st = got["stats"]
    assert st["n_bed_skipped"] == 1 and st["n_target_rows"] == 4 and st["n_groups"] == (4 if per == "row" else 2)
    if per == "contig":
        assert set(zip(got["tid"].tolist(), got["start"].tolist(), got["end"].tolist(), got["length"].tolist())) == {(0, 100, 2700, 1400), (1, 0, 2000, 110)}


# ---- device against device ----
def test_the_devices_own_bam_depth_and_bam_bedgraph():
    reads = [R(0, i % 2, 1000 + 40 * i, 30, cg, ramp) for i, cg in enumerate(CIGARS)] + [R(0, 2, 100 + 3 * i, 30, "50M", ramp) for i in range(40)]
    data = H.bam(H.REFS, reads)
    rows = [(t, 0, l) for t, (_, l) in enumerate(H.REFS)]
    for kw in (dict(), dict(min_baseq=20, include_deletions=1)):
        got = duckhts_amd.bam_depth_hist(data, depth_cap=9, **kw)
        dep = duckhts_amd.bam_depth(data, all_positions=2, **kw)
        runs = duckhts_amd.bam_bedgraph(data, zero_runs=1, **kw)
        by_runs = M.from_bedgraph(runs, rows, 9, "row")
        at = 0
        for t, (_, l) in enumerate(H.REFS):
            counts = np.bincount(np.minimum(dep["depth"][dep["tid"] == t], 9), minlength=10)
            bins = np.flatnonzero(counts)
            sel = slice(at, at + len(bins))
            assert got["tid"][sel].tolist() == [t] * len(bins) and got["depth"][sel].tolist() == bins.tolist() and got["n_positions"][sel].tolist() == counts[bins].tolist()
            at += len(bins)
        assert at == got["n_rows"] and all(np.array_equal(got[k], by_runs[k]) for k in M.COLUMNS)
        assert {k: got["stats"][k] for k in M.COUNTERS} == {k: dep["stats"][k] for k in M.COUNTERS}


# ---- pages and projection ----
@pytest.fixture(scope="module")
def paged():
    case = H.seams()
    data = H.bam(case["refs"], case["reads"] + [R(0, 1, 10 + i, 30, f"{5 + i}M", 30) for i in range(24)])      # a staircase: more than seven bins in c2's group
    refs, _ = M.reads_from_bam(data)
    reads = M.reads_from_cols(duckhts_amd.read_bam(data, region=case["region"]))
    rows = H.rows_of_region(refs, case["region"])
    return data, case["region"], {per: M.hist(reads, refs, rows=rows, per=per, exclude_flags=M.DEFAULT_EXCLUDE) for per in H.PERS}, rows


@pytest.mark.parametrize("per", H.PERS)
@pytest.mark.parametrize("max_rows", [1, 2, 7, 0])
def test_pages_of_every_size(paged, max_rows, per):
    data, region, exp, rows = paged
    got = duckhts_amd.bam_depth_hist(data, region=region, max_rows=max_rows, per=per)
    same(got, exp[per], rows=rows, per=per, max_rows=max_rows)
    sizes = np.bincount(np.unique(np.stack([got["tid"], got["start"]]), axis=1, return_inverse=True)[1].ravel())
    assert exp[per]["n_rows"] > 14 and sizes.max() > 7                            # a seam of every page size lies inside a group


def test_projection_of_each_single_column(paged):
    data, region, exp, rows = paged
    full = duckhts_amd.bam_depth_hist(data, region=region, max_rows=5)
    for cols in [[k] for k in duckhts_amd.DEPTH_HIST_COLUMNS] + [["n_at_least", "tid"]]:
        got = duckhts_amd.bam_depth_hist(data, region=region, max_rows=5, columns=cols)
        assert got["n_rows"] == full["n_rows"] and got["pages"] == full["pages"]
        for k in duckhts_amd.DEPTH_HIST_COLUMNS:
            assert (got[k] is None) if k not in cols else np.array_equal(got[k], full[k]), k
    # the batch itself: null pointers for the columns that were left out, and 8 bytes per row for length alone
    ctx = open_ctx(data)
    try:
        ctx.bam_depth_hist_open(exclude_flags=0x704)
        ctx.bam_depth_hist_scan()
        b = duckhts_amd.BedBatch()
        ctx._chk(ctx.L.dhts_bam_hist_next(ctx.h, 3, 1 << duckhts_amd.DEPTH_HIST_COLUMNS.index("length"), C.byref(b)))
        assert b.n_rows == 3 and b.n_cols == 7 and [bool(b.cols[i].fixed) for i in range(7)] == [False] * 6 + [True] and not b.cols[6].valid
        assert ctx.L.dhts_bam_hist_batch_host_bytes(C.byref(b)) == 24
    finally:
        ctx.close()


def test_accumulate_after_a_page_was_taken():
    reads = [R(0, i % 3, 100 + 5 * i, 30, "10M", ramp) for i in range(12)]
    data = H.bam(H.REFS, reads, one_record_per_block=True)
    refs, mreads = M.reads_from_bam(data)
    ctx = open_ctx(data)
    try:
        ctx.bam_depth_hist_open(min_baseq=15, depth_cap=2)
        assert ctx.bam_depth_hist_stats()["n_result_rows"] == 0
        seen, stale = 0, None
        while True:
            b = ctx.next_batch(1, duckhts_amd.DEPTH_HIST_COLMASK)
            if stale is not None and b.n_rows:
                with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_STALE):
                    ctx.bam_depth_hist_accumulate(stale)
                stale = None
            ctx.bam_depth_hist_accumulate(b)
            seen += int(b.n_rows)
            if seen == 1 and stale is None:
                stale = duckhts_amd.BamBatch()
                C.memmove(C.byref(stale), C.byref(b), C.sizeof(b))
            if seen == 5:                                                  # a whole result in the middle: the reads so far; the table and the counters stay intact
                exp = M.hist(mreads[:seen], refs, min_baseq=15, depth_cap=2)
                cols, sizes = drain(ctx, 3)
                assert sum(sizes) == exp["n_rows"] and all(np.array_equal(cols[k], exp[k]) for k in M.COLUMNS)
                assert ctx.bam_depth_hist_stats()["n_result_rows"] == exp["n_rows"]
            if seen == 9:                                                  # one page of a result taken: the next accumulate starts the result over
                exp = M.hist(mreads[:seen], refs, min_baseq=15, depth_cap=2)
                cols, st = ctx.bam_depth_hist_next(4)
                assert cols["n_rows"] == 4 and st == 0 and cols["n_positions"].tolist() == exp["n_positions"][:4].tolist()
            if b.status:
                break
        exp = M.hist(mreads, refs, min_baseq=15, depth_cap=2)
        assert ctx.bam_depth_hist_stats()["n_result_rows"] == 0            # (no result of the table as it is now was taken)
        cols, sizes = drain(ctx)                                           # the histogram is made anew from the table: nothing is counted twice
        assert sizes == [exp["n_rows"]] and all(np.array_equal(cols[k], exp[k]) for k in M.COLUMNS)
        st = ctx.bam_depth_hist_stats()
        assert {k: st[k] for k in M.COUNTERS} == exp["stats"] and st["n_result_rows"] == exp["n_rows"] and st["status"] == 1
        cols, st = ctx.bam_depth_hist_next()                                # behind the last page: nothing, and still the end
        assert cols["n_rows"] == 0 and st == 1
        ctx.bam_depth_hist_open(per="contig")                               # a second open zeroes everything
        st = ctx.bam_depth_hist_stats()
        assert st["n_rows"] == 0 and st["status"] == 0 and st["n_target_rows"] == 3 and st["n_groups"] == 3 and st["n_result_rows"] == 0
        cols, sizes = drain(ctx, 2)
        assert sizes == [2, 1] and cols["n_positions"].tolist() == [100000] * 3 and not cols["depth"].any()
    finally:
        ctx.close()


# ---- limits and states ----
@pytest.fixture(scope="module")
def rng():
    return read_golden("range.bam")


def test_both_table_caps(rng):
    refs, _ = M.reads_from_bam(rng)
    rows = [(t, 0, l) for t, (_, l) in enumerate(refs)]
    need, hneed = M.table_bytes(rows), M.hist_bytes(rows, 1000, "row")
    ctx = open_ctx(rng)
    L = ctx.L
    try:
        L.dhts_debug_coverage_max_table_bytes(need - 1)
        with pytest.raises(duckhts_amd.DhtsError) as e:
            ctx.bam_depth_hist_open()
        assert str(e.value) == M.err_table(need, need - 1)
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_NOT_OPEN):    # an open that failed leaves nothing open
            ctx.bam_depth_hist_stats()
        L.dhts_debug_coverage_max_table_bytes(need)
        L.dhts_debug_hist_max_table_bytes(hneed - 1)
        with pytest.raises(duckhts_amd.DhtsError) as e:
            ctx.bam_depth_hist_open()
        assert str(e.value) == M.err_hist(hneed, hneed - 1)
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_NOT_OPEN):
            ctx.bam_depth_hist_stats()
        ctx.bam_depth_hist_open(depth_cap=999)                              # a smaller depth_cap fits
        L.dhts_debug_hist_max_table_bytes(hneed)
        ctx.bam_depth_hist_open()
        st = ctx.bam_depth_hist_stats()
        assert st["table_bytes"] == need and st["hist_bytes"] == hneed
        L.dhts_debug_hist_max_table_bytes(0)
        with pytest.raises(duckhts_amd.DhtsError) as e:                     # the contract's 1 GiB: 129 rows of 1,048,576 bins are 8 MiB more
            duckhts_amd.bam_depth_hist(rng, region=",".join(f"CHROMOSOME_I:{1 + 10 * i}-{10 + 10 * i}" for i in range(129)), depth_cap=M.MAX_DEPTH_CAP)
        assert str(e.value) == M.err_hist(129 * (M.MAX_DEPTH_CAP + 1) * 8, M.MAX_HIST_BYTES)
    finally:
        L.dhts_debug_coverage_max_table_bytes(0)
        L.dhts_debug_hist_max_table_bytes(0)
        ctx.close()


def test_timing_a_table_pass_leaves_the_result_intact(rng):
    """dhts_debug_hist_pass_ms runs dep_tile_reduce or dhi_hist over the table; the next result is made anew, so repeated passes add nothing"""
    refs, reads = M.reads_from_bam(rng)
    exp = M.hist(reads, refs, exclude_flags=M.DEFAULT_EXCLUDE)
    ctx = open_ctx(rng)
    try:
        assert ctx.L.dhts_debug_hist_pass_ms(ctx.h, 1, 1) < 0 and M.ERR_NOT_OPEN in ctx.L.dhts_error(ctx.h).decode()
        ctx.bam_depth_hist_open(exclude_flags=M.DEFAULT_EXCLUDE)
        ctx.bam_depth_hist_scan()
        cols, st = ctx.bam_depth_hist_next(2)                               # a page taken; the passes below start the result over
        assert cols["n_rows"] == 2 and st == 0
        for which, reps in ((0, 1), (1, 3), (0, 2)):
            assert ctx.L.dhts_debug_hist_pass_ms(ctx.h, which, reps) >= 0
        for which, reps in ((2, 1), (-1, 1), (1, 0)):
            assert ctx.L.dhts_debug_hist_pass_ms(ctx.h, which, reps) < 0
        assert ctx.bam_depth_hist_stats()["n_result_rows"] == 0
        cols, sizes = drain(ctx)
        assert sizes == [exp["n_rows"]] and all(np.array_equal(cols[k], exp[k]) for k in M.COLUMNS)
    finally:
        ctx.close()


def test_calls_in_the_wrong_state_and_every_refusal(rng):
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(rng)
        ctx.bgzf_index()
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_BAM_NOT_OPEN):
            ctx.bam_depth_hist_open()
        ctx.bam_open()
        b = ctx.next_batch(0, duckhts_amd.DEPTH_HIST_COLMASK)
        for call in (lambda: ctx.bam_depth_hist_accumulate(b), ctx.bam_depth_hist_scan, ctx.bam_depth_hist_stats, ctx.bam_depth_hist_next):
            with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_NOT_OPEN):
                call()
        for kw, msg in ((dict(min_mapq=256), M.err_range("min_mapq")), (dict(min_mapq=-1), M.err_range("min_mapq")), (dict(min_baseq=256), M.err_range("min_baseq")),
                        (dict(min_baseq=-1), M.err_range("min_baseq")), (dict(include_flags=65536), M.err_range("include_flags")), (dict(require_flags=-1), M.err_range("require_flags")),
                        (dict(exclude_flags=70000), M.err_range("exclude_flags")), (dict(min_read_len=-1), M.ERR_READ_LEN),
                        (dict(include_deletions=2), M.ERR_DELETIONS), (dict(include_deletions=-1), M.ERR_DELETIONS),
                        (dict(depth_cap=0), M.ERR_DEPTH_CAP), (dict(depth_cap=-5), M.ERR_DEPTH_CAP), (dict(depth_cap=M.MAX_DEPTH_CAP + 1), M.ERR_DEPTH_CAP), (dict(depth_cap=2**40), M.ERR_DEPTH_CAP),
                        (dict(per="total"), M.ERR_PER), (dict(per="ROW"), M.ERR_PER), (dict(per=""), M.ERR_PER), (dict(per=2), M.ERR_PER), (dict(per=-1), M.ERR_PER),
                        # wrong in two ways: the first in the order of the checks is reported
                        (dict(min_read_len=-1, min_mapq=256), M.ERR_READ_LEN), (dict(depth_cap=0, exclude_flags=70000), M.err_range("exclude_flags")),
                        (dict(depth_cap=0, include_deletions=2), M.ERR_DELETIONS), (dict(depth_cap=0, per="total"), M.ERR_DEPTH_CAP)):
            with pytest.raises(duckhts_amd.DhtsError) as e:
                ctx.bam_depth_hist_open(**kw)
            assert str(e.value) == msg
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_NOT_OPEN):
            ctx.bam_depth_hist_stats()
        ctx.bam_depth_hist_open(depth_cap=M.MAX_DEPTH_CAP, per=1)            # the largest cap, and the C struct's own per
        st = ctx.bam_depth_hist_stats()
        assert st["n_groups"] == sum(l > 0 for _, l in M.reads_from_bam(rng)[0]) and st["hist_bytes"] == st["n_groups"] * (M.MAX_DEPTH_CAP + 1) * 8
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_BED_CTX):
            ctx.bam_depth_hist_open(bed_ctx=ctx)
        other = duckhts_amd.Context(0)
        try:
            other.open(b"c\t0\t1\n")
            with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_BED_NOT_OPEN):
                ctx.bam_depth_hist_open(bed_ctx=other)
        finally:
            other.close()
        if duckhts_amd.lib().dhts_device_count() > 1:                      # a BED context on another device
            far = duckhts_amd.Context(1)
            try:
                far.open(b"c\t0\t1\n")
                with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_BED_CTX):
                    ctx.bam_depth_hist_open(bed_ctx=far)
            finally:
                far.close()
        ctx.set_shard(0, 2)                                                # a shard or a block range of the file
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_SHARD):
            ctx.bam_depth_hist_open()
        ctx.set_shard(0, 1)
        ctx.bam_depth_hist_open()
        ctx.set_block_range(0, 1, 1)
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_SHARD):
            ctx.bam_depth_hist_scan()
    finally:
        ctx.close()
    with pytest.raises(duckhts_amd.DhtsError) as e:
        duckhts_amd.bam_depth_hist(rng, region="CHROMOSOME_I:1-1000", bed=b"CHROMOSOME_I\t0\t10\n")
    assert str(e.value) == M.ERR_BED_AND_REGION
    with pytest.raises(duckhts_amd.DhtsError) as e:
        duckhts_amd.bam_depth_hist(rng, region="CHROMOSOME_I:1-1000,CHROMOSOME_II:1-10,CHROMOSOME_I:1000-1200")
    assert str(e.value) == M.err_overlap("CHROMOSOME_I:1-1000", "CHROMOSOME_I:1000-1200")


def test_the_golden_file_against_the_model(rng):
    refs, reads = M.reads_from_bam(rng)
    for kw in (dict(), dict(per="contig", min_baseq=25, depth_cap=3)):
        got = duckhts_amd.bam_depth_hist(rng, **kw)
        same(got, M.hist(reads, refs, **model_params(kw)), rows=[(t, 0, l) for t, (_, l) in enumerate(refs)], cap=kw.get("depth_cap", 1000), per=kw.get("per", "row"))
