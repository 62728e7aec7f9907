"""The arena of the six column fetchers (dhts_bam_{bins,coverage,depth,pileup,bedcov}_batch_fetch, dhts_bed_batch_fetch), as include/duckhts_amd.h
states it: the columns in order, every part 8-byte aligned.  bins / coverage: valid[n] padded, then 8 n.  bedcov / read_bed: valid[n] padded,
then 8 n for an integer column, off[(n + 1) * 4] padded and bytes[nbytes] padded for a string.  depth / pileup: width * n padded per column
that is present, no validity; a column the colmask leaves out has null pointers and takes no bytes.  The expected offsets are computed here
from that rule; the library is asked only for the batch.  Result sizes on both sides of the padding: 0, 1, 7, 8, 9 rows."""
import ctypes as C

import numpy as np
import pytest

import duckhts_amd
import bam_coverage_cases as K

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 7, 8, 9]
DEPTH_WIDTH = (4, 8, 4)
PILEUP_WIDTH = (4, 8, 1, 1, 4)


def pad8(x):
    return (x + 7) & ~7


def bam_ctx(data):
    ctx = duckhts_amd.Context(0)
    ctx.open(data)
    ctx.bgzf_index()
    ctx.bam_open()
    return ctx


def bed_ctx(text):
    ctx = duckhts_amd.Context(0)
    ctx.open(text)
    ctx.L.dhts_bgzf_index(ctx.h)
    ctx._chk(ctx.L.dhts_bed_open(ctx.h))
    return ctx


def bed_text(n):
    """n rows on c1; row 0 has three fields (name, score and strand are NULL), row 1 a name of no bytes (read_bed reads an empty field as NULL)"""
    rows = [] if n else ["#no row"]
    for r in range(n):
        rows.append("c1\t%d\t%d" % (10 * r, 10 * r + 5) + ("" if r == 0 else "\t\t7\t+" if r == 1 else "\tn%d\t7\t-" % r))
    return ("".join(x + "\n" for x in rows)).encode()


def check(ctx, who, b, parts_of):
    """b: the device batch.  parts_of(device column) -> [(field, bytes)] in arena order, [] for a column that is left out."""
    L = ctx.L
    host_bytes, fetch = getattr(L, "dhts_%s_batch_host_bytes" % who[0]), getattr(L, "dhts_%s_batch_fetch" % who[0])
    n = int(b.n_rows)
    want, at = [], 0
    for i in range(b.n_cols):
        d = {"valid": None, "fixed": None, "off": None, "bytes": None}
        for field, nbytes in parts_of(b.cols[i]):
            d[field] = at if n else None
            at += pad8(nbytes)
        want.append(d)
    need = int(host_bytes(C.byref(b)))
    assert need == at, (who, n, need, at)
    arena = np.zeros(need + 8, np.uint8)
    host = (duckhts_amd.BcfCol * max(b.n_cols, 1))()
    ctx._chk(fetch(ctx.h, C.byref(b), arena.ctypes.data, need, host))
    base = arena.ctypes.data
    for i in range(b.n_cols):
        assert host[i].col == b.cols[i].col == i
        for field, off in want[i].items():
            got = getattr(host[i], field)
            assert (got - base if got else None) == off, (who, n, i, field, got and got - base, off)
    if need:
        assert fetch(ctx.h, C.byref(b), arena.ctypes.data, need - 1, host) != 0
        assert L.dhts_error(ctx.h).decode() == who[1] + ": fetch buffer too small"
    return host, arena


def valid_int64(n):
    return lambda col: [("valid", n), ("fixed", 8 * n)]


def bed_parts(n, int_cols):
    return lambda col: [("valid", n), ("fixed", 8 * n)] if col.col in int_cols else [("valid", n), ("off", 4 * (n + 1)), ("bytes", int(col.nbytes))]


def bare(n, width, mask):
    return lambda col: [("fixed", width[col.col] * n)] if n and (mask >> col.col) & 1 else []


@pytest.fixture(scope="module")
def one_read():
    return K.bam([("c1", 100)], [K.read(pos0=10, cigar="20M")])


@pytest.mark.parametrize("n", SIZES)
def test_bins(one_read, n):
    ctx = bam_ctx(one_read)
    try:
        ctx.bam_bins_open(bin_width=10, emit_zero_bins=n > 0, min_mapq=0 if n else 255)       # ten bins; none with the read filtered
        assert ctx.bam_bins_scan() == 1
        b = duckhts_amd.BedBatch()
        ctx._chk(ctx.L.dhts_bam_bins_next(ctx.h, n, C.byref(b)))
        assert b.n_rows == n and b.n_cols == len(duckhts_amd.BINS_COLUMNS)
        check(ctx, ("bam_bins", "bam_bin_counts"), b, valid_int64(n))
    finally:
        ctx.close()


@pytest.mark.parametrize("n", SIZES)
def test_coverage(n):
    m = max(n, 1)
    ctx = bam_ctx(K.bam([("c%d" % t, 50 + t) for t in range(m)], [K.read(pos0=10, cigar="20M")]))
    try:
        ctx.bam_coverage_open()
        assert ctx.bam_coverage_scan() == 1
        b = duckhts_amd.BedBatch()
        ctx._chk(ctx.L.dhts_bam_coverage_next(ctx.h, 0, C.byref(b)))
        assert b.n_rows == m and b.status == 1
        if n == 0:                                                                            # behind the last row: an empty page
            ctx._chk(ctx.L.dhts_bam_coverage_next(ctx.h, 0, C.byref(b)))
        assert b.n_rows == n and b.n_cols == len(duckhts_amd.COVERAGE_COLUMNS)
        check(ctx, ("bam_coverage", "bam_coverage"), b, valid_int64(n))
    finally:
        ctx.close()


@pytest.mark.parametrize("mask", [7, 5])
@pytest.mark.parametrize("n", SIZES)
def test_depth(one_read, n, mask):
    ctx = bam_ctx(one_read)
    try:
        ctx.bam_depth_open(min_mapq=0 if n else 255)
        assert ctx.bam_depth_scan() == 1
        b = duckhts_amd.BedBatch()
        ctx._chk(ctx.L.dhts_bam_depth_next(ctx.h, n, mask, C.byref(b)))
        assert b.n_rows == n and b.n_cols == 3
        host, arena = check(ctx, ("bam_depth", "bam_depth"), b, bare(n, DEPTH_WIDTH, mask))
        if n and mask == 7:
            assert arena[host[1].fixed - arena.ctypes.data:][:8 * n].view(np.int64).tolist() == list(range(11, 11 + n))
    finally:
        ctx.close()


@pytest.mark.parametrize("mask", [31, 27])
@pytest.mark.parametrize("n", SIZES)
def test_pileup(one_read, n, mask):
    ctx = bam_ctx(one_read)
    try:
        ctx.bam_pileup_open(min_mapq=0 if n else 255)
        assert ctx.bam_pileup_scan() == 1
        b = duckhts_amd.BedBatch()
        ctx._chk(ctx.L.dhts_bam_pileup_next(ctx.h, n, mask, C.byref(b)))
        assert b.n_rows == n and b.n_cols == 5
        host, arena = check(ctx, ("bam_pileup", "bam_pileup"), b, bare(n, PILEUP_WIDTH, mask))
        if n and mask == 31:
            assert arena[host[3].fixed - arena.ctypes.data:][:n].tobytes() == b"A" * n
    finally:
        ctx.close()


@pytest.mark.parametrize("n", SIZES)
def test_bedcov(one_read, n):
    ctx, bctx = bam_ctx(one_read), bed_ctx(bed_text(n))
    try:
        ctx.bam_bedcov_open(bctx)
        assert ctx.bam_bedcov_scan() == 1
        b = duckhts_amd.BedBatch()
        ctx._chk(ctx.L.dhts_bam_bedcov_next(ctx.h, bctx.h, 0, C.byref(b)))
        assert b.n_rows == n and b.n_cols == len(duckhts_amd.BEDCOV_COLUMNS)
        if n:
            assert int(b.cols[3].nbytes) == sum(len("n%d" % r) for r in range(2, n))              # NULL and the empty name take no bytes
        host, arena = check(ctx, ("bam_bedcov", "bam_bedcov"), b, bed_parts(n, duckhts_amd.BEDCOV_INT_COLUMNS))
        if n > 1:
            valid = arena[host[3].valid - arena.ctypes.data:][:n].tolist()
            assert valid == [0, 0] + [1] * (n - 2)
    finally:
        bctx.close()
        ctx.close()


@pytest.mark.parametrize("n", SIZES)
def test_read_bed(n):
    ctx = bed_ctx(bed_text(n))
    try:
        b = duckhts_amd.BedBatch()
        ctx._chk(ctx.L.dhts_bed_next_batch(ctx.h, 0, C.byref(b)))
        assert b.n_rows == n and b.n_cols == len(duckhts_amd.BED_COLUMNS)
        if n:
            assert int(b.cols[3].nbytes) == sum(len("n%d" % r) for r in range(2, n))
        check(ctx, ("bed", "read_bed"), b, bed_parts(n, duckhts_amd.BED_INT_COLUMNS))
    finally:
        ctx.close()
