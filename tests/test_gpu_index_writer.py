"""The BAI / CSI / TBI writers (hts_index.hip, dhts_index_write.inc) against tests/hts_index_ref.py, the record-by-record model of htslib's
index builder that tests/test_hts_index_ref.py pins to htslib's own index files.

Every input is built here (bamwriter / bcfwriter, stored blocks where offsets must be predictable) to reach one branch of the writers: bins
that stay or join, chunk coalescing, the linear index's window logic, the wave and batch edges of bam_index_rows, the reader's offsets at
block ends.  test_inputs_reach_every_branch (no GPU) runs the model over all of them and asserts that the branch tags it collects cover the
list; the GPU tests then compare the parsed index in full: bins and chunks, linear index, pseudo-bin, n_no_coor, and for CSI min_shift,
depth and every loff."""
import ctypes as C
import functools

import numpy as np
import pytest

import bamwriter as bw
import bcfwriter as cw
import hts_index_ref as R
from test_gpu_bam import _parse_bai
from test_gpu_bcf import _parse_csi
from test_vcf_region import parse_tabix

MB = 1 << 20
W = 1 << 14                                        # a window of the BAI's linear index = a deepest-level bin
LONG = "q" * 40                                    # a record with this name and one CIGAR operation is 81 bytes


def rec(tid, pos, cigar="10M", flag=0, qname=LONG):
    """pos: 0-based (-1 is POS 0)"""
    return bw.record(qname=qname, flag=flag, tid=tid, pos=pos, cigar=cigar)


def spread(tid, lo, hi, n, cigar="10M"):
    """n records with ascending positions inside [lo, hi - 10)"""
    return [rec(tid, lo + (hi - 10 - lo) * k // n, cigar) for k in range(n)]


def blocks_file(payloads, eof=True):
    """one stored BGZF block per payload (an empty payload is an empty block)"""
    return b"".join(bw.bgzf_block(p, 0) for p in payloads) + (bw.EOF_BLOCK if eof else b"")


# ---- bins, chunks and the linear index: one layout, indexed as BAI and as three CSI geometries -------------------------------------------
def layout_records():
    a = []
    a += [rec(0, -1, "4M")]                                                     # POS 0: begin -1 is clamped
    # window group 1 (the 128 kb bin of 1 Mb ..): the bin has pieces of its own around a child that stays
    g = 1 * MB
    a += [rec(0, g + W - 5)]                                                    # crosses windows 0|1: the 128 kb bin's own piece A
    a += spread(0, g + W, g + 2 * W, 1000)                                      # ~80 KB in one window: a deepest bin that stays
    a += [rec(0, g + 2 * W - 5)]                                                # piece B: not in the block where A ended
    a += spread(0, g + 2 * W, g + 3 * W, 5)                                     # a small child: joins the 128 kb bin
    a += [rec(0, g + 3 * W - 5)]                                                # piece C: touches the block of B and the child
    # group 2: a 128 kb bin that is small on its own and stays only because three joined children widen it past 64 KiB
    g = 2 * MB
    a += [rec(0, g + W - 5)]
    for k in (1, 2, 3):
        a += spread(0, g + k * W, g + (k + 1) * W, 400)
    # group 3: a deepest bin whose parent is absent
    a += spread(0, 5 * MB + 3 * W, 5 * MB + 4 * W, 3)
    # the linear index: a long read (one N skip of 1 Mb: 65 windows), a short read inside it, a medium one beyond the short one
    g = 8 * MB + 100
    a += [rec(0, g, "5M1048576N5M"), rec(0, g + 50, "4M"), rec(0, g + 200, "5M40000N5M"), rec(0, g + 3 * MB, "4M")]
    # sequence 1 has no records; sequence 2: a chain of joins 1 Mb bin -> 8 Mb bin -> 64 Mb bin -> bin 0
    b = [rec(2, MB - 5), rec(2, MB + 128 * 1024 - 5), rec(2, MB + 128 * 1024 + 50, "4M"), rec(2, 8 * MB - 5), rec(2, 64 * MB - 5)]
    return a + b


@functools.lru_cache(maxsize=None)
def layout_bam(ln):
    return bw.bam_bytes([("a", ln), ("e", 1000), ("b", ln)], layout_records(), level=0, payload=4000)


GEOMETRY = {"bai": (0, 100 * MB), "csi12": (12, 80 * MB), "csi14": (14, (1 << 29) + 5), "csi17": (17, 100 * MB)}


@functools.lru_cache(maxsize=None)
def exact_64k_bam():
    """a deepest bin whose first and last block are exactly 0x10000 bytes of file apart (two stored blocks of 32737 + 31 bytes between
    them): `< 0x10000` lets it stay, and its parent is there to take it if the comparison were off by one"""
    recs = [rec(0, W - 5)] + spread(0, W, 2 * W, 850) + [rec(0, 5 * W)]
    return bw.bam_bytes([("a", MB)], recs, level=0, cuts=[32737, 32737], payload=65280)


# ---- rows and CIGARs ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cigar_bam():
    recs = [rec(0, 100, "2H3S5M2I3D10N4=2X1P3M4S2H"), rec(0, 200, "5M3B5M"), rec(0, 300, "10M", flag=4), rec(0, 400, "*"), rec(0, 500, "20S"),
            rec(0, 600, "3I"), rec(0, 700, "16384N"), rec(0, 800, "*", flag=4), rec(-1, -1, "*", flag=4)]
    return bw.bam_bytes([("a", MB)], recs, level=0)


# ---- wave edges --------------------------------------------------------------------------------------------------------------------------------
def small(tid, pos, flag=0):
    return bw.record(qname="r", flag=flag, tid=tid, pos=pos, cigar="3M")


@functools.lru_cache(maxsize=None)
def nrows_bam(n):
    return bw.bam_bytes([("a", MB)], [small(0, 7 * k, 4 if k % 5 == 0 else 0) for k in range(n)], payload=1000)


@functools.lru_cache(maxsize=None)
def edge_bam(k, what):
    """320 rows; at row k the bin changes (to a window whose 128 kb parent is absent, as the first one's is: both bins stay, and a run start
    missed at row k would lose the second; the rows in front of k have a CIGAR that lane 0 has to walk again) or the sequence does"""
    recs = []
    for r in range(320):
        if what == "bin":
            recs.append(rec(0, 100 + r, "100M200N100M", qname="r") if r < k else small(0, 8 * W + r))
        else:
            recs.append(small(0 if r < k else 1, 3 * r, 4 if r == k - 1 else 0))
    return bw.bam_bytes([("a", MB), ("b", MB)], recs, payload=700)


@functools.lru_cache(maxsize=None)
def waves_bam():
    """wave 0: one sequence; wave 1: three sequences; wave 2: placed rows, then unplaced ones; wave 3: partial, unplaced"""
    recs = [small(0, 5 * r, 4 if r % 3 == 0 else 0) for r in range(64)]
    recs += [small(0, 1000 + r) for r in range(20)] + [small(1, 5 * r, 4 if r % 2 else 0) for r in range(30)] + [small(2, 9 * r) for r in range(14)]
    recs += [small(2, 500 + r) for r in range(40)] + [small(-1, -1, 4) for r in range(24)]
    recs += [small(-1, -1, 4) for r in range(17)]
    return bw.bam_bytes([("a", MB), ("b", MB), ("c", MB)], recs, payload=900)


# ---- more than one batch: 25000 blocks of one 48-byte record each ------------------------------------------------------------------------------
N_TINY = 25000
BATCH_ROWS = 16384                                 # a scan begins with the first record's block: 16384 one-record blocks make its first batch


def tiny(tid, pos):
    r = bw.record(qname="r234567", tid=tid, pos=pos, cigar="1M")
    assert len(r) == 48
    return r


@functools.lru_cache(maxsize=None)
def tiny_bam(kind):
    k = BATCH_ROWS
    if kind == "run":                              # one (sequence, bin) run across the boundary
        recs = [tiny(0, 100 + r) for r in range(N_TINY)]
    elif kind == "tid":                            # the sequence changes exactly at the boundary
        recs = [tiny(0 if r < k else 1, r) for r in range(N_TINY)]
    elif kind == "unsorted":                       # the first row of the second batch lies in front of the last row of the first
        recs = [tiny(0, r if r != k else r - 2) for r in range(N_TINY)]
    elif kind == "returns":                        # sequence 0, five rows of sequence 1, and sequence 0 again with the second batch
        recs = [tiny(1 if k - 5 <= r < k else 0, r) for r in range(N_TINY)]
    return bw.bam_bytes([("a", MB), ("b", MB)], recs, level=0, payload=48)


# ---- the reader's offsets ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def offsets_bam(kind):
    hdr = bw.bam_header([("a", MB)])
    r = [rec(0, 100 * k) for k in range(12)]
    body = b"".join(r[4:])
    if kind == "block_ends":                       # header in its own block; a record ends at a block end; an empty block at a record boundary;
        pay = [hdr, r[0] + r[1], b"", r[2] + r[3][:20], r[3][20:50], r[3][50:70], r[3][70:] + body]          # a record over four blocks
        return blocks_file(pay)
    if kind == "first_nonzero":                    # the first record starts inside the header's block
        return blocks_file([hdr + r[0], r[1] + r[2]] + [body])
    if kind == "no_eof":
        return blocks_file([hdr, r[0] + r[1], body], eof=False)
    if kind == "three_eof":                        # several trailing empty blocks
        return blocks_file([hdr, r[0] + r[1], body, b"", b""])
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def lincap_bam():
    """the header understates LN and a read lies more than 1 Mb beyond it: the build's second attempt"""
    recs = [rec(0, 10), rec(0, 900), rec(0, 5 * MB, "50M"), rec(0, 5 * MB + 20, "5M40000N5M"), rec(0, 40 * MB), rec(1, 7)]
    return bw.bam_bytes([("a", 1000), ("b", 100 * MB)], recs, level=0)


BAM_CASES = {}
for _g, (_ms, _ln) in GEOMETRY.items():
    BAM_CASES["layout_" + _g] = (functools.partial(layout_bam, _ln), _ms)
BAM_CASES["exact_64k"] = (exact_64k_bam, 0)
BAM_CASES["cigars"] = (cigar_bam, 0)
BAM_CASES["cigars_csi"] = (cigar_bam, 14)
for _n in (1, 63, 64, 65, 255, 256, 257):
    BAM_CASES["nrows_%d" % _n] = (functools.partial(nrows_bam, _n), 0)
for _k in R.WAVE_EDGES:
    for _w in ("bin", "tid"):
        BAM_CASES["edge_%s_%d" % (_w, _k)] = (functools.partial(edge_bam, _k, _w), 0)
BAM_CASES["waves"] = (waves_bam, 0)
BAM_CASES["tiny_run"] = (functools.partial(tiny_bam, "run"), 0)
BAM_CASES["tiny_tid"] = (functools.partial(tiny_bam, "tid"), 0)
for _k in ("block_ends", "first_nonzero", "no_eof", "three_eof"):
    BAM_CASES["offsets_" + _k] = (functools.partial(offsets_bam, _k), 0)
BAM_CASES["lincap"] = (lincap_bam, 0)
BAM_CASES["lincap_csi"] = (lincap_bam, 14)


# ---- errors ------------------------------------------------------------------------------------------------------------------------------------
def _err_rows(kind):
    if kind == "unsorted_in_wave":
        return [small(0, 10 * r if r != 37 else 5) for r in range(100)]
    if kind == "unsorted_wave_edge":
        return [small(0, 10 * r if r != 64 else 600) for r in range(100)]
    if kind == "returns":
        return [small(0, 1), small(1, 1), small(0, 2)]
    if kind == "placed_behind_unplaced":
        return [small(0, 1), small(-1, -1, 4), small(1, 1)]
    if kind == "beyond_bai":
        return [small(0, 1), small(0, (1 << 29) + 5)]
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def error_bam(kind):
    if kind.startswith("tiny_"):
        return tiny_bam(kind[5:])
    return bw.bam_bytes([("a", (1 << 30)), ("b", MB)], _err_rows(kind), payload=500)


ERRORS = {"unsorted_in_wave": (R.UnsortedPositions, "Unsorted positions"), "unsorted_wave_edge": (R.UnsortedPositions, "Unsorted positions"),
          "tiny_unsorted": (R.UnsortedPositions, "Unsorted positions"), "returns": (R.BlocksNotContinuous, "Chromosome blocks not continuous"),
          "tiny_returns": (R.BlocksNotContinuous, "Chromosome blocks not continuous"),
          "placed_behind_unplaced": (R.NoCoorNotLast, "NO_COOR reads not in a single block at the end"),
          "beyond_bai": (R.BeyondMaxPos, "Region cannot be stored in a bai index")}


# ---- the host passes that share finish(): BCF, bgzipped VCF text, a tabix preset ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big_bcf():
    """~200 KB of stored blocks: a deepest bin of ~80 KB that stays, and a 128 kb bin that stays because three children of ~33 KB join it"""
    hdr = cw.header([], contigs=[("##contig=<ID=1,length=%d>" % (100 * MB),), ("##contig=<ID=2,length=%d>" % MB,)])
    one = lambda rid, pos, rlen=1: cw.record(rid=rid, pos=pos, rlen=rlen, alleles=(b"A" * rlen if rlen < 50 else b"A", b"C"), id=b"id234567")
    n = len(one(0, 0))
    recs = [one(0, p) for p in np.linspace(W, 2 * W - 1, 80000 // n).astype(int)]
    recs += [one(0, 2 * MB + W - 5, 10)]
    for k in (1, 2, 3):
        recs += [one(0, p) for p in np.linspace(2 * MB + k * W, 2 * MB + (k + 1) * W - 1, 33000 // n).astype(int)]
    recs += [one(0, 9 * MB), one(1, 5), one(1, 70000, 20000)]
    return cw.bcf_bytes(hdr, recs, level=0, payload=4000)


@functools.lru_cache(maxsize=None)
def text_vcf():
    lines = ["##fileformat=VCFv4.2", "##contig=<ID=chrA,length=%d>" % (300 * MB), "##contig=<ID=chrB,length=5000>",
             '##INFO=<ID=END,Number=1,Type=Integer,Description="e">', "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    for k in range(3000):
        lines.append("chrA\t%d\t.\tACG\tA\t.\t.\t." % (20000 + 11 * k))
    lines.append("chrA\t%d\t.\tA\t<DEL>\t.\t.\tEND=%d" % (70000, 70000 + 3 * MB))
    lines.append("chrA\t%d\t.\tA\tT\t.\t.\t." % (200 * MB))
    for k in range(50):
        lines.append("chrB\t%d\t.\tA\tT\t.\t.\t." % (1 + 3 * k))
    return bw.bgzf_file(("\n".join(lines) + "\n").encode(), payload=9000, level=6)


@functools.lru_cache(maxsize=None)
def text_bed():
    lines = ["#track"] + ["chrA\t%d\t%d\tx" % (100 * k, 100 * k + 250) for k in range(2000)] + ["chrA\t300000\t2000000\tlong"]
    lines += ["chrB\t%d\t%d\ty" % (0 if k == 0 else 40000 * k, 40000 * k + 5) for k in range(40)]
    return bw.bgzf_file(("\n".join(lines) + "\n").encode(), payload=5000, level=6)


# ---- the condition on the inputs (no GPU) ------------------------------------------------------------------------------------------------------
REQUIRED = {
    # bins and chunks
    "bin_stays_64k_level_deepest", "bin_joins_parent", "bin_stays_parent_absent", "mid_bin_stays_widened_by_children",
    "join_chain_3_levels_into_bin0", "chunks_coalesced_same_block", "chunks_not_coalesced", "empty_sequence_between",
    # linear index
    "read_covers_64_windows", "lin_long_short_medium", "lin_empty_window_filled_from_right", "pos_clamped",
    # rows and CIGARs
    *("cigar_op_" + c for c in "MIDNSHP=XB"), "placed_unmapped_with_cigar", "mapped_no_cigar",
    # wave and batch edges
    *("nrows_%d" % n for n in (1, 63, 64, 65, 255, 256, 257)),
    *("%s_change_at_row_%d" % (w, k) for w in ("bin", "tid") for k in R.WAVE_EDGES),
    "wave_one_sequence", "wave_three_sequences", "wave_placed_to_unplaced", "partial_last_wave",
    "more_than_16384_blocks", "run_straddles_batch_boundary", "tid_change_at_batch_boundary",
    # offsets
    "record_ends_at_block_end", "empty_block_mid_file", "record_spans_3_blocks", "first_record_at_offset_0", "first_record_at_nonzero_offset",
    "final_eof_present", "final_eof_absent", "final_several_empty_blocks",
    # geometry
    "fmt_bai", "fmt_csi", "fmt_tbi", "min_shift_12", "min_shift_14", "min_shift_17", "depth_4", "depth_5", "depth_6", "ref_len_gt_2^29",
    "read_1mb_beyond_header_length",
    # errors
    "err_unsorted_in_wave", "err_unsorted_wave_edge", "err_at_batch_boundary", "err_not_continuous", "err_nocoor", "err_maxpos_bai",
    # the host passes
    "src_bcf", "src_text_vcf_tbi", "src_text_vcf_csi", "src_text_generic_tbi",
}


def test_inputs_reach_every_branch():
    """A condition on the inputs, met by the model alone: every branch the list names is reached by at least one constructed input, so the
    GPU comparisons below are known to exercise it."""
    tags = set()
    for name, (make, ms) in BAM_CASES.items():
        R.bam_index(make(), ms, tags)
    for kind, (exc, _) in ERRORS.items():
        t = set()
        with pytest.raises(exc):
            R.bam_index(error_bam(kind), 0, t)
        assert ("err_at_batch_boundary" in t) == kind.startswith("tiny_"), kind
        tags |= t
    t = set()
    R.bcf_index(big_bcf(), 14, t)
    assert len([x for x in t if x.startswith("bin_stays_64k_at_level_")]) >= 2, t      # the BCF's bins stay at two levels
    tags |= t
    for ms in (0, 14):
        R.tabix_index(text_vcf(), R.CONF_VCF, ms, tags)
    R.tabix_index(text_bed(), R.CONF_BED, 0, tags)
    assert not REQUIRED - tags, sorted(REQUIRED - tags)
    # the two-batch files are what they are meant to be
    for kind, want in (("run", "run_straddles_batch_boundary"), ("tid", "tid_change_at_batch_boundary")):
        t = set()
        src = R.bam_rows(tiny_bam(kind), t)
        assert src["first_batch_rows"] == BATCH_ROWS and src["n_blocks"] > 16384 and len(tiny_bam(kind)) < 2.2 * MB
        R.bam_index(tiny_bam(kind), 0, t)
        assert want in t
    # the bin of exact_64k_bam spans exactly 0x10000 bytes of file and stays
    refs, _ = R.bam_index(exact_64k_bam()).parsed()
    c = refs[0][0][4681 + 1]
    assert (c[-1][1] >> 16) - (c[0][0] >> 16) == 0x10000 and 585 in refs[0][0]


# ---- the device against the model --------------------------------------------------------------------------------------------------------------
def _device_index(data, min_shift, check_rows=None):
    import duckhts_amd
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(data); ctx.bgzf_index(); ctx.bam_open()
        out = ctx.build_index(min_shift)
        if check_rows is not None:                 # the scan is usable afterwards
            assert _count_rows(ctx) == check_rows
        return out
    finally:
        ctx.close()


def _count_rows(ctx):
    n = 0
    while True:
        b = ctx.next_batch(0)
        n += b.n_rows
        if b.status != 0:
            assert b.status > 0
            return n


def _same(got, exp):
    if isinstance(exp, tuple) and len(exp) == 2:                     # BAI
        assert got[1] == exp[1]
        assert len(got[0]) == len(exp[0])
        for t, (g, e) in enumerate(zip(got[0], exp[0])):
            assert set(g[0]) == set(e[0]), ("bins of sequence", t, sorted(set(g[0]) ^ set(e[0])))
            for b in e[0]:
                assert g[0][b] == e[0][b], ("sequence", t, "bin", b)
            assert g[1] == e[1], ("linear index of sequence", t)
    else:
        assert got[:3] == exp[:3] and got[4] == exp[4]
        assert len(got[3]) == len(exp[3])
        for t, (g, e) in enumerate(zip(got[3], exp[3])):
            assert set(g) == set(e), ("bins of sequence", t, sorted(set(g) ^ set(e)))
            for b in e:
                assert g[b] == e[b], ("sequence", t, "bin", b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in BAM_CASES if not n.startswith("tiny_")])
def test_bam_index_equals_model(name):
    make, ms = BAM_CASES[name]
    data = make()
    exp = R.bam_index(data, ms).parsed()
    raw = _device_index(data, ms)
    _same(_parse_csi(raw) if ms else _parse_bai(raw), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["run", "tid"])
def test_bam_index_over_two_batches_equals_model(kind):
    """more than 16384 blocks: the second batch starts from the carry of the first (IdxCarry)"""
    import duckhts_amd
    data = tiny_bam(kind)
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(data); ctx.bgzf_index(); ctx.bam_open()
        b = ctx.next_batch(0)
        assert b.status == 0 and b.n_rows == BATCH_ROWS            # at least two batches, cut where the inputs expect it
        ctx.rewind()
        raw = ctx.build_index()
        assert _count_rows(ctx) == N_TINY
    finally:
        ctx.close()
    _same(_parse_bai(raw), R.bam_index(data).parsed())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(ERRORS))
def test_bam_index_errors(kind):
    import duckhts_amd
    data = error_bam(kind)
    n = N_TINY if kind.startswith("tiny_") else len(_err_rows(kind))
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(data); ctx.bgzf_index(); ctx.bam_open()
        with pytest.raises(duckhts_amd.DhtsError, match=ERRORS[kind][1]):
            ctx.build_index()
        assert _count_rows(ctx) == n                               # the scan is still usable
    finally:
        ctx.close()


def _host_pass_index(data, call):
    import duckhts_amd
    L = duckhts_amd.lib()
    L.dhts_bcf_build_index.restype = C.c_int64; L.dhts_bcf_build_index.argtypes = [C.c_void_p, C.c_int]
    L.dhts_tabix_build_index.restype = C.c_int64; L.dhts_tabix_build_index.argtypes = [C.c_void_p] + [C.c_int] * 7
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(data); ctx.bgzf_index()
        n = call(L, ctx)
        assert n > 0, L.dhts_error(ctx.h)
        raw = np.zeros(n, np.uint8)
        assert L.dhts_bam_index_bytes(ctx.h, raw.ctypes.data, n) == 0
        return raw.tobytes()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_bcf_index_equals_model():
    import duckhts_amd
    data = big_bcf()
    assert 150_000 < len(data) < 260_000

    def call(L, ctx):
        duckhts_amd.BcfScan(ctx)
        return L.dhts_bcf_build_index(ctx.h, 14)
    _same(_parse_csi(_host_pass_index(data, call)), R.bcf_index(data, 14).parsed())


@pytest.mark.gpu
@pytest.mark.parametrize("min_shift", [0, 14])
def test_vcf_text_index_equals_model(min_shift):
    import duckhts_amd
    data = text_vcf()

    def call(L, ctx):
        duckhts_amd.BcfScan(ctx)
        return L.dhts_bcf_build_index(ctx.h, min_shift)
    idx, names = R.tabix_index(data, R.CONF_VCF, min_shift)
    assert parse_tabix(_host_pass_index(data, call)) == idx.parsed(R.CONF_VCF, names)


@pytest.mark.gpu
def test_tabix_preset_index_equals_model():
    data = text_bed()
    c = R.CONF_BED
    idx, names = R.tabix_index(data, c, 0)
    raw = _host_pass_index(data, lambda L, ctx: L.dhts_tabix_build_index(ctx.h, c[0], c[1], c[2], c[3], c[4], c[5], 0))
    assert parse_tabix(raw) == idx.parsed(c, names)
