"""Every BGZF reader is held to the clean file when ISIZE fields lie.

htslib never reads the ISIZE field of a BGZF trailer; the scan here places every block at the prefix sum of those fields and corrects the
table from the decoded lengths after phase A (isize_repair).  Every consumer derives state from that table -- buffer sizes, the first
record's offset, window ends, index virtual offsets, .gzi entries, the walks over trailing empty blocks, shard hand-offs -- so each of them
is run here on files that differ from a clean one in ISIZE fields only (tests/isize_lies.py; test_isize_lies_ref.py shows that the oracles
do not see the difference) and must return exactly what it returns for the clean file from the same call.  No tolerances.

Out of scope: DHTS_INFLATE=fused and DHTS_PHASE_A=lane.  The fused path never calls isize_repair and what it does with such blocks has
not been examined; no lying file is run under either setting here."""
import ctypes as C
import functools
import os
import random
import struct

import numpy as np
import pytest

import bamwriter as bw
import bcf_cases
import bcfwriter
import cases
import duckhts_amd
import isize_lies as il
import orc
from duckhts_amd import synth

pytestmark = pytest.mark.gpu

COLS = duckhts_amd.BAM_COLUMNS
MB = 1 << 20


# ---- exact equality of whole results ------------------------------------------------------------------------------------------------
def same(a, b, path="result"):
    if isinstance(b, dict):
        assert isinstance(a, dict) and sorted(map(str, a)) == sorted(map(str, b)), f"{path}: keys {sorted(map(str, a))} != {sorted(map(str, b))}"
        for k in b:
            same(a[k], b[k], f"{path}[{k!r}]")
    elif isinstance(b, np.ndarray):
        assert isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{path} differs"
    elif isinstance(b, (list, tuple)):
        assert isinstance(a, (list, tuple)) and len(a) == len(b), f"{path}: length {len(a)} != {len(b)}"
        plain = (bytes, str, int, bool, type(None))
        if not (all(isinstance(x, plain) for x in b) and all(isinstance(x, plain) for x in a) and list(a) == list(b)):
            for i, (x, y) in enumerate(zip(a, b)):         # (floats by their bits, nested lists and arrays: element by element)
                same(x, y, f"{path}[{i}]")
    elif isinstance(b, float):
        assert isinstance(a, float) and struct.pack("<d", a) == struct.pack("<d", b), f"{path}: {a!r} != {b!r}"
    else:
        assert type(a) is type(b) and a == b, f"{path}: {a!r} != {b!r}"


_clean = {}


def clean_result(key, fn):
    """the clean file's result of a call, computed once per distinct call"""
    if key not in _clean:
        _clean[key] = fn()
    return _clean[key]


def n_lies(clean, lying):
    return len(il.lying_blocks(clean, lying))


# ---- inputs (built once per module) ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bam(name):
    p, n = {"p61": (61, 200), "p777": (777, 200), "p65280": (65280, 3000)}[name]
    return cases.case_basic(payload=p, n=n, seed=2)


@functools.lru_cache(maxsize=None)
def sorted_bam(n, payload, seed=2):
    """cases.basic_records in coordinate order (unplaced last; a placed record with POS 0 would be "Unsorted positions" twice in a row and is
    left out), so that the index writers accept the file"""
    rng = random.Random(seed)
    recs = [r for r in cases.basic_records(rng, n) if not (struct.unpack_from("<i", r, 4)[0] >= 0 and struct.unpack_from("<i", r, 8)[0] < 0)]
    key = lambda r: ((struct.unpack_from("<i", r, 4)[0] + (1 << 31)) % (1 << 32) if struct.unpack_from("<i", r, 4)[0] >= 0 else 1 << 40, struct.unpack_from("<i", r, 8)[0])
    recs.sort(key=key)
    return bw.bam_bytes(cases.REFS, recs, text=cases.TEXT.replace("SO:unsorted", "SO:coordinate"), payload=payload)


@functools.lru_cache(maxsize=None)
def genome_bam():
    return synth.bam_file(30000, seed=29, payload=4000)


@functools.lru_cache(maxsize=None)
def bcf(payload, n):
    return bcfwriter.bcf_bytes(bcf_cases.std_header(), bcf_cases.fuzz_records(7, n, len(bcf_cases.SAMPLES)), payload=payload)


@functools.lru_cache(maxsize=None)
def sorted_bcf(n, payload):
    hdr = bcfwriter.header([], contigs=[("##contig=<ID=1,length=%d>" % (100 * MB),), ("##contig=<ID=2,length=%d>" % MB,)])
    recs = [bcfwriter.record(rid=0, pos=1000 + 37 * k, rlen=1 + k % 3, alleles=(b"ACG"[:1 + k % 3], b"C"), id=b"id%07d" % k) for k in range(n - n // 8)]
    recs += [bcfwriter.record(rid=1, pos=5 + 11 * k, rlen=1, alleles=(b"A", b"T"), id=b"x%d" % k) for k in range(n // 8)]
    return bcfwriter.bcf_bytes(hdr, recs, payload=payload)


@functools.lru_cache(maxsize=None)
def vcf_text(payload=777, n=1500):
    lines = ["##fileformat=VCFv4.2", "##contig=<ID=chrA,length=%d>" % (300 * MB), "##contig=<ID=chrB,length=5000>",
             '##INFO=<ID=END,Number=1,Type=Integer,Description="e">', '##INFO=<ID=DP,Number=1,Type=Integer,Description="d">', "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    for k in range(n):
        lines.append("chrA\t%d\trs%d\tACG\tA\t%d\tPASS\tDP=%d" % (20000 + 11 * k, k, k % 90, k % 13))
    lines.append("chrA\t%d\t.\tA\t<DEL>\t.\t.\tEND=%d" % (70000, 70000 + 3 * MB))
    for k in range(50):
        lines.append("chrB\t%d\t.\tA\tT\t.\t.\t." % (1 + 3 * k))
    return bw.bgzf_file(("\n".join(lines) + "\n").encode(), payload=payload)


@functools.lru_cache(maxsize=None)
def gff_text():
    L = [b"##gff-version 3"]
    for s, name in enumerate((b"seqA", b"seqB", b"seqC")):
        for i in range(600):
            beg = i * 50 + 1 + s
            L.append(b"%s\tsrc\texon\t%d\t%d\t%d.5\t+\t.\tID=e%d_%d;Note=n%d" % (name, beg, beg + 29 + (i % 5) * 20, i % 50, s, i, i))
    return bw.bgzf_file(b"\n".join(L) + b"\n", payload=777)


@functools.lru_cache(maxsize=None)
def bed_text():
    L = ["#track"] + ["chrA\t%d\t%d\tx%d\t%d\t+" % (100 * k, 100 * k + 250, k, k % 900) for k in range(1200)] + ["chrB\t%d\t%d\ty\t0\t-" % (40 * k, 40 * k + 5) for k in range(200)]
    return bw.bgzf_file(("\n".join(L) + "\n").encode(), payload=777)


@functools.lru_cache(maxsize=None)
def fastq_text():
    rng = random.Random(5)
    out = []
    for i in range(400):
        n = rng.choice([1, 36, 100, 151])
        out.append("@r%d extra\n%s\n+\n%s\n" % (i, "".join(rng.choice("ACGTN") for _ in range(n)), "".join(chr(33 + rng.randrange(40)) for _ in range(n))))
    return bw.bgzf_file("".join(out).encode(), payload=777)


@functools.lru_cache(maxsize=None)
def fasta_text():
    rng = random.Random(6)
    out = []
    for name, n in (("one", 7000), ("two", 61), ("three", 12345), ("four", 3000)):
        s = "".join(rng.choice("ACGTNacgt") for _ in range(n))
        out.append(">%s some words\n" % name + "".join(s[i:i + 60] + "\n" for i in range(0, n, 60)))
    return bw.bgzf_file("".join(out).encode(), payload=777)


@functools.lru_cache(maxsize=None)
def lib():
    L = duckhts_amd.lib()
    L.dhts_bcf_build_index.restype = C.c_int64
    L.dhts_bcf_build_index.argtypes = [C.c_void_p, C.c_int]
    L.dhts_tabix_build_index.restype = C.c_int64
    L.dhts_tabix_build_index.argtypes = [C.c_void_p] + [C.c_int] * 7
    L.dhts_bgzf_wrap.restype = C.c_int64
    L.dhts_bgzf_wrap.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    L.dhts_set_super_blocks.restype = None
    L.dhts_set_super_blocks.argtypes = [C.c_void_p, C.c_int64]
    return L


CONF_GFF = (0, 1, 4, 5, ord("#"), 0)
CONF_BED = (0x10000, 1, 2, 3, ord("#"), 0)


def wrap(raw):
    """the bytes as a BGZF file (what a .csi / .tbi on disk is)"""
    a = np.frombuffer(raw, np.uint8)
    need = lib().dhts_bgzf_wrap(a.ctypes.data, len(raw), None, 0)
    out = np.zeros(need, np.uint8)
    assert lib().dhts_bgzf_wrap(a.ctypes.data, len(raw), out.ctypes.data, need) == need
    return out.tobytes()


def build_index(data, kind, min_shift=0, super_blocks=0, repair_stats=None):
    """index bytes built on the device: kind "bam" (BAI, or CSI with min_shift), "bcf" (BCF or bgzipped VCF text: CSI, or TBI with
    min_shift 0 on text), a tabix conf tuple (TBI / CSI of bgzipped text lines)"""
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(data); ctx.bgzf_index()
        if super_blocks:
            lib().dhts_set_super_blocks(ctx.h, super_blocks)
        if kind == "bam":
            ctx.bam_open()
            out = ctx.build_index(min_shift)
        else:
            if kind == "bcf":
                duckhts_amd.BcfScan(ctx)
                n = lib().dhts_bcf_build_index(ctx.h, min_shift)
            else:
                n = lib().dhts_tabix_build_index(ctx.h, *kind, min_shift)
            assert n > 0, lib().dhts_error(ctx.h)
            raw = np.zeros(n, np.uint8)
            assert lib().dhts_bam_index_bytes(ctx.h, raw.ctypes.data, n) == 0
            out = raw.tobytes()
        if repair_stats is not None:
            repair_stats.update(ctx.bgzf_repair_stats())
        return out
    finally:
        ctx.close()


def scan_bam(data, block_range=None, max_blocks=0, super_blocks=0):
    """one context's scan through the C ABI: the rows, the hand-off offsets in both forms and the repair counters"""
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(data); ctx.bgzf_index()
        if super_blocks:
            lib().dhts_set_super_blocks(ctx.h, super_blocks)
        hdr = ctx.bam_open()
        if block_range is not None:
            ctx.set_block_range(*block_range)
        parts, first, end, status = [], None, None, 0
        while status == 0:
            b = ctx.next_batch(max_blocks)
            if b.n_rows:
                parts.append(ctx.batch_to_host(b, hdr))
                first = int(b.first_rec_uoff) if first is None else first
            end, status = int(b.end_uoff), int(b.status)
        out = {k: [x for p in parts for x in list(p[k])] for k in COLS}
        out.update(n_rows=sum(p["n_rows"] for p in parts), status=status, first=first, end=end, header=hdr,
                   tell_first=None if first is None else ctx.tell(first), tell_end=ctx.tell(end), repair=ctx.bgzf_repair_stats())
        return out
    finally:
        ctx.close()


def rows_of(res):
    return {k: list(res[k]) for k in COLS}


# ---- read_bam: every plan, every batch size ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", il.PLANS)
@pytest.mark.parametrize("name", ["p61", "p777", "p65280"])
def test_read_bam_reads_a_lying_file_like_the_clean_one(name, plan):
    data = bam(name)
    clean, lying = il.clean_for(data, plan), il.lie(data, plan)
    lies = n_lies(clean, lying)
    assert lies == len(il.plan_blocks(data, plan)) >= 1
    for mb in (0, 1, 2, 3, 7):
        exp = clean_result(("read_bam", name, plan == "empty_mid", mb), lambda: duckhts_amd.read_bam(clean, max_blocks=mb))
        assert exp["n_rows"] == (3000 if name == "p65280" else 200) and exp["status"] == 1
        st = {}
        got = duckhts_amd.read_bam(lying, max_blocks=mb, repair_stats=st)
        same(got, exp, f"{name}/{plan}/mb{mb}")          # every column, status, the header with first_rec_uoff, the hand-off offsets
        assert st["replaced"] == lies and st["scratch_retries"] == 0, (name, plan, mb, st)


@pytest.mark.parametrize("name", ["p61", "p777"])
def test_read_bam_with_the_next_batch_prefetch_on_a_lying_file(monkeypatch, name):
    monkeypatch.setenv("DHTS_PREFETCH", "1")
    data = bam(name)
    lying = il.lie(data, "all")
    for mb in (2, 7):
        exp = clean_result(("read_bam_prefetch", name, mb), lambda: duckhts_amd.read_bam(data, max_blocks=mb))
        same(duckhts_amd.read_bam(lying, max_blocks=mb), exp, f"prefetch/{name}/mb{mb}")


# ---- block-range shards ---------------------------------------------------------------------------------------------------------------
def _shard_lies(data, cuts, where):
    """block -> claimed value for lies in a predecessor's range, on the cut blocks and in the halo blocks behind a cut"""
    bl = il.blocks(data)
    idx = []
    for c in cuts:
        if "pred" in where:
            idx += [c - 4, c - 3, c - 2]
        if "cut" in where:
            idx += [c]
        if "halo" in where:
            idx += [c + 1, c + 2]
    return il.lie(data, sorted(idx)), sorted(idx)


@pytest.mark.parametrize("where", ["pred", "cut", "halo", "pred+cut+halo"])
@pytest.mark.parametrize("world", [2, 3])
def test_block_range_shards_of_a_lying_file(world, where):
    """the concatenated rows of the shards equal the clean scan; the hand-off is compared as virtual offsets (Context.tell: the block that
    holds the byte, decoded by both neighbours), which do not depend on ISIZE fields -- absolute inflated offsets of two contexts do"""
    data = bam("p777")
    nb = len(il.blocks(data))
    cuts = [nb * r // world for r in range(1, world)]
    lying, idx = _shard_lies(data, cuts, where)
    assert il.lying_blocks(data, lying) == idx and min(idx) > il.first_record_block(data)
    exp = clean_result(("read_bam", "p777", False, 0), lambda: duckhts_amd.read_bam(data, max_blocks=0))
    bounds = [0] + cuts + [nb]
    for mb in (0, 3):
        parts = [scan_bam(lying, (bounds[r], bounds[r + 1], r > 0), mb) for r in range(world)]
        ref = [clean_result(("shard", world, r, mb), lambda: scan_bam(data, (bounds[r], bounds[r + 1], r > 0), mb)) for r in range(world)]
        for r in range(world):
            assert parts[r]["status"] == 1 and parts[r]["n_rows"] == ref[r]["n_rows"] > 0, (world, where, mb, r)
            same(rows_of(parts[r]), rows_of(ref[r]), f"world {world} {where} mb{mb} rank {r}")
            assert (parts[r]["tell_first"], parts[r]["tell_end"]) == (ref[r]["tell_first"], ref[r]["tell_end"]), (world, where, mb, r)
        for k in COLS:
            assert [x for p in parts for x in p[k]] == list(exp[k]), (world, where, mb, k)
        for r in range(world - 1):
            assert parts[r]["tell_end"] == parts[r + 1]["tell_first"], (world, where, mb, r)
            print(f"hand-off world={world} lies={where} mb={mb} rank {r}->{r + 1}: virtual offsets chain; absolute offsets "
                  f"{parts[r]['end']} vs {parts[r + 1]['first']}: {'chain' if parts[r]['end'] == parts[r + 1]['first'] else 'DO NOT chain'}")


# ---- region queries through index windows -------------------------------------------------------------------------------------------------
REGION = "chr2:1-120000000,chr9:20000000-90000000,chrX:1-60000000"


@functools.lru_cache(maxsize=None)
def _window_blocks():
    """for each of REGION's three intervals the (first, last) block that holds a kept record, by the region oracle on the clean file"""
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import region_oracle
    data = genome_bam()
    exp = orc.bam_read(data)
    keep = region_oracle.keep_mask(exp, REGION)
    bl = il.blocks(data)
    uoff = np.cumsum([0] + [il.isize(data, b) for b in bl])
    starts = np.asarray(exp["rec_off"]).astype(np.int64)      # the records' offsets in the inflated stream
    assert len(starts) == exp["n_rows"] == len(keep)
    blk = np.searchsorted(uoff, starts, side="right") - 1
    tid = np.asarray(exp["tid"])
    wins = []
    for t in sorted(set(int(x) for x in tid[keep])):
        b = blk[keep & (tid == t)]
        wins.append((int(b.min()), int(b.max())))
    assert len(wins) == 3 and all(wins[i][1] + 20 < wins[i + 1][0] for i in range(2)) and all(b - a >= 4 for a, b in wins)
    return wins


def _region_lie(where):
    data, w = genome_bam(), _window_blocks()
    idx = {"front": [il.first_record_block(data), w[0][0] - 3, w[1][0] - 2, w[2][0] - 1],
           "first_block": [a for a, _ in w],
           "inside": [(a + b) // 2 for a, b in w],
           "between": [(w[0][1] + w[1][0]) // 2, (w[1][1] + w[2][0]) // 2, w[2][1] + 5],
           "everywhere": None}[where]
    return il.lie(data, "all") if idx is None else il.lie(data, sorted(idx))


@pytest.mark.parametrize("where", ["front", "first_block", "inside", "between", "everywhere"])
def test_region_query_on_a_lying_file(monkeypatch, where):
    monkeypatch.setenv("DHTS_WINDOW_GAP_MB", "0.05")             # (the default, 32 MB, would merge every window of a file this small)
    data = genome_bam()
    lying = _region_lie(where)
    bai = clean_result("genome_bai", lambda: build_index(data, "bam"))
    bai_lying = build_index(lying, "bam")
    assert bai_lying == bai
    for region in (REGION, "chr9:20000000-90000000"):        # disjoint windows, and a single one
        for mb in (0, 5):
            exp = clean_result(("region", region, mb), lambda: duckhts_amd.read_bam(data, region=region, index=bai, max_blocks=mb))
            assert exp["status"] == 1 and 100 < exp["n_rows"] < 20000
            for index in (bai, bai_lying):
                got = duckhts_amd.read_bam(lying, region=region, index=index, max_blocks=mb)
                same(rows_of(got), rows_of(exp), f"region {where} mb{mb}")
                assert got["status"] == 1 and got["n_rows"] == exp["n_rows"]
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(lying); ctx.bgzf_index(); ctx.bam_open()
        assert ctx.set_regions(REGION)
        ctx.load_index(bai)
        assert ctx.scan_window_stats()[0] == 3
    finally:
        ctx.close()


# ---- index writers: byte-identical to the clean file's index ------------------------------------------------------------------------------
INDEX_PLANS = [("all", il.ALL_VALUES), ("eof_block", il.ALL_VALUES), ("last_data_block", "zero"), ("empty_mid", None)]
INDEX_INPUTS = {
    "bam61_bai": (lambda: sorted_bam(200, 61), "bam", 0), "bam777_bai": (lambda: sorted_bam(200, 777), "bam", 0), "bam777_csi": (lambda: synth.bam_file(3000, seed=3, payload=777), "bam", 14),
    "bam65280_bai": (lambda: sorted_bam(3000, 65280), "bam", 0),
    "bcf_csi": (lambda: sorted_bcf(3000, 777), "bcf", 14), "vcf_tbi": (vcf_text, "bcf", 0), "vcf_csi": (vcf_text, "bcf", 14),
    "gff_tbi": (gff_text, CONF_GFF, 0), "bed_csi": (bed_text, CONF_BED, 14),
}


@pytest.mark.parametrize("plan, values", INDEX_PLANS)
@pytest.mark.parametrize("which", list(INDEX_INPUTS))
def test_index_of_a_lying_file_is_byte_identical(which, plan, values):
    make, kind, min_shift = INDEX_INPUTS[which]
    data = make()
    clean = il.clean_for(data, plan)
    lying = il.lie(data, plan, values) if values else il.lie(data, plan)
    assert n_lies(clean, lying) >= 1
    exp = clean_result(("index", which, plan == "empty_mid"), lambda: build_index(clean, kind, min_shift))
    assert len(exp) > 100
    assert build_index(lying, kind, min_shift) == exp, (which, plan)


# ---- read_bcf on BCF and on bgzipped VCF text -------------------------------------------------------------------------------------------------
BCF_INPUTS = {"bcf61": lambda: bcf(61, 300), "bcf777": lambda: bcf(777, 1000), "vcf777": vcf_text}


def bcf_same(got, exp, what):
    d = orc.bcf_cols_diff(exp, got)
    assert d is None, (what, d)
    for k in ("n_rows", "status", "first_rec_uoff", "end_uoff", "header_first_rec_uoff", "samples"):
        assert got[k] == exp[k], (what, k, got[k], exp[k])


@pytest.mark.parametrize("plan", il.PLANS)
@pytest.mark.parametrize("which", list(BCF_INPUTS))
def test_read_bcf_reads_a_lying_file_like_the_clean_one(which, plan):
    data = BCF_INPUTS[which]()
    clean, lying = il.clean_for(data, plan), il.lie(data, plan)
    lies = n_lies(clean, lying)
    for mb in (0, 1, 3):
        exp = clean_result(("read_bcf", which, plan == "empty_mid", mb), lambda: duckhts_amd.read_bcf(clean, max_blocks=mb))
        assert exp["n_rows"] >= 300 and exp["status"] == 1
        st = {}
        bcf_same(duckhts_amd.read_bcf(lying, max_blocks=mb, repair_stats=st), exp, (which, plan, mb))
        assert st["replaced"] == lies and st["scratch_retries"] == 0, (which, plan, mb, st)


@pytest.mark.parametrize("which", ["bcf777", "vcf777"])
def test_read_bcf_block_range_split_of_a_lying_file(which):
    data = BCF_INPUTS[which]()
    nb = len(il.blocks(data))
    cut = nb // 2
    whole = clean_result(("read_bcf", which, False, 0), lambda: duckhts_amd.read_bcf(data, max_blocks=0))
    for idx in ([cut - 3, cut - 2], [cut], [cut + 1, cut + 2], [cut - 3, cut - 2, cut, cut + 1, cut + 2]):
        lying = il.lie(data, idx)
        n = 0
        for r, rng in enumerate(((0, cut, False), (cut, nb, True))):
            exp = clean_result(("read_bcf_range", which, r), lambda: duckhts_amd.read_bcf(data, block_range=rng))
            got = duckhts_amd.read_bcf(lying, block_range=rng)
            d = orc.bcf_cols_diff(exp, got)
            assert d is None and got["n_rows"] == exp["n_rows"] > 0 and got["status"] == exp["status"], (which, idx, r, d)
            n += got["n_rows"]
        assert n == whole["n_rows"]


@pytest.mark.parametrize("which, min_shift, region", [("bcf", 14, "1:20000-60000,2:100-3000"), ("vcf", 0, "chrA:25000-30000,chrB")])
def test_read_bcf_region_of_a_lying_file_through_a_clean_index(monkeypatch, which, min_shift, region):
    monkeypatch.setenv("DHTS_WINDOW_GAP_MB", "0.05")
    data = sorted_bcf(3000, 777) if which == "bcf" else vcf_text()
    index = wrap(build_index(data, "bcf", min_shift))
    exp = duckhts_amd.read_bcf(data, region=region, index=index)
    assert 50 < exp["n_rows"] < 2500 and exp["status"] == 1
    for plan in ("all", "block0", "first_record_block", "run8", "eof_block"):
        got = duckhts_amd.read_bcf(il.lie(data, plan), region=region, index=index, max_blocks=3)
        d = orc.bcf_cols_diff(exp, got)
        assert d is None and got["n_rows"] == exp["n_rows"] and got["status"] == 1, (which, plan, d)


# ---- read_tabix, read_bed, read_gff on bgzipped text ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("isize_lies")
    out = {"dir": str(d)}
    for name, data, conf in (("gff", gff_text(), CONF_GFF), ("bed", bed_text(), CONF_BED)):
        tbi = wrap(build_index(data, conf, 0))
        for plan in ("clean", "all", "block0", "eof_block"):
            p = str(d / f"{name}_{plan}.gz")
            open(p, "wb").write(data if plan == "clean" else il.lie(data, plan))
            open(p + ".tbi", "wb").write(tbi)
            out[name, plan] = p
    return out


TEXT_READERS = {
    "read_gff": ("gff", lambda src, **kw: duckhts_amd.read_gff(src, attributes_map=True, **kw), "seqB:5002-9000"),
    "read_tabix": ("gff", lambda src, **kw: duckhts_amd.read_tabix(src, **kw), "seqA:1-700"),
    "read_bed": ("bed", lambda src, **kw: duckhts_amd.read_bed(src, **kw), "chrA:50000-60000"),
}


@pytest.mark.parametrize("plan", ["all", "block0", "eof_block"])
@pytest.mark.parametrize("reader", list(TEXT_READERS))
def test_text_readers_read_a_lying_file_like_the_clean_one(text_files, reader, plan):
    name, fn, region = TEXT_READERS[reader]
    data = gff_text() if name == "gff" else bed_text()
    for mb in (0, 2):
        exp = clean_result((reader, "bytes", mb), lambda: fn(data, max_blocks=mb))
        assert exp["n_rows"] >= 1400 and exp["status"] == 1
        same(fn(il.lie(data, plan), max_blocks=mb), exp, f"{reader}/{plan}/mb{mb}")
    exp = clean_result((reader, "region"), lambda: fn(text_files[name, "clean"], region=region))
    assert 5 < exp["n_rows"] < 1000 and exp["status"] == 1
    same(fn(text_files[name, plan], region=region), exp, f"{reader}/{plan}/region")


# ---- FASTQ through read_bam; FASTA through fasta_index, the fetch and fasta_nuc -----------------------------------------------------------------
@pytest.mark.parametrize("plan", ["all", "eof_block", "empty_mid"])
def test_fastq_and_fasta_on_a_lying_file(tmp_path, plan):
    fq = fastq_text()
    for mb in (0, 3):
        exp = clean_result(("fastq", plan == "empty_mid", mb), lambda: duckhts_amd.read_bam(il.clean_for(fq, plan), max_blocks=mb))
        assert exp["n_rows"] == 400
        same(duckhts_amd.read_bam(il.lie(fq, plan), max_blocks=mb), exp, f"fastq/{plan}/mb{mb}")
    fa = fasta_text()
    clean, lying = il.clean_for(fa, plan), il.lie(fa, plan)
    fai, gzi = clean_result(("fasta_index", plan == "empty_mid"), lambda: duckhts_amd.fasta_index(clean))
    assert len(fai.splitlines()) == 4 and len(gzi) >= 8 + 16 * 20
    assert duckhts_amd.fasta_index(lying) == (fai, gzi)
    regions = "one:7-23,three:6000-12345,four"

    def fetch(src):
        ctx = duckhts_amd.Context(0)
        try:
            ctx.open(src); ctx.fasta_load_index(fai)
            return ctx.fasta_fetch(regions)
        finally:
            ctx.close()
    want = fetch(clean)
    assert [len(s) for _, s in want] == [17, 6346, 3000]
    assert fetch(lying) == want
    paths = {}
    for nm, d in (("clean", clean), ("lying", lying)):
        paths[nm] = str(tmp_path / f"{nm}.fa.gz")
        open(paths[nm], "wb").write(d)
        open(paths[nm] + ".fai", "wb").write(fai)
        open(paths[nm] + ".gzi", "wb").write(gzi)
    assert duckhts_amd.fasta_fetch(paths["lying"], fai, regions) == duckhts_amd.fasta_fetch(paths["clean"], fai, regions) == want
    for kw in ({"bin_width": 1000}, {"bin_width": 977, "region": "three:100-9000"}):
        same(duckhts_amd.fasta_nuc(lying, fai=fai, **kw), duckhts_amd.fasta_nuc(clean, fai=fai, **kw), f"fasta_nuc/{plan}/{kw}")
        same(duckhts_amd.fasta_nuc(paths["lying"], **kw), duckhts_amd.fasta_nuc(paths["clean"], **kw), f"fasta_nuc by path/{plan}/{kw}")


# ---- the coverage functions ---------------------------------------------------------------------------------------------------------------------
COVERAGE_BED = b"chr1\t0\t50000\ta\nchr1\t60000\t61000\tb\nchr2\t100\t20000\tc\nchrM\t0\t16569\td\n"
COVERAGE_FUNCTIONS = {
    "bam_bin_counts": lambda src: duckhts_amd.bam_bin_counts(src, bin_width=1000, max_blocks=2),
    "bam_bedcov": lambda src: duckhts_amd.bam_bedcov(src, COVERAGE_BED, max_blocks=2),
    "bam_coverage": lambda src: duckhts_amd.bam_coverage(src, max_blocks=2),
    "bam_depth": lambda src: duckhts_amd.bam_depth(src, max_blocks=2),
}


@pytest.mark.parametrize("fn", list(COVERAGE_FUNCTIONS))
@pytest.mark.parametrize("name", ["p61", "p777"])
def test_coverage_functions_on_a_lying_file(name, fn):
    data = sorted_bam(200, 61 if name == "p61" else 777)
    exp = COVERAGE_FUNCTIONS[fn](data)
    assert exp["n_rows"] > 0
    same(COVERAGE_FUNCTIONS[fn](il.lie(data, "all")), exp, f"{fn}/{name}")           # the rows, the stats and the status


# ---- bgzipped side inputs: the overlap join's BED, a .csi and a .tbi whose own BGZF wrapper lies -------------------------------------------------
def test_bgzipped_side_inputs_that_lie(tmp_path, monkeypatch):
    monkeypatch.setenv("DHTS_WINDOW_GAP_MB", "0.05")
    bed = bw.bgzf_file(b"".join(b"chr%d\t%d\t%d\n" % (1 + k % 2, 137 * k, 137 * k + 400) for k in range(300)), payload=777)
    data = bam("p777")
    paths = {}
    for nm, d in (("clean", bed), ("all", il.lie(bed, "all")), ("block0", il.lie(bed, "block0")), ("eof", il.lie(bed, "eof_block"))):
        paths[nm] = str(tmp_path / f"{nm}.bed.gz")
        open(paths[nm], "wb").write(d)
    exp = duckhts_amd.read_bam(data, overlap_bed=paths["clean"])
    assert exp["n_bed_rows"] == 300 and sum(len(x) for x in exp["OVERLAPS"]) > 100
    for nm in ("all", "block0", "eof"):
        same(duckhts_amd.read_bam(data, overlap_bed=paths[nm]), exp, f"overlap_bed/{nm}")
    # an index whose BGZF wrapper lies: a .csi for a BAM region query, a .tbi for a region of bgzipped VCF text
    gen = genome_bam()
    csi = wrap(build_index(gen, "bam", 14))
    exp = duckhts_amd.read_bam(gen, region=REGION, index=csi)
    assert exp["n_rows"] > 100
    txt = vcf_text()
    tbi = wrap(build_index(txt, "bcf", 0))
    expt = duckhts_amd.read_bcf(txt, region="chrA:25000-30000,chrB", index=tbi)
    assert expt["n_rows"] > 50
    for plan in ("all", "block0", "eof_block"):
        same(rows_of(duckhts_amd.read_bam(gen, region=REGION, index=il.lie(csi, plan))), rows_of(exp), f"lying csi/{plan}")
        got = duckhts_amd.read_bcf(txt, region="chrA:25000-30000,chrB", index=il.lie(tbi, plan))
        assert orc.bcf_cols_diff(expt, got) is None and got["n_rows"] == expt["n_rows"], plan


# ---- Context.bgzf_inflate and bgunzip_file ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", il.PLANS)
@pytest.mark.parametrize("name", ["p777", "p65280"])
def test_bgzf_inflate_of_a_lying_file(name, plan):
    data = bam(name)
    clean, lying = il.clean_for(data, plan), il.lie(data, plan)
    want = il.inflate_all(clean)
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(lying)
        nb = ctx.bgzf_index()
        assert nb == len(il.blocks(lying))
        out, bst = ctx.bgzf_inflate(0, nb, len(want) + 65536)
        assert np.all(bst == 0) and out.tobytes() == want
        assert ctx.bgzf_repair_stats()["replaced"] == n_lies(clean, lying)
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def chunked_bam():
    """more than 4096 blocks: bgunzip inflates the file in chunks of 4096 blocks"""
    data = cases.case_basic(payload=61, n=1100, seed=2)
    assert 4096 + 50 < len(il.blocks(data)) < 8192
    return data


@pytest.mark.parametrize("case", ["p777/all", "p777/eof_block", "p777/empty_mid", "chunk/last_of_chunk_0", "chunk/first_of_chunk_1", "chunk/both", "chunk/all"])
def test_bgunzip_file_of_a_lying_file(tmp_path, case):
    which, plan = case.split("/")
    data = bam("p777") if which == "p777" else chunked_bam()
    idx = {"last_of_chunk_0": [4095], "first_of_chunk_1": [4096], "both": [4095, 4096]}.get(plan)
    clean = il.clean_for(data, plan) if idx is None else data
    lying = il.lie(data, plan) if idx is None else il.lie(data, idx)
    want = il.inflate_all(clean)
    src, dst = str(tmp_path / "in.gz"), str(tmp_path / "out")
    open(src, "wb").write(lying)
    ctx = duckhts_amd.Context(0)
    try:
        assert ctx.bgunzip_file(src, dst) == (len(lying), len(want))
        assert ctx.bgzf_repair_stats()["replaced"] == n_lies(clean, lying)
    finally:
        ctx.close()
    assert open(dst, "rb").read() == want


# ---- a second phase-A launch in mid-scan ------------------------------------------------------------------------------------------------------
SUPER = 16384


@functools.lru_cache(maxsize=None)
def long_bam():
    data = sorted_bam(5000, 61)
    assert len(il.blocks(data)) > il.first_record_block(data) + SUPER + 1000
    return data


@functools.lru_cache(maxsize=None)
def long_bcf():
    data = sorted_bcf(26000, 61)
    assert len(il.blocks(data)) > il.first_record_block(data) + SUPER + 1000
    return data


def _tail_lie(data, plan, both):
    """lies beyond the first phase-A launch (first record block + SUPER blocks); `both`: in the first launch as well"""
    t0 = il.first_record_block(data) + SUPER + 1
    nb = len(il.blocks(data))
    if plan == "all":
        idx = list(range(t0, nb))
    elif plan == "run8":
        idx = list(range(t0 + 300, t0 + 308))
    else:
        idx = [t0 + 500, t0 + 501]
    bl = il.blocks(data)
    if plan == "net_zero":
        assert all(il.isize(data, bl[i]) >= 30 for i in idx)
        lying = il.set_isize(data, [(idx[0], il.isize(data, bl[idx[0]]) - 30), (idx[1], il.isize(data, bl[idx[1]]) + 30)])
    else:
        lying = il.lie(data, idx)
    if both:
        lying = il.lie(lying, [3, 4, 5, 2000, 2001, t0 - 2000])
    return lying, len(idx)


@pytest.mark.parametrize("both", [False, True], ids=["tail", "both_launches"])
@pytest.mark.parametrize("plan", ["run8", "net_zero", "all"])
def test_bam_scan_and_index_across_a_second_phase_a_launch(plan, both):
    data = long_bam()
    lying, tail_lies = _tail_lie(data, plan, both)
    exp = clean_result("long_bam_scan", lambda: scan_bam(data, max_blocks=5000, super_blocks=SUPER))
    assert exp["status"] == 1 and exp["n_rows"] > 4500
    got = scan_bam(lying, max_blocks=5000, super_blocks=SUPER)
    same(rows_of(got), rows_of(exp), f"long bam {plan} {both}")
    assert (got["n_rows"], got["status"], got["first"], got["end"]) == (exp["n_rows"], 1, exp["first"], exp["end"])
    assert got["repair"]["replaced"] >= tail_lies and got["repair"]["replaced"] == n_lies(data, lying)
    bai = clean_result("long_bam_bai", lambda: build_index(data, "bam", super_blocks=SUPER))
    st = {}
    assert build_index(lying, "bam", super_blocks=SUPER, repair_stats=st) == bai
    assert st["replaced"] >= tail_lies


@pytest.mark.parametrize("both", [False, True], ids=["tail", "both_launches"])
@pytest.mark.parametrize("plan", ["run8", "net_zero", "all"])
def test_bcf_index_across_a_second_phase_a_launch(plan, both):
    data = long_bcf()
    lying, tail_lies = _tail_lie(data, plan, both)
    csi = clean_result("long_bcf_csi", lambda: build_index(data, "bcf", 14, super_blocks=SUPER))
    st = {}
    assert build_index(lying, "bcf", 14, super_blocks=SUPER, repair_stats=st) == csi
    assert st["replaced"] >= tail_lies


# ---- a table that grows while the scan runs -------------------------------------------------------------------------------------------------------
def test_block_table_of_a_lying_file_extended_piece_by_piece():
    L = duckhts_amd.lib()
    L.dhts_debug_index_prefix.argtypes = [C.c_void_p, C.c_uint64]
    L.dhts_debug_index_prefix.restype = C.c_int64
    L.dhts_blocks_ahead.argtypes = [C.c_void_p]
    L.dhts_blocks_ahead.restype = C.c_int64
    data = synth.bam_file(20000, seed=11, payload=777)
    lying = il.lie(data, "all")
    step = 100000
    exp = duckhts_amd.read_bam(data)
    one = duckhts_amd.Context(0)
    try:
        one.open(lying); nb_ref = one.bgzf_index(); hdr = one.bam_open()
        while one.next_batch(0).status == 0:
            pass
        table_ref = one.bgzf_table(nb_ref)
    finally:
        one.close()
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(lying)
        hdr = None; names = []; pos = []; extensions = 0; finished = False; upto = step; last_nb = 0
        while not finished:
            nb = L.dhts_debug_index_prefix(ctx.h, upto); extensions += 1
            assert nb >= last_nb
            last_nb = nb
            whole = upto >= len(lying)
            if nb > 0 and hdr is None:
                hdr = ctx.bam_open()
            while hdr is not None:
                if not whole and L.dhts_blocks_ahead(ctx.h) < 8:
                    break                                   # leave the last blocks: a record may run into bytes that "are not there yet"
                b = ctx.next_batch(5)
                if b.n_rows:
                    h = ctx.batch_to_host(b, hdr)
                    names += h["QNAME"]; pos += list(h["POS"])
                if b.status != 0:
                    assert b.status == 1
                    finished = True
                    break
            upto += step
        assert extensions >= 4
        assert names == list(exp["QNAME"]) and pos == list(exp["POS"]), (len(names), exp["n_rows"])
        table = ctx.bgzf_table(nb_ref)
        assert table[3] == table_ref[3] == 0
        for a_, b_ in zip(table[:3], table_ref[:3]):
            assert (a_ == b_).all()
        assert [int(x) for x in table[2]] == [il.isize(data, b) for b in il.blocks(data)]          # the corrected table says what the blocks inflate to
    finally:
        ctx.close()


# ---- lies together with the packed-scratch retry ---------------------------------------------------------------------------------------------------
# A pool of 64 bytes per block is far below what any 64 KiB block needs, so every data block is marked DHTS_BLK_ERR_SCRATCH and the range is
# decoded again with full-size room.  The first isize_repair passes over those blocks; the repeat re-places them, and the batch has to be
# sized and placed again from the table as it then stands (the three retry sites: batch_status_resolve, batch_begin, dhts_bgzf_inflate_to_host).
# Understating lies are capped at 46 bytes per file (isize_lies.small_understatement): under half of the pad every stream buffer carries.
def _big(data):
    bl = il.blocks(data)
    return [i for i, b in enumerate(bl) if il.isize(data, b) >= 60000]


def _retry_lie(data, kind):
    big = _big(data)
    assert len(big) >= 6
    if kind == "net_zero":
        bl = il.blocks(data)
        a, b = big[2], big[2] + 1
        assert b in big
        return il.set_isize(data, [(a, il.isize(data, bl[a]) - 30), (b, il.isize(data, bl[b]) + 30)])
    if kind == "small_understatement":
        return il.small_understatement(data, [big[0], big[2], big[-1]])
    if kind == "overstating_mix":
        return il.lie(data, big, il.OVERSTATING)
    return il.lie(data, [big[0], big[1], big[3], big[-1]], kind)


RETRY_KINDS = list(il.OVERSTATING) + ["overstating_mix", "net_zero", "small_understatement"]


def _retry_counters(st, data, lying, what):
    lying_big = len(set(il.lying_blocks(data, lying)) & set(_big(data)))
    assert lying_big >= 2
    assert st["scratch_retries"] >= 1 and st["replaced_in_retry"] >= lying_big, (what, st, lying_big)


@pytest.mark.parametrize("kind", RETRY_KINDS)
def test_scratch_retry_on_a_lying_file_read_bam(monkeypatch, kind):
    """the deferred status: batch_status_resolve"""
    data = bam("p65280")
    lying = _retry_lie(data, kind)
    exp = clean_result(("read_bam", "p65280", False, 0), lambda: duckhts_amd.read_bam(data, max_blocks=0))
    exp7 = clean_result(("read_bam", "p65280", False, 7), lambda: duckhts_amd.read_bam(data, max_blocks=7))
    monkeypatch.setenv("DHTS_POOL_PER_BLOCK", "64")
    for mb, e in ((0, exp), (7, exp7)):
        st = {}
        same(duckhts_amd.read_bam(lying, max_blocks=mb, repair_stats=st), e, f"retry read_bam {kind} mb{mb}")
        _retry_counters(st, data, lying, (kind, mb))


@pytest.mark.parametrize("kind", RETRY_KINDS)
def test_scratch_retry_on_a_lying_file_read_bcf(monkeypatch, kind):
    """batch_begin's own loop"""
    data = bcf(65280, 3000)
    lying = _retry_lie(data, kind)
    exp = clean_result(("read_bcf", "bcf65280", False, 0), lambda: duckhts_amd.read_bcf(data, max_blocks=0))
    assert exp["n_rows"] == 3000
    monkeypatch.setenv("DHTS_POOL_PER_BLOCK", "64")
    for mb in (0, 5):
        st = {}
        bcf_same(duckhts_amd.read_bcf(lying, max_blocks=mb, repair_stats=st), exp, (kind, mb))
        _retry_counters(st, data, lying, (kind, mb))


@pytest.mark.parametrize("kind", RETRY_KINDS)
def test_scratch_retry_on_a_lying_file_inflate_to_host(monkeypatch, kind):
    """dhts_bgzf_inflate_to_host, directly and under bam_open (which sizes its buffer from the table before the call), with a lie on block 0"""
    data = bam("p65280")
    lying = il.lie(_retry_lie(data, kind), [0], "plus1" if kind in ("net_zero", "small_understatement", "overstating_mix") else kind)
    want = il.inflate_all(data)
    hdr_exp = clean_result(("read_bam", "p65280", False, 0), lambda: duckhts_amd.read_bam(data, max_blocks=0))["header"]
    monkeypatch.setenv("DHTS_POOL_PER_BLOCK", "64")
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(lying)
        nb = ctx.bgzf_index()
        out, bst = ctx.bgzf_inflate(0, nb, len(want) + 65536)
        assert np.all(bst == 0) and out.tobytes() == want
        _retry_counters(ctx.bgzf_repair_stats(), data, lying, kind)
    finally:
        ctx.close()
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(lying); ctx.bgzf_index()
        same(ctx.bam_open(), hdr_exp, f"bam_open {kind}")
        st = ctx.bgzf_repair_stats()
        assert st["scratch_retries"] >= 1 and st["replaced_in_retry"] >= len(set(il.lying_blocks(data, lying)) & {1, 2, 3}), (kind, st)
    finally:
        ctx.close()
