"""bam_bedgraph_export on the device (dhts_bedgraph_export, csrc/rows_text.hip) against the CPU model bam_bedgraph_export_ref: the row-text encoder
alone, byte for byte against Python's %d; the exported file read back by Python's gzip module; the identity with bgzip_file of the plain text under
every page and chunk size; the index against the tabix writer on the exported file and through read_bed; the empty result; every refusal and what
is left behind it."""
import ctypes as C
import gzip
import os
import struct

import numpy as np
import pytest

import bam_bedgraph_cases as G
import bam_bedgraph_export_ref as X
import bam_bedgraph_ref as M
import bam_depth_cases as D
import duckhts_amd
from conftest import read_golden
from test_gpu_bam_coverage import parse_rows

pytestmark = pytest.mark.gpu
R = G.R

# start / end at every digit boundary and the largest value asked for; the depths
EDGES = [v for k in range(19) for v in (10**k - 1, 10**k)] + [2**62]
DEPTHS = [0, 9, 10, 2**31 - 1]
NAME_LENS = [1, 15, 16, 17, 63, 64, 65, 255, 1000]
ROW_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1025]


def name_of(n, salt=0):
    return bytes(33 + (i * 7 + n + salt) % 90 for i in range(n))               # printable, no tab, no newline


def python_text(names, tid, start, end, depth):
    return b"".join(b"%s\t%d\t%d\t%d\n" % (names[t], s, e, d) for t, s, e, d in zip(tid, start, end, depth))


@pytest.fixture(scope="module")
def ctx():
    c = duckhts_amd.Context(0)
    yield c
    c.close()


def encode_and_check(ctx, names, tid, start, end, depth):
    got, paths = ctx.debug_rows_text(names, tid, start, end, depth)
    exp = python_text(names, tid, start, end, depth)
    if got != exp:
        at = next(i for i, (a, b) in enumerate(zip(got, exp)) if a != b) if len(got) == len(exp) else min(len(got), len(exp))
        raise AssertionError((len(got), len(exp), at, got[max(0, at - 30):at + 30], exp[max(0, at - 30):at + 30]))
    return paths


# ---- 1. the encoder alone ----
def test_every_digit_boundary(ctx):
    n = len(EDGES)
    paths = encode_and_check(ctx, [b"c"], [0] * n, EDGES, EDGES[::-1], [DEPTHS[i % 4] for i in range(n)])
    assert paths == {"staged": 1, "fallback": 0}
    # every edge in each of the two 64-bit columns beside every depth
    tid, start, end, depth = [], [], [], []
    for i, v in enumerate(EDGES):
        for d in DEPTHS:
            tid.append(0); start.append(v); end.append(EDGES[(i * 5 + 3) % n]); depth.append(d)
    encode_and_check(ctx, [b"chr1"], tid, start, end, depth)


def test_negative_values_and_an_id_outside_the_table(ctx):
    got, _ = ctx.debug_rows_text([b"a", b"bb"], [0, 1, 2, -1], [-1, -10, -(2**63), 0], [5, -99, 2**63 - 1, 7], [-1, -(2**31), 3, 0])
    assert got == b"a\t-1\t5\t-1\nbb\t-10\t-99\t-2147483648\n\t-9223372036854775808\t9223372036854775807\t3\n\t0\t7\t0\n"


@pytest.mark.parametrize("length", NAME_LENS)
def test_name_lengths(ctx, length):
    names = [name_of(length), b"s"]
    n = 300                                                                   # more than one workgroup
    tid = [0] * n
    paths = encode_and_check(ctx, names, tid, [EDGES[i % len(EDGES)] for i in range(n)], [i * 977 for i in range(n)], [DEPTHS[i % 4] for i in range(n)])
    assert paths["staged"] + paths["fallback"] == 2
    if length == 1000:
        assert paths == {"staged": 0, "fallback": 2}                          # 256 rows of 1,000 bytes and more are far over the LDS budget
    if length <= 17:
        assert paths == {"staged": 2, "fallback": 0}                          # at most 17 + 3 * 20 + 4 bytes a row


def test_both_paths_in_one_call(ctx):
    names = [name_of(n) for n in NAME_LENS]
    tid = [k for k in range(len(names)) for _ in range(256)]                  # a workgroup per name length
    n = len(tid)
    start, end, depth = [i * 31 for i in range(n)], [i * 31 + 17 for i in range(n)], [i % 11 for i in range(n)]
    paths = encode_and_check(ctx, names, tid, start, end, depth)
    spans = [len(python_text(names, tid[g:g + 256], start[g:g + 256], end[g:g + 256], depth[g:g + 256])) for g in range(0, n, 256)]
    exp_staged = sum(1 for b in spans if b <= duckhts_amd.ROWS_TEXT_LDS_BYTES)
    assert paths == {"staged": exp_staged, "fallback": len(NAME_LENS) - exp_staged} and 0 < exp_staged < len(NAME_LENS)
    # rows of long and short names mixed inside one workgroup, both ways round
    mixed = [8 if (i < 256 and i % 10 == 0) or i == 300 else 0 for i in range(700)]     # 26 rows of 1,000 bytes in the first workgroup, one in the second
    paths = encode_and_check(ctx, names, mixed, list(range(700)), list(range(1, 701)), [1] * 700)
    assert paths == {"staged": 2, "fallback": 1}


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts(ctx, n):
    names = [b"CHROMOSOME_I", b"x", name_of(40)]
    paths = encode_and_check(ctx, names, [i % 3 for i in range(n)], [i * 1009 for i in range(n)], [i * 1009 + i for i in range(n)], [i % 300 for i in range(n)])
    assert paths == {"staged": -(-n // 256), "fallback": 0}


def test_a_seeded_random_mix(ctx):
    rs = np.random.RandomState(20260117)
    names = [name_of(int(l), k) for k, l in enumerate(list(rs.randint(1, 41, 30)) + [300, 90])]
    n = 5000
    tid = rs.randint(0, len(names), n)
    tid[rs.randint(0, n, 40)] = 30                                             # a few rows of the 300-byte name, scattered
    digits = rs.randint(1, 19, (2, n))
    vals = [[int(rs.randint(10**(int(d) - 1) if d > 1 else 0, 10**int(d), dtype=np.int64)) for d in digits[j]] for j in range(2)]
    depth = np.where(rs.rand(n) < 0.1, 2**31 - 1 - rs.randint(0, 1000, n), rs.randint(0, 500, n))
    paths = encode_and_check(ctx, names, tid.tolist(), vals[0], vals[1], depth.tolist())
    assert paths["staged"] + paths["fallback"] == -(-n // 256) and paths["staged"] > 0
    assert {len(str(v)) for v in vals[0]} == set(range(1, 19))                # every digit count took part


def test_the_lane_per_row_form_writes_the_same_bytes(ctx):
    """the form the staged write pass is measured against (tools/bench_bedgraph_export.py)"""
    names = [name_of(n) for n in (3, 40, 300)]
    n = 1500
    args = ([i % 3 for i in range(n)], [EDGES[i % len(EDGES)] for i in range(n)], [i * 7919 for i in range(n)], [DEPTHS[i % 4] for i in range(n)])
    ctx.debug_rows_text_form("lane")
    try:
        assert encode_and_check(ctx, names, *args) == {"staged": 0, "fallback": 0}
        with pytest.raises(duckhts_amd.DhtsError, match="debug_rows_text_form: the form must be 0"):
            ctx.debug_rows_text_form("other")
    finally:
        ctx.debug_rows_text_form("staged")
    paths = encode_and_check(ctx, names, *args)
    assert paths["staged"] + paths["fallback"] == 6


# ---- 2. the exported file, read back by a reader the project did not write ----
def export(data, tmp_path, name="out.bed.gz", **kw):
    out = os.path.join(str(tmp_path), name)
    st = duckhts_amd.bam_bedgraph_export(data, out, **kw)
    z = open(out, "rb").read()
    assert z.endswith(X.EOF_BLOCK) and st["bytes_out"] == len(z) and st["output_path"] == out
    text = gzip.decompress(z)
    assert st["bytes_text"] == len(text) and st["n_rows"] == text.count(b"\n") == st["stats"]["n_runs"]
    kind = kw.get("index", "tbi")
    if kind == "none":
        assert st["index_path"] is None and st["bytes_index"] == 0 and not os.path.exists(out + ".tbi") and not os.path.exists(out + ".csi")
    else:
        assert st["index_path"] == out + "." + kind and os.path.getsize(st["index_path"]) == st["bytes_index"] > 0
    return text, st, out


def model_params(kw):
    p = {k: v for k, v in kw.items() if k in M.FILTERS + ("zero_runs", "breaks")}
    p.setdefault("exclude_flags", M.DEFAULT_EXCLUDE)
    return p


def check(data, tmp_path, **kw):
    refs, reads = M.reads_from_bam(data)
    exp, res = X.export(reads, refs, **model_params(kw))
    text, st, out = export(data, tmp_path, **kw)
    assert text == exp and X.parse(text) == X.rows_of(res, refs)
    assert {k: st["stats"][k] for k in M.COUNTERS} == res["stats"] and st["status"] == 1
    return text, st, out


@pytest.fixture(scope="module")
def rng():
    return read_golden("range.bam")


@pytest.mark.parametrize("kw", [dict(), dict(zero_runs=1), dict(breaks="2,4"), dict(zero_runs=1, breaks=[1, 5, 150], index="csi"),
                                dict(min_mapq=1, exclude_flags=16, min_baseq=25, include_deletions=1, zero_runs=1), dict(min_read_len=100, require_flags=64, include_flags=48, index="none")],
                         ids=["defaults", "zero_runs", "breaks", "zero_runs-breaks-csi", "filter", "filter-flags-none"])
def test_the_golden_file(rng, tmp_path, kw):
    text, st, _ = check(rng, tmp_path, **kw)
    assert st["n_rows"] > 0


@pytest.mark.parametrize("zero_runs,breaks", G.COMBOS)
@pytest.mark.parametrize("case", ["tile_edges", "row_lengths", "many_runs"])
def test_the_bedgraph_case_files(tmp_path, case, zero_runs, breaks):
    check(G.bam(*getattr(G, case)()), tmp_path, zero_runs=zero_runs, breaks=breaks)


def test_a_bed(tmp_path):
    data = G.bam(G.TOUCH_REFS, G.TOUCH_READS)
    refs, reads = M.reads_from_bam(data)
    rows, skipped = M.merge_bed(G.TOUCH_BED, refs)
    for kw in (dict(), dict(zero_runs=1, breaks="2")):
        exp, res = X.export(reads, refs, rows=rows, exclude_flags=M.DEFAULT_EXCLUDE, **kw)
        text, st, _ = export(data, tmp_path, bed=D.bed_text(G.TOUCH_BED), overwrite=True, **kw)
        assert text == exp and st["stats"]["n_bed_skipped"] == skipped and st["n_rows"] == res["n_rows"] > 0


def test_regions_with_an_index(rng, tmp_path):
    region = "CHROMOSOME_I:901-1000,CHROMOSOME_I:1001-1100,CHROMOSOME_II:1-3000"
    bai = read_golden("range.bam.bai")
    scanned = duckhts_amd.read_bam(rng, region=region, index=bai)
    refs, _ = M.reads_from_bam(rng)
    rows = parse_rows(refs, region)
    assert X.in_file_order(rows)
    for kind in ("tbi", "csi"):
        exp, res = X.export(M.reads_from_cols(scanned), refs, rows=rows, exclude_flags=M.DEFAULT_EXCLUDE, zero_runs=1)
        text, st, out = export(rng, tmp_path, name=kind + ".bed.gz", region=region, bam_index=bai, zero_runs=1, index=kind)
        assert text == exp and res["n_rows"] > 3
        got = duckhts_amd.read_bed(out, region="CHROMOSOME_I:950-1050", index_path=None if kind == "tbi" else out + ".csi")
        want = X.overlapping(X.rows_of(res, refs), b"CHROMOSOME_I", 949, 1050)
        assert want and list(zip(got["chrom"], got["start"], got["end"], got["name"])) == [(c, s, e, b"%d" % d) for c, s, e, d in want]


# ---- 3. the identity: the file is bgzip_file of the plain text, whatever the page and the chunk ----
BIG_NAME = "contig_with_a_name_of_forty_characters_0"
BIG_REFS = [(BIG_NAME, 221000), ("second", 5000), ("untouched", 3000)]


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """a zero_runs input whose text is more than five blocks: 3,001 reads 40 apart behind position 100,000, so that the rows are 57 bytes"""
    assert len(BIG_NAME) == 40
    reads = [R(0, 0, 100000 + 40 * i, 30, "10M", 30) for i in range(3001)] + G.at(1, 4990, 10, 2) + G.at(1, 100, 50)
    data = G.bam(BIG_REFS, reads)
    refs, mreads = M.reads_from_bam(data)
    text, res = X.export(mreads, refs, exclude_flags=M.DEFAULT_EXCLUDE, zero_runs=1)
    assert X.n_blocks(text) >= 6 and len(text) >= 5 * X.BLOCK and X.straddlers(text) == X.n_blocks(text) - 1       # a row lies across every block boundary
    assert res["n_rows"] > 6000 and res["n_rows"] % 7 != 0                                                           # and the pages of 7 rows end inside blocks
    d = tmp_path_factory.mktemp("export_identity")
    plain = str(d / "plain.bed")
    open(plain, "wb").write(text)
    ctx = duckhts_amd.Context(0)
    try:
        want = {}
        for level in (0, 6):
            ctx.bgzip_file(plain, str(d / f"plain.{level}.gz"), level)
            want[level] = open(str(d / f"plain.{level}.gz"), "rb").read()
    finally:
        ctx.close()
    assert len(want[6]) < len(want[0]) // 2 and gzip.decompress(want[6]) == text
    return {"data": data, "text": text, "res": res, "refs": refs, "want": want, "dir": str(d)}


@pytest.mark.parametrize("level", [0, 6])
@pytest.mark.parametrize("limits", [None, (1, 1), (7, 2)], ids=["defaults", "1row-1block", "7rows-2blocks"])
def test_the_file_is_bgzip_of_the_text_under_every_page_and_chunk(big, tmp_path, limits, level):
    out = os.path.join(str(tmp_path), "big.bed.gz")
    st = duckhts_amd.bam_bedgraph_export(big["data"], out, index="none", level=level, zero_runs=1, limits=limits)
    got = open(out, "rb").read()
    assert st["bytes_text"] == len(big["text"]) and st["n_rows"] == big["res"]["n_rows"]
    assert got == big["want"][level], (len(got), len(big["want"][level]))


def test_level_minus_one_is_the_compressing_setting(big, tmp_path):
    out = os.path.join(str(tmp_path), "big.bed.gz")
    duckhts_amd.bam_bedgraph_export(big["data"], out, index="none", zero_runs=1, limits=(1000, 3))
    assert open(out, "rb").read() == big["want"][6]


# ---- 4. the index ----
def tabix_index_of(path, min_shift):
    """what dhts_tabix_build_index with the BED preset gives on the file, wrapped as a BGZF file"""
    L = duckhts_amd.lib()
    L.dhts_tabix_build_index.restype = C.c_int64; L.dhts_tabix_build_index.argtypes = [C.c_void_p] + [C.c_int] * 7
    L.dhts_bgzf_wrap.restype = C.c_int64; L.dhts_bgzf_wrap.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(path); ctx.bgzf_index()
        n = L.dhts_tabix_build_index(ctx.h, *X.CONF_BED, min_shift)
        assert n > 0, L.dhts_error(ctx.h)
        raw = np.zeros(n, np.uint8)
        assert L.dhts_bam_index_bytes(ctx.h, raw.ctypes.data, n) == 0
    finally:
        ctx.close()
    need = L.dhts_bgzf_wrap(raw.ctypes.data, n, None, 0)
    out = np.zeros(need, np.uint8)
    return out[:L.dhts_bgzf_wrap(raw.ctypes.data, n, out.ctypes.data, need)].tobytes(), raw.tobytes()


@pytest.mark.parametrize("kind,min_shift", [("tbi", 0), ("csi", 0), ("csi", 12)])
def test_the_index_is_the_tabix_writers_and_answers_regions(big, tmp_path, kind, min_shift):
    out = os.path.join(str(tmp_path), "big.bed.gz")
    st = duckhts_amd.bam_bedgraph_export(big["data"], out, index=kind, min_shift=min_shift, zero_runs=1)
    idx = open(out + "." + kind, "rb").read()
    want, raw = tabix_index_of(out, 0 if kind == "tbi" else (min_shift or 14))
    assert idx == want and st["bytes_index"] == len(idx) and raw[:4] == (b"TBI\1" if kind == "tbi" else b"CSI\1")
    assert gzip.decompress(idx) == raw
    rows = X.rows_of(big["res"], big["refs"])
    name, second, untouched = BIG_NAME.encode(), b"second", b"untouched"
    # inside a run; across a contig's end (the last run of the first contig; the region runs on behind the contig); an untouched contig
    for region, (nm, beg, end) in ((f"{BIG_NAME}:100005-100006", (name, 100004, 100006)), (f"{BIG_NAME}:220990-300000", (name, 220989, 300000)), ("untouched", (untouched, 0, 1 << 29)),
                                   ("second:4995-5000", (second, 4994, 5000))):
        got = duckhts_amd.read_bed(out, region=region, index_path=out + "." + kind)
        exp = X.overlapping(rows, nm, beg, end)
        assert exp and list(zip(got["chrom"], got["start"], got["end"], got["name"])) == [(c, s, e, b"%d" % d) for c, s, e, d in exp], region
    assert X.overlapping(rows, name, 100004, 100006) == [(name, 100000, 100010, 1)] and X.overlapping(rows, untouched, 0, 9999) == [(untouched, 0, 3000, 0)]


# ---- 5. the empty result ----
def test_an_empty_result_is_the_eof_block(tmp_path):
    data = G.bam([("a", 1500), ("b", 7)], [R(0x400, 0, 10, 30, "10M", 30), R(0, 1, 10, 3, "10M", 30), R(4, -1, -1, 0, "*", 30)])
    for kind in ("none", "tbi", "csi"):
        out = os.path.join(str(tmp_path), kind + ".bed.gz")
        st = duckhts_amd.bam_bedgraph_export(data, out, index=kind, min_mapq=10)
        assert st["n_rows"] == 0 and st["bytes_text"] == 0 and st["bytes_out"] == 28 and st["stats"]["n_counted"] == 0
        assert open(out, "rb").read() == X.EOF_BLOCK and gzip.decompress(open(out, "rb").read()) == b""
        if kind == "none":
            continue
        # the index is what the tabix writer makes of that file: a valid index without a sequence name
        idx = open(out + "." + kind, "rb").read()
        want, raw = tabix_index_of(out, 0 if kind == "tbi" else 14)
        assert idx == want and raw[:4] == (b"TBI\1" if kind == "tbi" else b"CSI\1")
        l_aux = 0 if kind == "tbi" else struct.unpack_from("<i", raw, 12)[0]
        assert struct.unpack_from("<i", raw, 4 if kind == "tbi" else 16 + l_aux)[0] == 0                            # n_ref: no sequence
        with pytest.raises(duckhts_amd.BedIteratorError, match="read_bed: failed to create region iterator"):
            duckhts_amd.read_bed(out, region="a:1-100", index_path=out + "." + kind)
        assert duckhts_amd.read_bed(out)["n_rows"] == 0


# ---- 6. refusals and what is left behind them ----
def open_ctx(data, region=None):
    ctx = duckhts_amd.Context(0)
    ctx.open(data)
    ctx.bgzf_index()
    ctx.bam_open()
    if region:
        assert ctx.set_regions(region)
    return ctx


def test_refusals_and_cleanup(rng, tmp_path):
    d = str(tmp_path)
    out = os.path.join(d, "o.bed.gz")
    ctx = open_ctx(rng)
    L = ctx.L
    p, st = duckhts_amd.BedgraphExportParams(-1, 1, 0, 0), duckhts_amd.BedgraphExportStats()
    try:
        # before open
        with pytest.raises(duckhts_amd.DhtsError) as e:
            ctx.bam_bedgraph_export(out)
        assert str(e.value) == X.ERR_NOT_OPEN and L.dhts_bedgraph_export(ctx.h, out.encode(), C.byref(p), C.byref(st)) == -1 and os.listdir(d) == []
        ctx.bam_bedgraph_open(exclude_flags=0x704, zero_runs=1)
        ctx.bam_bedgraph_scan()
        with pytest.raises(duckhts_amd.DhtsError, match="bam_bedgraph_export: index must be one of: tbi, csi, none"):
            ctx.bam_bedgraph_export(out, index="bai")
        p.index = 3
        assert L.dhts_bedgraph_export(ctx.h, out.encode(), C.byref(p), C.byref(st)) == -1 and b"bam_bedgraph_export: index must be 0 (none), 1 (TBI) or 2 (CSI)" in L.dhts_error(ctx.h)
        p.index = 1
        assert os.listdir(d) == []
        # an existing file without overwrite: refused by its own code, and left alone
        open(out, "wb").write(b"mine")
        with pytest.raises(duckhts_amd.DhtsError) as e:
            ctx.bam_bedgraph_export(out)
        assert str(e.value) == X.err_exists(out)
        assert L.dhts_bedgraph_export(ctx.h, out.encode(), C.byref(p), C.byref(st)) == -6 and open(out, "rb").read() == b"mine" and os.listdir(d) == ["o.bed.gz"]
        # an unwritable directory
        nowhere = os.path.join(d, "no", "such", "dir", "o.bed.gz")
        with pytest.raises(duckhts_amd.DhtsError) as e:
            ctx.bam_bedgraph_export(nowhere)
        assert str(e.value).startswith(X.ERR_OPEN_OUTPUT + nowhere) and L.dhts_bedgraph_export(ctx.h, nowhere.encode(), C.byref(p), C.byref(st)) == -3
        assert os.listdir(d) == ["o.bed.gz"]
        # a success replaces it; the paging state is as after an accumulate
        first, _ = ctx.bam_bedgraph_next(5)
        res = ctx.bam_bedgraph_export(out, overwrite=True)
        assert sorted(os.listdir(d)) == ["o.bed.gz", "o.bed.gz.tbi"] and res["n_rows"] == ctx.bam_bedgraph_stats()["n_runs"] > 5
        again, status = ctx.bam_bedgraph_next(5)
        assert status == 0 and all(np.array_equal(again[k], first[k]) for k in duckhts_amd.BEDGRAPH_COLUMNS)      # page one again
        refs, reads = M.reads_from_bam(rng)
        assert gzip.decompress(open(out, "rb").read()) == X.export(reads, refs, exclude_flags=M.DEFAULT_EXCLUDE, zero_runs=1)[0]
    finally:
        ctx.close()


def test_regions_out_of_file_order(rng, tmp_path):
    d = str(tmp_path)
    out = os.path.join(d, "r.bed.gz")
    refs, _ = M.reads_from_bam(rng)
    for region in ("CHROMOSOME_I:1001-1100,CHROMOSOME_I:901-1000", "CHROMOSOME_I:901-1000,CHROMOSOME_II:1-100,CHROMOSOME_I:1001-1100"):
        rows = parse_rows(refs, region)
        assert not X.in_file_order(rows)
        for kind in ("tbi", "csi"):
            with pytest.raises(duckhts_amd.DhtsError) as e:
                duckhts_amd.bam_bedgraph_export(rng, out, region=region, index=kind, zero_runs=1)
            assert str(e.value) == X.ERR_ORDER and os.listdir(d) == []
        # without an index the rows are written as answered
        scanned = duckhts_amd.read_bam(rng, region=region)
        exp, res = X.export(M.reads_from_cols(scanned), refs, rows=rows, exclude_flags=M.DEFAULT_EXCLUDE, zero_runs=1)
        st = duckhts_amd.bam_bedgraph_export(rng, out, region=region, index="none", zero_runs=1, overwrite=True)
        assert gzip.decompress(open(out, "rb").read()) == exp and st["n_rows"] == res["n_rows"] > 2 and os.listdir(d) == ["r.bed.gz"]
        os.unlink(out)
    ctx = open_ctx(rng, "CHROMOSOME_I:1001-1100,CHROMOSOME_I:901-1000")
    try:
        ctx.bam_bedgraph_open(zero_runs=1)
        ctx.bam_bedgraph_scan()
        p, st = duckhts_amd.BedgraphExportParams(-1, 2, 0, 0), duckhts_amd.BedgraphExportStats()
        assert ctx.L.dhts_bedgraph_export(ctx.h, out.encode(), C.byref(p), C.byref(st)) == -7 and os.listdir(d) == []
    finally:
        ctx.close()
