"""The surface of interval_merge / interval_overlap without a device: the header's block and its contract, the debug hooks, the exports, the
Python mirror's signatures and structure layouts, the sources in the build, the registration line behind fasta_nuc's, the error strings in the
sources, and the documents."""
import ctypes as C
import inspect
import os
import re

import duckhts_amd
import interval_ref as R
from conftest import ROOT

ENTRIES = ["dhts_ivl_load", "dhts_ivl_stats_get", "dhts_ivl_chrom_name", "dhts_ivl_merge_open", "dhts_ivl_merge_next", "dhts_ivl_overlap_open", "dhts_ivl_overlap_next",
           "dhts_ivl_batch_host_bytes", "dhts_ivl_batch_fetch"]
HOOKS = ["dhts_debug_ivl_sort", "dhts_debug_ivl_ms"]
REGISTER = ["register_interval_merge_function", "register_interval_overlap_function"]


def source(name):
    return open(os.path.join(ROOT, "duckhts_amd", "csrc", name)).read()


def header(name="duckhts_amd.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def test_the_header_block_and_its_contract():
    text = header()
    at = text.index("---- interval algebra")
    assert at > text.index("---- utilities") and text.count("---- interval algebra") == 1        # a new block at the end: nothing in front of the existing ones
    block = text[at:]
    code = re.sub(r"/\*.*?\*/", "", block, flags=re.S)
    for fn in ENTRIES:
        assert re.search(r"\b%s\(" % fn, code), fn
    assert re.search(r"int dhts_ivl_load\(dhts_ctx \*bed, int64_t max_blocks\);", code)
    assert re.search(r"int dhts_ivl_overlap_open\(dhts_ctx \*left, dhts_ctx \*right, int32_t mode\);", code)
    assert re.search(r"int dhts_ivl_merge_next\(dhts_ctx \*bed, int64_t max_rows, uint32_t colmask, dhts_ivl_batch \*out\);", code)
    for phrase in ("Meta lines (empty, '#', \"track\", \"browser\") do not count".lower(), "a row's number is its 0-based index among read_bed's rows",
                   "end < start", "outside [-2^62, 2^62)", "counted in n_skipped", "empty rows (start == end) are valid",
                   "compared byte for byte", "memcmp, the shorter name first on a common prefix",
                   "start <= run_end + max_gap", "bedtools merge -d", "interval_merge: max_gap must be between 0 and", "1099511627776",
                   "any: rs < e && s < re", "contain: s <= rs && re <= e && rs < e", "within: rs <= s && e <= re && s < re", "max(0, min(e, re) - max(s, rs))",
                   "by left_row; within a left row by (right_start, right_row)", "a left chrom the right file lacks gives no rows", "no column is",
                   "whatever max_rows is (0 = 1,048,576)", "at least one left row", "more than 4294967279 rows",
                   "interval_nearest", "strand-aware merge", "a region parameter", "unmatched left rows", "counts-only output", "beyond the first three",
                   "table-valued (subquery) arguments", "dhts_bam_set_overlap_intervals", "two files on different devices", "fewer than 2^63 pairs",
                   "every error is prefixed with the function's name", "names what is missing"):
        assert phrase in re.sub(r"\s*\n \*\s*", " ", block).lower(), phrase
    assert "enum { DHTS_IVL_MERGE_CHROM = 0, DHTS_IVL_MERGE_START, DHTS_IVL_MERGE_END, DHTS_IVL_MERGE_N, DHTS_IVL_MERGE_COL_COUNT };" in code
    assert re.search(r"enum \{ DHTS_IVL_OV_CHROM = 0, DHTS_IVL_OV_START, DHTS_IVL_OV_END, DHTS_IVL_OV_LEFT_ROW, DHTS_IVL_OV_RIGHT_START, DHTS_IVL_OV_RIGHT_END, DHTS_IVL_OV_RIGHT_ROW,\s+DHTS_IVL_OV_OVERLAP, DHTS_IVL_OV_COL_COUNT \};", code)
    assert "enum { DHTS_IVL_ANY = 0, DHTS_IVL_CONTAIN = 1, DHTS_IVL_WITHIN = 2 };" in code
    dbg = re.sub(r"/\*.*?\*/", "", header("duckhts_amd_debug.h"), flags=re.S)
    assert "int dhts_debug_ivl_sort(dhts_ctx *, const uint64_t *keys_u64, const uint32_t *rank_u32, uint64_t n, uint32_t *rows_out_u32, int32_t *passes);" in dbg
    ext = header("duckhts_extension.h")
    for fn in REGISTER:
        assert ("void %s(duckdb_connection connection);" % fn) in ext
    assert "DHTS_ALGEBRA_FUNCTIONS=1" in ext


def test_exports_and_the_python_mirror():
    import __graft_entry__ as ge
    assert set(ENTRIES + HOOKS + REGISTER) <= set(ge.declared_exports())
    L = duckhts_amd.lib()
    for fn in ENTRIES:
        assert fn in duckhts_amd.EXPORTS and getattr(L, fn).argtypes is not None, fn
    for fn in HOOKS + REGISTER:
        assert hasattr(L, fn), fn
    assert len(L.dhts_debug_ivl_sort.argtypes) == 6 and L.dhts_ivl_overlap_open.argtypes == [C.c_void_p, C.c_void_p, C.c_int32]
    # the structures' layouts: dhts_ivl_stats is six 64-bit counters and two 32-bit words, a batch has dhts_bedgraph_batch's layout
    assert [f for f, _ in duckhts_amd.IvlStats._fields_] == ["n_rows", "n_skipped", "n_chroms", "n_name_runs", "n_runs", "n_pairs", "sort_passes", "status"]
    assert C.sizeof(duckhts_amd.IvlStats) == 56 and duckhts_amd.IvlStats.sort_passes.offset == 48 and duckhts_amd.IvlStats.status.offset == 52
    stats = re.search(r"typedef struct \{([^}]*)\} dhts_ivl_stats;", re.sub(r"/\*.*?\*/", "", header(), flags=re.S)).group(1)
    assert re.findall(r"\b(n_\w+|sort_passes|status)\b", stats) == [f for f, _ in duckhts_amd.IvlStats._fields_]
    assert L.dhts_ivl_merge_next.argtypes[-1] == C.POINTER(duckhts_amd.BedBatch)
    assert duckhts_amd.IVL_SORT_TILE == 4096 and duckhts_amd.INTERVAL_MODES == {"any": 0, "contain": 1, "within": 2}
    assert duckhts_amd.INTERVAL_MERGE_COLUMNS == R.MERGE_COLUMNS and duckhts_amd.INTERVAL_OVERLAP_COLUMNS == R.OVERLAP_COLUMNS
    for m in ("ivl_load", "ivl_stats", "ivl_merge_open", "ivl_merge_next", "ivl_overlap_open", "ivl_overlap_next", "debug_ivl_sort"):
        assert callable(getattr(duckhts_amd.Context, m)), m
    sig = inspect.signature(duckhts_amd.interval_merge).parameters
    assert list(sig) == ["bed", "max_gap", "columns", "device", "max_rows", "max_blocks", "stats"]
    assert [sig[k].default for k in list(sig)[1:]] == [0, None, 0, 0, 0, None]
    sig = inspect.signature(duckhts_amd.interval_overlap).parameters
    assert list(sig) == ["left", "right", "mode", "columns", "device", "max_rows", "max_blocks", "stats"]
    assert [sig[k].default for k in list(sig)[2:]] == ["any", None, 0, 0, 0, None]
    assert list(inspect.signature(duckhts_amd.Context.ivl_overlap_open).parameters) == ["self", "right", "mode"]
    assert list(inspect.signature(duckhts_amd.Context.debug_ivl_sort).parameters) == ["self", "keys", "rank"]


def test_the_sources_are_part_of_the_build_and_registered_behind_fasta_nuc():
    import __graft_entry__ as ge
    deps = {os.path.basename(p) for p in ge.HIP_DEPS}
    assert {"interval_sort.hip", "interval_algebra.hip", "dhts_interval.inc", "duckdb_interval_algebra.inc", "dev_scan.hip"} <= deps
    api, ext = source("dhts_api.hip"), source("duckdb_ext.cpp")
    assert api.index('#include "interval_algebra.hip"') > api.index('#include "interval_sort.hip"') > api.index('#include "vcf_text.hip"')
    assert api.index('#include "dhts_interval.inc"') > api.index('#include "dhts_bam_accum.inc"')
    assert ext.index('#include "duckdb_interval_algebra.inc"') > ext.index('#include "duckdb_interval.inc"')
    lines = ext.splitlines()
    nuc = [i for i, ln in enumerate(lines) if "register_fasta_nuc_function(conn)" in ln]
    assert len(nuc) == 1
    ln = lines[nuc[0] + 1]
    assert ln.strip().startswith('if (const char *e = getenv("DHTS_ALGEBRA_FUNCTIONS")) if (atoi(e) == 1) { register_interval_merge_function(conn); register_interval_overlap_function(conn); }')
    assert ext.index("register_interval_overlap_function(conn)") < ext.index("register_kmer_udf_functions(conn)") and ext.count("DHTS_ALGEBRA_FUNCTIONS") == 1
    # the sort: the block scan is dev_scan.hip's, the carry the shared one, the tile a stated constant
    srt, alg, inc = source("interval_sort.hip"), source("interval_algebra.hip"), source("dhts_interval.inc")
    assert '#include "dev_scan.hip"' in srt and "block_scan<uint32_t, ScanSum>(tot, sh)" in srt and not re.search(r"for \((?:uint32_t|int) d = 1; d <", srt + alg)
    for kernel in ("ivl_sort_bits", "ivl_sort_count", "ivl_sort_scatter"):
        assert kernel in srt and kernel in inc
    assert "__ballot(" in srt and "__popcll(" in srt and "#define IVL_SORT_TILE (IVL_SORT_NT * IVL_SORT_PER)" in srt
    assert "depth_carry<uint32_t>(c, S.part, (uint32_t *)S.counts.p, ncounts)" in inc
    assert "struct ScanMax" in source("dev_scan.hip") and "scan_carry<IvlPair, ScanMax, false>(" in inc and "depth_carry<unsigned long long>(c, S.part, (unsigned long long *)S.cnt.p, n)" in inc
    assert "std::stable_sort" in source("dhts_bam_join.inc")                       # the BAM join keeps its host sort
    for kernel in ("ivl_lines", "ivl_append", "ivl_index_gather", "ivl_index_finish", "ivl_merge_heads", "ivl_merge_emit", "ivl_overlap_cells", "ivl_page_cut"):
        assert kernel in alg and kernel in inc, kernel
    assert "bed_intervals" in inc and "line_table(c, " in inc


def test_the_error_strings_in_the_sources():
    inc, ddb, py = source("dhts_interval.inc"), source("duckdb_interval_algebra.inc"), open(os.path.join(ROOT, "duckhts_amd", "__init__.py")).read()
    for line in (R.ERR_MAX_GAP, R.ERR_MODE):
        assert line in inc and line in ddb and line in py, line
    for line in (R.ERR_MERGE_PATH, R.ERR_OVERLAP_PATH, R.ERR_RIGHT_PATH, '"' + R.ERR_OPEN + '"'):
        assert line in ddb, line
    assert R.ERR_RIGHT_PATH in py and ('"%s: ' + R.ERR_TOO_MANY + '"') in inc and ("interval_overlap: " + R.ERR_TOO_MANY) in inc
    assert "read_bed: BED line has fewer than 3 tab-delimited fields (line %lld)" in inc
    msgs = re.findall(r'fail\(c, "([^"]*)"', inc)
    assert len(msgs) >= 15
    for m in msgs:
        assert m.split(":")[0] in ("interval_merge", "interval_overlap", "%s", "read_bed", "dhts_ivl_load", "dhts_ivl_stats_get", "debug_ivl_sort", "internal"), m
    for who in ("dhts_ivl_load not called", "dhts_ivl_merge_open not called", "dhts_ivl_overlap_open not called", "dhts_bed_open not called"):
        assert who in inc


def test_the_documents_name_them():
    for doc, phrases in (("README.md", ("interval_merge", "interval_overlap", "DHTS_ALGEBRA_FUNCTIONS=1")),
                         ("INTEGRATION.md", ("interval_merge", "interval_overlap", "DHTS_ALGEBRA_FUNCTIONS=1", "right_path", "max_gap", "Not built", "interval_nearest")),
                         ("DESIGN.md", ("4t", "interval_sort.hip", "interval_algebra.hip", "ScanMax", "not measured", "IVL_SORT_TILE", "tools/bench_intervals.py"))):
        text = open(os.path.join(ROOT, doc)).read()
        for p in phrases:
            assert p in text, (doc, p)
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_intervals.py"))
