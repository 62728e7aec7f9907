"""The surface of interval_nearest without a device: the header's block and its contract, the debug hook's indices, the exports, the Python
mirror's signatures and structure layout, the sources in the build, the registration line behind interval_overlap's, the error strings in the
three layers, and the documents."""
import ctypes as C
import inspect
import os
import re

import duckhts_amd
import interval_nearest_ref as N
from conftest import ROOT

ENTRIES = ["dhts_ivl_nearest_open", "dhts_ivl_nearest_next", "dhts_ivl_nearest_stats_get"]
REGISTER = ["register_interval_nearest_function"]


def source(name):
    return open(os.path.join(ROOT, "duckhts_amd", "csrc", name)).read()


def header(name="duckhts_amd.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def test_the_header_block_and_its_contract():
    text = header()
    at = text.index("---- interval nearest")
    assert at > text.index("---- interval algebra") and text.count("---- interval algebra") == 1 and text.count("---- interval nearest") == 1
    block = text[at:]
    code = re.sub(r"/\*.*?\*/", "", block, flags=re.S)
    assert "int dhts_ivl_nearest_open(dhts_ctx *left, dhts_ctx *right, int64_t k, int64_t max_distance, int32_t ties);" in code
    assert "int dhts_ivl_nearest_next(dhts_ctx *left, int64_t max_rows, uint32_t colmask, dhts_ivl_batch *out);" in code
    assert "int dhts_ivl_nearest_stats_get(dhts_ctx *left, dhts_ivl_nearest_stats *out);" in code
    assert re.search(r"enum \{ DHTS_IVL_NEAR_CHROM = 0, DHTS_IVL_NEAR_START, DHTS_IVL_NEAR_END, DHTS_IVL_NEAR_LEFT_ROW, DHTS_IVL_NEAR_RIGHT_START, DHTS_IVL_NEAR_RIGHT_END,\s+"
                     r"DHTS_IVL_NEAR_RIGHT_ROW, DHTS_IVL_NEAR_OVERLAP, DHTS_IVL_NEAR_DISTANCE, DHTS_IVL_NEAR_COL_COUNT \};", code)
    assert "enum { DHTS_IVL_TIES_ALL = 0, DHTS_IVL_TIES_FIRST = 1 };" in code and "#define DHTS_IVL_MAX_K 1048576" in code
    stats = re.search(r"typedef struct \{([^}]*)\} dhts_ivl_nearest_stats;", code).group(1)
    assert re.findall(r"\b(u?int\d+_t) (\w+);", stats) == [("uint64_t", "n_pairs"), ("uint64_t", "n_unmatched"), ("uint32_t", "end_sort_passes"), ("int32_t", "status")]
    flat = re.sub(r"\s*\n \*\s*", " ", block).lower()
    for phrase in ("distance = max(0, rs - e, s - re)", "0 for rows that overlap or touch", "`bedtools closest -d` prints this plus one", "the largest is 2^63 - 1",
                   "overlap = max(0, min(e, re) - max(s, rs))", "ranked by (distance, right_start, right_row)", "the first min(k, candidates)",
                   "every candidate whose distance is at most that of the k-th", "counted in n_unmatched", "no column is ever null", "counted in n_skipped",
                   "a left chrom the right file lacks gives no rows", "by left_row; within a left row by (right_start, right_row)", "not distance order",
                   "whole left rows", N.ERR_K, "max_distance must not be negative", N.ERR_TIES, "-1 in this abi", "bedtools closest -k -t all|first",
                   "strand or direction restriction", "-iu / -id", "ignoring overlaps (-io)", "a left join", "distance-ordered output",
                   "partition search of two sorted sequences", "nb(e + d + 1) - ne(s - d)", "dropped by dhts_ivl_load", "one result is open per context"):
        assert phrase.lower() in flat, phrase
    # the algebra block keeps what it said
    algebra = text[text.index("---- interval algebra"):at]
    assert "Not in this contract: interval_nearest;" in algebra and "} dhts_ivl_stats;" in algebra
    dbg = re.sub(r"\s*\n \*\s*", " ", header("duckhts_amd_debug.h"))
    for phrase in ("6 the end sort and gather", "7 the selection pass and its carry", "8 the write passes of the pages taken since"):
        assert phrase in dbg, phrase
    ext = header("duckhts_extension.h")
    assert "void register_interval_nearest_function(duckdb_connection connection);" in ext and "DHTS_NEAREST_FUNCTIONS=1" in ext


def test_exports_and_the_python_mirror():
    import __graft_entry__ as ge
    assert set(ENTRIES + REGISTER) <= set(ge.declared_exports())
    L = duckhts_amd.lib()
    for fn in ENTRIES:
        assert fn in duckhts_amd.EXPORTS and getattr(L, fn).argtypes is not None, fn
    assert hasattr(L, REGISTER[0])
    assert L.dhts_ivl_nearest_open.argtypes == [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32]
    assert L.dhts_ivl_nearest_next.argtypes == [C.c_void_p, C.c_int64, C.c_uint32, C.POINTER(duckhts_amd.BedBatch)]
    assert [f for f, _ in duckhts_amd.IvlNearestStats._fields_] == ["n_pairs", "n_unmatched", "end_sort_passes", "status"]
    assert C.sizeof(duckhts_amd.IvlNearestStats) == 24 and duckhts_amd.IvlNearestStats.end_sort_passes.offset == 16 and duckhts_amd.IvlNearestStats.status.offset == 20
    assert C.sizeof(duckhts_amd.IvlStats) == 56                                      # dhts_ivl_stats keeps its layout
    assert duckhts_amd.INTERVAL_NEAREST_COLUMNS == N.NEAREST_COLUMNS and duckhts_amd.INTERVAL_TIES == {"all": 0, "first": 1}
    assert len(duckhts_amd.INTERVAL_DTYPES) == len(N.NEAREST_COLUMNS)
    for m in ("ivl_nearest_open", "ivl_nearest_next", "ivl_nearest_stats"):
        assert callable(getattr(duckhts_amd.Context, m)), m
    sig = inspect.signature(duckhts_amd.interval_nearest).parameters
    assert list(sig) == ["left", "right", "k", "max_distance", "ties", "columns", "device", "max_rows", "max_blocks", "stats"]
    assert [sig[k].default for k in list(sig)[2:]] == [1, None, "all", None, 0, 0, 0, None]
    sig = inspect.signature(duckhts_amd.Context.ivl_nearest_open).parameters
    assert list(sig) == ["self", "right", "k", "max_distance", "ties"] and [sig[k].default for k in list(sig)[2:]] == [1, None, "all"]
    sig = inspect.signature(duckhts_amd.Context.ivl_nearest_next).parameters
    assert list(sig) == ["self", "max_rows", "columns"] and [sig[k].default for k in list(sig)[1:]] == [0, None]


def test_the_sources_are_part_of_the_build_and_registered_behind_interval_overlap():
    import __graft_entry__ as ge
    deps = {os.path.basename(p) for p in ge.HIP_DEPS}
    assert {"interval_nearest.hip", "dhts_interval_nearest.inc", "duckdb_interval_nearest.inc"} <= deps
    api, ext = source("dhts_api.hip"), source("duckdb_ext.cpp")
    assert api.index('#include "interval_nearest.hip"') > api.index('#include "interval_algebra.hip"')
    assert api.index('#include "dhts_interval_nearest.inc"') > api.index('#include "dhts_interval.inc"')
    assert ext.index('#include "duckdb_interval_nearest.inc"') > ext.index('#include "duckdb_interval_algebra.inc"')
    lines = ext.splitlines()
    alg = [i for i, ln in enumerate(lines) if "DHTS_ALGEBRA_FUNCTIONS" in ln]
    assert len(alg) == 1 and ext.count("DHTS_NEAREST_FUNCTIONS") == 1
    assert lines[alg[0] + 1].strip().startswith('if (const char *e = getenv("DHTS_NEAREST_FUNCTIONS")) if (atoi(e) == 1) register_interval_nearest_function(conn);')
    # the kernels: reuse of the algebra's search and index, the shared carry and page cut, no walk in the selection
    hip, inc, ddb = source("interval_nearest.hip"), source("dhts_interval_nearest.inc"), source("duckdb_interval_nearest.inc")
    for name in ("ivl_end_input", "ivl_end_gather", "ivl_nearest_cells<false>", "ivl_nearest_cells<true>", "ivl_page_cut", "ivl_sort(", "depth_carry<unsigned long long>(c, S.part, (unsigned long long *)S.cnt.p, n)"):
        assert name in inc, name
    for name in ("ivl_lower(", "IvlRight R;", "IVL_POS_LIMIT", "ivl_nearest_cells", "a.R.pmax[mid]", "a.R.bmax[k >> 6]"):
        assert name in hip, name
    select = hip[hip.index("ivl_near_select("):hip.index("ivl_near_emit(")]
    assert "for (" not in select and select.count("while (lo < hi)") == 1            # binary searches and one partition search
    for name in ("ivl_open_file(", "scan_chunks(", "IvlScanState", "DHTS_INTERVAL_PAGE_ROWS", "map_projection("):
        assert name in ddb, name
    assert "end_ready" in source("dhts_interval.inc")                                # dhts_ivl_load drops the end order


def test_the_error_strings_in_the_three_layers():
    inc, ddb, py = source("dhts_interval_nearest.inc"), source("duckdb_interval_nearest.inc"), open(os.path.join(ROOT, "duckhts_amd", "__init__.py")).read()
    for line in (N.ERR_K, N.ERR_MAX_DISTANCE, N.ERR_TIES):
        assert line in inc and line in ddb and line in py, line
    for line in (N.ERR_NEAREST_PATH, N.ERR_RIGHT_PATH, '"' + N.ERR_OPEN + '"'):
        assert line in ddb, line
    assert N.ERR_RIGHT_PATH in py and ("interval_nearest: " + N.ERR_TOO_MANY) in inc
    ddb_order = [ddb.index(e) for e in (N.ERR_NEAREST_PATH, N.ERR_RIGHT_PATH, N.ERR_K, N.ERR_MAX_DISTANCE, N.ERR_TIES, N.ERR_OPEN)]
    assert ddb_order == sorted(ddb_order)
    msgs = re.findall(r'fail\(c, "([^"]*)"', inc)
    assert len(msgs) >= 12 and all(m.startswith("interval_nearest: ") for m in msgs), msgs
    for who in ("dhts_ivl_load not called", "dhts_ivl_load not called on the right context", "dhts_ivl_nearest_open not called", "the two contexts have to be on one device",
                "the right context was loaded anew or closed since dhts_ivl_nearest_open"):
        assert ("interval_nearest: " + who) in inc, who


def test_the_documents_name_it():
    for doc, phrases in (("README.md", ("interval_nearest", "DHTS_NEAREST_FUNCTIONS=1", "Not built")),
                         ("INTEGRATION.md", ("interval_nearest", "DHTS_NEAREST_FUNCTIONS=1", "max_distance", "ties", "Not built", "-iu / -id", "(`-io`)", "left join", "distance-ordered")),
                         ("DESIGN.md", ("4u", "interval_nearest.hip", "e_end", "partition search", "ivl_nearest_cells", "tools/bench_intervals.py", "profiles/interval_nearest/"))):
        text = open(os.path.join(ROOT, doc)).read()
        for p in phrases:
            assert p in text, (doc, p)
    prof = os.path.join(ROOT, "profiles", "interval_nearest")
    assert os.path.isdir(prof) and any(f.endswith(".json") for f in os.listdir(prof))
    bench = open(os.path.join(ROOT, "tools", "bench_intervals.py")).read()
    assert "NEAREST_K = (1, 8)" in bench and "debug_ivl_ms(6)" in bench and "debug_ivl_ms(7)" in bench and "debug_ivl_ms(8)" in bench
