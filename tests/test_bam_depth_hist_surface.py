"""The surface of bam_depth_hist without a device: the header declares the seven dhts_bam_hist_* entries, both structures and the contract, the built
library exports exactly what the headers declare, the Python mirror binds the entries, the structures of the two sides have one layout, the
constants of the histogram pass are the kernel's, the sources are part of the build, the error lines stand in both parts, and the table function
is registered last behind a variable of its own."""
import ctypes as C
import inspect
import os
import re
import subprocess

import bam_depth_hist_ref as M
import duckhts_amd
from conftest import ROOT
from test_duckdb_surface import HOST

ENTRIES = ["dhts_bam_hist_open", "dhts_bam_hist_accumulate", "dhts_bam_hist_scan", "dhts_bam_hist_stats", "dhts_bam_hist_next", "dhts_bam_hist_batch_host_bytes",
           "dhts_bam_hist_batch_fetch"]
OTHERS = ["register_bam_hist_function", "dhts_debug_hist_max_table_bytes", "dhts_debug_hist_pass_ms"]


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def source(name):
    return open(os.path.join(ROOT, "duckhts_amd", "csrc", name)).read()


def test_the_header_declares_the_entries_and_the_contract():
    text = header("duckhts_amd.h")
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(dhts_bam_hist_[a-z_]+)\s*\(", code))) == sorted(ENTRIES)
    for word in ("dhts_depth_hist_params", "dhts_depth_hist_stats", "dhts_depth_hist_batch", "DHTS_DEPTH_HIST_COL_COUNT"):
        assert word in code
    block = text[text.index("---- bam_depth_hist"):text.index("enum { DHTS_DEPTH_HIST_CHROM")]
    for phrase in ("mosdepth", "samtools stats", "exactly bam_depth's", "include_deletions", "n_bed_skipped", "refused by name", "per = 0 ('row')", "per = 1 ('contig')",
                   "header order", "empty after", M.ERR_PER, "bin(d) = min(d, depth_cap)", "[1000<]", "1,048,575", M.ERR_DEPTH_CAP, "all_positions = 2", "Padding slots", "ascending",
                   "n_at_least", "No column is ever NULL", "(chrom, 0, L, 0, L, L, L)", "fraction_at_least", "64-bit words", "1 GiB", "dhts_debug_hist_max_table_bytes",
                   "(8 per bin of every group)", "per := 'contig' or a smaller depth_cap", "200,000", "starts the result over", "pure function", "0x704", "16 GiB",
                   "dhts_debug_coverage_max_table_bytes", "'total' group", "dense output", "--thresholds", "suppress_overlaps", "several input files", "reference / CRAM", "max_depth",
                   "4,096 bins", 'prefixed "bam_depth_hist:"'):
        assert phrase in block, phrase
    assert "1,048,576" in text[text.index("int dhts_bam_hist_stats"):text.index("int dhts_bam_hist_next")]            # the default page is stated
    names = re.search(r"enum \{ (DHTS_DEPTH_HIST_CHROM[^}]*)\}", code).group(1)
    assert [n.strip().split(" ")[0].replace("DHTS_DEPTH_HIST_", "").lower() for n in names.split(",")][:-1] == ["chrom", "start", "end", "depth", "n_positions", "n_at_least", "length"]
    ext = header("duckhts_extension.h")
    assert re.search(r"\bregister_bam_hist_function\s*\(", ext) and "DHTS_HIST_FUNCTIONS=1" in ext and "DHTS_DEPTH_HIST_PAGE_ROWS" in ext and "fraction_at_least DOUBLE" in ext
    dbg = re.sub(r"/\*.*?\*/", "", header("duckhts_amd_debug.h"), flags=re.S)
    assert re.search(r"void dhts_debug_hist_max_table_bytes\(uint64_t n\);", dbg) and re.search(r"double dhts_debug_hist_pass_ms\(", dbg)
    # the function the two older blocks called missing is named where they did
    assert "bam_depth_hist" in text[text.index("---- bam_bedgraph"):text.index("enum { DHTS_BEDGRAPH_CHROM")]


def test_the_library_exports_what_the_headers_declare():
    import __graft_entry__ as ge
    out = subprocess.run(["nm", "-D", "--defined-only", duckhts_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    declared = set(ge.declared_exports())
    assert exported <= declared                                                   # no kernel stub, pool or helper leaks
    assert not [n for n in declared - exported if "diag" not in n and n != "idx_t"]      # what is missing is the diagnostic builds' and a type name
    for n in ENTRIES + OTHERS:
        assert n in exported, n
    assert not [n for n in exported if ("hist" in n or "dhi_" in n) and n not in ENTRIES + OTHERS]


def test_the_python_mirror_binds_the_entries():
    L = duckhts_amd.lib()
    for n in ENTRIES:
        assert n in duckhts_amd.EXPORTS and getattr(L, n).argtypes, n
    for m in ("bam_depth_hist_open", "bam_depth_hist_accumulate", "bam_depth_hist_scan", "bam_depth_hist_stats", "bam_depth_hist_next"):
        assert callable(getattr(duckhts_amd.Context, m))
    assert duckhts_amd.DEPTH_HIST_COLUMNS == M.COLUMNS and [4, 8, 8, 4, 8, 8, 8] == [duckhts_amd.np.dtype(d).itemsize for d in duckhts_amd.DEPTH_HIST_DTYPES]
    assert duckhts_amd.DEPTH_HIST_COLMASK == duckhts_amd.DEPTH_COLMASK and not duckhts_amd.DEPTH_HIST_COLMASK & 1      # no string column in the scan (QNAME is bit 0)
    assert duckhts_amd.DEPTH_HIST_PER == {"row": 0, "contig": 1}
    sig = inspect.signature(duckhts_amd.bam_depth_hist).parameters
    assert list(sig)[:8] == ["src", "region", "index", "bed", "max_blocks", "max_rows", "columns", "device"]
    assert [sig[k].default for k in ("region", "index", "bed", "max_blocks", "max_rows", "columns", "device", "min_read_len", "min_mapq", "min_baseq", "include_flags", "require_flags",
                                     "exclude_flags", "include_deletions", "depth_cap", "per")] == [None, None, None, 0, 0, None, 0, 0, 0, 0, 0, 0, 0x704, 0, 1000, "row"]
    bsig = inspect.signature(duckhts_amd.bam_bedgraph).parameters                                    # the shared parameters keep bam_bedgraph's defaults
    assert all(sig[k].default == bsig[k].default for k in sig if k in bsig)
    ctx_sig = inspect.signature(duckhts_amd.Context.bam_depth_hist_open).parameters                  # the ABI's rule: the masks as given
    assert ctx_sig["exclude_flags"].default == 0 and ctx_sig["bed_ctx"].default is None and ctx_sig["depth_cap"].default == 1000 and ctx_sig["per"].default == "row"
    # the structures: field order and sizes of include/duckhts_amd.h
    fields = [f[0] for f in duckhts_amd.DepthHistParams._fields_]
    assert C.sizeof(duckhts_amd.DepthHistParams) == 48 and fields == ["min_read_len", "min_mapq", "min_baseq", "require_flags", "exclude_flags", "include_flags", "include_deletions",
                                                                       "depth_cap", "per", "reserved"]
    assert duckhts_amd.DepthHistParams.depth_cap.offset == 32 and duckhts_amd.DepthHistParams.per.offset == 36 and duckhts_amd.DepthHistParams.reserved.offset == 40
    assert fields[:7] == [f[0] for f in duckhts_amd.BedgraphParams._fields_][:7]                    # the filter fields and include_deletions
    sfields = [f[0] for f in duckhts_amd.DepthHistStats._fields_]
    assert C.sizeof(duckhts_amd.DepthHistStats) == 112 and sfields == M.STATS + ["status", "reserved"]
    assert sfields[:7] == [f[0] for f in duckhts_amd.CoverageStats._fields_][:7]                  # the seven counters of dhts_coverage_stats
    code = re.sub(r"/\*.*?\*/", "", header("duckhts_amd.h"), flags=re.S)
    m = re.search(r"typedef struct \{([^}]*)\} dhts_depth_hist_params;", code)
    assert re.findall(r"\b(" + "|".join(fields) + r")\b", m.group(1)) == fields and "int32_t reserved[2];" in m.group(1) and "int64_t min_read_len;" in m.group(1)
    m = re.search(r"typedef struct \{([^}]*)\} dhts_depth_hist_stats;", code)
    assert re.findall(r"\b(n_[a-z_]+|table_bytes|hist_bytes|status|reserved)\b", m.group(1)) == sfields
    m = re.search(r"int dhts_bam_hist_open\(([^)]*)\)", code)
    assert [a.strip().split(" ")[-1].lstrip("*") for a in m.group(1).split(",")] == ["bam", "params", "bed"]
    m = re.search(r"int dhts_bam_hist_next\(([^)]*)\)", code)
    assert [a.strip().split(" ")[-1].lstrip("*") for a in m.group(1).split(",")] == ["bam", "max_rows", "colmask", "out"]


def test_the_constants_of_the_histogram_pass_are_the_kernels():
    hip = source("bam_depth_hist.hip")
    defs = {k: int(v) for k, v in re.findall(r"#define (DHI_[A-Z_]+) (\d+)u", hip)}
    assert defs["DHI_LDS_BINS"] == duckhts_amd.DEPTH_HIST_LDS_BINS == 4096 and defs["DHI_GRID_TARGET"] == duckhts_amd.DEPTH_HIST_GRID_TARGET
    assert defs["DHI_SPAN_MIN_TILES"] == duckhts_amd.DEPTH_HIST_SPAN_MIN_TILES
    t, m = duckhts_amd.DEPTH_HIST_GRID_TARGET, duckhts_amd.DEPTH_HIST_SPAN_MIN_TILES
    assert [duckhts_amd.depth_hist_span_tiles(n) for n in (1, m * t, m * t + 1, 100 * t, 100 * t + 1)] == [m, m, m + 1, 100, 101]
    # the bound of the 32-bit LDS counters: the 16 GiB table has 2^22 tiles, its span 2^21 slots; the host refuses a span of 2^22 tiles
    assert duckhts_amd.depth_hist_span_tiles((16 << 30) // 4096) * 1024 == 1 << 21 and "span >= (1ull << 22)" in source("dhts_bam_depth_hist.inc")
    assert "printf" not in hip and "assert" not in hip and "asm" not in hip


def test_both_parts_state_the_errors_the_header_promises():
    inc, ddb = source("dhts_bam_depth_hist.inc"), source("duckdb_depth_hist.inc")
    msgs = re.findall(r'"(bam_depth_hist[^"]+ [^"]*)"', inc)                                # (every literal but the bare name dep_layout is given)
    assert msgs and all(m.startswith("bam_depth_hist: ") for m in msgs)
    assert inc.count('bam_filter_check(m, "bam_depth_hist", p->min_read_len, ') == 1 and ddb.count('bam_filter_check(m, "bam_depth_hist", min_read_len, ') == 1
    assert M.ERR_DELETIONS in inc                                                           # (the table function takes it as BOOLEAN)
    for line in (M.ERR_DEPTH_CAP, M.ERR_PER, M.ERR_BED_AND_REGION):
        assert line in inc and line in ddb, line
    assert ddb.index(M.ERR_DEPTH_CAP) < ddb.index(M.ERR_PER) < ddb.index(M.ERR_BED_AND_REGION) < ddb.index("bam_bind_file(")     # the order bind checks in
    assert inc.index(M.ERR_DEPTH_CAP) < inc.index(M.ERR_PER) < inc.index(M.ERR_BED_AND_REGION)
    assert M.ERR_NOT_OPEN in inc and M.ERR_BAM_NOT_OPEN in inc and M.ERR_SHARD in inc and M.ERR_BED_CTX in inc and M.ERR_BED_NOT_OPEN in inc
    assert M.err_hist(12, 8).replace("12", "%llu").replace(" 8 are", " %llu are") in inc
    # on the scaffold: the layout and the BED merge are shared, not copied; the state is the scaffold's two parts
    acc = source("dhts_bam_accum.inc")
    assert inc.count("dep_layout(c, S,") == 1 and inc.count("dep_bed_target_rows(c, b, S,") == 1 and "stable_sort" not in inc and "bam_depth_hist" in acc
    for shared in ("accum_batch_ok(", "accum_scan(", "accum_steps(", "dep_target_rows(", "dep_args(", "dep_stats_common(", "cols_reset(", "cols_host_bytes(", "cols_fetch("):
        assert shared in inc, shared
    assert "struct HistState : AccumBase, DepLayout {" in source("dhts_api.hip") and "HistState &S = c->dhi;" in inc
    # accumulate launches bam_depth's kernels, unchanged; the carry of the tile sums is reused
    assert "bam_depth_classify_del" in inc and "bam_depth_classify," in inc and "bam_depth_add_nowords<BQ, DEL>" in inc and "dep_tile_sum" in inc and "depth_carry<uint32_t>" in inc


def test_the_sources_are_part_of_the_build():
    import __graft_entry__ as ge
    deps = {os.path.basename(p) for p in ge.HIP_DEPS}
    assert {"bam_depth_hist.hip", "dhts_bam_depth_hist.inc", "duckdb_depth_hist.inc", "dhts_bam_accum.inc"} <= deps
    assert set(ENTRIES + OTHERS) <= set(ge.declared_exports())
    api, ext = source("dhts_api.hip"), source("duckdb_ext.cpp")
    assert api.index('#include "bam_depth_hist.hip"') > api.index('#include "bam_bedgraph.hip"')
    assert api.index('#include "dhts_bam_depth_hist.inc"') > api.index('#include "dhts_bam_bedgraph.inc"') > api.index('#include "dhts_bam_accum.inc"')
    assert ext.index('#include "duckdb_depth_hist.inc"') > ext.index('#include "duckdb_bedgraph.inc"')
    hip = source("bam_depth_hist.hip")
    assert '#include "bam_depth.hip"' in hip
    for kernel in ("dhi_hist", "dhi_group_count", "dhi_emit"):
        assert re.search(r"__global__ void __launch_bounds__\(256\) " + kernel + r"\(", hip), kernel
        assert kernel in source("dhts_bam_depth_hist.inc")


def test_registered_last_under_a_variable_of_its_own():
    ext = source("duckdb_ext.cpp")
    assert ext.index("register_bam_hist_function(conn)") > ext.index("register_bam_bedgraph_function(conn)") and 'getenv("DHTS_HIST_FUNCTIONS")' in ext

    def catalog(**kv):
        env = {k: x for k, x in os.environ.items() if not (k.startswith("DHTS_") and k.endswith("_FUNCTIONS"))}
        env.update(kv)
        return subprocess.run([HOST, duckhts_amd.LIB_PATH, "--catalog", "-"], capture_output=True, text=True, env=env).stdout.splitlines()

    default = catalog()
    assert default and not any("bam_depth_hist" in ln for ln in default)
    # absent under every value of every existing variable, whose sets are what they were
    existing = ("DHTS_SEQ_FUNCTIONS", "DHTS_INTERVAL_FUNCTIONS", "DHTS_NUC_FUNCTIONS", "DHTS_KMER_FUNCTIONS", "DHTS_TABIX_FUNCTIONS", "DHTS_COVERAGE_FUNCTIONS", "DHTS_DEPTH_FUNCTIONS",
                "DHTS_PERBASE_FUNCTIONS", "DHTS_PILEUP_FUNCTIONS", "DHTS_BEDGRAPH_FUNCTIONS")
    for var in existing:
        for v in ("0", "1", "2", "3"):
            assert not any("bam_depth_hist" in ln for ln in catalog(**{var: v})), (var, v)
    for v in ("0", "2", "true"):
        assert catalog(DHTS_HIST_FUNCTIONS=v) == default
    line = ("TF bam_depth_hist pushdown=1 bind=1 init=1 local_init=0 func=1 named=depth_cap:5,per:17,bed_path:17,region:17,index_path:17,min_read_len:5,min_mapq:5,"
            "min_baseq:5,include_deletions:1,include_flags:5,require_flags:5,exclude_flags:5")
    assert catalog(DHTS_HIST_FUNCTIONS="1") == default + [line]
    bdg = catalog(DHTS_BEDGRAPH_FUNCTIONS="1")
    both = catalog(DHTS_HIST_FUNCTIONS="1", DHTS_BEDGRAPH_FUNCTIONS="1")
    assert both == bdg + [line] and both[-2].startswith("TF bam_bedgraph ")                          # bam_bedgraph stays last but one
    # (the test host holds sixteen table functions: the sets below stay under that)
    others = dict(DHTS_BEDGRAPH_FUNCTIONS="1", DHTS_PILEUP_FUNCTIONS="1", DHTS_PERBASE_FUNCTIONS="1", DHTS_DEPTH_FUNCTIONS="1", DHTS_COVERAGE_FUNCTIONS="2", DHTS_KMER_FUNCTIONS="1")
    every = catalog(DHTS_HIST_FUNCTIONS="1", **others)
    assert every[-1] == line and every[:-1] == catalog(**others)
