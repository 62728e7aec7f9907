"""The surface of bam_bedgraph without a device: the header declares the dhts_bam_bedgraph_* entries and states the contract, the built library
exports them, the Python mirror binds them, the structures of the two sides have one layout, the sources are part of the build, and the error
lines the header promises stand in both parts."""
import ctypes as C
import inspect
import os
import re
import subprocess

import bam_bedgraph_ref as M
import duckhts_amd
from conftest import ROOT

ENTRIES = ["dhts_bam_bedgraph_open", "dhts_bam_bedgraph_accumulate", "dhts_bam_bedgraph_scan", "dhts_bam_bedgraph_stats", "dhts_bam_bedgraph_next",
           "dhts_bam_bedgraph_batch_host_bytes", "dhts_bam_bedgraph_batch_fetch"]
OTHERS = ["register_bam_bedgraph_function"]


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def source(name):
    return open(os.path.join(ROOT, "duckhts_amd", "csrc", name)).read()


def test_the_header_declares_the_entries_and_the_contract():
    text = header("duckhts_amd.h")
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(dhts_bam_bedgraph_[a-z_]+)\s*\(", code))) == sorted(ENTRIES)
    for word in ("dhts_bedgraph_params", "dhts_bedgraph_stats", "dhts_bedgraph_batch", "DHTS_BEDGRAPH_CHROM", "DHTS_BEDGRAPH_START", "DHTS_BEDGRAPH_END", "DHTS_BEDGRAPH_DEPTH",
                 "DHTS_BEDGRAPH_COL_COUNT"):
        assert word in code
    block = text[text.index("---- bam_bedgraph"):text.index("enum { DHTS_BEDGRAPH_CHROM")]
    for phrase in ("zero_runs", "breaks", "strictly increasing", "the number of breaks <= d", "breaks[j - 1]", "maximal stretch", "never spans two target rows", "0-based", "exclusive",
                   "No column is ever NULL", "all_positions = 2", "all_positions = 0", "no counterpart of all_positions = 1", "include_deletions", "n_bed_skipped", "0x704",
                   "refused by name", "dhts_debug_coverage_max_table_bytes", "1,024 slots", "suppress_overlaps", "several input files", "reference / CRAM", "histogram",
                   "mean depth per class run", 'prefixed "bam_bedgraph:"', "(chrom, 0, L, 0)"):
        assert phrase in block, phrase
    assert "1,048,576" in text[text.index("int dhts_bam_bedgraph_stats"):text.index("int dhts_bam_bedgraph_next")]            # the default page is stated
    ext = header("duckhts_extension.h")
    assert re.search(r"\bregister_bam_bedgraph_function\s*\(", ext) and "DHTS_BEDGRAPH_FUNCTIONS=1" in ext and "DHTS_BEDGRAPH_PAGE_ROWS" in ext
    names = re.search(r"enum \{ (DHTS_BEDGRAPH_CHROM[^}]*)\}", code).group(1)
    assert [n.strip().split(" ")[0].replace("DHTS_BEDGRAPH_", "").lower() for n in names.split(",")][:-1] == ["chrom", "start", "end", "depth"]
    # bam_depth's block no longer calls the run-length form missing: it names the function that has it
    depth_block = text[text.index("---- bam_depth"):text.index("enum { DHTS_DEPTH_CHROM")]
    assert "bedGraph" in depth_block and "bam_bedgraph" in depth_block


def test_the_library_exports_the_entries():
    out = subprocess.run(["nm", "-D", "--defined-only", duckhts_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in ENTRIES + OTHERS:
        assert n in exported, n
    assert not [n for n in exported if ("bam_bedgraph" in n or "bdg_" in n) and n not in ENTRIES + OTHERS]


def test_the_python_mirror_binds_the_entries():
    L = duckhts_amd.lib()
    for n in ENTRIES:
        assert n in duckhts_amd.EXPORTS and getattr(L, n).argtypes, n
    for m in ("bam_bedgraph_open", "bam_bedgraph_accumulate", "bam_bedgraph_scan", "bam_bedgraph_stats", "bam_bedgraph_next"):
        assert callable(getattr(duckhts_amd.Context, m))
    assert duckhts_amd.BEDGRAPH_COLUMNS == ["tid", "start", "end", "depth"] and [4, 8, 8, 4] == [duckhts_amd.np.dtype(d).itemsize for d in duckhts_amd.BEDGRAPH_DTYPES]
    assert duckhts_amd.BEDGRAPH_COLMASK == duckhts_amd.DEPTH_COLMASK and not duckhts_amd.BEDGRAPH_COLMASK & 1      # no string column in the scan (QNAME is bit 0)
    sig = inspect.signature(duckhts_amd.bam_bedgraph).parameters
    assert list(sig)[:8] == ["src", "region", "index", "bed", "max_blocks", "max_rows", "columns", "device"]
    assert [sig[k].default for k in ("region", "index", "bed", "max_blocks", "max_rows", "columns", "device", "min_read_len", "min_mapq", "min_baseq", "include_flags", "require_flags",
                                     "exclude_flags", "include_deletions", "zero_runs", "breaks")] == [None, None, None, 0, 0, None, 0, 0, 0, 0, 0, 0, 0x704, 0, 0, None]
    ctx_sig = inspect.signature(duckhts_amd.Context.bam_bedgraph_open).parameters                    # the ABI's rule: the masks as given
    assert ctx_sig["exclude_flags"].default == 0 and ctx_sig["bed_ctx"].default is None and ctx_sig["breaks"].default is None
    # the structures: field order and sizes of include/duckhts_amd.h
    fields = [f[0] for f in duckhts_amd.BedgraphParams._fields_]
    assert C.sizeof(duckhts_amd.BedgraphParams) == 112 and fields == ["min_read_len", "min_mapq", "min_baseq", "require_flags", "exclude_flags", "include_flags", "include_deletions",
                                                                      "zero_runs", "n_breaks", "breaks", "reserved"]
    assert duckhts_amd.BedgraphParams.breaks.offset == 40 and duckhts_amd.BedgraphParams.breaks.size == 64 and duckhts_amd.BedgraphParams.reserved.offset == 104
    assert fields[:7] == [f[0] for f in duckhts_amd.DepthParams._fields_][:7]                       # the depth filter fields and include_deletions
    sfields = [f[0] for f in duckhts_amd.BedgraphStats._fields_]
    assert C.sizeof(duckhts_amd.BedgraphStats) == 96 and sfields == ["n_rows", "n_flag_filtered", "n_unplaced", "n_short", "n_low_mapq", "n_outside", "n_counted", "n_target_rows",
                                                                     "n_bed_skipped", "table_bytes", "n_runs", "status", "reserved"]
    assert sfields[:7] == [f[0] for f in duckhts_amd.CoverageStats._fields_][:7]                  # the seven counters of dhts_coverage_stats
    code = re.sub(r"/\*.*?\*/", "", header("duckhts_amd.h"), flags=re.S)
    m = re.search(r"typedef struct \{([^}]*)\} dhts_bedgraph_params;", code)
    assert re.findall(r"\b(" + "|".join(fields) + r")\b", m.group(1)) == fields and "int32_t breaks[16];" in m.group(1) and "int32_t reserved[2];" in m.group(1)
    m = re.search(r"typedef struct \{([^}]*)\} dhts_bedgraph_stats;", code)
    assert re.findall(r"\b(n_[a-z_]+|table_bytes|status|reserved)\b", m.group(1)) == sfields
    m = re.search(r"int dhts_bam_bedgraph_open\(([^)]*)\)", code)
    assert [a.strip().split(" ")[-1].lstrip("*") for a in m.group(1).split(",")] == ["bam", "params", "bed"]
    m = re.search(r"int dhts_bam_bedgraph_next\(([^)]*)\)", code)
    assert [a.strip().split(" ")[-1].lstrip("*") for a in m.group(1).split(",")] == ["bam", "max_rows", "colmask", "out"]


def test_both_parts_state_the_errors_the_header_promises():
    inc, ddb, acc = source("dhts_bam_bedgraph.inc"), source("duckdb_bedgraph.inc"), source("dhts_bam_accum.inc")
    msgs = re.findall(r'"(bam_bedgraph[^"]+ [^"]*)"', inc)                                  # (every literal but the bare name dep_layout is given)
    assert msgs and all(m.startswith("bam_bedgraph: ") for m in msgs)
    assert inc.count('bam_filter_check(m, "bam_bedgraph", p->min_read_len, ') == 1 and ddb.count('bam_filter_check(m, "bam_bedgraph", min_read_len, ') == 1
    for line in (M.ERR_ZERO_RUNS, M.ERR_DELETIONS):                                         # (the table function takes the two as BOOLEAN)
        assert line in inc
    for line in (M.ERR_MANY_BREAKS, M.ERR_BREAKS, M.ERR_BED_AND_REGION):
        assert line in inc and line in ddb, line
    assert M.ERR_NOT_OPEN in inc and M.ERR_BAM_NOT_OPEN in inc and M.ERR_SHARD in inc
    # on the scaffold: the layout and the BED merge are shared, not copied; the state is the scaffold's three parts
    dep = source("dhts_bam_depth.inc")
    assert inc.count("dep_layout(c, S,") == 1 and acc.count("static int dep_bed_target_rows(") == 1 and inc.count("dep_bed_target_rows(c, b, S,") == 1 and dep.count("dep_bed_target_rows(c, b, S,") == 1
    assert "stable_sort" not in inc and "stable_sort" not in dep
    assert "struct BedgraphState : AccumBase, DepLayout, DepPager {" in source("dhts_api.hip") and "BedgraphState &S = c->bdg;" in inc
    # accumulate launches bam_depth's kernels, unchanged
    assert "bam_depth_classify_del" in inc and "bam_depth_classify," in inc and "bam_depth_add_nowords<BQ, DEL>" in inc


def test_the_sources_are_part_of_the_build():
    import __graft_entry__ as ge
    deps = {os.path.basename(p) for p in ge.HIP_DEPS}
    assert {"bam_bedgraph.hip", "dhts_bam_bedgraph.inc", "duckdb_bedgraph.inc", "dhts_bam_accum.inc", "bam_filter_check.h"} <= deps
    assert "register_bam_bedgraph_function" in ge.declared_exports() and set(ENTRIES) <= set(ge.declared_exports())
    api, ext = source("dhts_api.hip"), source("duckdb_ext.cpp")
    assert api.index('#include "bam_bedgraph.hip"') > api.index('#include "bam_pileup.hip"')
    assert api.index('#include "dhts_bam_bedgraph.inc"') > api.index('#include "dhts_bam_pileup.inc"') > api.index('#include "dhts_bam_accum.inc"')
    assert ext.index('#include "duckdb_bedgraph.inc"') > ext.index('#include "duckdb_pileup.inc"')
    assert ext.index("register_bam_bedgraph_function(conn)") > ext.index("register_bam_pileup_function(conn)") and 'getenv("DHTS_BEDGRAPH_FUNCTIONS")' in ext
    hip = source("bam_bedgraph.hip")
    assert '#include "bam_depth.hip"' in hip
    for kernel in ("bdg_tile_count", "bdg_emit"):
        assert re.search(r"__global__ void __launch_bounds__\(256\) " + kernel + r"\(", hip), kernel
        assert kernel in source("dhts_bam_bedgraph.inc")
    # the suffix minimum is the shared carry in its reverse / min form: the three kernels of dev_scan.hip, one launcher, no copy of them left
    scan = source("dev_scan.hip")
    for kernel in ("carry_reduce", "carry_scan", "carry_apply"):
        assert re.search(r"template <[^>]*> __global__ void __launch_bounds__\(256\) " + kernel + r"\(", scan), kernel
        assert source("dhts_bam_accum.inc").count("(" + kernel + "<T, Op, ") == 1
    assert source("dhts_bam_bedgraph.inc").count("scan_carry<unsigned long long, ScanMin, true>(c, S.part, (unsigned long long *)S.tnext.p, ntiles, (unsigned long long)S.slots)") == 1
    csrc = os.path.join(ROOT, "duckhts_amd", "csrc")
    assert not [f for f in sorted(os.listdir(csrc)) if "bdg_suffix_" in source(f)]
