"""The surface of bam_depth without a device: the header declares the dhts_bam_depth_* entries and states the contract, the built library
exports them, the Python mirror binds them, the structures of the two sides have one layout, and the sources are part of the build."""
import ctypes as C
import inspect
import os
import re
import subprocess

import duckhts_amd
from conftest import ROOT

ENTRIES = ["dhts_bam_depth_open", "dhts_bam_depth_accumulate", "dhts_bam_depth_scan", "dhts_bam_depth_stats", "dhts_bam_depth_next",
           "dhts_bam_depth_batch_host_bytes", "dhts_bam_depth_batch_fetch"]
OTHERS = ["register_bam_depth_function"]


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def source(name):
    return open(os.path.join(ROOT, "duckhts_amd", "csrc", name)).read()


def test_the_header_declares_the_entries_and_the_contract():
    text = header("duckhts_amd.h")
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(dhts_bam_depth_[a-z_]+)\s*\(", code))) == sorted(ENTRIES)
    for word in ("dhts_depth_params", "dhts_depth_stats", "dhts_depth_batch", "DHTS_DEPTH_CHROM", "DHTS_DEPTH_POS", "DHTS_DEPTH_DEPTH", "DHTS_DEPTH_COL_COUNT"):
        assert word in code
    block = text[text.index("---- bam_depth"):text.index("enum { DHTS_DEPTH_CHROM")]
    for phrase in ("include_deletions", "all_positions", "touched", "1-based", "n_bed_skipped", "at least 4 KiB", "1,024 slots", "0x704", "suppress_overlaps", "reference / CRAM",
                   "max_depth", "bedGraph", "several input files", "dhts_debug_coverage_max_table_bytes", "refused by name", 'prefixed "bam_depth:"', "N and P never count",
                   "leading or trailing D"):
        assert phrase in block, phrase
    assert "1,048,576" in text[text.index("int dhts_bam_depth_stats"):text.index("int dhts_bam_depth_next")]            # the default page is stated
    assert re.search(r"\bregister_bam_depth_function\s*\(", header("duckhts_extension.h")) and "DHTS_PERBASE_FUNCTIONS=1" in header("duckhts_extension.h")
    names = re.search(r"enum \{ (DHTS_DEPTH_CHROM[^}]*)\}", code).group(1)
    assert [n.strip().split(" ")[0].replace("DHTS_DEPTH_", "").lower() for n in names.split(",")][:-1] == ["chrom", "pos", "depth"]


def test_the_library_exports_the_entries():
    out = subprocess.run(["nm", "-D", "--defined-only", duckhts_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in ENTRIES + OTHERS:
        assert n in exported, n
    assert not [n for n in exported if "bam_depth" in n and n not in ENTRIES + OTHERS]


def test_the_python_mirror_binds_the_entries():
    L = duckhts_amd.lib()
    for n in ENTRIES:
        assert n in duckhts_amd.EXPORTS and getattr(L, n).argtypes, n
    for m in ("bam_depth_open", "bam_depth_accumulate", "bam_depth_scan", "bam_depth_stats", "bam_depth_next"):
        assert callable(getattr(duckhts_amd.Context, m))
    assert duckhts_amd.DEPTH_COLUMNS == ["tid", "pos", "depth"] and [C.sizeof(C.c_int32), 8, 4] == [duckhts_amd.np.dtype(d).itemsize for d in duckhts_amd.DEPTH_DTYPES]
    assert duckhts_amd.DEPTH_COLMASK == duckhts_amd.COVERAGE_COLMASK and not duckhts_amd.DEPTH_COLMASK & 1      # no string column in the scan (QNAME is bit 0)
    sig = inspect.signature(duckhts_amd.bam_depth).parameters
    assert list(sig)[:7] == ["src", "region", "index", "bed", "max_blocks", "max_rows", "columns"]
    assert [sig[k].default for k in ("region", "index", "bed", "max_blocks", "max_rows", "columns", "min_read_len", "min_mapq", "min_baseq", "include_flags", "require_flags",
                                     "exclude_flags", "include_deletions", "all_positions")] == [None, None, None, 0, 0, None, 0, 0, 0, 0, 0, 0x704, 0, 0]
    ctx_sig = inspect.signature(duckhts_amd.Context.bam_depth_open).parameters                    # the ABI's rule: the masks as given
    assert ctx_sig["exclude_flags"].default == 0 and ctx_sig["bed_ctx"].default is None
    # the structures: field order and sizes of include/duckhts_amd.h
    fields = [f[0] for f in duckhts_amd.DepthParams._fields_]
    assert C.sizeof(duckhts_amd.DepthParams) == 40 and fields == ["min_read_len", "min_mapq", "min_baseq", "require_flags", "exclude_flags", "include_flags", "include_deletions",
                                                                   "all_positions", "reserved"]
    sfields = [f[0] for f in duckhts_amd.DepthStats._fields_]
    assert C.sizeof(duckhts_amd.DepthStats) == 96 and sfields == ["n_rows", "n_flag_filtered", "n_unplaced", "n_short", "n_low_mapq", "n_outside", "n_counted", "n_target_rows",
                                                                  "n_bed_skipped", "table_bytes", "n_positions", "status", "reserved"]
    assert sfields[:7] == [f[0] for f in duckhts_amd.CoverageStats._fields_][:7]                  # the seven counters of dhts_coverage_stats
    code = re.sub(r"/\*.*?\*/", "", header("duckhts_amd.h"), flags=re.S)
    m = re.search(r"typedef struct \{([^}]*)\} dhts_depth_params;", code)
    assert re.findall(r"\b(" + "|".join(fields) + r")\b", m.group(1)) == fields
    m = re.search(r"typedef struct \{([^}]*)\} dhts_depth_stats;", code)
    assert re.findall(r"\b(n_[a-z_]+|table_bytes|status|reserved)\b", m.group(1)) == sfields
    m = re.search(r"int dhts_bam_depth_open\(([^)]*)\)", code)
    assert [a.strip().split(" ")[-1].lstrip("*") for a in m.group(1).split(",")] == ["bam", "params", "bed"]
    m = re.search(r"int dhts_bam_depth_next\(([^)]*)\)", code)
    assert [a.strip().split(" ")[-1].lstrip("*") for a in m.group(1).split(",")] == ["bam", "max_rows", "colmask", "out"]


def test_the_inc_states_the_errors_the_header_promises():
    inc, ddb, acc, chk = source("dhts_bam_depth.inc"), source("duckdb_depth.inc"), source("dhts_bam_accum.inc"), source("bam_filter_check.h")
    msgs = re.findall(r'"(bam_depth[^"]+ [^"]*)"', inc)                                     # (every literal but the bare name dep_layout is given)
    assert msgs and all(m.startswith("bam_depth: ") for m in msgs)
    # the six range checks are written once, in the header both translation units include: one format each, which give the promised lines;
    # the open and the bind call it with this function's name
    assert chk.count('"%s: min_read_len must be >= 0"') == 1 and chk.count('"%s: %s must be between 0 and %d"') == 1 and chk.count("must be") == 2
    for which, top in (("min_mapq", 255), ("min_baseq", 255), ("include_flags", 65535), ("require_flags", 65535), ("exclude_flags", 65535)):
        assert '{"%s", %s, %d, ' % (which, which, top) in chk
        assert "%s: %s must be between 0 and %d" % ("bam_depth", which, top) == f"bam_depth: {which} must be between 0 and {255 if which.startswith('min_') else 65535}"
    assert "%s: min_read_len must be >= 0" % "bam_depth" == "bam_depth: min_read_len must be >= 0"
    assert inc.count('bam_filter_check(m, "bam_depth", p->min_read_len, ') == 1 and ddb.count('bam_filter_check(m, "bam_depth", min_read_len, ') == 1
    line = "bam_depth: a BED and regions cannot be combined (give the target rows one way)"
    assert line in inc and line in ddb
    assert "bam_depth: suppress_overlaps is not supported (mates are not paired on the device)" in ddb
    # the layout is shared, not copied: bam_coverage's open and bam_depth's both call dep_layout, and the overlap error is written once
    cov = source("dhts_bam_coverage.inc")
    assert acc.count("static int dep_layout(") == 1 and cov.count("dep_layout(c, S,") == 1 and inc.count("dep_layout(c, S,") == 1
    assert (acc + cov + inc).count("overlap (one row is answered per region") == 1 and "overlap (one row is answered per region" in acc
    assert "rbase" not in inc.split("int dhts_bam_depth_accumulate")[0]


def test_the_sources_are_part_of_the_build():
    import __graft_entry__ as ge
    deps = {os.path.basename(p) for p in ge.HIP_DEPS}
    assert {"bam_depth.hip", "dhts_bam_depth.inc", "duckdb_depth.inc"} <= deps
    assert "register_bam_depth_function" in ge.declared_exports() and set(ENTRIES) <= set(ge.declared_exports())
    api, ext = source("dhts_api.hip"), source("duckdb_ext.cpp")
    assert '#include "bam_depth.hip"' in api and '#include "dhts_bam_depth.inc"' in api
    # the scaffold of the five count functions and the shared range checks: built, and included in front of the first of them
    assert {"dhts_bam_accum.inc", "bam_filter_check.h"} <= deps
    assert api.index('#include "dhts_fasta_nuc.inc"') < api.index('#include "dhts_bam_accum.inc"') < api.index('#include "dhts_bam_bins.inc"')
    assert '#include "bam_filter_check.h"' in api and '#include "bam_filter_check.h"' in ext
    for name, fn in (("bins", "bam_bin_counts"), ("bedcov", "bam_bedcov"), ("coverage", "bam_coverage"), ("depth", "bam_depth"), ("pileup", "bam_pileup")):
        assert source(f"dhts_bam_{name}.inc").count(f'bam_filter_check(m, "{fn}", ') == 1 and source(f"duckdb_{name}.inc").count(f'bam_filter_check(m, "{fn}", ') == 1
    assert ext.index('#include "duckdb_depth.inc"') > ext.index('#include "duckdb_coverage.inc"')
    assert '#include "bam_coverage.hip"' in source("bam_depth.hip")
    # bam_coverage launches what it launched: the two instantiations of bam_depth_add; its result takes the carry in two levels like the
    # others, and the single-workgroup carry is gone
    cov = source("dhts_bam_coverage.inc")
    assert "bam_depth_add<true>" in cov and "bam_depth_add<false>" in cov and "depth_carry<uint32_t>" in cov and "nowords" not in cov
    csrc = os.path.join(ROOT, "duckhts_amd", "csrc")
    assert not [f for f in sorted(os.listdir(csrc)) if "dep_tile_carry" in source(f)]


def test_the_workgroup_scan_through_lds_is_written_once():
    """the Hillis-Steele loop over the 256 or 1,024 threads of a workgroup stands in dev_scan.hip alone: every count kernel and the record
    stage call block_scan (the wave-level loops, d < 64, are other algorithms and stay where they are)"""
    csrc = os.path.join(ROOT, "duckhts_amd", "csrc")
    loop = re.compile(r"for \((?:uint32_t|int) d = 1; d < (?:256|1024|NT)")
    assert [f for f in sorted(os.listdir(csrc)) if loop.search(source(f))] == ["dev_scan.hip"]
    assert len(loop.findall(source("dev_scan.hip"))) == 1 and "block_scan(T v, T *sh)" in source("dev_scan.hip")
    for f in sorted(os.listdir(csrc)):
        assert not re.search(r"\b(dep_block_scan|depc_block_scan|bdg_block_scan_min|cov_block_scan|dep_carry_|cov_scan_|DEPC_)", source(f)), f
