"""The surface of bam_coverage without a device: the header declares the dhts_bam_coverage_* entries, the built library exports them, the
Python mirror binds them, and the structures of the two sides have one layout."""
import ctypes as C
import inspect
import os
import re
import subprocess

import duckhts_amd
from conftest import ROOT

ENTRIES = ["dhts_bam_coverage_open", "dhts_bam_coverage_accumulate", "dhts_bam_coverage_scan", "dhts_bam_coverage_stats", "dhts_bam_coverage_next",
           "dhts_bam_coverage_batch_host_bytes", "dhts_bam_coverage_batch_fetch"]
OTHERS = ["register_bam_coverage_function", "dhts_debug_coverage_max_table_bytes"]


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_the_header_declares_the_entries_and_the_contract():
    text = header("duckhts_amd.h")
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(dhts_bam_coverage_[a-z_]+)\s*\(", code))) == sorted(ENTRIES)
    for word in ("dhts_coverage_params", "dhts_coverage_stats", "dhts_coverage_batch", "DHTS_COVERAGE_MEANMAPQ", "DHTS_COVERAGE_SUM_MAPQ", "DHTS_COVERAGE_COL_COUNT"):
        assert word in code
    block = text[text.index("---- bam_coverage"):text.index("enum { DHTS_COVERAGE_CHROM")]
    for phrase in ("n_flag_filtered", "n_unplaced", "n_short", "n_low_mapq", "n_outside", "n_counted", "max(1, rlen)", "min_baseq", "min_read_len", "min_depth", "0x704",
                   "16 GiB", "32-bit", "bam_list", "reference / CRAM", "depth histogram", "max_depth", "overlap each other are refused"):
        assert phrase in block, phrase
    assert re.search(r"\bregister_bam_coverage_function\s*\(", header("duckhts_extension.h"))
    assert re.search(r"\bdhts_debug_coverage_max_table_bytes\s*\(\s*uint64_t", header("duckhts_amd_debug.h"))
    names = re.search(r"enum \{ (DHTS_COVERAGE_CHROM[^}]*)\}", code).group(1)
    assert [n.strip().split(" ")[0].replace("DHTS_COVERAGE_", "").lower() for n in names.split(",")][:-1] == duckhts_amd.COVERAGE_COLUMNS


def test_the_library_exports_the_entries():
    out = subprocess.run(["nm", "-D", "--defined-only", duckhts_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in ENTRIES + OTHERS:
        assert n in exported, n
    assert not [n for n in exported if "coverage" in n and n not in ENTRIES + OTHERS]


def test_the_python_mirror_binds_the_entries():
    L = duckhts_amd.lib()
    for n in ENTRIES:
        assert n in duckhts_amd.EXPORTS and getattr(L, n).argtypes, n
    for m in ("bam_coverage_open", "bam_coverage_accumulate", "bam_coverage_scan", "bam_coverage_stats", "bam_coverage_next"):
        assert callable(getattr(duckhts_amd.Context, m))
    assert duckhts_amd.COVERAGE_COLUMNS[:9] == ["chrom", "start", "end", "numreads", "covbases", "coverage", "meandepth", "meanbaseq", "meanmapq"]
    assert duckhts_amd.COVERAGE_COLUMNS[9:] == ["sum_depth", "sum_baseq", "sum_mapq"] and duckhts_amd.COVERAGE_DOUBLE_COLUMNS == (5, 6, 7, 8)
    assert duckhts_amd.COVERAGE_COLMASK & 0b1111111100000 == 0 and not duckhts_amd.COVERAGE_COLMASK & 1     # no string column in the scan (QNAME is bit 0)
    sig = inspect.signature(duckhts_amd.bam_coverage).parameters
    assert [sig[k].default for k in ("min_read_len", "min_mapq", "min_baseq", "include_flags", "require_flags", "exclude_flags", "min_depth", "region", "index")] == \
        [0, 0, 0, 0, 0, 0x704, 1, None, None]
    ctx_sig = inspect.signature(duckhts_amd.Context.bam_coverage_open).parameters                # the ABI's rule: the masks as given
    assert ctx_sig["exclude_flags"].default == 0 and ctx_sig["min_depth"].default == 1
    # the structures: field order and sizes of include/duckhts_amd.h
    fields = [f[0] for f in duckhts_amd.CoverageParams._fields_]
    assert C.sizeof(duckhts_amd.CoverageParams) == 40 and fields == ["min_read_len", "min_depth", "min_mapq", "min_baseq", "require_flags", "exclude_flags", "include_flags", "reserved"]
    assert C.sizeof(duckhts_amd.CoverageStats) == 80 and [f[0] for f in duckhts_amd.CoverageStats._fields_][:9] == \
        ["n_rows", "n_flag_filtered", "n_unplaced", "n_short", "n_low_mapq", "n_outside", "n_counted", "n_target_rows", "table_bytes"]
    code = re.sub(r"/\*.*?\*/", "", header("duckhts_amd.h"), flags=re.S)
    m = re.search(r"typedef struct \{([^}]*)\} dhts_coverage_params;", code)
    assert re.findall(r"\b(" + "|".join(fields) + r")\b", m.group(1)) == fields
    m = re.search(r"typedef struct \{([^}]*)\} dhts_coverage_stats;", code)
    assert re.findall(r"\b(n_[a-z_]+|table_bytes|status|reserved)\b", m.group(1)) == [f[0] for f in duckhts_amd.CoverageStats._fields_]


def test_the_sources_are_part_of_the_build():
    import __graft_entry__ as ge
    deps = {os.path.basename(p) for p in ge.HIP_DEPS}
    assert {"bam_coverage.hip", "dhts_bam_coverage.inc", "duckdb_coverage.inc"} <= deps
    assert "dhts_debug_coverage_max_table_bytes" in ge.declared_exports() and "register_bam_coverage_function" in ge.declared_exports()
    api = open(os.path.join(ROOT, "duckhts_amd", "csrc", "dhts_api.hip")).read()
    assert '#include "bam_coverage.hip"' in api and '#include "dhts_bam_coverage.inc"' in api
