"""The surface of bam_pileup without a device: the header declares the dhts_bam_pileup_* entries and states the contract, the built library
exports them, the Python mirror binds them, the structures of the two sides have one layout, and the sources are part of the build."""
import ctypes as C
import inspect
import os
import re
import subprocess

import bam_pileup_ref as M
import duckhts_amd
from conftest import ROOT

ENTRIES = ["dhts_bam_pileup_open", "dhts_bam_pileup_accumulate", "dhts_bam_pileup_scan", "dhts_bam_pileup_stats", "dhts_bam_pileup_next",
           "dhts_bam_pileup_batch_host_bytes", "dhts_bam_pileup_batch_fetch"]
OTHERS = ["register_bam_pileup_function", "dhts_debug_pileup_add_form"]


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def source(name):
    return open(os.path.join(ROOT, "duckhts_amd", "csrc", name)).read()


def test_the_header_declares_the_entries_and_the_contract():
    text = header("duckhts_amd.h")
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(dhts_bam_pileup_[a-z_]+)\s*\(", code))) == sorted(ENTRIES)
    for word in ("dhts_pileup_params", "dhts_pileup_stats", "dhts_pileup_batch", "DHTS_PILEUP_CHROM", "DHTS_PILEUP_POS", "DHTS_PILEUP_STRAND", "DHTS_PILEUP_NUCLEOTIDE",
                 "DHTS_PILEUP_COUNT", "DHTS_PILEUP_COL_COUNT"):
        assert word in code
    block = text[text.index("---- bam_pileup"):text.index("enum { DHTS_PILEUP_CHROM")]
    for phrase in ("A C G T N = - +", "include_deletions", "include_insertions", "distinguish_strands", "min_nucleotide_depth", "1-based", "0x704", "PileupParam",
                   "count twice", "no anchor", "not N", "leading or trailing D", "N and P operations never count", "reference / CRAM", "max_depth", "mate-overlap", "several files",
                   "a region per contig", "15.9 GB", "dhts_debug_coverage_max_table_bytes", "the count table needs N bytes (B per position of every row)",
                   'prefixed "bam_pileup:"', "FLAG & 16", "no BED"):
        assert phrase in block, phrase
    assert "1,048,576" in text[text.index("int dhts_bam_pileup_stats"):text.index("int dhts_bam_pileup_next")]            # the default page is stated
    ext = header("duckhts_extension.h")
    assert re.search(r"\bregister_bam_pileup_function\s*\(", ext) and "DHTS_PILEUP_FUNCTIONS=1" in ext
    assert re.search(r"\bint dhts_debug_pileup_add_form\s*\(\s*dhts_ctx \*\s*,\s*int form\)", header("duckhts_amd_debug.h"))
    names = re.search(r"enum \{ (DHTS_PILEUP_CHROM[^}]*)\}", code).group(1)
    assert [n.strip().split(" ")[0].replace("DHTS_PILEUP_", "").lower() for n in names.split(",")][:-1] == ["chrom", "pos", "strand", "nucleotide", "count"]


def test_the_library_exports_the_entries():
    out = subprocess.run(["nm", "-D", "--defined-only", duckhts_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in ENTRIES + OTHERS:
        assert n in exported, n
    assert not [n for n in exported if "pileup" in n and n not in ENTRIES + OTHERS]


def test_the_python_mirror_binds_the_entries():
    L = duckhts_amd.lib()
    for n in ENTRIES:
        assert n in duckhts_amd.EXPORTS and getattr(L, n).argtypes, n
    assert L.dhts_debug_pileup_add_form.argtypes
    for m in ("bam_pileup_open", "bam_pileup_accumulate", "bam_pileup_scan", "bam_pileup_stats", "bam_pileup_next"):
        assert callable(getattr(duckhts_amd.Context, m))
    assert duckhts_amd.PILEUP_COLUMNS == ["tid", "pos", "strand", "nucleotide", "count"] and [4, 8, 1, 1, 4] == [duckhts_amd.np.dtype(d).itemsize for d in duckhts_amd.PILEUP_DTYPES]
    assert duckhts_amd.PILEUP_SYMBOLS.decode() == M.SYMBOLS
    assert duckhts_amd.PILEUP_COLMASK == duckhts_amd.COVERAGE_COLMASK and not duckhts_amd.PILEUP_COLMASK & 1     # no string column in the scan (QNAME is bit 0)
    sig = inspect.signature(duckhts_amd.bam_pileup).parameters
    assert list(sig)[:7] == ["src", "region", "index", "max_blocks", "max_rows", "columns", "device"]
    assert {k: sig[k].default for k in M.DEFAULTS} == M.DEFAULTS                                   # the documented defaults
    assert [sig[k].default for k in ("region", "index", "max_blocks", "max_rows", "columns")] == [None, None, 0, 0, None]
    ctx_sig = inspect.signature(duckhts_amd.Context.bam_pileup_open).parameters                   # the ABI's rule: everything as given
    assert [ctx_sig[k].default for k in ("exclude_flags", "include_deletions", "include_insertions", "distinguish_strands", "min_nucleotide_depth")] == [0, 0, 0, 0, 1]
    # the structures: field order and sizes of include/duckhts_amd.h
    fields = [f[0] for f in duckhts_amd.PileupParams._fields_]
    assert C.sizeof(duckhts_amd.PileupParams) == 48 and fields == ["min_read_len", "min_mapq", "min_baseq", "require_flags", "exclude_flags", "include_flags", "include_deletions",
                                                                    "include_insertions", "distinguish_strands", "min_nucleotide_depth", "reserved"]
    sfields = [f[0] for f in duckhts_amd.PileupStats._fields_]
    assert C.sizeof(duckhts_amd.PileupStats) == 88 and sfields == ["n_rows", "n_flag_filtered", "n_unplaced", "n_short", "n_low_mapq", "n_outside", "n_counted", "n_target_rows",
                                                                   "table_bytes", "n_result_rows", "status", "reserved"]
    assert sfields[:7] == [f[0] for f in duckhts_amd.CoverageStats._fields_][:7]                  # the seven counters of dhts_coverage_stats
    code = re.sub(r"/\*.*?\*/", "", header("duckhts_amd.h"), flags=re.S)
    m = re.search(r"typedef struct \{([^}]*)\} dhts_pileup_params;", code)
    assert re.findall(r"\b(" + "|".join(fields) + r")\b", m.group(1)) == fields
    m = re.search(r"typedef struct \{([^}]*)\} dhts_pileup_stats;", code)
    assert re.findall(r"\b(n_[a-z_]+|table_bytes|status|reserved)\b", m.group(1)) == sfields
    m = re.search(r"int dhts_bam_pileup_open\(([^)]*)\)", code)
    assert [a.strip().split(" ")[-1].lstrip("*") for a in m.group(1).split(",")] == ["bam", "params"]
    m = re.search(r"int dhts_bam_pileup_next\(([^)]*)\)", code)
    assert [a.strip().split(" ")[-1].lstrip("*") for a in m.group(1).split(",")] == ["bam", "max_rows", "colmask", "out"]


def test_the_inc_states_the_errors_the_header_promises():
    inc, ddb, acc, chk = source("dhts_bam_pileup.inc"), source("duckdb_pileup.inc"), source("dhts_bam_accum.inc"), source("bam_filter_check.h")
    msgs = re.findall(r'"(bam_pileup[^"]+ [^"]*)"', inc)                                    # (every literal but the bare name dep_layout is given)
    assert msgs and all(m.startswith("bam_pileup: ") for m in msgs)
    # the six range checks are written once, in the header both translation units include: one format each, which give the promised lines;
    # the open and the bind call it with this function's name
    assert chk.count('"%s: min_read_len must be >= 0"') == 1 and chk.count('"%s: %s must be between 0 and %d"') == 1 and chk.count("must be") == 2
    for which, top in (("min_mapq", 255), ("min_baseq", 255), ("include_flags", 65535), ("require_flags", 65535), ("exclude_flags", 65535)):
        assert '{"%s", %s, %d, ' % (which, which, top) in chk
        assert "%s: %s must be between 0 and %d" % ("bam_pileup", which, top) == M.err_range(which)
    assert "%s: min_read_len must be >= 0" % "bam_pileup" == M.ERR_READ_LEN
    assert inc.count('bam_filter_check(m, "bam_pileup", p->min_read_len, ') == 1 and ddb.count('bam_filter_check(m, "bam_pileup", min_read_len, ') == 1
    assert M.ERR_MIN_DEPTH in inc and M.ERR_MIN_DEPTH in ddb
    for which in ("include_deletions", "include_insertions", "distinguish_strands"):
        assert M.err_switch(which) in inc
    assert M.ERR_NOT_OPEN in inc and M.ERR_BAM_NOT_OPEN in inc and M.ERR_SHARD in inc and M.ERR_PATH in ddb
    # the stale-batch error: the scaffold's format, written once, with this function's name and what it reads where the scan left it
    stale = '"%s: the batch is not the one dhts_bam_next_batch returned last on this context (%s)"'
    assert acc.count(stale) == 1 and (stale[1:-1] % ("bam_pileup", "")).startswith(M.ERR_STALE)
    assert 'accum_batch_ok(c, PILEUP_WHO, S, b, false, "CIGAR, SEQ and QUAL are read where the scan left them")' in inc and 'PILEUP_WHO = {"bam_pileup", ' in inc
    # the layout is shared, not copied: the opens call dep_layout, and the overlap and the cap errors are written once, with the table's noun
    cov = source("dhts_bam_coverage.inc")
    assert inc.count("dep_layout(c, S,") == 1 and '"count table"' in inc and (acc + cov + inc).count("overlap (one row is answered per region") == 1
    assert (acc + cov + inc).count("per position of every row") == 1 and "per position of every row" in acc and 'noun = "depth table"' in acc


def test_the_sources_are_part_of_the_build():
    import __graft_entry__ as ge
    deps = {os.path.basename(p) for p in ge.HIP_DEPS}
    assert {"bam_pileup.hip", "dhts_bam_pileup.inc", "duckdb_pileup.inc", "dhts_bam_accum.inc", "bam_filter_check.h"} <= deps
    assert set(ENTRIES + OTHERS) <= set(ge.declared_exports())
    api = source("dhts_api.hip")
    assert '#include "bam_pileup.hip"' in api and api.index('#include "dhts_bam_pileup.inc"') > api.index('#include "dhts_bam_depth.inc"') > api.index('#include "dhts_bam_accum.inc"')
    ext = source("duckdb_ext.cpp")
    assert ext.index('#include "duckdb_pileup.inc"') > ext.index('#include "duckdb_depth.inc"')
    assert ext.index("register_bam_pileup_function(conn)") > ext.index("register_bam_depth_function(conn)")              # registered last
    assert '#include "bam_depth.hip"' in source("bam_pileup.hip") and "bam_depth_classify_del" in source("dhts_bam_pileup.inc")
