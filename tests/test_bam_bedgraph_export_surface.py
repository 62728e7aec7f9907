"""The surface of bam_bedgraph_export without a device: the header declares the entry and states the contract (the identity, the failure codes,
what is out of scope), the debug header declares the hooks, the built library exports them, the Python mirror binds them with the structures'
layout, the sources are part of the build, and the table function is registered last behind a variable of its own."""
import ctypes as C
import inspect
import os
import re
import subprocess

import bam_bedgraph_export_ref as X
import duckhts_amd
from conftest import ROOT

ENTRY = "dhts_bedgraph_export"
HOOKS = ["dhts_debug_rows_text", "dhts_debug_rows_text_paths", "dhts_debug_export_limits"]
REGISTER = "register_bedgraph_export_function"


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def source(name):
    return open(os.path.join(ROOT, "duckhts_amd", "csrc", name)).read()


def test_the_header_declares_the_entry_and_states_the_contract():
    text = header("duckhts_amd.h")
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int dhts_bedgraph_export\(([^)]*)\)", code)
    assert m and [a.strip().split(" ")[-1].lstrip("*") for a in m.group(1).split(",")] == ["bam", "out_path", "p", "out"]
    block = text[text.index("---- bam_bedgraph_export"):text.index("int dhts_bedgraph_export(")]
    # the identity
    for phrase in ("The identity that defines correctness", "equal what dhts_bgzip_file makes of the plain text of the same rows at the same", "whatever the page size and the chunk size",
                   "blocks of 0xff00 bytes of the row stream, the last one short", "the encoder compresses every block on its own"):
        assert phrase in block, phrase
    # the failure codes and the cleanup
    for phrase in ("-3 an output cannot be opened", "-5 write error", "-6 out_path exists and overwrite is 0", "-7 the regions are not in file order", "-8 the index could not be built",
                   "neither output file is left", 'prefix "bam_bedgraph_export:"', "the next dhts_bam_bedgraph_next returns page one"):
        assert phrase in block, phrase
    # the index, the empty result, what is out of scope
    for phrase in ("dhts_tabix_build_index", "BED preset", "0-based half-open", "columns 1 / 2 / 3", "dhts_bgzf_wrap", "each contig's rows together and ascending", "28-byte EOF block",
                   "without a", "Not in this contract", "building the index from the row arrays without reading the file back", "bam_bin_counts", "up to 8 integer columns",
                   "without a result row crossing PCIe", "10.5.4 / 10.7.4"):
        assert phrase in block, phrase
    for word in ("dhts_bedgraph_export_params", "dhts_bedgraph_export_stats"):
        assert word in code
    dbg = re.sub(r"/\*.*?\*/", "", header("duckhts_amd_debug.h"), flags=re.S)
    for n in HOOKS:
        assert re.search(r"\b" + n + r"\s*\(", dbg), n
    ext = header("duckhts_extension.h")
    assert re.search(r"\b" + REGISTER + r"\s*\(", ext) and "DHTS_EXPORT_FUNCTIONS=1" in ext and "index_path VARCHAR (NULL for 'none')" in ext


def test_the_library_exports_the_entry_and_the_hooks():
    out = subprocess.run(["nm", "-D", "--defined-only", duckhts_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in [ENTRY, REGISTER] + HOOKS:
        assert n in exported, n
    assert not [n for n in exported if "rtx_" in n or "rows_text_encode" in n]              # the kernels and the launcher stay local


def test_the_python_mirror_binds_them():
    L = duckhts_amd.lib()
    assert ENTRY in duckhts_amd.EXPORTS and L.dhts_bedgraph_export.argtypes and len(L.dhts_debug_rows_text.argtypes) == 11
    for m in ("bam_bedgraph_export", "debug_rows_text", "debug_export_limits"):
        assert callable(getattr(duckhts_amd.Context, m))
    sig = inspect.signature(duckhts_amd.Context.bam_bedgraph_export).parameters
    assert list(sig) == ["self", "out_path", "index", "level", "min_shift", "overwrite"]
    assert [sig[k].default for k in ("index", "level", "min_shift", "overwrite")] == ["tbi", -1, 0, False]
    sig = inspect.signature(duckhts_amd.bam_bedgraph_export).parameters
    assert list(sig)[:6] == ["src", "out_path", "index", "level", "min_shift", "overwrite"]
    same = ("region", "bed", "max_blocks", "device", "min_read_len", "min_mapq", "min_baseq", "include_flags", "require_flags", "exclude_flags", "include_deletions", "zero_runs", "breaks")
    theirs = inspect.signature(duckhts_amd.bam_bedgraph).parameters
    assert all(sig[k].default == theirs[k].default for k in same) and sig["exclude_flags"].default == 0x704
    assert duckhts_amd.BEDGRAPH_EXPORT_INDEX == {"none": 0, "tbi": 1, "csi": 2} and tuple(sorted(duckhts_amd.BEDGRAPH_EXPORT_INDEX)) == tuple(sorted(X.INDEX_KINDS))
    # the structures: field order and sizes of include/duckhts_amd.h
    code = re.sub(r"/\*.*?\*/", "", header("duckhts_amd.h"), flags=re.S)
    pf = [f[0] for f in duckhts_amd.BedgraphExportParams._fields_]
    assert C.sizeof(duckhts_amd.BedgraphExportParams) == 32 and pf == ["level", "index", "min_shift", "overwrite", "reserved"]
    m = re.search(r"typedef struct \{([^}]*)\} dhts_bedgraph_export_params;", code)
    assert re.findall(r"\b(" + "|".join(pf) + r")\b", m.group(1)) == pf and "int32_t reserved[4];" in m.group(1)
    sf = [f[0] for f in duckhts_amd.BedgraphExportStats._fields_]
    assert C.sizeof(duckhts_amd.BedgraphExportStats) == 40 and sf == ["n_rows", "bytes_text", "bytes_out", "bytes_index", "status", "reserved"]
    m = re.search(r"typedef struct \{([^}]*)\} dhts_bedgraph_export_stats;", code)
    assert re.findall(r"\b(" + "|".join(sf) + r")\b", m.group(1)) == sf
    hip = source("rows_text.hip")
    assert f"#define RTX_LDS_BYTES {duckhts_amd.ROWS_TEXT_LDS_BYTES}u" in hip


def test_the_sources_are_part_of_the_build_and_the_errors_stand_in_them():
    import __graft_entry__ as ge
    deps = {os.path.basename(p) for p in ge.HIP_DEPS}
    assert {"rows_text.hip", "dhts_bam_bedgraph_export.inc", "duckdb_bedgraph_export.inc", "dev_scan.hip"} <= deps
    assert {ENTRY, REGISTER} | set(HOOKS) <= set(ge.declared_exports())
    api, ext = source("dhts_api.hip"), source("duckdb_ext.cpp")
    assert api.index('#include "rows_text.hip"') > api.index('#include "bam_bedgraph.hip"')
    assert api.index('#include "dhts_bam_bedgraph_export.inc"') > api.index('#include "dhts_bam_bedgraph.inc"')
    assert ext.index('#include "duckdb_bedgraph_export.inc"') > ext.index('#include "duckdb_depth_hist.inc"')
    # registered last, behind a variable of its own
    line = 'if (const char *e = getenv("DHTS_EXPORT_FUNCTIONS")) if (atoi(e) == 1) register_bedgraph_export_function(conn);'
    assert ext.count(line) == 1 and ext.index(line) > ext.index("register_bam_hist_function(conn)") and ext.count("DHTS_EXPORT_FUNCTIONS") == 2
    assert ext.index(line) < ext.index("duckdb_disconnect") and "register_" not in ext[ext.index(line) + len(line):ext.index("duckdb_disconnect")]
    # the encoder: its own lengths and write kernels, the shared scan and carry and no third one
    hip, inc = source("rows_text.hip"), source("dhts_bam_bedgraph_export.inc")
    assert '#include "dev_scan.hip"' in hip
    for kernel in ("rtx_lengths", "rtx_write"):
        assert re.search(r"__global__ void __launch_bounds__\(256\) " + kernel + r"\(", hip) and kernel in inc, kernel
    assert inc.count("depth_carry<unsigned long long>(c, part, (unsigned long long *)off.p, n)") == 1 and "uint4" in hip and "__shared__" in hip
    assert not re.search(r"for \((?:uint32_t|int) d = 1; d <", hip)
    # the page is bam_bedgraph's own, and the compressor and the tabix writer are the existing ones
    assert inc.count("bedgraph_page(c, page_rows,") == 1 and source("dhts_bam_bedgraph.inc").count("bedgraph_page(c, max_rows, colmask, dst, &nrows, &last)") == 1
    assert "bgzf_compress_device(c, m, level, &ol, in + done)" in inc and "dhts_tabix_build_index(x, 0x10000, 1, 2, 3, '#', 0, min_shift)" in inc and "dhts_bgzf_wrap(" in inc
    msgs = re.findall(r'"(bam_bedgraph_export[^"]* [^"]*)"', inc)
    assert len(msgs) >= 10 and all(m.startswith("bam_bedgraph_export: ") for m in msgs)
    for line in (X.ERR_NOT_OPEN, X.ERR_ORDER, X.ERR_OPEN_OUTPUT + "%s: %s", X.err_exists("%s")):
        assert line in inc, line
    ddb = source("duckdb_bedgraph_export.inc")
    for line in (X.ERR_NO_OUT_PATH, X.ERR_NO_PATH, X.ERR_INDEX_KIND):
        assert line in ddb, line
    assert ddb.count('bam_filter_check(m, "bam_bedgraph_export", min_read_len, ') == 1 and ddb.index(X.ERR_NO_OUT_PATH) < ddb.index(X.ERR_NO_PATH) < ddb.index("bam_filter_check(m,")


def test_the_documents_name_it():
    for doc, phrases in (("README.md", ("bam_bedgraph_export", "DHTS_EXPORT_FUNCTIONS=1")), ("INTEGRATION.md", ("bam_bedgraph_export", "DHTS_EXPORT_FUNCTIONS=1", "out_path")),
                         ("DESIGN.md", ("bam_bedgraph_export", "rows_text.hip", "later optimisation", "without re-inflating"))):
        text = open(os.path.join(ROOT, doc)).read()
        for p in phrases:
            assert p in text, (doc, p)
