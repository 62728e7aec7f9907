"""The surface of bam_bedcov without a device: the header declares the dhts_bam_bedcov_* entries, the built library exports them, the Python
mirror binds them, and the structures of the two sides have one layout."""
import ctypes as C
import os
import re
import subprocess

import duckhts_amd
from conftest import ROOT

ENTRIES = ["dhts_bam_bedcov_open", "dhts_bam_bedcov_accumulate", "dhts_bam_bedcov_scan", "dhts_bam_bedcov_stats", "dhts_bam_bedcov_next",
           "dhts_bam_bedcov_batch_host_bytes", "dhts_bam_bedcov_batch_fetch"]


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_the_header_declares_the_entries_and_the_contract():
    text = header("duckhts_amd.h")
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(dhts_bam_bedcov_[a-z_]+)\s*\(", code))) == sorted(ENTRIES)
    for word in ("dhts_bedcov_params", "dhts_bedcov_stats", "dhts_bedcov_batch", "DHTS_BEDCOV_BASES_COVERED", "DHTS_BEDCOV_READ_COUNT"):
        assert word in code
    block = text[text.index("---- bam_bedcov"):text.index("enum { DHTS_BEDCOV_CHROM")]
    for phrase in ("n_flag_filtered", "n_unplaced", "n_low_mapq", "n_counted", "max(1, rlen)", "count_deletions", "count_ref_skips", "2^27", "0x704",
                   "depth thresholds (-d)", "several BAM files", "reference / CRAM", "a region on the BED side"):
        assert phrase in block, phrase
    assert re.search(r"\bregister_bam_bedcov_function\s*\(", header("duckhts_extension.h"))


def test_the_library_exports_the_entries():
    out = subprocess.run(["nm", "-D", "--defined-only", duckhts_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in ENTRIES + ["register_bam_bedcov_function", "dhts_debug_bedcov_max_rows"]:
        assert n in exported, n
    assert not [n for n in exported if "bedcov" in n and n not in ENTRIES + ["register_bam_bedcov_function", "dhts_debug_bedcov_max_rows"]]


def test_the_python_mirror_binds_the_entries():
    L = duckhts_amd.lib()
    for n in ENTRIES:
        assert n in duckhts_amd.EXPORTS and getattr(L, n).argtypes, n
    for m in ("bam_bedcov_open", "bam_bedcov_accumulate", "bam_bedcov_scan", "bam_bedcov_stats", "bam_bedcov_next"):
        assert callable(getattr(duckhts_amd.Context, m))
    assert duckhts_amd.BEDCOV_COLUMNS == ["chrom", "start", "end", "name", "score", "strand", "bases_covered", "read_count"]
    assert duckhts_amd.BEDCOV_COLMASK & 0b1111111100000 == 0                                   # no string column in the scan (QNAME is bit 0)
    assert not duckhts_amd.BEDCOV_COLMASK & 1
    import inspect
    sig = inspect.signature(duckhts_amd.bam_bedcov).parameters
    assert [sig[k].default for k in ("min_mapq", "require_flags", "exclude_flags", "include_flags", "count_deletions", "count_ref_skips", "region", "index", "max_blocks")] == \
        [0, 0, 0x704, 0, True, True, None, None, 0]
    # the structures: field order and sizes of include/duckhts_amd.h
    assert C.sizeof(duckhts_amd.BedcovParams) == 24 and [f[0] for f in duckhts_amd.BedcovParams._fields_] == \
        ["min_mapq", "require_flags", "exclude_flags", "include_flags", "count_deletions", "count_ref_skips"]
    assert C.sizeof(duckhts_amd.BedcovStats) == 64 and [f[0] for f in duckhts_amd.BedcovStats._fields_][:7] == \
        ["n_rows", "n_flag_filtered", "n_unplaced", "n_low_mapq", "n_counted", "n_bed_rows", "n_breakpoints"]
    code = re.sub(r"/\*.*?\*/", "", header("duckhts_amd.h"), flags=re.S)
    m = re.search(r"typedef struct \{([^}]*)\} dhts_bedcov_params;", code)
    assert re.findall(r"\b(min_mapq|require_flags|exclude_flags|include_flags|count_deletions|count_ref_skips)\b", m.group(1)) == [f[0] for f in duckhts_amd.BedcovParams._fields_]
