"""The reference side of every lying-ISIZE comparison is ISIZE-blind (CPU): isize_lies.lie changes nothing but the chosen four-byte fields,
every block still inflates to its CRC-32, and the oracles (like htslib, which never reads the field) return for the lying file exactly what
they return for the clean one."""
import os
import sys

import numpy as np
import pytest

import bcf_cases
import bcfwriter
import cases
import isize_lies as il
import orc
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import region_oracle  # noqa: E402

BAM_FILES = {"p61": lambda: cases.case_basic(payload=61, n=200, seed=2), "p777": lambda: cases.case_basic(payload=777, n=200, seed=2),
             "p65280": lambda: cases.case_basic(payload=65280, n=3000, seed=2)}
_cache = {}


def _file(name):
    if name not in _cache:
        if name == "bcf":
            _cache[name] = bcfwriter.bcf_bytes(bcf_cases.std_header(), bcf_cases.fuzz_records(7, 3000, len(bcf_cases.SAMPLES)), payload=777)
        else:
            _cache[name] = BAM_FILES[name]()
    return _cache[name]


def _lies(data, plan):
    """(clean, lying, label): single-block plans with every value, the others as the plan defines them"""
    single = plan in ("block0", "first_record_block", "one_mid", "last_data_block", "eof_block")
    clean = il.clean_for(data, plan)
    for v in (il.ALL_VALUES if single else (None,)):
        yield clean, (il.lie(data, plan, v) if v else il.lie(data, plan)), f"{plan}/{v}"


def _same_bam(a, b, what):
    assert a["n_rows"] == b["n_rows"] and a["status"] == b["status"], what
    for k in ("QNAME", "FLAG", "RNAME", "POS", "MAPQ", "CIGAR", "RNEXT", "PNEXT", "TLEN", "SEQ", "QUAL", "READ_GROUP_ID", "SAMPLE_ID"):
        x, y = a[k], b[k]
        assert (np.array_equal(np.asarray(x), np.asarray(y)) if isinstance(x, np.ndarray) else list(x) == list(y)), (what, k)


def test_helper_shapes():
    assert len(il.EOF_BLOCK) == 28 and il.inflate_block(il.EOF_BLOCK, (0, 28)) == b""
    assert len(il.ALL_VALUES) == 10 and set(il.OVERSTATING) < set(il.ALL_VALUES)
    for L in (0, 1, 61, 65280):
        assert il.VALUES["zero"](L) == (0 if L else 777)
        assert all(il.VALUES[v](L) > L for v in il.OVERSTATING)
    assert len(il.blocks(_file("p61"))) == 798 and len(il.blocks(_file("p777"))) == 65 and len(il.blocks(_file("p65280"))) == 13
    d = _file("p777")
    k = il.data_blocks(d)
    s = il.small_understatement(d, k[3:6])
    bl = il.blocks(d)
    assert il.lying_blocks(d, s) == k[3:6] and sum(il.isize(d, bl[i]) - il.isize(s, bl[i]) for i in k[3:6]) == 46


@pytest.mark.parametrize("plan", il.PLANS)
@pytest.mark.parametrize("name", ["p61", "p777", "p65280", "bcf"])
def test_the_oracles_read_a_lying_file_like_the_clean_one(name, plan):
    data = _file(name)
    read = orc.bcf_read if name == "bcf" else orc.bam_read
    want = {}
    for clean, lying, what in _lies(data, plan):
        idx = il.lying_blocks(clean, lying)                   # (asserts that only ISIZE fields differ)
        assert idx == sorted(il.plan_blocks(data, plan)), what
        bl = il.blocks(lying)
        assert [il.inflate_block(lying, b) for b in bl] == [il.inflate_block(clean, b) for b in bl], what      # raw zlib, CRC-32 checked
        if plan == "empty_mid":
            assert il.inflate_all(clean) == il.inflate_all(data)
        if id(clean) not in want:
            want[id(clean)] = read(clean)
            assert want[id(clean)]["n_rows"] > 0
        exp, got = want[id(clean)], read(lying)
        if name == "bcf":
            assert orc.bcf_cols_diff(exp, got) is None and got["n_rows"] == exp["n_rows"], what
        else:
            _same_bam(exp, got, what)
            for region in ("chr1:1000-30000,chr2", "chrM:1-9000,chr1:60,000-61,000"):
                assert np.array_equal(region_oracle.keep_mask(exp, region), region_oracle.keep_mask(got, region)), (what, region)
