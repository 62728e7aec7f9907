"""The walk over a record's auxiliary fields to RG:Z (aux_size / aux_skip_known / aux_find_t), every column against the oracle.

One record per case; each file is read twice: "near" packs the records one behind the other (nearly all of them lie inside the window a
tile's wave stages: the 32-bit LDS walk), "far" starts every case record 92 bytes in front of a tile's end behind 1,400 bytes of SEQ and QUAL,
so that it leaves the window and is walked out of HBM with 64-bit offsets.  A record whose aux data is broken only loses its read group
(bam_read1 does not look at aux data) unless its CIGAR asks for the CG:B,I swap: then the walk's `bad` flag ends the scan, and such records
end a file of their own."""
import functools
import random
import struct

import numpy as np
import pytest

import bamwriter as BW
import duckhts_amd
import orc
from tag_corpus import FIXED, barray, cg_record, cg_tag, field

pytestmark = pytest.mark.gpu

TILE = 8192
COLS = duckhts_amd.BAM_COLUMNS
TEXT = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:100000000\n@RG\tID:grp1\tSM:s1\n@RG\tID:grp2\tSM:s2\n@RG\tID:\tSM:s3\n"
RG = b"RGZgrp1\0"


def aux_cases():
    """(name, raw aux bytes) in file order"""
    out = []
    for t in range(256):                                     # every type byte in front of RG
        out.append(("type %d" % t, field(t) + RG))
    for ch in list(FIXED) + ["Z", "H"]:                      # every valid type before and behind RG
        out.append(("before " + ch, field(ord(ch)) + RG)); out.append(("behind " + ch, RG + field(ord(ch))))
    for sub in "cCsSiIf":
        for n in (0, 1, 7):
            out.append(("B:%s x%d before" % (sub, n), barray(sub, n) + RG)); out.append(("B:%s x%d behind" % (sub, n), RG + barray(sub, n)))
    for sub in "ZHB":                                        # (aux_type2size answers the byte itself for these sub-types)
        out.append(("B sub-type " + sub, b"XBB" + sub.encode() + struct.pack("<I", 1) + b"\x01" * ord(sub) + RG))
    five = b"NMC\x01MDZ100\0ASC\x64XSC\x00"
    out += [("RG first", RG + five), ("RG last", five + RG), ("RG absent", five), ("no aux", b""), ("two RG", b"RGZgrp2\0" + five + RG),
            ("RG:H", b"RGHgrp1\0" + five), ("RG:A", b"RGAg" + five), ("RG:i", b"RGi\1\0\0\0" + five), ("RG empty", five + b"RGZ\0"),
            ("RG unknown", five + b"RGZnone\0"), ("RG behind a long Z", b"XLZ" + b"x" * 700 + b"\0" + RG),
            ("decoy in Z", b"XDZabRGZgrp2\0" + RG), ("decoy in B", b"XDBC" + struct.pack("<I", 8) + b"RGZgrp2\0" + RG),
            ("Z without NUL", five + b"XZZabcdefghijk"), ("RG without NUL", five + b"RGZgrp1"), ("RG cut behind the type", five + b"RGZ"), ("tag only", five + b"RG"),
            ("one stray byte", five + b"R")]
    for ch, sz in FIXED.items():
        for short in range(1, min(sz, 7) + 1):
            out.append(("%s %d short" % (ch, short), five + b"XT" + ch.encode() + b"\x05" * (sz - short)))
            out.append(("%s %d short, RG in front" % (ch, short), RG + b"XT" + ch.encode() + b"\x05" * (sz - short)))
    for n, have in ((3, 2), (1 << 20, 16), (0xffffffff, 0), (0x40000001, 8)):
        out.append(("B:I count %d overruns" % n, five + b"XBBI" + struct.pack("<I", n) + b"\x01" * have))
        out.append(("B:I count %d overruns, RG in front" % n, RG + b"XBBI" + struct.pack("<I", n) + b"\x01" * have))
    out.append(("B cut in its header", five + b"XBBI\x01\x00"))
    return out


def plain(i, aux, far):
    n = 900 if far else 30 + i % 7
    rnd = random.Random(i)
    return BW.record(qname="r%d" % i, flag=0, tid=0, pos=i, mapq=20, cigar="%dM" % n, seq="".join(rnd.choice("ACGT") for _ in range(n)),
                     qual=bytes(rnd.randrange(1, 60) for _ in range(n)), raw_aux=aux)


def layout(records, far):
    """far: every record starts 92 bytes in front of a tile's end, behind filler records"""
    if not far:
        return list(records)
    out, pos = [], 0
    for k, rec in enumerate(records):
        assert len(rec) > 92 + 1024
        t = pos // TILE
        while t * TILE + TILE - 92 - pos < 0 or 0 < t * TILE + TILE - 92 - pos < 60:
            t += 1
        gap = t * TILE + TILE - 92 - pos
        while gap:
            take = gap if gap < 1100 else 1000
            if 0 < gap - take < 60:
                take -= 60
            out.append(BW.record(qname="f", tid=0, pos=k, cigar="*", seq="*", raw_aux=b"RGZgrp2\0XXZ" + b"p" * (take - 38 - 8 - 4) + b"\0")); pos += take; gap -= take
            assert len(out[-1]) == take
        out.append(rec); pos += len(rec)
    return out


@functools.lru_cache(maxsize=None)
def _walk_file(far):
    recs = [plain(i, aux, far) for i, (_, aux) in enumerate(aux_cases())]
    n = 900 if far else 40
    # the CG swap with RG in front of and behind the CG tag, and the swap beside every kind of field; a Z without NUL that is not CG ends
    # the walk, not the scan; a CG array shorter than the CIGAR is not swapped in
    for aux in (RG + cg_tag(n), cg_tag(n) + RG, b"NMC\1" + cg_tag(n) + b"XBBs" + struct.pack("<I", 2) + b"\1\2\3\4" + RG, RG + b"XZZabc\0" + cg_tag(n) + b"XDd" + b"\1" * 8,
                cg_tag(n), b"CGBi" + cg_tag(n)[4:] + RG, b"CGZabc\0" + RG, RG + b"XZZabcdefg", b"CGBI" + struct.pack("<I", 1) + struct.pack("<I", (n << 4)) + RG):
        recs.append(cg_record(len(recs), aux, far))
    data = BW.bam_bytes([("chr1", 100000000)], layout(recs, far), text=TEXT)
    exp = orc.bam_read(data)
    assert exp["status"] >= 0 and exp["n_rows"] >= len(recs)
    return data, exp


# aux data that makes the CG walk fail: the record is invalid and ends the scan (the oracle says so; each ends a file of its own)
BROKEN = [("unknown type", b"XT?\1\2\3\4"), ("i 2 short", b"XTi\1\2"), ("d 7 short", b"XTd\1"), ("B overruns", b"XBBI" + struct.pack("<I", 9) + b"\1" * 8),
          ("B of unknown sub-type", b"XBBx" + struct.pack("<I", 1) + b"\1"), ("CG:Z without NUL", b"CGZabc"), ("CG:i 1 short", b"CGi\1\2\3")]


@functools.lru_cache(maxsize=None)
def _broken_file(k, far):
    name, aux = BROKEN[k]
    recs = [plain(0, RG, far), cg_record(1, RG + aux, far), plain(2, RG, far)]
    data = BW.bam_bytes([("chr1", 100000000)], layout(recs, far), text=TEXT)
    return data, orc.bam_read(data)


def _same(got, exp, ctx):
    assert got["n_rows"] == exp["n_rows"], (ctx, got["n_rows"], exp["n_rows"])
    assert (got["status"] < 0) == (exp["status"] < 0), (ctx, got["status"], exp["status"])
    for k in COLS:
        a, b = got[k], exp[k]
        if isinstance(b, np.ndarray):
            assert np.array_equal(np.asarray(a), b), f"{ctx}: column {k} differs"
        else:
            for r, (x, y) in enumerate(zip(a, b)):
                assert x == y, f"{ctx}: column {k} row {r}: {x!r:.80} != {y!r:.80}"
            assert len(a) == len(b), (ctx, k)


@pytest.mark.parametrize("far", [False, True], ids=["near", "far"])
def test_walk_to_rg(far):
    data, exp = _walk_file(far)
    names = [n for n, _ in aux_cases()]
    if not far:                                              # what the cases are for, by the oracle: the walk passes every valid type and stops at the others
        rg = exp["READ_GROUP_ID"]
        valid = {ord(c) for c in "AcCsSiIfdZHB"}
        for t in range(256):
            assert (rg[t] == b"grp1") == (t in valid), (t, rg[t])
        assert rg[names.index("decoy in Z")] == b"grp1" and rg[names.index("decoy in B")] == b"grp1" and rg[names.index("two RG")] == b"grp2"
        assert rg[names.index("RG:A")] is None and rg[names.index("Z without NUL")] is None and rg[names.index("RG empty")] == b""
    _same(duckhts_amd.read_bam(data), exp, "far" if far else "near")


@pytest.mark.parametrize("far", [False, True], ids=["near", "far"])
def test_broken_aux_data_under_the_cg_walk_ends_the_scan(far):
    for k, (name, _) in enumerate(BROKEN):
        data, exp = _broken_file(k, far)
        rows_before = sum(1 for q in exp["QNAME"] if not q.startswith(b"c"))
        print(name, "far" if far else "near", "oracle: rows", exp["n_rows"], "status", exp["status"])
        assert exp["status"] < 0 and 1 <= rows_before == exp["n_rows"], (name, exp["n_rows"], exp["status"])
        _same(duckhts_amd.read_bam(data), exp, name)
