"""Record streams for the two tile-scan kernels (bam_tile_scan: one wave per tile out of LDS; bam_tile_scan_lanes: one lane per tile out of
HBM), shared by test_gpu_tile_scan_lanes.py and test_hostsim_scan.py.  Small on purpose: each stream is the shortest at which the lane
kernel can still go wrong -- a 128-byte line's last candidates (their fields lie in the next line), tiles without a record start, tiles
with more than 64 and with more than 200 starts, a block_size word across a tile boundary, the stream's end next to a tile boundary, and
damage that the prefilter passes and only the full filter or the walk can catch.

case(name) -> {"recs": [record bytes, ...] (a truncated file: one piece), "damaged": bool (the oracle reports an error)}
bam(name)  -> the BAM file of the case (header in BGZF blocks of its own, the record stream in blocks of 9,000 bytes: more than a tile, so
              that every batch of max_blocks 1 or 3 but a file's last has at least two tiles and runs the lane kernel, which takes tiles
              t >= 1; the batches end inside records)."""
import functools
import random
import struct

import bamwriter as BW

TILE = 8192
REFS = [("chr1", 100000000), ("chr2", 50000000)]
TEXT = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:100000000\n@SQ\tSN:chr2\tLN:50000000\n@RG\tID:grp1\tSM:s1\n"
PAYLOAD = 9000
END_D = (-17, -16, -4, -3, -1, 0, 1, 3, 4, 15, 16)


def _bases(rnd, n):
    return "".join(rnd.choice("ACGT") for _ in range(n))


def short(i, tid=0):
    """the shortest record: l_qname 1, no CIGAR, l_seq 0 -> 37 bytes"""
    r = BW.record(qname="", flag=4, tid=tid, pos=i, mapq=0, cigar="*", seq="*")
    assert len(r) == 37
    return r


def rec(i, l_seq=60, pad=0):
    rnd = random.Random(i)
    tags = [("RG", "Z", "grp1")] + ([("XX", "Z", "p" * (pad - 4))] if pad >= 4 else [])
    return BW.record(qname="q%d" % (i % 7), flag=0, tid=i % 2, pos=100 + i, mapq=20, cigar="%dM" % l_seq, seq=_bases(rnd, l_seq),
                     qual=bytes(rnd.randrange(0, 50) for _ in range(l_seq)), tags=tags)


MINR = len(rec(0, 60, 0))


def _exact(target, seed=0):
    """records of mixed lengths whose sizes sum to `target` (the last record ends on the last byte)"""
    rnd, recs, pos = random.Random(seed * 7919 + target), [], 0
    while target - pos >= 3000:
        recs.append(rec(len(recs), (60, 151, 33, 250)[len(recs) % 4], rnd.randrange(4, 40))); pos += len(recs[-1])
    while target - pos >= 2 * MINR + 60:
        recs.append(rec(len(recs), 60, 4 + (target - pos) % 3 + rnd.randrange(0, 8))); pos += len(recs[-1])
    left = target - pos
    if left:
        if left - MINR >= 4:
            recs.append(rec(len(recs), 60, left - MINR))
        else:                                                      # any length from 37 bytes on: an unmapped record with a read name that makes it up
            recs.append(BW.record(qname="n" * (left - 37), flag=4, tid=0, pos=5, seq="*"))
        pos += len(recs[-1])
    assert pos == target, (pos, target)
    return recs


def _straddle(k):
    """the block_size word of a record lies across the boundary of tiles 1 and 2 with k of its bytes in tile 1 (k = 0: it begins tile 2)"""
    start = 2 * TILE - k
    recs = _exact(start, seed=k)
    recs += [rec(5000 + i, 151, 9) for i in range(30)]
    return recs


def _dense():
    """37-byte records only: 221 record starts per tile"""
    return [short(i, i % 2) for i in range(700)]


def _dense_and_one():
    """tile 1 holds more than 64 record starts; tile 2 exactly one (a long record begins in it and runs into tile 3)"""
    recs = _exact(TILE - 40, seed=3)                               # tile 0
    recs += [short(i) for i in range(216)]                         # 7,992 bytes: the next record starts 8,152 + 7,992 = at 16,144 in tile 1
    pos = sum(len(r) for r in recs)
    assert TILE < pos < 2 * TILE
    recs.append(rec(1, 60, 2 * TILE + 100 - pos - MINR))          # runs to 100 bytes into tile 2
    recs.append(rec(2, 9000, 9))                                   # the one record that starts in tile 2: about 13.7 KB
    assert sum(len(r) for r in recs) > 3 * TILE + 200
    recs += [rec(10 + i, 60, 5) for i in range(20)]
    return recs


def _long40k():
    recs = [rec(i, 60, 6) for i in range(40)]
    recs.append(rec(99, 27000, 9))                                 # 36 + ... + 13,500 + 27,000: about 40.5 KB -> five tiles without a record start
    recs += [rec(100 + i, 60, 6) for i in range(60)]
    return recs


def _set_block_size(r, v):
    return struct.pack("<i", v) + r[4:]


def _damage_block_size(v):
    """valid records for three tiles, one block_size overwritten in mid-chain (tile 1)"""
    recs = [rec(i, 100, 8) for i in range(160)]
    pos, k = 0, 0
    while pos < TILE + 3000:
        pos += len(recs[k]); k += 1
    recs[k] = _set_block_size(recs[k], v)
    return recs


def _damage_runs_past():
    recs = [rec(i, 100, 8) for i in range(130)]
    recs[-1] = _set_block_size(recs[-1], 1 << 20)                  # the last record claims a megabyte
    return recs


def _near_miss(which):
    """a candidate in front of tile 1's first record that passes the prefilter (block_size >= 32, ids in range, l_seq >= 0, l_qname >= 1, core
    fits) and fails ONE later test of the speculation filter: the QNAME's last byte is not NUL ("nul"), or the auxiliary part is larger
    than 8 * core + 65,536 ("aux").  It sits inside the QUAL field of a long record, so the file is valid."""
    recs = _exact(TILE - 600, seed=11 if which == "nul" else 12)
    if which == "nul":
        fake = struct.pack("<iiiIIiiii", 60, 0, 7, (9 << 8) | 4, 0, 8, -1, -1, 0) + b"abcd" + bytes(20)      # l_qname 4, QNAME "abcd": no NUL
    else:
        fake = struct.pack("<iiiIIiiii", 32 + 6 + 70000, 0, 7, (9 << 8) | 2, 0, 2, -1, -1, 0) + b"a\x00" + bytes(20)   # core 5, aux 70,001 > 40 + 65,536
    l_seq = 1400
    qual = bytearray(b"\x11" * l_seq)
    qual[700:700 + len(fake)] = fake                                # lands a little behind the boundary of tiles 0 and 1
    recs.append(BW.record(qname="host", flag=0, tid=0, pos=9, mapq=1, cigar="%dM" % l_seq, seq="A" * l_seq, qual=bytes(qual)))
    pos = sum(len(r) for r in recs)
    assert pos > TILE + 200
    recs += [rec(300 + i, 60, 6) for i in range(150)]
    return recs


def names():
    out = ["dense", "dense_and_one", "long40k"] + ["straddle%d" % k for k in range(4)]
    out += ["end_%d_%d" % (j, d) for j in (1, 2, 3) for d in END_D]
    out += ["cut_%d_%d" % (j, d) for j in (1, 2, 3) for d in END_D]
    out += ["bs31", "bs_minus1", "runs_past", "near_nul", "near_aux"]
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "dense":
        return {"recs": _dense(), "damaged": False}
    if name == "dense_and_one":
        return {"recs": _dense_and_one(), "damaged": False}
    if name == "long40k":
        return {"recs": _long40k(), "damaged": False}
    if name.startswith("straddle"):
        return {"recs": _straddle(int(name[8:])), "damaged": False}
    if name.startswith("end_"):
        _, j, d = name.split("_")
        return {"recs": _exact(TILE * int(j) + int(d), seed=1), "damaged": False}
    if name.startswith("cut_"):
        # the same lengths as a truncated file: a stream 300 bytes longer whose last record is cut at the length
        _, j, d = name.split("_")
        n = TILE * int(j) + int(d)
        raw = b"".join(_exact(n + 300, seed=2))
        return {"recs": [raw[:n]], "damaged": True}
    if name == "bs31":
        return {"recs": _damage_block_size(31), "damaged": True}
    if name == "bs_minus1":
        return {"recs": _damage_block_size(-1), "damaged": True}
    if name == "runs_past":
        return {"recs": _damage_runs_past(), "damaged": True}
    if name == "near_nul":
        return {"recs": _near_miss("nul"), "damaged": False}
    if name == "near_aux":
        return {"recs": _near_miss("aux"), "damaged": False}
    raise KeyError(name)


def stream(name):
    return b"".join(case(name)["recs"])


@functools.lru_cache(maxsize=None)
def bam(name):
    return BW.bam_bytes(REFS, case(name)["recs"], text=TEXT, payload=PAYLOAD)
