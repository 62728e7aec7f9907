"""Valid BAM and BCF files whose payload holds byte patterns that pass the record stage's speculation filter (test inputs).

Every file here is one the oracle reads to the end without an error.  The decoys travel as the value of an auxiliary B:C array (BAM) or of
an INFO Integer vector (BCF), so they are data like any other; what they do is make the tile scan guess wrong (tests/tile_spec_ref.py
says where), which sends the batch through the repair rounds, the sequential fallback and the retries of a speculated shard start.

Layout of the "grid" files: every record is exactly 1024 bytes and the header is padded so that records start at 960 (mod 1024) in the
inflated stream.  The header shares its BGZF block with the first records, so a whole-file batch begins at byte 0 of the stream (a header in
blocks of its own is skipped, and the tiles would count from the first record).  Tiles (8192 bytes) then begin 64 bytes into a record, in front of that record's decoy, and the
tile's first true record starts at tile + 960.

A case is a dict: data (the file), stream (its inflated bytes), starts (true record offsets in the stream), first (the first record),
rule (the tile_spec_ref rule for it), kind ("bam" | "bcf"), and for the shard cases block (the block the second shard begins with), cut (that
block's offset in the stream) and k (decoy candidates in front of the shard's first true record)."""
import functools
import random
import struct

import bamwriter as BW
import bcfwriter as CW
from tile_spec_ref import BamRule, BcfRule, TILE

REC = 1024
H = 960                       # header bytes of every file here: records start at 960 (mod 1024)
BAM_VOFF, BAM_VLEN = 206, 818   # the B:C value inside a grid record
BCF_VOFF, BCF_VLEN = 44, 980    # the INFO vector's values inside a grid record
AT = 144                      # decoys sit at tile + 144 (inside the value of the record that straddles the tile's first byte)


# ---- decoys ---------------------------------------------------------------------------------------------------------------------------
def bam_decoy(block_len=48, l_seq=4):
    """52 bytes that pass the speculation filter and fail bam_read1's CIGAR / l_seq test (9M against l_seq 4, or whatever l_seq says)"""
    core = struct.pack("<iiiIIiiii", block_len, 0, 0, 2, 1, l_seq, -1, -1, 0)
    return core + b"d\0" + struct.pack("<I", 9 << 4) + b"\x11\x11" + b"\x1e" * 4 + b"ZZCx"


def bcf_decoy(size=32):
    """a 32-byte core the filter accepts (rid 0, one allele, no samples) that claims `size` bytes; bcf_record_check refuses it: the shared
    block holds no ID descriptor (size 32) or one of the wrong type"""
    return struct.pack("<IIiiiIII", size - 8, 0, 0, 0, 1, 0x7F800001, 1 << 16, 0)


BAM_STOP = struct.pack("<i", 1)       # block_size < 32: the walk stops with an error
BCF_STOP = struct.pack("<I", 1)       # l_shared < 24


def chain(kind, links):
    return (bam_decoy() * links + BAM_STOP) if kind == "bam" else (bcf_decoy() * links + BCF_STOP)


def chain3(kind):
    return chain(kind, 3)


# ---- grid files -----------------------------------------------------------------------------------------------------------------------
def _bam_header_text():
    text = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:100000000\n"
    fixed = 4 + 4 + 4 + (4 + 5 + 4)
    pad = H - fixed - len(text) - len("@CO\t\n")
    return text + "@CO\t" + "x" * pad + "\n"


def _bam_record(i, value, bases=100):
    rnd = random.Random(i)
    seq = "".join(rnd.choice("ACGT") for _ in range(bases))
    return BW.record(qname="%07d" % i, flag=0, tid=0, pos=10 * i, mapq=30, cigar="%dM" % bases, seq=seq, qual=bytes([30]) * bases,
                     tags=[("XD", "B:C", list(value))])


def _bcf_header_text():
    lines = ['##INFO=<ID=XD,Number=.,Type=Integer,Description="d">']
    base = CW.header(lines, contigs=("1", "2"))
    pad = H - (5 + 4 + len(base) + 1) - len("##padding=\n")
    return CW.header(lines + ["##padding=" + "x" * pad], contigs=("1", "2"))


def _bcf_record(i, value, id=b"ab"):
    assert len(value) % 4 == 0
    vals = list(struct.unpack("<%di" % (len(value) // 4), value))
    assert CW.INT32_MISSING not in vals and CW.INT32_END not in vals
    return CW.record(rid=0, pos=i, rlen=1, id=id, alleles=(b"A",), info=[(1, CW.tv_ints(vals, width=4))])


class Grid:
    """n records of 1024 bytes (extra[i]: that record is longer by extra[i] * 1024 bytes); put() writes bytes at an offset of the stream,
    which must lie inside a record's value"""

    def __init__(self, kind, n, extra=None):
        self.kind, self.n = kind, n
        self.voff, vlen = (BAM_VOFF, BAM_VLEN) if kind == "bam" else (BCF_VOFF, BCF_VLEN)
        extra = extra or {}
        self.values = [bytearray(vlen + REC * extra.get(i, 0)) for i in range(n)]
        self.starts, o = [], H
        for v in self.values:
            self.starts.append(o)
            o += self.voff + len(v)
        self.ulen = o

    def put(self, off, data):
        import bisect
        i = bisect.bisect_right(self.starts, off) - 1
        p = off - self.starts[i] - self.voff
        assert 0 <= p and p + len(data) <= len(self.values[i]), (off, i, p)
        self.values[i][p:p + len(data)] = data

    def build(self, cuts=None, **more):
        if self.kind == "bam":
            hdr = BW.bam_header([("chr1", 100000000)], _bam_header_text())
            recs = [_bam_record(i, v) for i, v in enumerate(self.values)]
            data = BW.bgzf_file(hdr + b"".join(recs), cuts=cuts)
            rule = BamRule(1)
        else:
            hdr = CW.bcf_raw(_bcf_header_text(), [])
            recs = [_bcf_record(i, v) for i, v in enumerate(self.values)]
            data = BW.bgzf_file(hdr + b"".join(recs), cuts=cuts)
            rule = BcfRule(2, 0)
        assert len(hdr) == H, len(hdr)
        stream = hdr + b"".join(recs)
        assert len(stream) == self.ulen and all(len(r) == self.voff + len(v) for r, v in zip(recs, self.values))
        return dict(more, kind=self.kind, data=data, stream=stream, starts=list(self.starts), first=H, rule=rule)


def _control(kind, n=404):
    """no decoys; the last tile holds a record start too, so no tile of a whole-file batch is touched by a repair round"""
    return Grid(kind, n).build()


def _every_tile_chain3(kind, n=2400):
    g = Grid(kind, n)
    for s in g.starts:
        g.put(s + 64 + AT, chain3(kind))
    return g.build()


def _every_tile_rejoin(kind, n=2400):
    """one fake record per true record that ends exactly on the next true record: the tile leaves at the right place with the wrong first
    record and one record too many"""
    g = Grid(kind, n)
    size = REC - 64 - AT
    for s in g.starts:
        g.put(s + 64 + AT, bam_decoy(block_len=size - 4) if kind == "bam" else bcf_decoy(size))
    return g.build()


def _leap(kind, n=400):
    """a decoy whose length claims the next three tiles and lands on a true record start four tiles on"""
    g = Grid(kind, n)
    jump = 4 * TILE + 960 - AT
    for t in (3, 10, 11, 20, 21, 22, 30):
        g.put(t * TILE + AT, bam_decoy(block_len=jump - 4, l_seq=20000) if kind == "bam" else bcf_decoy(jump))
    return g.build()


LONG_AT = 200                   # window_edge: the record that is 17 KiB long


def _window_edge(kind, n=400):
    """(a) tile 5: the candidate's first follow-up lies in the last bytes of the staged window (tile + 1 KiB halo), where the filter reads
    global memory; (b) tile 26 lies inside a 17 KiB record and its candidate straddles the tile's end; (c) BAM only: the candidate of the last
    tile lies within 300 bytes of the end of the stream (a BCF candidate there is incomplete, never accepted)"""
    g = Grid(kind, n, extra={LONG_AT: 16})
    assert g.ulen % TILE == 960 and g.starts[LONG_AT] == 25 * TILE + 960
    if kind == "bam":
        g.put(5 * TILE + 736, bam_decoy(block_len=TILE - 4))
        g.put(6 * TILE + 736, chain3(kind))
        g.put((g.ulen // TILE) * TILE + 736, chain3(kind))
    else:
        g.put(5 * TILE + 900, bcf_decoy(8300))
        g.put(5 * TILE + 9200, bcf_decoy() * 2 + BCF_STOP)
    g.put(27 * TILE - 20, chain3(kind))
    return g.build()


def _sparse(kind, n=700, seed=5):
    """mixed record lengths, a decoy chain somewhere in the value of half of the records"""
    rnd = random.Random(seed)
    recs, starts, o = [], [], H
    for i in range(n):
        vlen = 4 * rnd.randrange(45, 300)
        v = bytearray(vlen)
        if rnd.random() < 0.5:
            p = 4 * rnd.randrange(0, (vlen - len(chain3(kind))) // 4)
            v[p:p + len(chain3(kind))] = chain3(kind)
        if kind == "bam":
            r = _bam_record(i, v, bases=rnd.choice((36, 100, 151, 250)))
        else:
            r = _bcf_record(i, v, id=b"id%d" % rnd.randrange(10 ** rnd.randrange(1, 9)))
        starts.append(o)
        o += len(r)
        recs.append(r)
    if kind == "bam":
        hdr = BW.bam_header([("chr1", 100000000)], _bam_header_text())
        data = BW.bgzf_file(hdr + b"".join(recs), payload=30000)
        rule = BamRule(1)
    else:
        hdr = CW.bcf_raw(_bcf_header_text(), [])
        data = BW.bgzf_file(hdr + b"".join(recs), payload=30000)
        rule = BcfRule(2, 0)
    return dict(kind=kind, data=data, stream=hdr + b"".join(recs), starts=starts, first=H, rule=rule)


SHARD_KS = (1, 2, 16, 17, 40)
SHARD_AT = 64                   # the record the shard boundary is cut into


def _shard(kind, k, rejoin=False, far=False, links=3):
    """64 grid records, one long record S, 300 grid records.  A BGZF block begins 300 bytes into S; behind that boundary S's value holds k
    decoy chains back to back (rejoin: one fake record that ends exactly where S ends, so that its chain holds and only the full validation of
    its "records" can refuse it; far: S is 16 KiB long and the chains lie in the second tile behind the boundary; links: decoys per chain -- with more than three, several offsets of ONE chain
    pass the three-deep filter and all of them break at the same stop word).  The first true record of
    the shard that begins with that block is the record behind S."""
    g = Grid(kind, SHARD_AT + 1 + 300, extra={SHARD_AT: 15 if far else 7})
    s0 = g.starts[SHARD_AT]
    cut = s0 + 300
    at = cut + (9000 if far else 8)
    if rejoin:
        size = g.starts[SHARD_AT + 1] - at
        g.put(at, bam_decoy(block_len=size - 4) if kind == "bam" else bcf_decoy(size))
    else:
        g.put(at, chain(kind, links) * k)
    return g.build(cuts=[32768, cut - 32768], block=2, cut=cut, k=k, rejoin=rejoin)


TILE_CASES = ("control", "every_tile_chain3", "every_tile_rejoin", "sparse", "leap", "window_edge")
SHARD_CASES = tuple("shard_start_%d" % k for k in SHARD_KS) + ("shard_start_rejoin", "shard_start_far", "shard_start_links4", "shard_start_links20",
                                                              "shard_start_2x_links20")


@functools.lru_cache(maxsize=None)
def case(kind, name):
    if name in TILE_CASES:
        return globals()["_" + name](kind)
    if name == "shard_start_rejoin":
        return _shard(kind, 1, rejoin=True)
    if name == "shard_start_far":
        return _shard(kind, 2, far=True)
    if name == "shard_start_links4":
        return _shard(kind, 1, links=4)
    if name == "shard_start_links20":
        return _shard(kind, 1, links=20)
    if name == "shard_start_2x_links20":
        return _shard(kind, 2, links=20)
    assert name.startswith("shard_start_")
    return _shard(kind, int(name.rsplit("_", 1)[1]))
