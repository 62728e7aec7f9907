"""The row passes at the edges of the staged window: records placed byte-exactly around a tile's end (tile + 8,192) and the end of the
window a tile's wave stages (tile + 9,216), every column against the oracle.

bam_tile_unpack and bam_tile_strings decide once per record whether it lies inside the window (LDS, 32-bit offsets) or not (HBM), and
read SEQ / QUAL / QNAME / RG in 8- and 16-byte pieces that may reach past a field's end.  The file is built so that each of QNAME, CIGAR,
SEQ, QUAL and the RG value ends at (edge + d) for every d in -17..17 at both edges, records start in the last 1..36 bytes of a tile, and
l_seq takes the values around the 16-base chunk and the 512-base "long field" threshold.  The header sits in BGZF blocks of its own and the
file is read in one batch, so tiles count from the first record: a record's offset is the sum of the lengths before it (computed here)."""
import functools
import random

import numpy as np
import pytest

import bamwriter as BW
import duckhts_amd
import orc

pytestmark = pytest.mark.gpu

TILE, WINDOW = 8192, 9216
COLS = duckhts_amd.BAM_COLUMNS
TEXT = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:100000000\n@RG\tID:grp1\tSM:s1\n@RG\tID:" + "g" * 40 + "\tSM:s2\n"
LONG_RG = "g" * 40


def _seq(rnd, n):
    return "".join(rnd.choice("ACGTN") for _ in range(n)) if n else "*"


class Stream:
    """records in stream order; place() pads with filler records so that the next record starts at a chosen offset"""

    def __init__(self):
        self.recs, self.starts, self.pos, self.rnd = [], [], 0, random.Random(7)
        self.min_fill = len(self._filler_rec(0))

    def add(self, rec):
        self.recs.append(rec); self.starts.append(self.pos); self.pos += len(rec)
        return self.starts[-1]

    def _filler_rec(self, pad):
        n = 60
        return BW.record(qname="f%d" % (len(self.recs) % 10), flag=0, tid=0, pos=len(self.recs), mapq=9, cigar="%dM" % n, seq=_seq(random.Random(len(self.recs)), n),
                         qual=bytes(random.Random(len(self.recs)).randrange(0, 60) for _ in range(n)), tags=[("RG", "Z", "grp1"), ("XX", "Z", "p" * pad)])

    def fill(self, gap):
        while gap >= 900 + self.min_fill:
            self.add(self._filler_rec(900 - self.min_fill)); gap -= 900
        assert gap == 0 or gap >= self.min_fill, gap
        if gap:
            self.add(self._filler_rec(gap - self.min_fill))

    def place(self, rec, rel):
        """rec starts at (some tile's base + rel); rel may exceed TILE (the record then starts in the following tile); returns that base"""
        t = max(0, (self.pos - rel) // TILE)
        while t * TILE + rel != self.pos and t * TILE + rel - self.pos < self.min_fill:
            t += 1
        self.fill(t * TILE + rel - self.pos)
        assert self.pos == t * TILE + rel
        self.add(rec)
        return t * TILE


def _shaped(rnd, i, n_ops, l_seq, rg=LONG_RG, qual=None):
    """a record with n_ops CIGAR operations over l_seq bases, QNAME of 20 characters, RG last; returns (record, ends of the five fields in it)"""
    qn = "q%019d" % i
    ops = "1M" * (n_ops - 1) + "%dM" % (l_seq - (n_ops - 1))
    q = qual if qual is not None else bytes(rnd.randrange(0, 90) for _ in range(l_seq))
    rec = BW.record(qname=qn, flag=0, tid=0, pos=i, mapq=30, cigar=ops, seq=_seq(rnd, l_seq), qual=q, tags=[("NM", "C", 1), ("RG", "Z", rg)])
    e_qn = 36 + 21
    e_cig = e_qn + 4 * n_ops
    e_seq = e_cig + (l_seq + 1) // 2
    e_qual = e_seq + l_seq
    e_rg = len(rec) - 1                                   # the value's last byte is followed by its NUL, the record's last byte
    assert e_rg == e_qual + 4 + 3 + len(rg)
    return rec, {"QNAME": e_qn, "CIGAR": e_cig, "SEQ": e_seq, "QUAL": e_qual, "RG": e_rg}


# field -> (CIGAR operations, l_seq): shapes whose field ends more than 1,042 bytes into the record, so that a record whose field ends at the
# window's end still starts inside the tile that stages that window (QNAME cannot: its record then starts in the next tile)
SHAPES = {"QNAME": (1, 100), "CIGAR": (300, 300), "SEQ": (200, 500), "QUAL": (100, 500), "RG": (100, 500), "SEQ_long": (1, 2200), "QUAL_long": (1, 800)}
L_SEQ = [0, 1, 2, 15, 16, 17, 18, 511, 512, 513, 514, 1100, 1101, 5000, 5001]      # the issue's values, each in both parities


@functools.lru_cache(maxsize=None)
def _file():
    rnd, s, want = random.Random(11), Stream(), []
    i = 0
    # fields ending at (edge + d)
    for field, (n_ops, l_seq) in SHAPES.items():
        for edge in (WINDOW, TILE):
            for d in range(-17, 18):
                rec, ends = _shaped(rnd, i, n_ops, l_seq); i += 1
                fe = ends[field.split("_")[0]]
                base = s.place(rec, edge + d - fe)
                want.append((field, edge, d, s.starts[-1] + fe - base))
    for w in want:
        assert w[3] == w[1] + w[2], w                       # the field ends where the case says, relative to a tile's base
    # records starting in the last 1..36 bytes of a tile
    for k in range(1, 37):
        rec, _ = _shaped(rnd, i, 3, 151, rg="grp1"); i += 1
        s.place(rec, TILE - k)
        assert s.starts[-1] % TILE == TILE - k
    # l_seq values (with qualities, with 0xff qualities), wherever they fall
    for n in L_SEQ:
        for star in (False, True):
            q = (b"\xff" * n) if star else bytes(rnd.randrange(0, 94) for _ in range(n))
            s.add(BW.record(qname="l%d" % n, flag=4 if n == 0 else 0, tid=0, pos=i, mapq=1, cigar=("%dM" % n) if n else "*", seq=_seq(rnd, n), qual=q, tags=[("RG", "Z", "grp1")])); i += 1
    # QUAL bytes that become NUL after +33 (223), at the chunk boundaries of a short and of a long field; 0xff in front and inside
    for n in (40, 600):
        for at in (0, 1, 14, 15, 16, 17, n - 17, n - 16, n - 1):
            q = bytearray(rnd.randrange(0, 94) for _ in range(n)); q[at] = 223
            s.add(BW.record(qname="z%d_%d" % (n, at), tid=0, pos=i, cigar="%dM" % n, seq=_seq(rnd, n), qual=bytes(q), tags=[("RG", "Z", "grp1")])); i += 1
            q2 = bytearray(q); q2[at] = 255
            s.add(BW.record(qname="y%d_%d" % (n, at), tid=0, pos=i, cigar="%dM" % n, seq=_seq(rnd, n), qual=bytes(q2), tags=[("RG", "Z", "grp1")])); i += 1
    s.fill(1000)
    data = BW.bam_bytes([("chr1", 100000000)], s.recs, text=TEXT)
    exp = orc.bam_read(data)
    assert exp["n_rows"] == len(s.recs) and exp["status"] >= 0
    assert 2000 <= len(s.recs) <= 9000, len(s.recs)
    return data, exp, s.starts, want


def _scan(data, colmask=0x1FFF, packed=False, strings=True):
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(data); ctx.bgzf_index(); hdr = ctx.bam_open()
        if packed:
            ctx.set_seq_packed(True)
        parts, status = [], 0
        while True:
            b = ctx.next_batch(0, colmask=colmask)
            if b.n_rows:
                if strings:
                    parts.append(ctx.batch_to_host(b, hdr))
                else:
                    n = int(b.n_rows)
                    parts.append({"n_rows": n, "FLAG": ctx.d2h(b.flag, n, np.uint16), "POS": ctx.d2h(b.pos, n, np.int64), "MAPQ": ctx.d2h(b.mapq, n, np.int32),
                                  "PNEXT": ctx.d2h(b.pnext, n, np.int64), "TLEN": ctx.d2h(b.tlen, n, np.int64), "tid": ctx.d2h(b.tid, n, np.int32), "mtid": ctx.d2h(b.mtid, n, np.int32)})
            status = b.status
            if b.status != 0:
                break
        out = {"n_rows": sum(p["n_rows"] for p in parts), "status": status}
        for k in (parts[0] if parts else {}):
            if k != "n_rows" and k != "status":
                out[k] = np.concatenate([p[k] for p in parts]) if isinstance(parts[0][k], np.ndarray) else [x for p in parts for x in p[k]]
        return out
    finally:
        ctx.close()


def _same(got, exp, cols, ctx):
    assert got["n_rows"] == exp["n_rows"], (ctx, got["n_rows"], exp["n_rows"])
    assert (got["status"] < 0) == (exp["status"] < 0), (ctx, got["status"], exp["status"])
    for k in cols:
        a, b = got[k], exp[k]
        if isinstance(b, np.ndarray):
            assert np.array_equal(np.asarray(a), b), f"{ctx}: column {k} differs at row {int(np.argmax(np.asarray(a) != b))}"
        else:
            for r, (x, y) in enumerate(zip(a, b)):
                assert x == y, f"{ctx}: column {k} row {r}: {x!r:.80} != {y!r:.80}"
            assert len(a) == len(b), (ctx, k)


def test_every_column_with_all_columns_projected():
    data, exp, starts, want = _file()
    assert len(want) == len(SHAPES) * 2 * 35
    _same(_scan(data), exp, COLS, "all columns")


def test_fixed_columns_without_the_string_columns():
    data, exp, _, _ = _file()
    mask = sum(1 << b for b in (1, 3, 4, 7, 8))              # FLAG POS MAPQ PNEXT TLEN: no string pass, no walk to RG
    _same(_scan(data, colmask=mask, strings=False), exp, ["FLAG", "POS", "MAPQ", "PNEXT", "TLEN", "tid", "mtid"], "no strings")


def test_every_column_with_packed_seq():
    data, exp, _, _ = _file()
    _same(_scan(data, packed=True), exp, COLS, "packed SEQ")
