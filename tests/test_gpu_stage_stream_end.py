"""The stream's end inside a staged window: every column against the oracle for files whose inflated batch ends at chosen bytes.

A tile's wave stages tile + 9,216 bytes in 16-byte pieces, nine pieces per lane (five at 128 threads), all loads issued before the first
wait.  A piece at or past the stream's padded end is not loaded from there: its address is clamped to the tile's first bytes and what it
stores lands behind the window's valid length.  What can go wrong is therefore the end of the stream inside a window -- a piece that is
clamped although it holds bytes of the stream, a piece that is not clamped although it lies past the padding, a clamped piece whose
bytes are read as if they were the stream's.  The files here end `d` bytes behind 1,024 * j (the pieces of one round of the 64 lanes) for
j in 0..9 and d in -17, -16, -1, 0, 1, 15, 16 (j = 0 has no negative d), which includes one tile exactly (8,192) and one window exactly
(9,216); the same lengths again behind two whole tiles, so that the window that holds the end is not tile 0's.  The header sits in BGZF
blocks of its own, so the batch is the record stream and its length is the sum of the record lengths.  Every file's last record ends on
the stream's last byte: with QUAL as its last field (the 16-byte chunk reads of SEQ and QUAL then reach past the stream's end) or with the
RG value.  Lengths below the shortest record (1, 15, 16) are the first bytes of a record: a truncated file, an error on both sides.

Each file is read as one batch and with max_blocks 1 and 3 (BGZF blocks of 1,000 bytes: the batches then end inside records and the
carried bytes move every later window), with all columns, without the string columns and with packed SEQ.  BCF: the same lengths (header
included, so j >= 1) through bcf_tile_scan, as one batch and with max_blocks 1."""
import functools
import random

import numpy as np
import pytest

import bamwriter as BW
import bcfwriter as CW
import duckhts_amd
import orc

pytestmark = pytest.mark.gpu

TILE, WINDOW = 8192, 9216
COLS = duckhts_amd.BAM_COLUMNS
TEXT = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:100000000\n@RG\tID:grp1\tSM:s1\n"
D = (-17, -16, -1, 0, 1, 15, 16)
BASES = (0, 2 * TILE)
PAYLOAD = 1000
FIXED = ["FLAG", "POS", "MAPQ", "PNEXT", "TLEN", "tid", "mtid"]


def _sizes(j):
    return [1024 * j + d for d in D if 1024 * j + d >= 0]


def _bases(rnd, n):
    return "".join(rnd.choice("ACGTN") for _ in range(n))


def _filler(i, l_seq, pad):
    rnd = random.Random(i)
    return BW.record(qname="f%d" % (i % 10), flag=0, tid=0, pos=i, mapq=9, cigar="%dM" % l_seq, seq=_bases(rnd, l_seq),
                     qual=bytes(rnd.randrange(0, 60) for _ in range(l_seq)), tags=[("RG", "Z", "grp1"), ("XX", "Z", "p" * pad)])


def _tail(kind):
    """the last record: 33 bases (two whole 16-byte chunks and one byte), QUAL last ("qual") or the RG value last ("rg")"""
    rnd = random.Random(5)
    return BW.record(qname="t", flag=0, tid=0, pos=77, mapq=40, cigar="33M", seq=_bases(rnd, 33), qual=bytes(rnd.randrange(0, 90) for _ in range(33)),
                     tags=[] if kind == "qual" else [("RG", "Z", "grp1")])


MINF = len(_filler(0, 60, 0))


def _records(length, kind):
    """records whose lengths sum to `length` exactly, the tail last"""
    tail = _tail(kind)
    if length < len(tail):
        return [tail[:length]] if length else []              # the first bytes of a record: a truncated file
    front = length - len(tail)
    assert front == 0 or front >= MINF, (length, front)
    rnd, recs, pos = random.Random(length), [], 0
    while front - pos >= 2000:                                  # reads of 60, 151, 600 (a "long" field) and 33 bases
        recs.append(_filler(len(recs), (60, 151, 600, 33)[len(recs) % 4], rnd.randrange(0, 40))); pos += len(recs[-1])
    if front - pos:
        recs.append(_filler(len(recs), 60, front - pos - MINF)); pos += len(recs[-1])
    assert pos == front
    return recs + [tail]


@functools.lru_cache(maxsize=None)
def _bam(length, kind):
    recs = _records(length, kind)
    assert sum(len(r) for r in recs) == length
    data = BW.bam_bytes([("chr1", 100000000)], recs, text=TEXT, payload=PAYLOAD)
    return data, orc.bam_read(data)


def _scan(data, max_blocks, colmask=0x1FFF, packed=False, strings=True):
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(data); ctx.bgzf_index(); hdr = ctx.bam_open()
        if packed:
            ctx.set_seq_packed(True)
        parts, status = [], 0
        while True:
            b = ctx.next_batch(max_blocks, colmask=colmask)
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
    if not exp["n_rows"]:
        return
    for k in cols:
        a, b = got[k], exp[k]
        if isinstance(b, np.ndarray):
            assert np.array_equal(np.asarray(a), b), f"{ctx}: column {k} differs at row {int(np.argmax(np.asarray(a) != b))}"
        else:
            for r, (x, y) in enumerate(zip(a, b)):
                assert x == y, f"{ctx}: column {k} row {r}: {x!r:.80} != {y!r:.80}"
            assert len(a) == len(b), (ctx, k)


def _cases(j):
    """(length, kind of the last record): every size of class j at both bases; the two kinds alternate, the other way round at the other base"""
    for bi, base in enumerate(BASES):
        for di, size in enumerate(_sizes(j)):
            yield base + size, ("qual", "rg")[(bi + di) % 2]


@pytest.mark.parametrize("j", range(10))
def test_all_columns(j):
    for length, kind in _cases(j):
        data, exp = _bam(length, kind)
        if length >= 1000:
            assert exp["n_rows"] >= 1 and exp["status"] >= 0, (length, exp["n_rows"], exp["status"])
        for mb in (0, 1, 3):
            _same(_scan(data, mb), exp, COLS, f"length {length}, last field {kind}, max_blocks {mb}")


@pytest.mark.parametrize("j", range(10))
def test_without_the_string_columns(j):
    mask = sum(1 << b for b in (1, 3, 4, 7, 8))              # FLAG POS MAPQ PNEXT TLEN: no string pass, no walk to RG
    for length, kind in _cases(j):
        data, exp = _bam(length, kind)
        for mb in (0, 1, 3):
            _same(_scan(data, mb, colmask=mask, strings=False), exp, FIXED, f"no strings: length {length}, last field {kind}, max_blocks {mb}")


@pytest.mark.parametrize("j", range(10))
def test_packed_seq(j):
    for length, kind in _cases(j):
        data, exp = _bam(length, kind)
        for mb in (0, 1, 3):
            _same(_scan(data, mb, packed=True), exp, COLS, f"packed SEQ: length {length}, last field {kind}, max_blocks {mb}")


def test_one_tile_and_one_window_exactly():
    """the lengths the loop above names as 1,024 * 8 and 1,024 * 9 with d = 0, spelled out: a stream of one tile exactly has no second tile,
    a stream of one window exactly fills tile 0's window to its last byte and is tile 1's first 1,024 bytes"""
    for length in (TILE, WINDOW):
        for kind in ("qual", "rg"):
            data, exp = _bam(length, kind)
            assert sum(len(r) for r in _records(length, kind)) == length and exp["status"] >= 0
            for mb in (0, 1, 3):
                _same(_scan(data, mb), exp, COLS, f"length {length}, last field {kind}, max_blocks {mb}")


# ---- BCF (bcf_tile_scan stages its tiles the same way) --------------------------------------------------------------------------------
BCF_HEADER = CW.header(['##INFO=<ID=XD,Number=.,Type=Integer,Description="d">'], contigs=("1", "2"))


def _bcf_record(i, id_len):
    return CW.record(rid=i % 2, pos=10 * i, rlen=1, qual=float(i % 50), id=b"i" * id_len, alleles=(b"A", b"TG"[i % 2:i % 2 + 1]),
                     info=[(1, CW.tv_ints([i % 100, 5, 7][:1 + i % 3], width=1))])


@functools.lru_cache(maxsize=None)
def _bcf(length):
    """a BCF file whose inflated stream (header and records) is `length` bytes: the last records' ID lengths make up the difference"""
    head = len(CW.bcf_raw(BCF_HEADER, []))
    recs, pos = [], head
    while length - pos >= 400:
        recs.append(_bcf_record(len(recs), len(recs) % 20)); pos += len(recs[-1])
    for a in range(0, 300):                                     # two records: every remainder is reachable although the length prefix of a string grows at 15 bytes
        for b in range(0, 40):
            two = [_bcf_record(len(recs), a), _bcf_record(len(recs) + 1, b)]
            if pos + len(two[0]) + len(two[1]) == length:
                raw = CW.bcf_raw(BCF_HEADER, recs + two)
                assert len(raw) == length
                data = BW.bgzf_file(raw, payload=PAYLOAD)
                return data, orc.bcf_read(data)
    raise AssertionError(("no BCF stream of this length", length))


@pytest.mark.parametrize("j", range(1, 10))
def test_bcf_every_column(j):
    for base in BASES:
        for size in _sizes(j):
            data, exp = _bcf(base + size)
            assert exp["n_rows"] >= 2
            for mb in (0, 1):
                got = duckhts_amd.read_bcf(data, device=0, max_blocks=mb)
                assert got["n_rows"] == exp["n_rows"], (base + size, mb, got["n_rows"], exp["n_rows"])
                assert orc.bcf_cols_diff(exp, got) is None, (base + size, mb, orc.bcf_cols_diff(exp, got))
