"""Phase B's CRC epilogue (lz_block, bgzf_inflate.hip) on every tail length.

A block's output is flushed in 2,048-byte chunks whose CRC every lane carries as one state over its 32-byte piece; the bytes behind the
last full chunk (outlen mod 2,048 of them) are one more, short chunk, and the 64 states are combined by table multiplications whose
constants depend on how many whole pieces and how many odd bytes the tail holds.  So the blocks here have

  * every inflated length 0..6,143: every tail length 0..2,047 behind 0, 1 and 2 flushed chunks;
  * 63,488 + n (31 chunks) for n in 0, 1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 1,023, 1,024, 2,046, 2,047;
  * 65,280 and 65,536 bytes.

The content cycles with the length over three kinds: stored (level 0, framed here as one final stored block so that the stream ends with
data bytes whatever the zlib at hand writes: long literal runs, the oversized-batch branch), compressible text at level 6, random
bytes at level 1.  A BGZF block holds at most 65,536 bytes with its 26 bytes of framing, so where a length's
kind does not fit (stored or random data of 65,5xx bytes) the next kind of the cycle is taken; text always fits.

The CPU part proves the fixtures: CPython's zlib inflates every block to the expected bytes.  The GPU part runs them through
ctx.bgzf_inflate, on the default path and with DHTS_INFLATE=fused (the other caller of lz_block; a child process, the knob is read
once per process), and expects zlib's bytes and status 0 of every block.  The negative part damages one bit of the trailer's CRC field
(every 97th block, and the blocks with tail length 0, 1, 4 and 2,047), and in a second copy one payload bit of the stored blocks among
them: a one-block file inflated alone must report DHTS_BLK_ERR_CRC."""
import functools
import os
import random
import struct
import subprocess
import sys
import zlib

import pytest

import deflate_writer as W
from conftest import ROOT

FLUSH = 2048                   # bytes of a flush chunk (half of phase B's 4 KiB window ring)
BLK_ERR_CRC = -4               # DHTS_BLK_ERR_CRC (dhts_common.h)
LENGTHS = list(range(0, 3 * FLUSH)) + [31 * FLUSH + n for n in (0, 1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 1023, 1024, 2046, 2047)] + [65280, 65536]
KINDS = ("stored", "text", "random")
WORDS = ("chr1 chr2 chrX 60 255 * = 0 101M 76M25S 3S98M NM:i:0 MD:Z:101 AS:i:101 XS:i:87 RG:Z:grp1 ACGT TTAGGG GATTACA CCCCAAAATTTT "
         "IIIIIIIIHHHHGGFF #### read pair mate proper").split()


@functools.lru_cache(maxsize=None)
def _pools():
    rng = random.Random(2048)
    text = []
    n = 0
    while n < 3 * 65536:
        w = rng.choice(WORDS) + ("\t" if rng.randrange(8) else "\n")
        text.append(w)
        n += len(w)
    return "".join(text).encode(), rng.randbytes(3 * 65536)


def _deflate(data, level):
    if level == 0 and len(data) < 65536:              # one final stored block, as zlib >= 1.2.12 writes it: the stream ends with data
        return b"\x01" + struct.pack("<HH", len(data), len(data) ^ 0xffff) + data
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def make_block(length):
    """(kind, BGZF block, raw DEFLATE stream, expected bytes) of one length"""
    text, rnd = _pools()
    off = (length * 7919) % 65536
    for step in range(3):
        kind = KINDS[(length + step) % 3]
        data = (rnd if kind == "random" else text)[off:off + length]
        raw = _deflate(data, {"stored": 0, "text": 6, "random": 1}[kind])
        if 26 + len(raw) <= 65536:
            return kind, W.bgzf_block(raw, data), raw, data
    raise AssertionError("no kind of %d bytes fits a BGZF block" % length)


@functools.lru_cache(maxsize=None)
def build_blocks():
    return [make_block(n) for n in LENGTHS]


def negative_cases():
    """indices into build_blocks(): every 97th block and every block whose tail length is 0, 1, 4 or 2,047"""
    return [i for i, n in enumerate(LENGTHS) if i % 97 == 0 or n % FLUSH in (0, 1, 4, 2047)]


def damaged(blk, payload_bit):
    """a copy of a block with one bit flipped: of the trailer's CRC field, or of the last payload byte (of a stored block: a data byte)"""
    b = bytearray(blk)
    b[-9 if payload_bit else -6] ^= 0x10
    return bytes(b)


def test_fixtures_are_valid_deflate():
    """zlib inflates every block to the expected bytes; every tail length occurs behind 0, 1 and 2 chunks; all three kinds are there"""
    blocks = build_blocks()
    assert len(blocks) == 3 * FLUSH + 18
    assert {(len(d) // FLUSH, len(d) % FLUSH) for _, _, _, d in blocks} >= {(c, t) for c in range(3) for t in range(FLUSH)}
    kinds = {k: 0 for k in KINDS}
    for (kind, blk, raw, data), n in zip(blocks, LENGTHS):
        kinds[kind] += 1
        d = zlib.decompressobj(-15)
        assert len(data) == n and d.decompress(raw) == data and d.eof and not d.unused_data
        assert len(blk) <= 65536 and zlib.decompress(blk, 31) == data
    assert min(kinds.values()) >= FLUSH - 8, kinds
    assert sum(len(d) for _, _, _, d in blocks) > 18_000_000
    neg = negative_cases()
    assert {LENGTHS[i] % FLUSH for i in neg} >= {0, 1, 4, 2047} and len(neg) >= len(LENGTHS) // 97 + 4 * 3
    stored = [i for i in neg if blocks[i][0] == "stored" and LENGTHS[i] > 0]
    assert stored
    for i in stored:                                  # the damaged payload still inflates, to other bytes: only the CRC can tell
        bad = zlib.decompressobj(-15).decompress(damaged(blocks[i][1], True)[18:-8])
        assert len(bad) == LENGTHS[i] and bad != blocks[i][3]


def _first_difference(got, exp):
    return next((i for i in range(min(len(got), len(exp))) if got[i] != exp[i]), min(len(got), len(exp)))


def run_gpu_cases():
    """all blocks through ctx.bgzf_inflate, 512 at a time: status 0 and zlib's bytes for every block; then the damaged one-block files"""
    import duckhts_amd
    blocks = build_blocks()
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(b"".join(b[1] for b in blocks) + W.BGZF_EOF)
        nb = ctx.bgzf_index()
        assert nb == len(blocks) + 1, (nb, len(blocks))
        for b0 in range(0, len(blocks), 512):
            part = blocks[b0:b0 + 512]
            exp = b"".join(p[3] for p in part)
            out, bst = ctx.bgzf_inflate(b0, len(part), len(exp) + 64)
            bad = [(LENGTHS[b0 + i], int(x)) for i, x in enumerate(bst) if int(x) != 0]
            assert not bad, "blocks of these lengths report a status: %r" % bad[:20]
            got = out.tobytes()
            assert got == exp, "blocks %d..: output differs from zlib's at byte %d (lengths %d / %d)" % (b0, _first_difference(got, exp), len(got), len(exp))
    finally:
        ctx.close()
    n_bad = 0
    for i in negative_cases():
        kind, blk, _, data = blocks[i]
        for payload_bit in (False, True):
            if payload_bit and not (kind == "stored" and data):
                continue
            ctx = duckhts_amd.Context(0)
            try:
                ctx.open(damaged(blk, payload_bit) + W.BGZF_EOF)
                assert ctx.bgzf_index() == 2
                _, bst = ctx.bgzf_inflate(0, 1, len(data) + 64)
            finally:
                ctx.close()
            assert int(bst[0]) == BLK_ERR_CRC, (LENGTHS[i], kind, payload_bit, int(bst[0]))
            n_bad += 1
    return len(blocks), n_bad


@pytest.mark.gpu
def test_gpu_inflate_every_tail_length():
    n, n_bad = run_gpu_cases()
    assert n == len(LENGTHS) and n_bad > len(negative_cases())


@pytest.mark.gpu
def test_gpu_inflate_every_tail_length_fused():
    """the same through bgzf_inflate_fused, which resolves a block in the wave that decoded it (it shares lz_block)"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_lz_crc_tail as T\nprint('blocks ok', T.run_gpu_cases())\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DHTS_INFLATE="fused"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "blocks ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
