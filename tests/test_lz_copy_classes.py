"""Phase B's match copy (lz_block, bgzf_inflate.hip) on hand-placed matches: every way a match can meet the windowed copy body.

Ready matches of 3..32 bytes are copied lane-parallel through overlapping windows (8..32 bytes: four 8-byte windows, 4..7: two 4-byte
windows, 3: 2 + 1); the value of a window comes from the ring (near), from the replicated source byte (distance 1) or from registers
loaded from HBM (far: the source is older than the 4 KiB ring); a match that overlaps its source, wraps in the ring at its source or
destination, or is longer stays for the in-order replay.  The blocks built here aim at each of these:

  * every length 3..40 and 258, crossed with the distances 1, 2, 7, 8, 9, len - 1, len, len + 1, 2047, 2048, 4000, 4096, 4097, 32768
    (4096 and up are far), each placed so that its destination, and in a second placement its source, ends k bytes in front of the end
    of the ring, for every k in 0..40;
  * batches in which near matches read what a far match of each window class has just written (far copies are made by the first
    round, beside the near ones, so the near reader has to wait for them).

A block is one fixed-Huffman stream written by tests/deflate_writer.py's Stream from explicit symbol lists.  Phase B resolves 64 tokens
(a literal run and the match behind it) per batch, lane-parallel only when the batch advances the output by at most 1,536 bytes: a
filler token here advances it by at most 23 bytes (20 but for the first of a unit), so every batch of every block takes that path
whatever the placement adds; the CPU part adds up every batch to make sure.

The CPU part proves the fixtures: CPython's zlib inflates every stream to Stream.out.  The GPU part runs them through ctx.bgzf_inflate,
on the default path and with DHTS_INFLATE=fused (the other caller of lz_block; a child process, the knob is read once per process)."""
import functools
import os
import random
import subprocess
import sys
import zlib

import pytest

import deflate_writer as W
from conftest import ROOT

RING = 4096                    # bytes of phase B's window ring (B_RING_LOG2 = 12)
LENGTHS = list(range(3, 41)) + [258]
KS = range(0, 41)
TOKEN_MAX = 20                 # literals at the head of a filler unit; its other tokens advance the output by at most 19 bytes
BLOCK_MAX = 65536


def distances(mlen):
    return sorted({1, 2, 7, 8, 9, mlen - 1, mlen, mlen + 1, 2047, 2048, 4000, 4096, 4097, 32768})


class FastStream(W.Stream):
    """Stream with the meaning of a match computed by slices (the blocks here hold 64 KiB each)"""

    def _play(self, syms):
        out = self.out
        for s in syms:
            if isinstance(s, int):
                out.append(s)
                continue
            ln, d = s[0], s[1]
            assert d <= len(out)
            while ln:
                n = min(ln, d)
                p = len(out) - d
                out += out[p:p + n]
                ln -= n


def _make_unit(rng, ntok):
    """a filler unit: tokens of 0..3 literals and a match of 8..16 bytes that reaches back inside the unit only, so that its bits and
    its bytes are the same wherever it stands.  Returns (symbols, bits value, number of bits, output bytes)."""
    syms = [rng.randrange(256) for _ in range(TOKEN_MAX)]          # (the unit's first token: its literals and the first match)
    made = TOKEN_MAX
    first = True
    for _ in range(ntok):
        nl = 0 if first else rng.randrange(4)
        ln = rng.randrange(8, 17) if not first else 3
        first = False
        syms += [rng.randrange(256) for _ in range(nl)]
        made += nl
        syms.append((ln, rng.randrange(ln, made + 1)))
        made += ln
    s = FastStream()
    s._symbols(syms, W.canonical(W.FIXED_LL), W.FIXED_LL, W.canonical([5] * 32), [5] * 32)
    nbits = len(s.w.buf) * 8 + s.w.n
    value = int.from_bytes(bytes(s.w.buf), "little") | (s.w.acc << (len(s.w.buf) * 8))
    assert bytes(s.out) == bytes(_replay(syms))
    return syms, value, nbits, bytes(s.out)


def _replay(syms):
    s = FastStream()
    s._play(syms)
    return s.out


_rng = random.Random(20250)
# (the first token of a unit is 20 literals + a 3-byte match = 23 bytes; the batch budget below counts it)
BIG_UNITS = [_make_unit(_rng, 30) for _ in range(8)]
SMALL_UNITS = [_make_unit(_rng, 3) for _ in range(8)]


class Block:
    """one BGZF block under construction: a fixed-Huffman stream of filler and placements"""

    def __init__(self, rng):
        self.rng = rng
        self.s = FastStream()
        self.s.header(True, 1)
        self.n_units = 0
        self.placed = 0
        self.tokens, self.run = [], 0          # (literal run, match length) of every token so far

    @property
    def pos(self):
        return len(self.s.out)

    def _account(self, syms):
        for x in syms:
            if isinstance(x, int):
                self.run += 1
            else:
                self.tokens.append((self.run, x[0]))
                self.run = 0

    def _syms(self, syms):
        self._account(syms)
        self.s._symbols(syms, W.canonical(W.FIXED_LL), W.FIXED_LL, W.canonical([5] * 32), [5] * 32)

    def unit(self, units):
        syms, value, nbits, out = units[self.n_units % len(units)]
        self.n_units += 1
        self._account(syms)
        self.s.raw(value, nbits)
        self.s.out += out

    def advance_to(self, target):
        """filler up to output position `target`: units, then tokens of one literal and a match, then at most 8 literals (they become
        the literal run of the placement's first token)"""
        gap = target - self.pos
        assert gap >= 0
        for units in (BIG_UNITS, SMALL_UNITS):
            while gap >= len(units[self.n_units % len(units)][3]):
                gap -= len(units[self.n_units % len(units)][3])
                self.unit(units)
        syms = []
        while gap > 8:
            ln = 16 if gap >= 24 else gap - 4
            syms += [self.rng.randrange(256), (ln - 1, self.rng.randrange(ln - 1, min(self.pos, 300) + 1))]
            gap -= ln
        syms += [self.rng.randrange(256) for _ in range(gap)]
        self._syms(syms)
        assert self.pos == target

    def finish(self):
        self.s.fixed_code(256)
        return W.bgzf_block(self.s.bytes(), bytes(self.s.out)), bytes(self.s.out), self.s.bytes(), self.tokens


def placements():
    """(symbols, offset, k, reach): the symbols go where (start + offset) is k bytes in front of a ring end; `reach` is the largest
    distance, i.e. the least start"""
    near, deep = [], []
    for mlen in LENGTHS:
        for d in distances(mlen):
            for k in KS:
                for off in (mlen, mlen - d):                       # destination / source ends at the ring's end - k
                    (deep if d > 8192 else near).append(([(mlen, d)], off, k, d))
    # near matches that read a far match's destination: behind a far match of each window class, a reader of its first bytes, one of
    # its last bytes (through a literal), one that overlaps it from 2 bytes in front, and a reader of the reader
    for flen in (3, 4, 5, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 40):
        for fd in (4096, 4097, 5000, 32768):
            for k in (0, 1, 7, 8, 33, 100, 2000):
                a = min(flen, 11)
                syms = [(flen, fd), (a, flen), 65, (min(flen, 6), min(flen, 6) + 1), (flen + 2, flen + a + 1 + min(flen, 6) + 2), 66, 67,
                        (9, 9 + 2), (3, 3)]
                (deep if fd > 8192 else near).append((syms, flen, k, fd))
    return near, deep


def _span(syms):
    return sum(1 if isinstance(s, int) else s[0] for s in syms)


@functools.lru_cache(maxsize=None)
def build_blocks():
    """every placement in BGZF blocks: [(block bytes, output, raw deflate, tokens)], and the number of placements"""
    rng = random.Random(4096)
    near, deep = placements()
    near.reverse()
    deep.reverse()
    blocks, total = [], len(near) + len(deep)
    while near or deep:
        b = Block(rng)
        b.unit(BIG_UNITS)
        while True:
            # the far-reaching placements need 32 KiB in front of them: they take the block's second half
            q = deep if deep and (b.pos + RING >= 32768 or not near) else near
            if not q:
                break
            syms, off, k, reach = q[-1]
            start = max(b.pos, reach)
            start += (-(start + off) - k) % RING
            if start + _span(syms) + 64 > BLOCK_MAX:
                break
            q.pop()
            b.advance_to(start)
            assert (b.pos + off + k) % RING == 0 and b.pos >= reach
            b._syms(syms)
            b.placed += 1
        assert b.placed, "a placement that fits no block"
        blocks.append(b.finish())
    return blocks, total


def test_fixtures_are_valid_deflate():
    """zlib inflates every built stream to the bytes the writer says it means; every placement is in a block; the batches stay small"""
    blocks, total = build_blocks()
    near, deep = placements()
    assert total == len(near) + len(deep) and total > 2 * 41 * 39 * 10
    for blk, out, raw, tokens in blocks:
        for t0 in range(0, len(tokens), 64):          # phase B's batches: 64 tokens, lane-parallel up to 1,536 bytes / 1,024 literals
            assert sum(a + b for a, b in tokens[t0:t0 + 64]) <= 1536 and sum(a for a, _ in tokens[t0:t0 + 64]) <= 1024
        d = zlib.decompressobj(-15)
        assert d.decompress(raw) == out and d.eof and not d.unused_data
        assert len(out) <= BLOCK_MAX and len(blk) <= 65536
        assert zlib.decompress(blk, 31) == out


def test_every_placement_is_reached():
    """the cross product the module's docstring promises, counted"""
    near, deep = placements()
    single = [(s[0], off, k) for s, off, k, _ in near + deep if len(s) == 1]
    want = {((m, d), off, k) for m in LENGTHS for d in distances(m) for k in KS for off in (m, m - d)}
    assert set(single) == want and len(single) == len(want)
    assert {d for (m, d), _, _ in want} >= {1, 2, 7, 8, 9, 2047, 2048, 4000, 4096, 4097, 32768}


def run_gpu_cases():
    """all blocks through ctx.bgzf_inflate, 256 at a time: status 0 and zlib's bytes for every block"""
    import duckhts_amd
    blocks, _ = build_blocks()
    f = b"".join(b[0] for b in blocks) + W.BGZF_EOF
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(f)
        nb = ctx.bgzf_index()
        assert nb == len(blocks) + 1, (nb, len(blocks))
        for b0 in range(0, len(blocks), 256):
            part = blocks[b0:b0 + 256]
            exp = b"".join(zlib.decompress(p[0], 31) for p in part)
            out, bst = ctx.bgzf_inflate(b0, len(part), len(exp) + 64)
            assert [int(x) for x in bst] == [0] * len(part), (b0, [int(x) for x in bst])
            got = out.tobytes()
            if got != exp:
                at = next(i for i in range(min(len(got), len(exp))) if got[i] != exp[i]) if len(got) == len(exp) else -1
                raise AssertionError("blocks %d..: output differs from zlib's at byte %d (lengths %d / %d)" % (b0, at, len(got), len(exp)))
    finally:
        ctx.close()
    return len(blocks)


@pytest.mark.gpu
def test_gpu_inflate_matches_zlib():
    assert run_gpu_cases() > 0


@pytest.mark.gpu
def test_gpu_inflate_matches_zlib_fused():
    """the same through bgzf_inflate_fused, which resolves a block in the wave that decoded it (it shares lz_block)"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_lz_copy_classes as T\nprint('blocks ok', T.run_gpu_cases())\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DHTS_INFLATE="fused"), capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0 and "blocks ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
