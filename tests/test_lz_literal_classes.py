"""Phase B's literal pass (lz_block, bgzf_inflate.hip) on hand-placed literal runs: every way a run can meet the windowed store body.

A run of 1..32 bytes whose destination does not wrap in the 4 KiB window ring is copied lane-parallel through overlapping windows (8..32
bytes: four 8-byte windows, 4..7: two 4-byte windows, 2..3: two 2-byte windows, 1: a byte), read from the 2 KiB literal staging ring,
which is filled in 1 KiB pieces and mirrors its first 32 bytes behind its end; longer runs and runs whose destination wraps keep the
exact-length store chain and the whole-wave byte loop.  The blocks built here hold runs of every length 1..40 and 64, 510, 511, 512,
1,023, each placed, for every k in 0..40, so that

  * "dend": its destination ends k bytes in front of a multiple of 4,096 (the window ring; it never wraps there, k = 0 touches the end),
  * "dbeg": its destination starts k bytes in front of such a multiple (it wraps when it is longer than k),
  * "s2048", "s1024": its first byte is k bytes in front of a multiple of 2,048 (the staging ring) or 1,024 (a staging piece) in the
    block's literal stream.

A block is one fixed-Huffman stream written by tests/deflate_writer.py's Stream from explicit symbol lists, with the filler of
test_lz_copy_classes.py: short tokens that keep every 64-token batch on the lane-parallel path.  Runs of up to 32 bytes and longer ones
go to blocks of their own: a run of 511 bytes or more is split into tokens by phase A, which would move the batch boundaries behind it,
and long runs may make a batch oversized (that branch is wanted, and counted); in the blocks of short runs the tokens are exactly the
ones listed here, and the CPU part adds up every batch of them.

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
import test_lz_copy_classes as C
from conftest import ROOT

RING = 4096                    # bytes of phase B's window ring
LENGTHS = list(range(1, 41)) + [64, 510, 511, 512, 1023]
WINDOWED_MAX = 32              # the longest run the windowed body takes
KS = range(0, 41)
KINDS = ("dend", "dbeg", "s2048", "s1024")
BLOCK_MAX = 65536


def _make_lit_unit(rng, ntok):
    """a literal-dense filler unit: ntok tokens of 3 literals and a 3-byte match that reaches back inside the unit only"""
    syms, made = [], 0
    for _ in range(ntok):
        syms += [rng.randrange(256) for _ in range(3)]
        made += 3
        syms.append((3, rng.randrange(3, made + 1)))
        made += 3
    s = C.FastStream()
    s._symbols(syms, W.canonical(W.FIXED_LL), W.FIXED_LL, W.canonical([5] * 32), [5] * 32)
    nbits = len(s.w.buf) * 8 + s.w.n
    value = int.from_bytes(bytes(s.w.buf), "little") | (s.w.acc << (len(s.w.buf) * 8))
    return syms, value, nbits, bytes(s.out)


LIT_UNITS = [_make_lit_unit(random.Random(510 + i), 30) for i in range(8)]
LIT_UNIT_LITS = 90


class Block(C.Block):
    """C.Block that counts its literals and advances to an exact output position, or an exact literal count, with a match as the last
    symbol: the literal run of a placement is then the placement's own"""

    def __init__(self, rng):
        super().__init__(rng)
        self.nlit = 0
        self.places = []

    def _account(self, syms):
        super()._account(syms)
        self.nlit += sum(1 for x in syms if isinstance(x, int))

    def _match(self, ln):
        return (ln, self.rng.randrange(ln, min(self.pos, 300) + 1))

    def advance_out(self, target):
        gap = target - self.pos
        assert gap == 0 or gap >= 3
        for units in (C.BIG_UNITS, C.SMALL_UNITS):
            while True:
                n = len(units[self.n_units % len(units)][3])
                if not (gap - n == 0 or gap - n >= 3):
                    break
                gap -= n
                self.unit(units)
        syms = []
        while gap >= 27:
            syms += [self.rng.randrange(256), self._match(15)]
            gap -= 16
        if gap:
            syms.append(self._match(gap))
        self._syms(syms)
        assert self.pos == target and self.run == 0

    def advance_lit(self, target):
        gap = target - self.nlit
        assert gap >= 0
        while gap >= LIT_UNIT_LITS:
            self.unit(LIT_UNITS)
            gap -= LIT_UNIT_LITS
        syms = []
        while gap:
            n = min(3, gap)
            syms += [self.rng.randrange(256) for _ in range(n)] + [self._match(3)]
            gap -= n
        self._syms(syms)
        assert self.nlit == target and self.run == 0

    def place(self, length, kind, k):
        """the run where its kind wants it, if the block has room for that"""
        if kind in ("dend", "dbeg"):
            t = self.pos + (-(self.pos + (length if kind == "dend" else 0) + k)) % RING
            if t - self.pos in (1, 2):
                t += RING
            if t + length + 64 > BLOCK_MAX:
                return False
            self.advance_out(t)
            assert (self.pos + (length if kind == "dend" else 0) + k) % RING == 0
        else:
            period = 2048 if kind == "s2048" else 1024
            t = self.nlit + (-(self.nlit + k)) % period
            if self.pos + 2 * (t - self.nlit) + length + 128 > BLOCK_MAX:
                return False
            self.advance_lit(t)
            assert (self.nlit + k) % period == 0
        self.places.append((length, kind, k, self.pos, self.nlit, len(self.tokens)))
        self._syms([self.rng.randrange(256) for _ in range(length)] + [self._match(5)])
        assert self.tokens[-1] == (length, 5)
        return True


def placements():
    short = [(n, kind, k) for n in LENGTHS if n <= WINDOWED_MAX for kind in KINDS for k in KS]
    long_ = [(n, kind, k) for n in LENGTHS if n > WINDOWED_MAX for kind in KINDS for k in KS]
    return short, long_


@functools.lru_cache(maxsize=None)
def build_blocks():
    """every placement in BGZF blocks: [(block bytes, output, raw deflate, tokens, places, holds long runs)]"""
    rng = random.Random(2048)
    blocks = []
    for is_long, queue in zip((False, True), placements()):
        queue = queue[::-1]
        while queue:
            b = Block(rng)
            b.unit(C.BIG_UNITS)
            while queue and b.place(*queue[-1]):
                queue.pop()
            assert b.places, "a placement that fits no block: %r" % (queue[-1],)
            blk, out, raw, tokens = b.finish()
            blocks.append((blk, out, raw, tokens, b.places, is_long))
    return blocks


def test_fixtures_are_valid_deflate():
    """zlib inflates every built stream to the bytes the writer says it means; no placement was dropped; the batches of the short runs'
    blocks stay on the lane-parallel path; the long and the wrapping runs are there"""
    blocks = build_blocks()
    short, long_ = placements()
    placed = [p[:3] for b in blocks for p in b[4]]
    assert sorted(placed) == sorted(short + long_) and len(placed) == len(LENGTHS) * len(KINDS) * len(KS)
    n_long = n_wrap = n_wrap_short = n_src_wrap = n_oversized = 0
    for blk, out, raw, tokens, places, is_long in blocks:
        d = zlib.decompressobj(-15)
        assert d.decompress(raw) == out and d.eof and not d.unused_data
        assert len(out) <= BLOCK_MAX and len(blk) <= 65536 and zlib.decompress(blk, 31) == out
        for t0 in range(0, len(tokens), 64):          # phase B's batches: 64 tokens, lane-parallel up to 1,536 bytes / 1,024 literals
            adv, lit = sum(a + b for a, b in tokens[t0:t0 + 64]), sum(a for a, _ in tokens[t0:t0 + 64])
            if is_long:
                n_oversized += adv > 1536 or lit > 1024      # (the boundaries behind a run of 511+ bytes are phase A's: a tally, no more)
            else:
                assert adv <= 1536 and lit <= 1024, (t0, adv, lit)
        for length, kind, k, pos, nlit, ti in places:
            assert is_long == (length > WINDOWED_MAX) and tokens[ti] == (length, 5)
            n_long += is_long
            wraps = pos // RING != (pos + length - 1) // RING
            n_wrap += wraps
            n_wrap_short += wraps and not is_long
            n_src_wrap += nlit // 2048 != (nlit + length - 1) // 2048
            if kind == "dbeg":
                assert wraps == (length > k > 0)
            if kind == "dend":
                assert not wraps or length > RING
    assert n_long == (8 + 5) * len(KINDS) * len(KS) and n_oversized > 0
    assert n_wrap_short >= sum(min(n, 41) - 1 for n in LENGTHS if n <= WINDOWED_MAX) and n_wrap > n_wrap_short
    assert n_src_wrap >= n_wrap_short


def run_gpu_cases():
    """all blocks through ctx.bgzf_inflate, 256 at a time: status 0 and zlib's bytes for every block"""
    import duckhts_amd
    blocks = build_blocks()
    f = b"".join(b[0] for b in blocks) + W.BGZF_EOF
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(f)
        nb = ctx.bgzf_index()
        assert nb == len(blocks) + 1, (nb, len(blocks))
        for b0 in range(0, len(blocks), 256):
            part = blocks[b0:b0 + 256]
            exp = b"".join(p[1] for p in part)
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
            "import test_lz_literal_classes as T\nprint('blocks ok', T.run_gpu_cases())\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DHTS_INFLATE="fused"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "blocks ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
