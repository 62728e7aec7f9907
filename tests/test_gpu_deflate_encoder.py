"""The device DEFLATE encoder (duckhts_amd/csrc/bgzf_deflate.hip) on inputs built to reach its branches.

zlib reading a member back proves the stream valid; it does not show that the encoder decided by its own rules, nor that a branch was
reached.  So every member is also parsed token by token (tests/deflate_reader.py) and held to the CPU restatement of the encoder's rules
(tests/deflate_code_ref.py): the header's lengths are the ones the builder makes of the counts in the same stream, the block type is the
smallest of the three, the payload's size is the predicted one.  Every case then asserts, from the parsed stream, the property it was
built for -- a case that stops reaching its branch fails.  Bytes are never compared across runs (the hash insert is a race by design).

How the inputs are built (the parse: 64 positions per step; a lane's candidates are the two last positions of its bucket entered in
EARLIER steps; every position is entered, covered by a match or not): a match at an exact distance d is a fresh 8-byte key at p - d and
again at p, p the first position of a step; what lies between is zeros, which fill one bucket only and so evict nothing.
"""
import random
import time

import numpy as np
import pytest

import deflate_code_ref as Cr
import deflate_reader as R
import deflate_writer as W
from test_bgzip import bgzf_members, check_file

pytestmark = pytest.mark.gpu
LEVELS = (-1, 1, 6)
BLK = 65280


@pytest.fixture(scope="module")
def ctx():
    import duckhts_amd
    c = duckhts_amd.Context(0)
    yield c
    c.close()


# ---- the checks on every input and member -----------------------------------------------------------------------------------------------
class Member:
    """one parsed member: blk (deflate_reader.Block), raw (its input), syms (the tokens' symbols), pos (each token's offset in raw)"""

    def __init__(self, blk, raw, pay):
        self.blk, self.raw, self.pay = blk, raw, pay
        self.syms = [t[0] for t in blk.tokens]
        self.pos, at = [], 0
        for s in self.syms:
            self.pos.append(at)
            at += 1 if isinstance(s, int) else s[0]
        self.matches = [s for s in self.syms if not isinstance(s, int)]

    def token_at(self, p):
        return self.syms[self.pos.index(p)] if p in self.pos else None


def check_member(pay, piece, level):
    p = R.parse(pay, max_out=65536)
    assert len(p.blocks) == 1 and p.blocks[0].final == 1 and p.out == piece and (p.nbits + 7) // 8 == len(pay)
    b = p.blocks[0]
    m = Member(b, piece, pay)
    if level == 0:
        assert b.btype == 0 and len(pay) == len(piece) + 5
        return m
    if b.btype == 0:
        assert len(pay) == len(piece) + 5                       # (a stored block does not show its tokens: the choice is checked on the others)
        return m
    assert R.replay(b.tokens) == piece
    assert all(4 <= s[0] <= 258 and 1 <= s[1] <= 32768 for s in m.matches)
    ch = Cr.block_choice(m.syms, len(piece))
    assert b.btype == ch["btype"], (b.btype, ch["btype"], ch["dyn_bits"], ch["fix_bits"], len(piece))
    assert len(pay) == ch["nbytes"] and p.nbits == (ch["dyn_bits"] if b.btype == 2 else ch["fix_bits"])
    if b.btype == 2:
        assert (b.hlit, b.hdist, b.hclen) == (ch["hlit"], ch["hdist"], ch["hclen"])
        assert b.ll_lens == ch["ll_lens"][:b.hlit] and b.d_lens == ch["d_lens"][:b.hdist]
        assert b.cl_items == ch["cl_items"] and b.cl_lens == ch["cl_lens"]
    return m


def compress_checked(ctx, raw, level):
    """[Member] of raw compressed at level, every check made"""
    z = ctx.bgzf_compress(raw, level)
    check_file(raw, z)
    return [check_member(pay, raw[k * BLK:(k + 1) * BLK], level) for k, (pay, _, _) in enumerate(bgzf_members(z)[:-1])]


def at_levels(ctx, raw, prop, levels=LEVELS):
    for level in levels:
        prop(compress_checked(ctx, raw, level), level)


# ---- builders ------------------------------------------------------------------------------------------------------------------------
def rand_bytes(n, seed, alphabet=None):
    r = random.Random(seed)
    return bytes(r.choice(alphabet) for _ in range(n)) if alphabet is not None else r.randbytes(n)


def fresh(n, seed, alphabet=range(1, 256)):
    """n bytes without a repeated 4-byte group (so: no matches), none of them zero"""
    r, out, seen = random.Random(seed), bytearray(), set()
    alphabet = list(alphabet)
    while len(out) < n:
        out.append(r.choice(alphabet))
        if len(out) >= 4:
            g = bytes(out[-4:])
            if g in seen:
                out.pop()
                continue
            seen.add(g)
    return bytes(out)


class Layout:
    """a zero-filled buffer that keys are placed in; refuses overlaps"""

    def __init__(self, n):
        self.b, self.used = bytearray(n), np.zeros(n, bool)

    def put(self, at, data):
        assert at >= 0 and at + len(data) <= len(self.b) and not self.used[max(at - 1, 0):at + len(data) + 1].any(), at
        self.b[at:at + len(data)] = data
        self.used[at:at + len(data)] = True


def exact_distance_input(dists, seed, first_base=32768 + 64, n=None):
    """(bytes, [(p, d)]): for every d a match at distance exactly d that starts at p, p the first position of a step"""
    r = random.Random(seed)
    L = Layout(first_base + 256 * (len(dists) + 1) if n is None else n)
    base, where = first_base, []
    for d in dists:
        while True:
            assert base + 64 <= len(L.b), "no room left"
            try:
                if d >= 10:                                   # (the bytes around the keys differ, and so do the keys' first bytes:
                    key = bytes([4 + len(where)]) + fresh(7, r.getrandbits(30), range(100, 256))      # nothing else matches at p - 1 or p)
                    L.put(base - d - 1, b"\x03" + key + b"\x01")
                    L.put(base, key + b"\x02")
                else:                                         # the copy overlaps its source: one period of d distinct bytes, then 12 more
                    unit = bytes(r.sample(range(100, 256), d))
                    L.put(base - d, (unit * 24)[:d + 12] + b"\x01")
                break
            except AssertionError:
                base += 64
        where.append((base, d))
        base += 128
    return bytes(L.b), where


# ---- the code builder on the device, against its restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("nsym,maxbits", Cr.ALPHABETS)
def test_device_code_builder_equals_the_restatement(ctx, nsym, maxbits):
    """dfl_build_lengths + dfl_assign_codes through dhts_debug_deflate_codes, every vector of tests/test_deflate_code_ref.py in one launch;
    only vectors the CPU restatement has carried through to a complete code are sent"""
    import test_deflate_code_ref as T
    vecs, exp_l, exp_c, n_over = [], [], [], 0
    for name, v in T.families(nsym, maxbits):
        info = {}
        lens = Cr.build_lengths(v, maxbits, info)
        assert sum((1 << maxbits) >> l for l in lens if l) == 1 << maxbits
        n_over += info["oversubscribed"]
        vecs.append(v); exp_l.append(lens); exp_c.append(Cr.table_words(lens))
    assert n_over >= 20
    lens, codes = ctx.debug_deflate_codes(np.array(vecs, np.uint32), maxbits)
    bad = np.nonzero((lens != np.array(exp_l, np.uint8)).any(axis=1) | (codes != np.array(exp_c, np.uint32)).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), T.families(nsym, maxbits)[bad[0]], lens[bad[0]].tolist(), exp_l[bad[0]])


# ---- built inputs, end to end ----------------------------------------------------------------------------------------------------------
def wide_token_input():
    """12 KB of fresh literals; 17 KB over a 4-letter alphabet (short near matches, few buckets touched: the literals' buckets survive);
    then 60 pieces of 131..257 bytes of the first part again, more than 16,384 behind their source, each used once"""
    r = random.Random(7)
    src = fresh(12300, 70)
    out = bytearray(src) + rand_bytes(17000, 71, b"\x00\x40\x80\xc0")
    at = 0
    for k in range(60):
        ln = r.randint(131, 257)
        out += src[at:at + ln] + rand_bytes(r.randint(60, 200), 72 + k, b"\x00\x40\x80\xc0")
        at += ln + 3
    assert at <= len(src)
    return bytes(out)


def test_wide_tokens_reach_the_third_word(ctx):
    """the bit packer's third atomicOr: a token with (start bit % 32) + width > 64.  On the device: 28 long far matches, the widest token 39 bits
    (40 at level 1), 3 tokens (5) that reach a third word"""
    raw = wide_token_input()
    assert len(raw) <= BLK

    def prop(ms, level):
        b = ms[0].blk
        far = [t for t in b.tokens if not isinstance(t[0], int) and t[0][0] >= 131 and t[0][1] > 16384]
        widest = max(t[2] for t in b.tokens)
        spill = [t for t in b.tokens if t[1] % 32 + t[2] > 64]
        print(f"wide tokens, level {level}: {len(far)} long far matches, widest token {widest} bits, {len(spill)} tokens reach a third word")
        assert b.btype == 2 and len(far) >= 24 and widest >= 34 and spill
    at_levels(ctx, raw, prop)


def test_fifteen_bit_literal_code_is_used(ctx):
    """>= 16,385 tokens and a byte value that occurs once: its Shannon length is the cap, and it keeps it"""
    body = bytearray(fresh(40000, 15, range(1, 101)))
    r = random.Random(16)
    at = r.sample(range(0, 40000, 3), 200 + 100 + 50 + 25 + 12 + 6 + 3 + 1 + 1)
    # the completing loop hands what is left of the code space down the ranks; a symbol of each length 8..14 and one more of 15 bits in
    # front of 0xEE take it up binary digit by digit, and nothing is left for 0xEE and the end of block
    for v, c in zip(range(0xE0, 0xE8), (200, 100, 50, 25, 12, 6, 3, 1)):
        for _ in range(c):
            body[at.pop()] = v
    body[at.pop()] = 0xEE
    raw = bytes(body)

    def prop(ms, level):
        b = ms[0].blk
        assert b.btype == 2 and len(b.tokens) >= 16385 and raw.count(0xEE) == 1
        assert b.ll_lens[0xEE] == 15 and [t for t in b.tokens if t[0] == 0xEE][0][2] == 15
    at_levels(ctx, raw, prop)


def period_input(period):
    return (fresh(300, 32) + bytes(period - 300)) * 2


def test_distance_32768_is_taken_and_32769_refused(ctx):
    def taken(ms, level):
        assert any(s[1] == 32768 for s in ms[0].matches)
    at_levels(ctx, period_input(32768)[:BLK], taken)

    def refused(ms, level):
        assert max(s[1] for s in ms[0].matches) <= 32768
        # the second copy of the key has no candidate within reach: literals (its first bytes at least, before it can match itself)
        assert all(isinstance(ms[0].token_at(32769 + k), int) for k in range(8))
    at_levels(ctx, period_input(32769)[:BLK], refused)


def test_every_distance_code_at_both_ends(ctx):
    ends = sorted({d for c in range(30) for d in (W.DIST_BASE[c], W.DIST_BASE[c] + (1 << W.DIST_EXTRA[c]) - 1)})
    raw, where = exact_distance_input(ends, 5)
    assert len(ends) == 56 and len(raw) <= BLK

    def prop(ms, level):
        seen = {s[1] for s in ms[0].matches}
        assert not set(ends) - seen, sorted(set(ends) - seen)
        assert {W.dist_code(d)[0] for d in seen} == set(range(30))
        for p, d in where:
            if d >= 2:                                        # (distance 1 comes from the zero runs; 2.. from the keys placed for them)
                assert ms[0].token_at(p) is not None and ms[0].token_at(p)[1] == d, (p, d, ms[0].token_at(p))
    at_levels(ctx, raw, prop)


def every_length_input():
    """for every L in 4..258: L fresh bytes and the same L bytes again, the copy at the first position of a step; two blocks"""
    out, r = bytearray(), random.Random(9)
    for L in range(4, 259):
        s = fresh(L, 1000 + L)
        start = -(-(len(out) + L) // 64) * 64                  # the copy's position
        if (start - L) // BLK != (start + L) // BLK:           # source and copy in one block (0xff00 is a multiple of 64)
            start = (start + L) // BLK * BLK + 64 * (-(-L // 64))
        out += bytes(start - L - len(out)) + s + s + bytes([s[0] ^ 0xff])
    return bytes(out)


def test_every_match_length(ctx):
    raw = every_length_input()
    assert BLK < len(raw) <= 2 * BLK

    def prop(ms, level):
        assert len(ms) == 2
        seen = {s[0] for m in ms for s in m.matches if s[0] == s[1]}
        assert seen >= set(range(4, 259)), sorted(set(range(4, 259)) - seen)
    at_levels(ctx, raw, prop)


LIT40 = fresh(600, 21, range(60, 100))


def test_hlit_and_hdist_extremes(ctx):
    def literal_only(ms, level):
        b = ms[0].blk
        assert b.btype == 2 and not ms[0].matches and (b.hlit, b.hdist) == (257, 2) and b.d_lens == [1, 1]      # the dummy second leaf
    at_levels(ctx, LIT40, literal_only)

    lay = Layout(704)
    lay.put(0, LIT40)
    lay.b[600:] = fresh(104, 22, range(100, 140))
    key = bytes(lay.b[640 - 40:640 - 32])
    lay.b[640:648] = key                                      # one match, distance 40: distance code 10

    def one_distance_code(ms, level):
        b = ms[0].blk
        assert b.btype == 2 and {W.dist_code(s[1])[0] for s in ms[0].matches} == {10}
        assert b.hdist == 11 and b.d_lens == [1] + [0] * 9 + [1]
    at_levels(ctx, bytes(lay.b), one_distance_code)

    far = fresh(300, 23)
    raw = far + bytes(24700) + far + LIT40

    def widest_header(ms, level):
        b = ms[0].blk
        assert b.btype == 2 and (b.hlit, b.hdist) == (286, 30)
        assert any(s[0] == 258 and s[1] > 24576 for s in ms[0].matches)
    at_levels(ctx, raw, widest_header)


def test_zero_runs_in_the_code_length_section(ctx):
    """literal alphabets with gaps: zero runs of 2 (plain zeros), 3 and 10 (17 with extra 0 and 7), 11 and 138 (18 with extra 0 and 127),
    139 (18 with extra 127, then a plain zero)"""
    raw = rand_bytes(3000, 31, bytes([0, 3, 7, 18, 30, 169]))

    def gaps(ms, level):
        b = ms[0].blk
        assert b.btype == 2 and [l > 0 for l in b.ll_lens[:170]] == [s in (0, 3, 7, 18, 30, 169) for s in range(170)]
        assert b.cl_items[1:3] == [(0, 0), (0, 0)] and b.cl_items[3][0] not in (0, 17, 18)
        assert [b.cl_items[k] for k in (4, 6, 8, 10)] == [(17, 0), (17, 7), (18, 0), (18, 127)]
    at_levels(ctx, raw, gaps)
    raw = rand_bytes(3000, 33, bytes([0] + list(range(140, 150))))

    def split_run(ms, level):
        b = ms[0].blk
        assert b.btype == 2 and b.ll_lens[0] and not any(b.ll_lens[1:140]) and b.ll_lens[140]
        assert b.cl_items[1:3] == [(18, 127), (0, 0)] and b.cl_items[3][0] not in (0, 17, 18)
    at_levels(ctx, raw, split_run)


def skewed_bytes(c, seed):
    """254 c bytes of about 7.97 bits each by the encoder's own code: 2 values 2 c times (7 bits), 250 values c times (8 bits), shuffled.
    (Exact counts: the builder's lengths are ceil(log2(total / count)), and a count a little under total / 256 would cost 9 bits.)"""
    b = bytearray(bytes([0, 1]) * (2 * c) + bytes(range(2, 252)) * c)
    random.Random(seed).shuffle(b)
    return bytes(b)


def btype_is(t):
    def prop(ms, level):
        assert ms[0].blk.btype == t, (ms[0].blk.btype, t)
    return prop


def test_block_types_follow_the_size_rule(ctx):
    for raw in (b"abc", b"the quick brown fox "):
        at_levels(ctx, raw, btype_is(1))
    at_levels(ctx, rand_bytes(5000, 41), btype_is(0))
    raw = skewed_bytes(255, 42)

    def barely(ms, level):
        b = ms[0].blk
        print(f"barely dynamic, level {level}: payload {len(ms[0].pay)} bytes of {len(raw)} + 5 stored")
        assert b.btype == 2 and len(raw) + 5 - len(ms[0].pay) < len(raw) // 100
    at_levels(ctx, raw, barely)
    # the stored threshold itself: n distinct bytes above 143 are 9 bits each in the fixed code, 3 + 9 n + 7 bits, ceil(../8) reaches n + 5 at n = 23
    hi = bytes(range(150, 190))
    for n in range(20, 27):
        ch = Cr.block_choice(list(hi[:n]), n)
        assert ch["fix_bits"] == 10 + 9 * n and ch["dyn_bits"] > ch["fix_bits"] and ch["btype"] == (1 if n < 23 else 0) and (n != 23 or ch["nbytes"] == (ch["fix_bits"] + 7) // 8)

        def typ(ms, level, n=n, ch=ch):
            assert ms[0].blk.btype == ch["btype"] and len(ms[0].pay) == ch["nbytes"], (n, ms[0].blk.btype)
        at_levels(ctx, hi[:n], typ)
    for raw in (b"abc", hi[:23], skewed_bytes(12, 43)):            # level 0 stores whatever the input
        at_levels(ctx, raw, lambda ms, level: None, levels=(0,))


TEXT = b"".join(b"chr%d\t%d\trs%d\tA\tG\t%d\tPASS\tDP=%d\n" % (i % 22 + 1, 1000 + 37 * i, i * 7919 % 100003, i % 60, i % 97) for i in range(2600))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 65279, 65280, 65281])
def test_sizes_at_the_edges(ctx, n):
    assert len(TEXT) >= 65281
    for raw in (TEXT[:n], bytes(n), (b"abcdefg" * 10000)[:n]):
        def prop(ms, level):
            assert len(ms) == (2 if n > BLK else 1) and sum(len(m.raw) for m in ms) == n
            if n == BLK + 1:
                assert ms[1].blk.btype == 1 and len(ms[1].syms) == 1            # a last block of one byte: one literal in a fixed block
        at_levels(ctx, raw, prop)


def test_matches_clipped_at_the_end_of_a_block(ctx):
    unit = fresh(100, 51)
    raw = (unit * 1400)[:BLK + 5000]                              # period 100 on into the second block

    def clipped(ms, level):
        last = ms[0].syms[-1]
        assert not isinstance(last, int) and last[1] % 100 == 0 and ms[0].pos[-1] + last[0] == BLK and last[0] < 258      # (unclipped: 258)
        assert all(isinstance(s, int) for s in ms[1].syms[:64])   # block 1 starts from nothing: its first step has no candidates
        assert any(s[0] == 258 for s in ms[1].matches)
    at_levels(ctx, raw, clipped)
    key = fresh(12, 52)
    raw = key + b"\x01" + bytes(627) + key                        # the copy at 640, the first position of a step, ends the input

    def at_the_end(ms, level):
        assert ms[0].syms[-1] == (12, 640) and ms[0].pos[-1] + 12 == len(raw)
    at_levels(ctx, raw, at_the_end)


def test_lazy_evaluation_and_level_1(ctx):
    """position 640 holds a 4-byte match ("abcd" of the first source), 641 a 9-byte one ("bcdefghij" of the second)"""
    k = fresh(10, 61, range(200, 250))
    raw = k[:4] + b"\x01" + bytes(59) + b"\x02" + k[1:] + b"\x03"
    raw += bytes(640 - len(raw)) + k + b"\x04" + bytes(20)

    def prop(ms, level):
        m = ms[0]
        if level == 1:
            assert m.token_at(640) == (4, 640)
        else:
            assert m.token_at(640) == k[0] and m.token_at(641) == (9, 641 - 65)
    at_levels(ctx, raw, prop)


def test_second_launch_of_a_large_input(ctx):
    """more than 4,096 blocks: dhts_bgzf_compress launches twice.  zlib alone reads it back (no parse: 4,097 members)"""
    raw = (b"ACGTTGCATG" * 6528) * 4096 + b"A"
    assert len(raw) == 4096 * BLK + 1
    t0 = time.time()
    z = ctx.bgzf_compress(raw)
    t1 = time.time()
    check_file(raw, z)
    print(f"second launch: {len(raw)} -> {len(z)} bytes, compress {t1 - t0:.2f} s, read back {time.time() - t1:.2f} s")
