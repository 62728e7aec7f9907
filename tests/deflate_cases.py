"""Catalogue of hand-built raw DEFLATE streams for the conformance tests (tests/test_deflate_conformance.py, the GPU twin
tests/test_gpu_deflate_conformance.py).  Written with tests/deflate_writer.py, each aims at a shape zlib's deflate never or rarely
emits, or at a malformed header zlib's inflate rejects.  A case's expected result is NOT stored: the tests compute it with CPython's
zlib (the decoder htslib uses), and check that the case is of the class it was written to be (`valid` / `malformed`), so a writer
bug cannot quietly turn a malformed stream into a valid one.

Case fields: name, cls ('valid' | 'malformed'), note (the decoder path aimed at), build() -> raw DEFLATE bytes (the whole payload
of a BGZF block), intended (the output the symbols mean: the CRC-32 / ISIZE of the BGZF wrapper), far (malformed only by a distance
that reaches in front of the block: phase A of the device inflate leaves that test to phase B), libdeflate (None when libdeflate
decides as zlib does; else 'accepts' with the reason it differs).
"""
import random
import zlib
from collections import namedtuple

import deflate_writer as W

Case = namedtuple("Case", "name cls note build far libdeflate")
CASES = []
_BUILT = {}


def case(cls, note, far=False, libdeflate=None):
    def deco(fn):
        CASES.append(Case(fn.__name__, cls, note, fn, far, libdeflate))
        return fn
    return deco


def built(c):
    """(raw DEFLATE bytes, intended output) of a case, built once"""
    if c.name not in _BUILT:
        r = c.build()
        _BUILT[c.name] = (r.bytes(), bytes(r.out)) if isinstance(r, W.Stream) else r
    return _BUILT[c.name]


def zlib_inflate(payload, cap=65536):
    """what zlib makes of a BGZF payload as htslib hands it over (one inflate to Z_FINISH into 64 KiB; input behind the final
    block ignored): the output, or None when zlib rejects it"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload, cap + 1)
    except zlib.error:
        return None
    if not d.eof or len(out) > cap:
        return None
    return out


def by_name(name):
    return next(c for c in CASES if c.name == name)


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
def _rand(n, seed, alphabet=None):
    r = random.Random(seed)
    if alphabet is None:
        return bytes(r.getrandbits(8) for _ in range(n))
    return bytes(r.choice(alphabet) for _ in range(n))


TEXT = b"".join(b"read%05d\t%d\tACGT%sTTGA\t%d\n" % (i, i * 7919 % 100003, b"CAGT"[i % 4:] * (i % 7), i * 31 % 977) for i in range(4000))


def _code(syms, maxlen=15):
    """length-limited Huffman lengths for exactly the symbols used (EOB included); dist lens trimmed (empty tree: [0])"""
    fl, fd = W.symbol_freqs(syms)
    ll = W.huffman_lengths(fl, maxlen)
    dl = W.huffman_lengths(fd, maxlen)
    while len(ll) > 257 and ll[-1] == 0:
        ll.pop()
    while len(dl) > 1 and dl[-1] == 0:
        dl.pop()
    return ll, dl


def _dyn(syms, final=True, **kw):
    st = W.Stream()
    ll, dl = _code(syms)
    st.dynamic(syms, kw.pop("ll", ll), kw.pop("dl", dl), final, **kw)
    return st


def _lits(b):
    return list(b)


def _far_prefix():
    return _lits(_rand(32768, 11, bytes(range(32, 127))))


# ==== valid ========================================================================================================================
@case("valid", "distance 32,768 (no zlib stream has one): a match at output 32,768, chains of 258, a 3-byte match at 65,533 ending "
      "the block at exactly 65,536 bytes; phase A's distance tables past the 8-bit root, phase B's window at its full 32 KiB")
def v_dist_32768_full_block():
    s = _far_prefix() + [(258, 32768)] * 126 + [(257, 32768), (3, 32768)]
    st = _dyn(s)
    assert len(st.out) == 65536
    return st


@case("valid", "every distance 32,507..32,768 (above zlib's MAX_DIST 32,506), 3-byte matches behind a 32 KiB literal prefix")
def v_dist_above_zlib_max():
    return _dyn(_far_prefix() + [(3, d) for d in range(32507, 32769)])


@case("valid", "distance == output position (a copy from the block's first byte), at every size from 3 to 32,768")
def v_dist_equals_position():
    s, pos = _lits(b"xyz"), 3
    while pos <= 32768:
        ln = min(pos, 258)
        s.append((ln, pos))
        pos += ln
    return _dyn(s)


@case("valid", "lengths 3 and 258 alternating at distance 32,768 (phase B's longest reach with the shortest and longest copies)")
def v_len3_len258_at_32768():
    return _dyn(_far_prefix() + [(3, 32768), (258, 32768)] * 40)


@case("valid", "overlapping copies: distances 1..4 with length 258 (the source overlaps the target: byte-serial semantics)")
def v_overlap_short_distances():
    s = _lits(b"abcd")
    for _ in range(20):
        s += [(258, 1), (258, 2), (258, 3), (258, 4), 0x41 + len(s) % 26]
    return _dyn(s)


@case("valid", "length 258 coded as 284 + 31 extra bits (zlib always codes it as 285), mixed with 285 and 284's other lengths")
def v_len258_as_284():
    s = _lits(TEXT[:300])
    for k in range(60):
        s += [(258, 1 + k % 200, 284), (258, 7), (227 + k % 31, 100, 284)]
    return _dyn(s)


@case("valid", "fixed Huffman block with length 258 as 284 + 31, every length code and distance code 0..29")
def v_fixed_all_codes():
    s = _lits(_rand(25000, 3, b"ACGT"))
    for lc in range(257, 286):
        s.append((W.LEN_BASE[lc - 257], 1 + lc, lc))
    for dc in range(30):
        s.append((5, W.DIST_BASE[dc]))
    s.append((258, 24577, 284))
    st = W.Stream()
    return st.fixed(s, final=True)


def _long_ll_block(n_light, f_light, f_heavy):
    """a literal/length code (package-merge, 15-bit limit) where n_light literals are rarer than the rest by f_heavy / f_light and
    three symbols (EOB among them) rarest of all: those take the longest codes; the block uses every literal by these weights"""
    f = [f_heavy] * (256 - n_light) + [f_light] * n_light + [1]
    f[254] = f[255] = 1
    ll = W.huffman_lengths(f, 15)
    pool = [v for v in range(256) for _ in range(f[v])]
    r = random.Random(n_light)
    return ll, [r.choice(pool) for _ in range(20000)]


def _long_prefixes(ll):
    """the 11-bit root prefixes the codes longer than 11 bits fall under (the wave kernel's second-level table has 512 entries)"""
    c = W.canonical(ll)
    return {c[k] >> (ll[k] - 11) for k in range(len(ll)) if ll[k] > 11}


@case("valid", "literal/length codes of 12..15 bits under few root prefixes: the wave kernel's second-level table (4 sub-bits)")
def v_ll_15bit_second_level():
    ll, s = _long_ll_block(100, 16, 1024)
    assert max(ll) == 15 and 0 < len(_long_prefixes(ll)) << 4 <= 512
    st = W.Stream()
    return st.dynamic(s, ll, [0], True)


@case("valid", "12..15-bit literal/length codes under more than 512 / 16 = 32 root prefixes: the canonical per-symbol fallback")
def v_ll_15bit_canonical_fallback():
    ll, s = _long_ll_block(100, 8, 256)
    assert max(ll) == 15 and len(_long_prefixes(ll)) << 4 > 512
    st = W.Stream()
    return st.dynamic(s, ll, [0], True)


@case("valid", "distance codes of 9..15 bits (all 30 used; the wave kernel's distance table past its 8-bit root)")
def v_dist_15bit_codes():
    s = _lits(_rand(30000, 5, b"ACGTN"))
    for k in range(600):
        dc = k % 30
        s.append((4 + k % 50, W.DIST_BASE[dc] + (k % (1 << W.DIST_EXTRA[dc]))))
    dl = W.assign_lengths(30, list(range(30)), W.shaped_lengths(30, 15, True))
    ll, _ = _code(s)
    st = W.Stream()
    return st.dynamic(s, ll, dl, True)


@case("valid", "a distance tree of one 1-bit codeword (the one incomplete code zlib allows), distance code 0 only")
def v_dist_single_1bit():
    s = _lits(b"GATTACA") + [(258, 1), 0x43, (100, 1)] * 30
    ll, _ = _code(s)
    st = W.Stream()
    return st.dynamic(s, ll, [1], True)


@case("valid", "a distance tree of one 1-bit codeword on distance code 17 behind HDIST = 30 (the symbol is not the first)")
def v_dist_single_1bit_code17():
    s = _lits(_rand(600, 6, b"ACGT")) + [(30, 385 + k) for k in range(100)]
    ll, _ = _code(s)
    dl = [0] * 30
    dl[17] = 1
    st = W.Stream()
    return st.dynamic(s, ll, dl, True)


@case("valid", "an empty distance tree (HDIST = 1, length 0) in a literal-only block; then one with HDIST = 30, all zero")
def v_dist_empty():
    st = W.Stream()
    s = _lits(TEXT[:2000])
    ll, _ = _code(s)
    st.dynamic(s, ll, [0], False)
    return st.dynamic(s[:500], ll, [0] * 30, True)


@case("valid", "a literal/length tree that holds only EOB with a 1-bit code (an empty block), between stored blocks")
def v_ll_eob_only():
    st = W.Stream()
    st.stored(TEXT[:100])
    ll = [0] * 257
    ll[256] = 1
    st.dynamic([], ll, [0], False)
    st.stored(TEXT[100:200])
    return st.dynamic([], ll, [1], True)


@case("valid", "all 286 literal/length and all 30 distance symbols present (HLIT = 29, HDIST = 29)")
def v_all_symbols():
    s = _lits(bytes(range(256)) * 40) + _lits(_rand(20000, 7))
    for lc in range(257, 286):
        s.append((W.LEN_BASE[lc - 257], 3 + lc, lc))
    for dc in range(30):
        s.append((9, W.DIST_BASE[dc]))
    ll, dl = _code(s)
    assert len(ll) == 286 and all(ll) and len(dl) == 30 and all(dl)
    st = W.Stream()
    return st.dynamic(s, ll, dl, True)


@case("valid", "150 tiny blocks in one BGZF block, cycling stored / fixed / dynamic, empty stored blocks among them")
def v_many_tiny_blocks():
    st = W.Stream()
    r = random.Random(8)
    for k in range(150):
        piece = TEXT[k * 37:k * 37 + r.randrange(0, 30)]
        kind = k % 4
        final = k == 149
        if kind == 0 or not piece:
            st.stored(piece, final, pad=r.getrandbits(7))
        elif kind == 1:
            st.fixed(W.greedy_parse(piece), final)
        elif kind == 2:
            p = W.greedy_parse(piece)
            ll, dl = _code(p)
            st.dynamic(p, ll, dl, final)
        else:
            st.stored(b"", final)
    return st


@case("valid", "stored blocks after non-zero padding bits (the header's free bits all ones), empty stored blocks, a final empty one")
def v_stored_padding_bits():
    st = W.Stream()
    s = _lits(b"abc") + [(10, 3)]
    ll, dl = _code(s)
    st.dynamic(s, ll, dl, False)
    st.stored(TEXT[:1000], pad=0x7f)
    st.fixed(_lits(b"Q"))
    st.stored(b"", pad=0x55)
    st.fixed(_lits(b"RS"))
    st.stored(TEXT[1000:3000], pad=0x3f)
    return st.stored(b"", True, pad=0x7f)


@case("valid", "a tiny dynamic block (one literal) trailing a large one: the trailing-block path of phase A")
def v_tiny_dynamic_after_large():
    st = W.Stream()
    p = W.greedy_parse(TEXT[:50000])
    ll, dl = _code(p)
    st.dynamic(p, ll, dl, False)
    st.dynamic([0x21], *_code([0x21]), True)
    return st


@case("valid", "2,500 1-bit literals inside one 64th of the block's bits: more than 1 KiB of literals in one lane's range "
      "(the wave kernel's staging-slice overflow, lane 0 alone)")
def v_1bit_literal_burst():
    ll = [0] * 257
    ll[ord("A")] = 1
    for v in range(256):
        if v != ord("A"):
            ll[v] = 9
    ll[256] = 9
    assert W.kraft(ll) == 1 << 15
    body = _lits(_rand(30000, 9, bytes(v for v in range(256) if v != ord("A"))))
    s = body[:15000] + [ord("A")] * 2500 + body[15000:]
    st = W.Stream()
    return st.dynamic(s, ll, [0], True)


@case("valid", "1,500 2-bit matches (1-bit length code, 1-bit distance code) in a row: more than 352 tokens in one lane's range")
def v_2bit_match_burst():
    ll = [0] * 258
    ll[257] = 1
    for v in range(255):
        ll[v] = 9
    ll[255] = 10
    ll[256] = 10
    assert W.kraft(ll) == 1 << 15
    body = _lits(_rand(20000, 10))
    s = body[:10000] + [(3, 1 + (k & 1)) for k in range(1500)] + body[10000:]
    st = W.Stream()
    return st.dynamic(s, ll, [1, 1], True)


@case("valid", "literal runs of 600..5,000 between matches: runs over 511 (split into 'no match' tokens) that cross lane ranges")
def v_long_literal_runs():
    body = _lits(_rand(60000, 12, bytes(range(97, 123))))
    s, i = [], 0
    for run in (600, 5000, 511, 512, 1023, 1024, 2047, 3000, 700, 9000):
        s += body[i:i + run]
        i += run
        s.append((40, 300))
    s += body[i:i + 4000]
    return _dyn(s)


@case("valid", "255 literals with 8-bit codes (one literal and EOB at 9): a decoder started at a wrong bit never falls into step")
def v_all_8bit_literals():
    ll = [8] * 256 + [9]
    ll[255] = 9
    assert W.kraft(ll) == 1 << 15
    s = _lits(_rand(60000, 13, bytes(range(255))))
    st = W.Stream()
    return st.dynamic(s, ll, [0], True)


@case("valid", "a block that inflates to exactly 65,536 bytes (text, greedy longest matches, one dynamic block)")
def v_exactly_65536():
    data = (TEXT * 2)[:65536]
    st = W.Stream()
    p = W.greedy_parse(data)
    ll, dl = _code(p)
    st.dynamic(p, ll, dl, True)
    assert len(st.out) == 65536
    return st


@case("valid", "bytes behind the final block inside the BGZF payload (htslib hands zlib the whole block: they are ignored)")
def v_bytes_after_final_block():
    st = W.Stream()
    p = W.greedy_parse(TEXT[:3000])
    st.dynamic(p, *_code(p), True)
    return st.bytes() + b"\x00\xff\x13junk behind the stream", bytes(st.out)


def _expand(items):
    """the code lengths a code-length section's items stand for"""
    got = []
    for s, x in items:
        got += [s] if s < 16 else [got[-1] if got else None] * (x + 3) if s == 16 else [0] * (x + 3 if s == 17 else x + 11)
    return got


@case("valid", "code-length section: a 16 that crosses from the literal/length into the distance lengths, an 18 run of 138, "
      "17 / 18 / 16 all used, HCLEN 19 (trailing zero lengths written)")
def v_cl_repeat_across_boundary():
    ll = [0] * 286
    for v in range(97, 109):
        ll[v] = 4                                                    # 'a'..'l'
    ll[256] = 4
    for v in range(280, 286):
        ll[v] = 5
    dl = [5, 5, 5, 5, 3, 2, 2, 2]
    assert W.kraft(ll) == W.kraft(dl) == 1 << 15
    items = [(18, 97 - 11), (4, 0), (16, 3), (16, 2), (18, 138 - 11), (17, 9 - 3), (4, 0), (18, 23 - 11),
             (5, 0), (16, 3), (16, 0), (3, 0), (2, 0), (2, 0), (2, 0)]        # the first 16 covers 281..285 and distance 0
    assert _expand(items) == ll + dl
    s = _lits(b"abcdefghijkl" * 40)
    for k, lc in enumerate(list(range(280, 286)) * 8):
        dc = k % 8
        s.append((W.LEN_BASE[lc - 257] + k % (1 << W.LEN_EXTRA[lc - 257]), W.DIST_BASE[dc], lc))
    st = W.Stream()
    return st.dynamic(s, ll, dl, True, cl_items=items, hclen=19)


@case("valid", "re-encoded text: 'farthest' matches (distances up to 32 KiB wherever one exists), 15-bit codes, one block")
def v_text_farthest_15bit():
    return W.encode(TEXT[:40000], policy="farthest", maxlen=15, long_first=True), TEXT[:40000]


@case("valid", "re-encoded text: 40 blocks of 1,000 bytes cycling dynamic / fixed / stored, 9-bit code limit")
def v_text_split_mixed():
    d = TEXT[40000:80000]
    return W.encode(d, policy="longest", maxlen=9, split=1000, btypes=("dynamic", "fixed", "stored", "dynamic")), d


@case("valid", "plain literal/length lengths only (no 16/17/18 in the code-length section), HLIT = 286")
def v_cl_no_repeats():
    s = _lits(TEXT[:5000]) + [(20, 19), (258, 4000)]
    ll, dl = _code(s)
    ll = ll + [0] * (286 - len(ll))
    st = W.Stream()
    return st.dynamic(s, ll, dl, True, max_run=False)


# ==== malformed ====================================================================================================================
def _ll_basic():
    """'a'..'c' 2 bits, 'd' 3 bits, EOB and length code 260 (length 6) 4 bits: complete"""
    ll = [0] * 261
    ll[97] = ll[98] = ll[99] = 2
    ll[100] = 3
    ll[256] = ll[260] = 4
    assert W.kraft(ll) == 1 << 15
    return ll


_S = _lits(b"abcdabcd") + [(6, 2)]


@case("malformed", "a literal/length tree of ONE codeword of 2 bits (EOB): zlib 'invalid literal/lengths set'")
def m_ll_single_2bit():
    ll = [0] * 257
    ll[256] = 2
    st = W.Stream()
    return st.dynamic([], ll, [0], True)


@case("malformed", "a distance tree of ONE codeword of 2 bits (zlib 'invalid distances set', htslib stops); the block never uses it")
def m_dist_single_2bit_unused():
    st = W.Stream()
    return st.dynamic(_lits(b"abcd" * 10), _ll_basic(), [2], True)


@case("malformed", "a distance tree of ONE codeword of 2 bits, used by every match")
def m_dist_single_2bit_used():
    st = W.Stream()
    return st.dynamic(_S, _ll_basic(), [0, 2], True)


@case("malformed", "a distance tree of ONE codeword of 15 bits")
def m_dist_single_15bit():
    st = W.Stream()
    return st.dynamic(_S, _ll_basic(), [0, 15], True)


@case("malformed", "a literal/length tree of ONE codeword of 9 bits (EOB), distance tree empty")
def m_ll_single_9bit():
    ll = [0] * 257
    ll[256] = 9
    st = W.Stream()
    return st.dynamic([], ll, [0], True)


@case("malformed", "an incomplete literal/length tree of several codewords (Kraft sum 7/8)")
def m_ll_incomplete():
    ll = [0] * 257
    ll[97] = ll[98] = 2
    ll[99] = ll[101] = ll[256] = 3
    assert W.kraft(ll) == 7 << 12
    st = W.Stream()
    return st.dynamic(_lits(b"abce"), ll, [0], True)


@case("malformed", "an incomplete distance tree of several codewords (2 + 2 + 3 bits)")
def m_dist_incomplete():
    st = W.Stream()
    return st.dynamic(_S, _ll_basic(), [2, 2, 3, 0], True)


@case("malformed", "an over-subscribed literal/length tree")
def m_ll_oversubscribed():
    ll = _ll_basic()
    ll[101] = 3
    st = W.Stream()
    return st.dynamic(_lits(b"abcde"), ll, [0], True)


@case("malformed", "an over-subscribed distance tree")
def m_dist_oversubscribed():
    st = W.Stream()
    return st.dynamic(_S, _ll_basic(), [1, 1, 1], True)


@case("malformed", "an incomplete code-length code (several codewords, Kraft sum below 1)")
def m_cl_incomplete():
    items = W.rle_lengths(_ll_basic() + [1, 1])
    cl = [0] * 19
    for s, _ in items:
        cl[s] = 4
    st = W.Stream()
    return st.dynamic(_S, _ll_basic(), [1, 1], True, cl_items=items, cl_lens=cl)


@case("malformed", "a code-length code of one 1-bit codeword (zlib requires the code-length code complete)")
def m_cl_single_1bit():
    ll = [0] * 257
    ll[256] = 1
    cl = [0] * 19
    cl[18] = 1
    st = W.Stream()
    return st.dynamic([], ll, [0], True, cl_items=[(18, 127), (18, 108)], cl_lens=cl)


@case("malformed", "an over-subscribed code-length code")
def m_cl_oversubscribed():
    items = W.rle_lengths(_ll_basic() + [1, 1])
    cl = [0] * 19
    for s, _ in items:
        cl[s] = 1
    st = W.Stream()
    return st.dynamic(_S, _ll_basic(), [1, 1], True, cl_items=items, cl_lens=cl)


@case("malformed", "HLIT field 30 (287 literal/length lengths)", libdeflate="accepts: it reads up to 288 literal/length lengths")
def m_hlit_30():
    ll = _ll_basic() + [0] * (287 - 261)
    st = W.Stream()
    return st.dynamic(_lits(b"abcd"), ll, [0], True)


@case("malformed", "HLIT field 31 (288 literal/length lengths)", libdeflate="accepts: it reads up to 288 literal/length lengths")
def m_hlit_31():
    ll = _ll_basic() + [0] * (288 - 261)
    st = W.Stream()
    return st.dynamic(_lits(b"abcd"), ll, [0], True)


@case("malformed", "HDIST field 30 (31 distance lengths)", libdeflate="accepts: it reads up to 32 distance lengths")
def m_hdist_31_codes():
    st = W.Stream()
    return st.dynamic(_S, _ll_basic(), [1, 1] + [0] * 29, True)


@case("malformed", "a 16 (repeat the previous length) as the first code length")
def m_first_length_16():
    ll = _ll_basic()
    items = [(16, 0)] + W.rle_lengths(ll[3:] + [1, 1])
    st = W.Stream()
    return st.dynamic(_S, ll, [1, 1], True, cl_items=items)


@case("malformed", "an 18 run of 138 zeros that overruns HLIT + HDIST", libdeflate="accepts: it lets a repeat run past the lengths")
def m_repeat_overruns():
    ll = _ll_basic()
    items = W.rle_lengths(ll + [1, 1])[:-1] + [(18, 127)]
    st = W.Stream()
    return st.dynamic(_S, ll, [1, 1], True, cl_items=items)


@case("malformed", "a 16 that overruns HLIT + HDIST by one", libdeflate="accepts: it lets a repeat run past the lengths")
def m_repeat16_overruns():
    ll = _ll_basic()
    items = W.rle_lengths(ll + [1])[:] + [(16, 0)]
    st = W.Stream()
    return st.dynamic(_S, ll, [1, 1], True, cl_items=items)


@case("malformed", "EOB with code length 0 (the block has no end-of-block code)")
def m_eob_length_0():
    ll = _ll_basic()
    ll[256] = 0
    ll[101] = 4
    st = W.Stream()
    return st.dynamic(_lits(b"abcde"), ll, [0], True, eob=False).raw(0, 16)


@case("malformed", "a fixed block that codes literal/length 286", libdeflate="accepts: its fixed code gives 286 / 287 a meaning")
def m_fixed_ll_286():
    return W.Stream().fixed(_lits(b"abc"), True, eob=False).fixed_code(286).raw(0, 16)


@case("malformed", "a fixed block that codes literal/length 287", libdeflate="accepts: its fixed code gives 286 / 287 a meaning")
def m_fixed_ll_287():
    return W.Stream().fixed(_lits(b"abc"), True, eob=False).fixed_code(287).raw(0, 16)


@case("malformed", "a fixed block that codes distance 30")
def m_fixed_dist_30():
    st = W.Stream().fixed(_lits(b"abcd"), True, eob=False).fixed_code(257)
    st.w.huff(30, 5)
    return st.raw(0, 16)


@case("malformed", "a fixed block that codes distance 31")
def m_fixed_dist_31():
    st = W.Stream().fixed(_lits(b"abcd"), True, eob=False).fixed_code(257)
    st.w.huff(31, 5)
    return st.raw(0, 16)


@case("malformed", "the codeword a one-codeword (1-bit) distance tree leaves unassigned")
def m_unassigned_dist_codeword():
    ll = [0] * 258
    ll[97] = ll[98] = ll[257] = 2
    ll[99] = ll[256] = 3
    st = W.Stream()
    st.dynamic(_lits(b"abcab"), ll, [1], True, eob=False)
    st.w.huff(W.canonical(ll)[257], 2)                               # a 3-byte match ...
    return st.raw(1, 1).raw(0, 16)                                   # ... whose distance is the codeword '1'


@case("malformed", "distance = output position + 1 at the block's first match", far=True)
def m_far_first_match():
    return _dyn(_lits(b"abcdefgh") + [(10, 9)])


@case("malformed", "distance = output position + 1 right after a stored block", far=True)
def m_far_after_stored():
    st = W.Stream()
    st.stored(TEXT[:1000])
    s = [(20, 1001)]
    return st.dynamic(s, *_code(s), True)


@case("malformed", "distance 32,768 at output position 32,767 (one past the block's first byte, behind a 65,535-byte block)", far=True)
def m_far_32768_at_32767():
    s = _lits(_rand(32767, 14, b"ACGT")) + [(100, 32768)]
    return _dyn(s)


@case("malformed", "65,537 bytes of output (one literal past a 65,536-byte block)")
def m_output_65537():
    s = _far_prefix() + [(258, 32768)] * 126 + [(257, 32768), (3, 32768), 0x41]
    st = _dyn(s)
    assert len(st.out) == 65537
    return st


@case("malformed", "BTYPE 3 (reserved) in the block header after a stored block")
def m_btype_3():
    return W.Stream().stored(b"ok").raw(1, 1).raw(3, 2).raw(0, 13)


@case("malformed", "stored block whose NLEN is not the complement of LEN")
def m_stored_nlen_mismatch():
    return W.Stream().stored(TEXT[:50], True, nlen_field=(50 ^ 0xFFFF) ^ 0x0100)


@case("malformed", "stored block whose LEN runs past the payload (and its 8-byte trailer)")
def m_stored_len_past_end():
    return W.Stream().stored(TEXT[:50], True, len_field=500)


@case("malformed", "no BFINAL before the payload ends (a fixed block, then a non-final empty stored block)")
def m_no_bfinal():
    st = W.Stream()
    st.fixed(_lits(b"abc"))
    return st.stored(b"", False)



# ---- the cases as BGZF files -------------------------------------------------------------------------------------------------------
_GOOD0 = (TEXT * 2)[3:3 + 65535]          # the block in front ends at output 65,535: a distance that reaches past the case block's
_GOOD2 = TEXT[777:777 + 5000]             # first byte must not find these bytes


def _zblock(raw):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    return W.bgzf_block(co.compress(raw) + co.flush(), raw)


def bgzf_case_file(c):
    """good block (65,535 bytes), the case's block, good block, EOF block; returns (file, [the four blocks' inflated bytes, or None
    for the case block when zlib rejects it])"""
    raw, intended = built(c)
    blk = W.bgzf_block(raw, intended, isize=min(len(intended), 65536))
    trailer = blk[-8:]
    z = zlib_inflate(raw + trailer)
    return _zblock(_GOOD0) + blk + _zblock(_GOOD2) + W.BGZF_EOF, [_GOOD0, z, _GOOD2, b""]
