"""Bit-level DEFLATE writer (RFC 1951), test tooling only.

Unlike zlib's deflate, which picks every block shape itself, this writer emits exactly what it is told: stored / fixed / dynamic
blocks with caller-given code lengths, an explicit symbol list (a literal, or a (length, distance) pair with a chosen length code
where two encode the same length), a hand-made code-length section (HLIT / HDIST / HCLEN, repeat codes 16 / 17 / 18 placed by the
caller), the value of the padding bits in front of a stored block, raw bits for malformed headers.  On top of that: a length-limited
Huffman helper, a greedy matcher with a 32 KiB window that re-encodes any payload in a chosen shape, and BGZF / gzip wrappers.

A symbol list is a list of items:
    int 0..255                  a literal
    (length, distance)          a match; length 258 is coded as 285
    (length, distance, code)    a match with its length code chosen (258 as 284 + 31)
    256 is never listed: every Huffman block ends with EOB, written by the block writer.
"""
import struct
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


def length_code(length):
    """the length code (257..285) RFC 1951 3.2.5 gives `length`, and its extra-bit value (258 -> 285)"""
    assert 3 <= length <= 258, length
    if length == 258:
        return 285, 0
    for i in range(27, -1, -1):
        if LEN_BASE[i] <= length:
            assert length - LEN_BASE[i] < (1 << LEN_EXTRA[i])
            return 257 + i, length - LEN_BASE[i]
    raise AssertionError


def dist_code(dist):
    assert 1 <= dist <= 32768, dist
    for i in range(29, -1, -1):
        if DIST_BASE[i] <= dist:
            return i, dist - DIST_BASE[i]
    raise AssertionError


def canonical(lens):
    """RFC 1951 3.2.2: code values (MSB-first) of the symbols with the given lengths (0 = unused)"""
    mx = max(lens) if lens else 0
    bl = [0] * (mx + 2)
    for l in lens:
        if l:
            bl[l] += 1
    code, nxt = 0, [0] * (mx + 2)
    for b in range(1, mx + 1):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            out[s] = nxt[l]
            nxt[l] += 1
    return out


def kraft(lens):
    """sum of 2^(15 - len) over the used symbols, against 2^15 for a complete code"""
    return sum(1 << (15 - l) for l in lens if l)


class BitWriter:
    """LSB-first bit packer (RFC 1951 3.1.1)"""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, n):
        assert 0 <= value < (1 << n) or n == 0, (value, n)
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def huff(self, code, length):
        """a Huffman code, most significant bit first"""
        code &= (1 << length) - 1                            # (an over-subscribed code's canonical values overflow their length)
        self.bits(int(format(code, "0%db" % length)[::-1], 2) if length else 0, length)

    def align(self, pad=0):
        """fill to the byte boundary with the bits of `pad` (their values are free in a stored block's header)"""
        k = (8 - self.n) % 8
        self.bits(pad & ((1 << k) - 1), k)

    def getvalue(self):
        return bytes(self.buf) + (bytes([self.acc & 255]) if self.n else b"")


class Stream:
    """a raw DEFLATE stream built block by block; `out` is the output the blocks mean (a distance in front of the stream reads zeros)"""

    def __init__(self):
        self.w = BitWriter()
        self.out = bytearray()

    # ---- the meaning of a symbol list
    def _play(self, syms):
        for s in syms:
            if isinstance(s, int):
                assert 0 <= s <= 255
                self.out.append(s)
            else:
                ln, d = s[0], s[1]
                for _ in range(ln):
                    self.out.append(self.out[-d] if d <= len(self.out) else 0)

    def header(self, final, btype):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(btype, 2)

    def stored(self, data, final=False, pad=0, len_field=None, nlen_field=None):
        self.header(final, 0)
        self.w.align(pad)
        ln = len(data) if len_field is None else len_field
        self.w.bits(ln, 16)
        self.w.bits((ln ^ 0xFFFF) if nlen_field is None else nlen_field, 16)
        for b in data:
            self.w.bits(b, 8)
        self.out += data
        return self

    def _symbols(self, syms, ll_codes, ll_lens, d_codes, d_lens):
        for s in syms:
            if isinstance(s, int):
                assert ll_lens[s], "literal %d has no code" % s
                self.w.huff(ll_codes[s], ll_lens[s])
                continue
            ln, d = s[0], s[1]
            if len(s) > 2:
                lc = s[2]
                ex = ln - LEN_BASE[lc - 257]
                assert 0 <= ex < (1 << LEN_EXTRA[lc - 257]) or (lc == 285 and ln == 258), (ln, lc)
            else:
                lc, ex = length_code(ln)
            assert ll_lens[lc], "length code %d has no code" % lc
            self.w.huff(ll_codes[lc], ll_lens[lc])
            self.w.bits(ex, LEN_EXTRA[lc - 257])
            dc, dx = dist_code(d)
            assert dc < len(d_lens) and d_lens[dc], "distance code %d has no code" % dc
            self.w.huff(d_codes[dc], d_lens[dc])
            self.w.bits(dx, DIST_EXTRA[dc])
        self._play(syms)

    def fixed(self, syms, final=False, eob=True):
        self.header(final, 1)
        ll = canonical(FIXED_LL)
        self._symbols(syms, ll, FIXED_LL, canonical([5] * 32), [5] * 32)
        if eob:
            self.w.huff(ll[256], 7)
        return self

    def fixed_code(self, sym):
        """a raw fixed-code literal/length symbol (286 / 287 included), no extra bits"""
        self.w.huff(canonical(FIXED_LL)[sym], FIXED_LL[sym])
        return self

    def dynamic(self, syms, ll_lens, d_lens, final=False, hlit=None, hdist=None, cl_items=None, cl_lens=None, hclen=None,
                eob=True, max_run=True):
        """a dynamic block.  ll_lens / d_lens: the code lengths (their lists' lengths give HLIT + 257 / HDIST + 1 unless hlit / hdist
        say otherwise -- the field value is written as given, 0..31).  cl_items: the code-length section as (symbol, extra) pairs
        (default: run-length coded from the lengths, runs of 138 / 6 where they fit); cl_lens: the 19 code-length code lengths
        (default: Huffman, at most 7 bits, over the items used); hclen: the HCLEN field + 4 (default: trimmed)."""
        ll_lens, d_lens = list(ll_lens), list(d_lens)
        nl, nd = len(ll_lens), len(d_lens)
        hlit_f = nl - 257 if hlit is None else hlit
        hdist_f = nd - 1 if hdist is None else hdist
        if cl_items is None:
            cl_items = rle_lengths(ll_lens + d_lens, max_run=max_run)
        if cl_lens is None:
            f = [0] * 19
            for s, _ in cl_items:
                f[s] += 1
            cl_lens = huffman_lengths(f, 7)
        if hclen is None:
            hclen = 19
            while hclen > 4 and cl_lens[CL_ORDER[hclen - 1]] == 0:
                hclen -= 1
        self.header(final, 2)
        self.w.bits(hlit_f, 5)
        self.w.bits(hdist_f, 5)
        self.w.bits(hclen - 4, 4)
        for i in range(hclen):
            self.w.bits(cl_lens[CL_ORDER[i]], 3)
        clc = canonical(cl_lens)
        for s, x in cl_items:
            self.w.huff(clc[s], cl_lens[s])
            if s == 16:
                self.w.bits(x, 2)
            elif s == 17:
                self.w.bits(x, 3)
            elif s == 18:
                self.w.bits(x, 7)
        llc, dcs = canonical(ll_lens), canonical(d_lens)
        self._symbols(syms, llc, ll_lens, dcs, d_lens)
        if eob:
            self.w.huff(llc[256], ll_lens[256])
        return self

    def raw(self, value, n):
        """raw bits, for headers no block writer would make"""
        self.w.bits(value, n)
        return self

    def bytes(self):
        return self.w.getvalue()


def rle_lengths(lens, max_run=True):
    """code-length section items (RFC 1951 3.2.7): 18 / 17 for runs of zeros, 16 for repeats of the previous length (a run may
    cross from the literal/length into the distance lengths, as the RFC allows).  max_run=False: plain lengths only."""
    items, i, n = [], 0, len(lens)
    while i < n:
        v = lens[i]
        j = i
        while j < n and lens[j] == v:
            j += 1
        run = j - i
        if not max_run:
            items += [(v, 0)] * run
        elif v == 0:
            while run >= 11:
                k = min(run, 138); items.append((18, k - 11)); run -= k
            if run >= 3:
                items.append((17, run - 3)); run = 0
            items += [(0, 0)] * run
        else:
            items.append((v, 0)); run -= 1
            while run >= 3:
                k = min(run, 6); items.append((16, k - 3)); run -= k
            items += [(v, 0)] * run
        i = j
    return items


def huffman_lengths(freqs, maxlen):
    """length-limited Huffman code lengths (package-merge); a single used symbol gets length 1, none gives all zeros"""
    used = [s for s, f in enumerate(freqs) if f]
    lens = [0] * len(freqs)
    if not used:
        return lens
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    assert len(used) <= (1 << maxlen)
    leaves = sorted((freqs[s], [s]) for s in used)
    cur = list(leaves)
    for _ in range(maxlen - 1):
        pk = [(cur[k][0] + cur[k + 1][0], cur[k][1] + cur[k + 1][1]) for k in range(0, len(cur) - 1, 2)]
        cur = sorted(leaves + pk, key=lambda t: t[0])
    for _, syms in cur[:2 * len(used) - 2]:
        for s in syms:
            lens[s] += 1
    assert kraft(lens) == 1 << 15 and max(lens) <= maxlen
    return lens


def shaped_lengths(n, maxlen, long_first=False):
    """n code lengths of a complete code whose longest code is exactly `maxlen` bits (n >= maxlen + 1).  Grown from the chain
    1, 2, .., maxlen, maxlen by splitting leaves: the shortest first (few long codes), or with long_first the longest below maxlen
    (as many maxlen-bit codes as n allows).  Sorted ascending."""
    assert maxlen + 1 <= n <= (1 << maxlen), (n, maxlen)
    lens = list(range(1, maxlen + 1)) + [maxlen]
    while len(lens) < n:
        cand = [l for l in lens if l < maxlen]
        l = max(cand) if long_first else min(cand)
        lens.remove(l)
        lens += [l + 1, l + 1]
    lens.sort()
    assert kraft(lens) == 1 << 15 and max(lens) == maxlen
    return lens


def assign_lengths(nsym, syms_by_rank, lens):
    """code lengths by symbol: the i-th symbol of syms_by_rank (most frequent first) takes the i-th of `lens` (ascending)"""
    out = [0] * nsym
    for s, l in zip(syms_by_rank, lens):
        out[s] = l
    return out


# ---- greedy matcher ------------------------------------------------------------------------------------------------------------
def _mlen(data, i, j, maxl):
    l = 0
    while l + 32 <= maxl and data[i + l:i + l + 32] == data[j + l:j + l + 32]:
        l += 32
    while l < maxl and data[i + l] == data[j + l]:
        l += 1
    return l


def greedy_parse(data, policy="longest", chain=24, window=32768):
    """LZ77 symbols of `data` (one stream: the window starts at data[0]).  policy 'longest': the longest match of the last `chain`
    candidates (ties: the nearest); 'farthest': the farthest candidate in the window that matches >= 3 bytes; 'literals': no matches."""
    syms, heads, n, i = [], {}, len(data), 0
    while i < n:
        best = None
        if policy != "literals" and i + 3 <= n:
            key = data[i:i + 3]
            cands = heads.get(key, ())
            maxl = min(258, n - i)
            for j in reversed(cands[-chain:]) if policy == "longest" else cands[-chain:]:
                if i - j > window:
                    continue
                l = _mlen(data, i, j, maxl)
                if l < 3:
                    continue
                if policy == "farthest":
                    best = (l, i - j)
                    break
                if best is None or l > best[0]:
                    best = (l, i - j)
                    if l == maxl:
                        break
        step = best[0] if best else 1
        for k in range(i, min(i + step, n - 2)):
            heads.setdefault(data[k:k + 3], []).append(k)
        if best:
            syms.append(best)
        else:
            syms.append(data[i])
        i += step
    return syms


def symbol_freqs(syms):
    fl, fd = [0] * 286, [0] * 30
    for s in syms:
        if isinstance(s, int):
            fl[s] += 1
        else:
            fl[s[2] if len(s) > 2 else length_code(s[0])[0]] += 1
            fd[dist_code(s[1])[0]] += 1
    fl[256] += 1
    return fl, fd


def shaped_code(syms, maxlen=15, long_first=False):
    """code lengths for `syms` whose longest code is maxlen bits (where the alphabet in use allows it): the most frequent symbols
    take the shortest codes of shaped_lengths; with fewer symbols than maxlen + 1, length-limited Huffman"""
    fl, fd = symbol_freqs(syms)
    out = []
    for f, n in ((fl, 286), (fd, 30)):
        used = sorted((s for s in range(n) if f[s]), key=lambda s: (-f[s], s))
        if len(used) >= maxlen + 1:
            out.append(assign_lengths(n, used, shaped_lengths(len(used), maxlen, long_first)))
        else:
            out.append(huffman_lengths(f, maxlen))
    ll, dl = out
    while len(dl) > 1 and dl[-1] == 0:
        dl.pop()
    while len(ll) > 257 and ll[-1] == 0:
        ll.pop()
    return ll, dl


def encode(data, policy="longest", maxlen=15, long_first=False, split=None, btypes=("dynamic",)):
    """one raw DEFLATE stream of `data` in a chosen shape: match policy, code shape, blocks of `split` bytes of input each
    (None: one block), the block types cycled through `btypes` ('dynamic', 'fixed', 'stored')"""
    syms = greedy_parse(data, policy)
    # split the symbol list at input offsets
    pieces, cur, size = [], [], 0
    for s in syms:
        cur.append(s)
        size += 1 if isinstance(s, int) else s[0]
        if split and size >= split:
            pieces.append((cur, size)); cur, size = [], 0
    if cur or not pieces:
        pieces.append((cur, size))
    st, pos = Stream(), 0
    for k, (p, sz) in enumerate(pieces):
        final = k == len(pieces) - 1
        bt = btypes[k % len(btypes)]
        if bt == "stored":
            st.stored(data[pos:pos + sz], final)
        elif bt == "fixed":
            st.fixed(p, final)
        else:
            ll, dl = shaped_code(p, maxlen, long_first)
            st.dynamic(p, ll, dl, final)
        pos += sz
    assert bytes(st.out) == data
    return st.bytes()


# ---- containers ----------------------------------------------------------------------------------------------------------------
def bgzf_block(deflate, raw, isize=None):
    """one BGZF block around a raw DEFLATE stream: CRC-32 and ISIZE of `raw` (the output the stream means)"""
    total = 18 + len(deflate) + 8
    assert total <= 65536, total
    hdr = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", total - 1)
    return hdr + deflate + struct.pack("<II", zlib.crc32(raw) & 0xffffffff, (len(raw) if isize is None else isize) & 0xffffffff)


def gzip_member(deflate, raw):
    return b"\x1f\x8b\x08\x00\0\0\0\0\x00\x03" + deflate + struct.pack("<II", zlib.crc32(raw) & 0xffffffff, len(raw) & 0xffffffff)


BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_reencode(raw, payload=65280, **shape):
    """a BGZF file of `raw` whose blocks are encode()d in a chosen shape; a block's input is cut short until its stream fits"""
    out, p = [], 0
    while p < len(raw):
        n = min(payload, len(raw) - p)
        while True:
            d = encode(raw[p:p + n], **shape)
            if 26 + len(d) <= 65536:
                break
            n //= 2
        out.append(bgzf_block(d, raw[p:p + n]))
        p += n
    return b"".join(out) + BGZF_EOF
