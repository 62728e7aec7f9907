"""Token-level DEFLATE parser (RFC 1951), test tooling only: the reading twin of tests/deflate_writer.py.

zlib says whether a stream is valid and what it means; it does not say what the stream is made of.  parse() does: per block the header
fields, for dynamic blocks the code-length code, the code-length section item by item and the two codes' lengths, and every token with
the bit it starts at and the bits it takes -- what a test of an encoder's own decisions needs (which block type it chose, which code it
built, how wide its tokens are and where they sit in their words).

It raises DeflateError on whatever zlib's inflate rejects in a raw stream: BTYPE 3, LEN / NLEN that do not match, HLIT above 286 or
HDIST above 30 lengths, an incomplete or over-subscribed code-length code, a repeat with nothing to repeat or past the last length, no
end-of-block code, an over-subscribed code, an incomplete one (but the one-codeword code of 1 bit, which zlib lets pass; no distance
code at all is fine while no match needs one), a codeword nothing was assigned to, literal/length symbols 286 / 287, distance symbols
30 / 31, a distance that reaches in front of the stream, a stream that ends before its final block does.
"""
import deflate_writer as W


class DeflateError(ValueError):
    pass


class Block:
    """one block of a parsed stream.  tokens: [(symbol, start bit, width)], symbol an int (literal) or (length, distance), as in a
    deflate_writer symbol list; the width counts the codes and their extra bits.  Dynamic blocks: hlit / hdist / hclen as counts (257..286,
    1..30, 4..19), cl_lens the 19 code-length code lengths by symbol, cl_items the code-length section as (symbol, extra value), ll_lens /
    d_lens the lengths it spells.  start / end: the block's first bit and the bit behind its last; out_start / out_end: the bytes it made."""
    __slots__ = ("final", "btype", "start", "end", "hlit", "hdist", "hclen", "cl_lens", "cl_items", "ll_lens", "d_lens", "tokens", "eob",
                 "out_start", "out_end", "stored_len")

    def __init__(self):
        self.hlit = self.hdist = self.hclen = self.cl_lens = self.cl_items = self.ll_lens = self.d_lens = self.eob = self.stored_len = None
        self.tokens = []


class Parsed:
    """blocks, nbits (the bit behind the final block), out (the replayed bytes)"""
    __slots__ = ("blocks", "nbits", "out")


def decode_table(lens, what, single_ok=True):
    """(table, mask) for a canonical code: table[the next `max length` bits, LSB first] = symbol | length << 16, or -1 where no codeword
    is; None for a code without codewords.  Raises on an over-subscribed code, and on an incomplete one unless it is one 1-bit codeword."""
    used = [l for l in lens if l]
    if not used:
        return None
    mx = max(used)
    k, full = sum(1 << (mx - l) for l in used), 1 << mx
    if k > full:
        raise DeflateError("over-subscribed %s code" % what)
    if k < full and not (single_ok and mx == 1):
        raise DeflateError("incomplete %s code" % what)
    codes = W.canonical(list(lens))
    tab = [-1] * full
    for s, l in enumerate(lens):
        if l:
            r = int(format(codes[s], "0%db" % l)[::-1], 2)
            e = s | (l << 16)
            for j in range(r, full, 1 << l):
                tab[j] = e
    return tab, full - 1


_FIXED = None


def _fixed_tables():
    global _FIXED
    if _FIXED is None:
        _FIXED = (decode_table(W.FIXED_LL, "fixed"), decode_table([5] * 32, "fixed distance"))
    return _FIXED


def parse(data, max_out=None):
    """parse one raw DEFLATE stream (bytes behind its final block are ignored, as zlib ignores them).  max_out: a cap on the output, for
    containers that have one (BGZF: 65,536)."""
    data = bytes(data)
    acc = nacc = bp = 0                                   # bit accumulator: nacc bits of the stream from bit bp * 8 - nacc on
    out = bytearray()
    blocks = []
    LB, LE, DB, DE = W.LEN_BASE, W.LEN_EXTRA, W.DIST_BASE, W.DIST_EXTRA

    def fill(acc, nacc, bp):
        ch = data[bp:bp + 8]
        return acc | (int.from_bytes(ch, "little") << nacc), nacc + 8 * len(ch), bp + len(ch)

    def take(n):
        nonlocal acc, nacc, bp
        if nacc < n:
            acc, nacc, bp = fill(acc, nacc, bp)
            if nacc < n:
                raise DeflateError("the stream ends inside a block")
        v = acc & ((1 << n) - 1)
        acc >>= n
        nacc -= n
        return v

    def sym(tab_mask, what):
        """one codeword of a header code"""
        nonlocal acc, nacc, bp
        tab, mask = tab_mask
        if nacc < 16:
            acc, nacc, bp = fill(acc, nacc, bp)
        e = tab[acc & mask]
        if e < 0:
            raise DeflateError("a codeword the %s code does not have" % what)
        l = e >> 16
        if l > nacc:
            raise DeflateError("the stream ends inside a block")
        acc >>= l
        nacc -= l
        return e & 0xffff

    while True:
        b = Block()
        b.start = bp * 8 - nacc
        b.out_start = len(out)
        b.final = take(1)
        b.btype = take(2)
        if b.btype == 3:
            raise DeflateError("BTYPE 3")
        if b.btype == 0:
            take(-(bp * 8 - nacc) % 8)                                   # the padding bits: any value
            ln, nl = take(16), take(16)
            if ln ^ nl != 0xffff:
                raise DeflateError("stored block: NLEN is not the complement of LEN")
            at = bp - nacc // 8
            if at + ln > len(data):
                raise DeflateError("stored block: LEN runs past the stream")
            out += data[at:at + ln]
            acc = nacc = 0
            bp = at + ln
            b.stored_len = ln
        else:
            if b.btype == 1:
                lt, dt = _fixed_tables()
            else:
                b.hlit, b.hdist, b.hclen = take(5) + 257, take(5) + 1, take(4) + 4
                if b.hlit > 286 or b.hdist > 30:
                    raise DeflateError("HLIT %d / HDIST %d: too many lengths" % (b.hlit, b.hdist))
                b.cl_lens = [0] * 19
                for k in range(b.hclen):
                    b.cl_lens[W.CL_ORDER[k]] = take(3)
                ct = decode_table(b.cl_lens, "code-length", single_ok=False)
                if ct is None:
                    raise DeflateError("incomplete code-length code")
                lens, b.cl_items, tot = [], [], b.hlit + b.hdist
                while len(lens) < tot:
                    s = sym(ct, "code-length")
                    if s < 16:
                        x = 0
                        lens.append(s)
                    elif s == 16:
                        x = take(2)
                        if not lens:
                            raise DeflateError("repeat with no length before it")
                        lens += [lens[-1]] * (3 + x)
                    elif s == 17:
                        x = take(3)
                        lens += [0] * (3 + x)
                    else:
                        x = take(7)
                        lens += [0] * (11 + x)
                    b.cl_items.append((s, x))
                if len(lens) > tot:
                    raise DeflateError("a repeat runs past the last length")
                b.ll_lens, b.d_lens = lens[:b.hlit], lens[b.hlit:]
                if b.ll_lens[256] == 0:
                    raise DeflateError("no end-of-block code")
                lt = decode_table(b.ll_lens, "literal/length")
                dt = decode_table(b.d_lens, "distance")
            ltab, lmask = lt
            dtab, dmask = dt if dt else (None, 0)
            toks = b.tokens
            while True:
                if nacc < 48:
                    ch = data[bp:bp + 8]
                    acc |= int.from_bytes(ch, "little") << nacc
                    nacc += 8 * len(ch)
                    bp += len(ch)
                start = bp * 8 - nacc
                e = ltab[acc & lmask]
                if e < 0:
                    raise DeflateError("a codeword the literal/length code does not have")
                l = e >> 16
                s = e & 0xffff
                acc >>= l
                nacc -= l
                if s < 256:
                    if nacc < 0:
                        raise DeflateError("the stream ends inside a block")
                    out.append(s)
                    toks.append((s, start, l))
                    continue
                if s == 256:
                    if nacc < 0:
                        raise DeflateError("the stream ends inside a block")
                    b.eob = (start, l)
                    break
                if s > 285:
                    raise DeflateError("literal/length symbol %d" % s)
                eb = LE[s - 257]
                length = LB[s - 257] + (acc & ((1 << eb) - 1))
                acc >>= eb
                if dtab is None:
                    raise DeflateError("a match in a block without a distance code")
                e = dtab[acc & dmask]
                if e < 0:
                    raise DeflateError("a codeword the distance code does not have")
                dl = e >> 16
                dc = e & 0xffff
                if dc > 29:
                    raise DeflateError("distance symbol %d" % dc)
                db = DE[dc]
                dist = DB[dc] + ((acc >> dl) & ((1 << db) - 1))
                acc >>= dl + db
                nacc -= eb + dl + db
                if nacc < 0:
                    raise DeflateError("the stream ends inside a block")
                if dist > len(out):
                    raise DeflateError("distance %d at output position %d" % (dist, len(out)))
                toks.append(((length, dist), start, l + eb + dl + db))
                if dist >= length:
                    p = len(out) - dist
                    out += out[p:p + length]
                else:
                    piece = bytes(out[-dist:])
                    out += (piece * (length // dist + 1))[:length]
            if max_out is not None and len(out) > max_out:
                raise DeflateError("more than %d bytes of output" % max_out)
        if max_out is not None and len(out) > max_out:
            raise DeflateError("more than %d bytes of output" % max_out)
        b.end = bp * 8 - nacc
        b.out_end = len(out)
        blocks.append(b)
        if b.final:
            break
    r = Parsed()
    r.blocks, r.nbits, r.out = blocks, blocks[-1].end, bytes(out)
    return r


def replay(tokens, prefix=b""):
    """the bytes a token list means behind `prefix`"""
    out = bytearray(prefix)
    for s, _, _ in tokens:
        if isinstance(s, int):
            out.append(s)
        else:
            ln, d = s
            assert 1 <= d <= len(out), (d, len(out))
            for _ in range(ln):
                out.append(out[-d])
    return bytes(out[len(prefix):])
