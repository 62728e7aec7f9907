"""tests/deflate_reader.py against zlib: the parser that the encoder tests (tests/test_gpu_deflate_encoder.py) read the device's streams with
must itself mean what zlib means by every stream -- hand-built ones (tests/deflate_cases.py), zlib's own, deflate_writer.encode's -- and
must refuse what zlib refuses."""
import zlib

import pytest

import deflate_cases as D
import deflate_reader as R
import deflate_writer as W
import test_bgzip
from test_deflate_conformance import SHAPES, _payload

IDS = [c.name for c in D.CASES]


def check_against_zlib(stream, raw=None):
    """parse(stream) replays to zlib's bytes, its blocks tile the stream and the output, and its bit count is the stream's length up to
    the padding of the last byte (bytes behind the final block, which zlib reports as unused, apart)"""
    d = zlib.decompressobj(-15)
    exp = d.decompress(stream)
    assert d.eof and (raw is None or exp == raw)
    p = R.parse(stream)
    assert p.out == exp
    assert (p.nbits + 7) // 8 == len(stream) - len(d.unused_data)
    at_bit = at_out = 0
    for k, b in enumerate(p.blocks):
        assert b.start == at_bit and b.out_start == at_out and b.final == (k == len(p.blocks) - 1)
        if b.btype == 0:
            assert b.end == (b.start + 3 + 7) // 8 * 8 + 32 + 8 * b.stored_len and not b.tokens
        else:
            pos = b.tokens[0][1] if b.tokens else b.eob[0]
            assert pos >= b.start + 3
            for s, bit, width in b.tokens:
                assert bit == pos and width > 0
                pos += width
            assert b.eob[0] == pos and b.end == pos + b.eob[1]
            assert R.replay(b.tokens, exp[:b.out_start]) == exp[b.out_start:b.out_end]
        at_bit, at_out = b.end, b.out_end
    assert at_out == len(exp)
    return p


@pytest.mark.parametrize("name", IDS)
def test_reader_decides_every_case_as_zlib_does(name):
    c = D.by_name(name)
    pay = _payload(c)
    z = D.zlib_inflate(pay)
    assert (z is not None) == (c.cls == "valid")
    if c.cls == "valid":
        p = check_against_zlib(pay)
        assert p.out == z == D.built(c)[1]
    else:
        with pytest.raises(R.DeflateError):
            R.parse(pay, max_out=65536)


def test_reader_reports_the_header_the_writer_wrote():
    """a dynamic block's fields come back as deflate_writer put them: counts, the code-length code, the section's items, both codes"""
    syms = W.greedy_parse(D.TEXT[:6000])
    ll, dl = W.shaped_code(syms, 12)
    items = W.rle_lengths(ll + dl)
    st = W.Stream().dynamic(syms, ll, dl, final=True, cl_items=items)
    p = check_against_zlib(st.bytes(), bytes(st.out))
    b, = p.blocks
    f = [0] * 19
    for s, _ in items:
        f[s] += 1
    assert (b.btype, b.hlit, b.hdist) == (2, len(ll), len(dl)) and b.ll_lens == ll and b.d_lens == dl and b.cl_items == items
    assert b.cl_lens == W.huffman_lengths(f, 7) and [s for s, _, _ in b.tokens] == [t if isinstance(t, int) else tuple(t) for t in syms]
    w = W.FIXED_LL
    fx, = check_against_zlib(W.Stream().fixed(syms, final=True).bytes()).blocks
    assert [t[2] for t in fx.tokens] == [w[s] if isinstance(s, int) else w[W.length_code(s[0])[0]] + W.LEN_EXTRA[W.length_code(s[0])[0] - 257] + 5 +
                                         W.DIST_EXTRA[W.dist_code(s[1])[0]] for s in syms]


@pytest.mark.parametrize("level", [1, 6, 9])
def test_reader_on_zlib_streams(level):
    for name, raw in test_bgzip.inputs().items():
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        check_against_zlib(c.compress(raw) + c.flush(), raw)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_reader_on_writer_shapes(shape):
    kw = {k: v for k, v in SHAPES[shape].items() if k != "payload"}
    for raw in (D.TEXT[:40000], bytes(range(256)) * 3 + D.TEXT[:500], b"a"):
        check_against_zlib(W.encode(raw, **kw), raw)
