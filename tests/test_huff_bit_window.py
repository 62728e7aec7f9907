"""Phase A's bit input (bgzf_huff_wave.hip, hw_span): the reader's state is the bit position, and every unit reads a 64-bit window of
three input-ring words.  Hand-built single-block BGZF files (tests/deflate_writer.py) that put the widest units -- a 15-bit length code
with 5 extra bits, then a 15-bit distance code with 13 extra bits: 48 bits -- at every bit phase and in every ring row, behind long codes
of both kinds, at the very end of the payload, in all 64 lanes, and in a burst that outruns the lane's input requests.

On the CPU the files go through the host build of the kernel text (tools/hostsim/run_wave.sh, ASAN + UBSAN): there every window read
asserts that its three ring rows hold the stream words w, w + 1, w + 2 (the commit invariant, the mirror rows, the wrap), the output must
equal the lane kernel's word for word and replay to the block's CRC32 / ISIZE.  On the device (-m gpu) the inflated bytes and their
CRC32 must be zlib's."""
import os
import re
import shutil
import subprocess
import zlib

import pytest

import deflate_writer as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAY0_BITS = 16          # a block at file offset 0: its payload starts at byte 18, i.e. at bit 16 of the aligned word the kernel counts from


def _lens(n, by_len):
    """code lengths by symbol from {length: [symbols]}"""
    out = [0] * n
    for ln, syms in by_len.items():
        for s in syms:
            out[s] = ln
    assert W.kraft(out) == 1 << 15, W.kraft(out)
    return out


# distance codes: 0..13 take 1..14 bits, 28 and 29 (13 extra bits) take 15
D_CHAIN = _lens(30, {k + 1: [k] for k in range(14)} | {15: [28, 29]})
A, Z = ord("a"), ord("Z")


def ll_chain(long_a, long_b):
    """16 literal/length symbols with 1..15, 15 bits: 'a' 1 bit, 285 (length 258) 2, 'b'..'l' 3..13, end of block 14, and two 15-bit
    symbols.  The codes above the 11-bit root share one root prefix: they are read through the second-level table."""
    return _lens(286, {1: [A], 2: [285]} | {k: [A + k - 2] for k in range(3, 14)} | {14: [256], 15: [long_a, long_b]})


def ll_many_long():
    """169 symbols: 'a' 1 bit, 285 2, 'b' 3, 'c' 4, end of block 5, 120 literals of 12 bits, 4 of 13, 8 of 14, and 30 literals + 281 + 284
    of 15 bits.  The codes above the 11-bit root span 64 root prefixes, more than the second-level table holds (32 x 16 entries): the
    kernel decodes them by canonical arithmetic."""
    lits = [s for s in range(256) if s not in (A, A + 1, A + 2)]
    return _lens(286, {1: [A], 2: [285], 3: [A + 1], 4: [A + 2], 5: [256], 12: lits[:120], 13: lits[120:124], 14: lits[124:132],
                       15: lits[132:162] + [281, 284]}), lits[132]


PREAMBLE = [A] + [(258, 1)] * 100            # 25,801 bytes of output, so that distances up to 25,801 reach inside the block


class Built:
    def __init__(self, name, deflate, raw, wide_at=(), tail=b""):
        self.name, self.raw, self.wide_at = name, bytes(raw), list(wide_at)
        self.payload = deflate + tail
        self.file = W.bgzf_block(self.payload, self.raw) + W.BGZF_EOF
        d = zlib.decompressobj(-15)
        assert d.decompress(self.payload) == self.raw and d.eof and d.unused_data == tail, name


def _wide_stream(name, ll, units, pads, in_front=(), lead=0, tail=b"", length_code=281):
    """a block with the preamble and `lead` one-bit literals, then a final block of `units` times {in_front, a wide unit, `pads`
    one-bit literals}; records the bit position (as the kernel counts it) of every wide unit"""
    st = W.Stream()
    st.dynamic(PREAMBLE + [A] * lead, ll, D_CHAIN, final=False)
    st.dynamic([], ll, D_CHAIN, final=True, eob=False)
    llc, dcs, at = W.canonical(ll), W.canonical(D_CHAIN), []
    for u in range(units):
        ln = W.LEN_BASE[length_code - 257] + u % (1 << W.LEN_EXTRA[length_code - 257])
        unit = (ln, 16385 + (u * 37) % 8192 if u % 2 == 0 else 24577 + (u * 5) % 1024, length_code)
        st._symbols(list(in_front), llc, ll, dcs, D_CHAIN)
        at.append(PAY0_BITS + 8 * len(st.w.buf) + st.w.n)
        st._symbols([unit] + [A] * pads, llc, ll, dcs, D_CHAIN)
    st.w.huff(llc[256], ll[256])
    assert len(st.out) <= 65536, len(st.out)
    return Built(name, st.bytes(), st.out, at, tail)


def _build_all():
    out = []
    ll = ll_chain(281, 284)
    # 1. wide units 49 bits apart: 256 units per block cover half of the 512 (row, phase) pairs, the second block starts 256 bits later
    out.append(_wide_stream("wide_every_phase_a", ll, 256, 1))
    out.append(_wide_stream("wide_every_phase_b", ll, 256, 1, lead=256))
    # 2. a 15-bit literal in front of every wide unit: through the second-level table, and by canonical arithmetic
    out.append(_wide_stream("wide_behind_second_level_literal", ll_chain(Z, 281), 200, 2, in_front=[Z]))
    llm, lit15 = ll_many_long()
    out.append(_wide_stream("wide_behind_canonical_literal", llm, 200, 2, in_front=[lit15, lit15 - 100]))
    # 3. the end-of-block symbol (14 bits, behind a wide unit) ends in the last byte of the payload, or 1..3 bytes in front of it
    #    (the one-bit literals in front are as many as make the payload end at byte k of a 4-byte word: the window of the last units
    #    reaches beyond the payload by a different amount in each)
    for k in range(4):
        b = next(b for b in (_wide_stream(f"eob_ends_{k + 1}_bytes_before_the_end", ll, 3, 0, lead=lead, tail=b"\0" * k) for lead in range(64))
                 if len(b.payload) % 4 == k)
        out.append(b)
    # 4. at least 64 x 256 bits of mixed symbols: 64 lanes, each starting wherever its range does
    import random
    rnd = random.Random(11)
    text = b"".join(b"read%05d\t%s\t%d\n" % (i, bytes(rnd.choice(b"ACGT") for _ in range(24)), rnd.randrange(10 ** 6)) for i in range(420))
    d = W.encode(text, maxlen=15, long_first=True)
    assert 8 * len(d) >= 64 * 256 + 2048                      # (the code-length section is well below 2,048 bits)
    out.append(Built("all_64_lanes_unaligned", d, text))
    # 5. 64 x 1,024 bits of match-only units, no literal between them.  A block holds 64 KiB of output, so the matches are 3 bytes long:
    #    a 15-bit length code without extra bits and the 28-bit distance, 43 bits a unit.  Four units take 172 bits and the lane's requests
    #    bring 128 per loop body: from the fourth body on the "fetch now and wait" path runs
    n = 64 * 1024 // 43 + 1
    out.append(_wide_stream("match_only_burst", ll_chain(257, 284), n, 0, length_code=257))
    # 6. stored + fixed + dynamic blocks in one member
    d = W.encode(text[:9000], maxlen=15, split=1500, btypes=("stored", "fixed", "dynamic"))
    out.append(Built("stored_fixed_dynamic", d, text[:9000]))
    return out


_BUILT = None


def built():
    global _BUILT
    if _BUILT is None:
        _BUILT = _build_all()
    return _BUILT


NAMES = ["wide_every_phase_a", "wide_every_phase_b", "wide_behind_second_level_literal", "wide_behind_canonical_literal",
         "eob_ends_1_bytes_before_the_end", "eob_ends_2_bytes_before_the_end", "eob_ends_3_bytes_before_the_end",
         "eob_ends_4_bytes_before_the_end", "all_64_lanes_unaligned", "match_only_burst", "stored_fixed_dynamic"]


def by_name(name):
    return next(b for b in built() if b.name == name)


def test_streams_are_what_they_claim():
    """zlib reads every stream (checked when built); the wide units of the two phase blocks start at all 512 (ring row, bit phase)
    pairs -- rows 14 and 15, whose windows run into the mirror rows, included; every file is one block of a few KiB"""
    assert [b.name for b in built()] == NAMES
    seen = set()
    for n in ("wide_every_phase_a", "wide_every_phase_b"):
        seen |= {p % 512 for p in by_name(n).wide_at}
    assert seen == set(range(512))
    for n in ("wide_behind_second_level_literal", "wide_behind_canonical_literal"):
        assert len({p % 32 for p in by_name(n).wide_at}) == 32 and len({(p >> 5) & 15 for p in by_name(n).wide_at}) == 16
    for b in built():
        assert len(b.file) < 16384, (b.name, len(b.file))
    for k in range(4):
        b = by_name(f"eob_ends_{k + 1}_bytes_before_the_end")
        assert b.payload.endswith(b"\0" * k) and zlib.decompressobj(-15).decompress(b.payload[:len(b.payload) - k]) == b.raw
        with pytest.raises(zlib.error):
            zlib.decompress(b.payload[:len(b.payload) - k - 1], -15)          # (the byte in front holds bits of the end-of-block symbol)
    assert {len(by_name(f"eob_ends_{k + 1}_bytes_before_the_end").payload) % 4 for k in range(4)} == {0, 1, 2, 3}


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("name", NAMES)
def test_host_simulation(name, tmp_path):
    """the file through the host build of both phase-A kernel texts (a process per file, so that a shadow assertion or a sanitizer
    report, which abort the run, name their file): the block and the EOF block decode in both kernels, the wave kernel's words equal
    the lane kernel's and replay to CRC32 / ISIZE, and every window read was checked against the shadow"""
    p = tmp_path / f"{name}.bgzf"
    p.write_bytes(by_name(name).file)
    r = subprocess.run([os.path.join(ROOT, "tools", "hostsim", "run_wave.sh"), "--per-block", str(p)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (name, r.stdout[-3000:] + r.stderr[-3000:])
    rows = [tuple(int(m.group(k)) for k in range(1, 4)) for m in re.finditer(r": block \d+ lane (-?\d+) wave (-?\d+) replay (-?\d+)$", r.stdout, re.M)]
    assert rows == [(0, 0, 0), (0, 0, 0)], (name, rows)
    assert "mismatching 0 differing-from-lane-kernel 0" in r.stdout, r.stdout
    m = re.search(r"windows read, each checked against the shadow of the ring: (\d+)", r.stdout)
    assert m and int(m.group(1)) > 0, r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_device_inflate_equals_zlib(name):
    """bgzf_inflate on the device: status 0, zlib's bytes, zlib's CRC32; and every phase-A kernel emits the lane kernel's words"""
    import duckhts_amd
    from test_gpu_bam import _huff_scratch
    b = by_name(name)
    want = zlib.decompressobj(-15).decompress(b.payload)
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(b.file)
        nb = ctx.bgzf_index()
        assert nb == 2
        out, bst = ctx.bgzf_inflate(0, nb, 65536 + 64)
        assert [int(x) for x in bst] == [0, 0], (name, bst)
        got = out.tobytes()
        assert got == want and zlib.crc32(got) == zlib.crc32(want) == int.from_bytes(b.file[-36:-32], "little")
        ref = _huff_scratch(ctx, nb, 0)
        assert ref[0] != ("failed",)
        for kernel in (2, 3):
            assert _huff_scratch(ctx, nb, kernel) == ref, f"{name}: kernel {kernel} differs from the lane kernel"
    finally:
        ctx.close()
