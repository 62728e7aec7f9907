"""tests/deflate_code_ref.py, the CPU restatement of the device encoder's code builder (dfl_build_lengths), on a few thousand count vectors
per alphabet: it terminates, the code is complete and within the cap, and it costs no more than the capped Shannon lengths it starts from.
The same vectors then go to the device (tests/test_gpu_deflate_encoder.py), which must give the same lengths and code words.

The cost against the optimum (package-merge, deflate_writer.huffman_lengths) is not bounded by design; the worst ratio over the committed
families is pinned (DESIGN.md records it next to the encoder): the run is deterministic, so the pin is a regression pin."""
import zlib
from fractions import Fraction

import pytest

import deflate_cases as D
import deflate_code_ref as Cr
import deflate_writer as W

# worst cost(restatement) / cost(package-merge) over families(nsym, maxbits), rounded up to 4 places
RECORDED_WORST = {(286, 15): Fraction(11702, 10000), (30, 15): Fraction(11572, 10000), (19, 7): Fraction(11583, 10000)}
_FAM = {}


def families(nsym, maxbits):
    if (nsym, maxbits) not in _FAM:
        _FAM[nsym, maxbits] = Cr.families(nsym, maxbits)
    return _FAM[nsym, maxbits]


@pytest.mark.parametrize("nsym,maxbits", Cr.ALPHABETS)
def test_restated_builder_on_the_families(nsym, maxbits):
    fam = families(nsym, maxbits)
    names = {f for f, _ in fam}
    assert len(fam) >= 2000 and names >= {"uniform", "heavy_tail", "giant_and_ones", "pow2_ladder", "fibonacci", "few_symbols", "all_equal", "ladder_and_ones"}
    assert max(sum(v) for _, v in fam) <= (316 if nsym == 19 else 65281) and all(len(v) == nsym for _, v in fam)
    one, n_over, worst = 1 << maxbits, 0, Fraction(0)
    for name, v in fam:
        info = {}
        lens = Cr.build_lengths(v, maxbits, info)                      # (raises NoProgress instead of spinning)
        used = sum(1 for f in v if f)
        assert sum(one >> l for l in lens if l) == one, (name, v)
        assert max(lens) <= maxbits, (name, v)
        if used >= 2:
            assert all((l == 0) == (f == 0) for l, f in zip(lens, v)), (name, v)
        else:
            assert sum(1 for l in lens if l) == 2 and all(l == 1 for f, l in zip(v, lens) if f), (name, v)      # the dummy second leaf
            continue
        n_over += info["oversubscribed"]
        if not info["oversubscribed"]:
            assert Cr.cost(v, lens) <= Cr.cost(v, Cr.shannon_lengths(v, maxbits)), (name, v)
        else:
            # what the lengthening loop is for: without it the code stays over-subscribed
            assert sum(one >> l for l in Cr.build_lengths(v, maxbits, lengthen=False) if l) > one
        worst = max(worst, Fraction(Cr.cost(v, lens), Cr.cost(v, W.huffman_lengths(v, maxbits))))
        tab = Cr.table_words(lens)
        assert all((t >> 16) == l for t, l in zip(tab, lens))
    print(f"code builder ({nsym} symbols, {maxbits} bits): {len(fam)} vectors, {n_over} over-subscribed, worst cost ratio to package-merge {float(worst):.4f}")
    assert n_over >= 20
    assert worst <= RECORDED_WORST[nsym, maxbits], float(worst)


def test_known_oversubscribing_vectors():
    for v, mb in ((Cr.OVERSUB_LL + [0] * (286 - 46), 15), (Cr.OVERSUB_CL + [0] * 5, 7)):
        info = {}
        lens = Cr.build_lengths(v, mb, info)
        assert info["oversubscribed"] and sum((1 << mb) >> l for l in lens if l) == 1 << mb and max(lens) == mb


def test_table_words_are_the_canonical_code_reversed():
    lens = [3, 3, 3, 3, 3, 2, 4, 4]                                   # RFC 1951 3.2.2: codes 010 011 100 101 110 00 1110 1111
    assert Cr.table_words(lens) == [0b010 | 3 << 16, 0b110 | 3 << 16, 0b001 | 3 << 16, 0b101 | 3 << 16, 0b011 | 3 << 16, 0b00 | 2 << 16, 0b0111 | 4 << 16, 0b1111 | 4 << 16]


def test_cl_sequence_runs():
    ll = [0] * 286
    for s in (0, 3, 7, 18, 30, 169, 256, 285):                        # zero runs of 2, 3, 10, 11, 138 and 86 (the rest of 224), 29 between them
        ll[s] = 8
    items = Cr.cl_sequence(ll, [5] + [0] * 29)
    assert items == [(8, 0), (0, 0), (0, 0), (8, 0), (17, 0), (8, 0), (17, 7), (8, 0), (18, 0), (8, 0), (18, 127), (8, 0), (18, 75), (8, 0), (18, 17), (8, 0), (5, 0)]
    ll = [0] * 286
    ll[0] = ll[140] = ll[256] = 2                                     # a run of 139: 138 and a plain zero
    assert Cr.cl_sequence(ll, [1, 1] + [0] * 28)[:4] == [(2, 0), (18, 127), (0, 0), (2, 0)]


@pytest.mark.parametrize("raw", [b"abc", b"a" * 20, D.TEXT[:3000], bytes(range(256)) * 8, D._rand(2000, 5)], ids=["abc", "run20", "text", "bytes", "random"])
def test_block_choice_sizes_are_the_sizes_of_real_blocks(raw):
    """dyn_bits and fix_bits are the bits deflate_writer needs for the same tokens with the header block_choice describes (zlib reads both)"""
    syms = W.greedy_parse(raw, chain=2)
    syms = [s if isinstance(s, int) or s[0] >= 4 else None for s in syms]
    if None in syms:                                                  # (the device takes no 3-byte matches: spell them as literals)
        out, pos = [], 0
        for s, g in zip(syms, W.greedy_parse(raw, chain=2)):
            out += list(raw[pos:pos + 3]) if s is None else [s]
            pos += 1 if isinstance(g, int) else g[0]
        syms = out
    ch = Cr.block_choice(syms, len(raw))
    st = W.Stream().dynamic(syms, ch["ll_lens"][:ch["hlit"]], ch["d_lens"][:ch["hdist"]], final=True, cl_items=ch["cl_items"], cl_lens=ch["cl_lens"])
    assert (len(st.bytes()) == (ch["dyn_bits"] + 7) // 8) and zlib.decompress(st.bytes(), -15) == raw
    fx = W.Stream().fixed(syms, final=True)
    assert (len(fx.bytes()) == (ch["fix_bits"] + 7) // 8) and zlib.decompress(fx.bytes(), -15) == raw
    best = min(ch["dyn_bits"], ch["fix_bits"])
    assert ch["btype"] == (0 if (best + 7) // 8 >= len(raw) + 5 else 2 if ch["dyn_bits"] < ch["fix_bits"] else 1)
    assert ch["nbytes"] == (len(raw) + 5 if ch["btype"] == 0 else (best + 7) // 8)
