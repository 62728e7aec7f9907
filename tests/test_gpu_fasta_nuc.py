"""fasta_nuc on the device (fasta_nuc.hip, dhts_fasta_nuc.inc) through the Python mirror, against the CPU model tests/fasta_nuc_ref.py.
Every comparison is exact: integers, bytes, and the bit patterns of the two fractions."""
import ctypes as C
import gzip
import os
import random
import struct

import numpy as np
import pytest

import fasta_index_ref as F
import fasta_nuc_ref as M

pytestmark = pytest.mark.gpu

ALPHABET = b"ACGTNacgtn" * 6 + b"RYKMSWBDHVrykmswbdhv" + b"*-."
#        name, bases, line_blen, line terminator
SEQS = [(b"one", 1, 1, b"\n"), (b"b1", 49, 1, b"\n"), (b"w7", 4097, 7, b"\n"), (b"w50", 70000, 50, b"\n"), (b"x49", 49, 50, b"\n"), (b"x50", 50, 50, b"\n"),
        (b"x51", 51, 50, b"\n"), (b"w60", 4097, 60, b"\n"), (b"crlf", 4097, 50, b"\r\n"), (b"long", 5000, 5000, b"\n"), (b"tail", 130, 60, b"\n")]


def corner_fasta():
    rng = random.Random(20)
    out = bytearray()
    for name, n, blen, nl in SEQS:
        out += b">" + name + b" description" + nl
        seq = bytes(rng.choice(ALPHABET) for _ in range(n))
        for i in range(0, n, blen):
            out += seq[i:i + blen] + nl
    while out[-1:] in (b"\n", b"\r"):                              # the last sequence has no final newline
        out.pop()
    return bytes(out)


def bgzf_of(raw):
    import duckhts_amd
    ctx = duckhts_amd.Context(0)
    try:
        z = ctx.bgzf_compress(raw)
    finally:
        ctx.close()
    assert gzip.decompress(z) == raw
    return z


@pytest.fixture(scope="module")
def fa(tmp_path_factory):
    d = tmp_path_factory.mktemp("nuc")
    text = corner_fasta()
    assert len(text) < 300_000
    fai = F.save(F.build(text))
    names, tab = F.read(fai)
    assert [tab[n][2] for n in names] == [min(s[1], s[2]) for s in SEQS] and tab[b"crlf"][3] == 52 and tab[b"tail"][0] == 130
    z = bgzf_of(text)
    paths = {"plain": str(d / "corner.fa"), "bgzf": str(d / "corner.fa.gz")}
    open(paths["plain"], "wb").write(text)
    open(paths["bgzf"], "wb").write(z)
    for p in paths.values():
        open(p + ".fai", "wb").write(fai)
    return {"text": text, "fai": fai, "names": names, "tab": tab, "bytes": {"plain": text, "bgzf": z}, "paths": paths, "dir": str(d)}


def dbits(xs):
    return struct.pack("<%dd" % len(xs), *xs)


def same(got, exp, cols=None):
    cols = [k for k in exp if k != "n_rows"] if cols is None else cols
    assert got["n_rows"] == exp["n_rows"]
    assert sorted(k for k in got if k in M.COLUMNS) == sorted(cols)
    for k in cols:
        assert len(got[k]) == len(exp[k]), k
        if k in ("pct_at", "pct_gc"):
            assert dbits(got[k]) == dbits(exp[k]), k
        bad = [i for i in range(len(exp[k])) if got[k][i] != exp[k][i]]
        assert not bad, (k, bad[:5], [(got[k][i], exp[k][i]) for i in bad[:2]])


def open_ctx(fa, kind="plain", include_seq=True):
    import duckhts_amd
    ctx = duckhts_amd.Context(0)
    ctx.open(fa["bytes"][kind])
    ctx.fasta_load_index(fa["fai"])
    ctx.nuc_open(include_seq)
    return ctx


def model_rows(fa, ivs, include_seq=True):
    """ivs: (tid or -1, start, end)"""
    return M.rows_of(fa["text"], fa["tab"], [(fa["names"][t] if 0 <= t < len(fa["names"]) else b"?", s, e) for t, s, e in ivs], include_seq)


def run_intervals(fa, ivs, kind="plain"):
    ctx = open_ctx(fa, kind)
    try:
        got = ctx.nuc_intervals([t for t, _, _ in ivs], [s for _, s, _ in ivs], [e for _, _, e in ivs])
    finally:
        ctx.close()
    exp = model_rows(fa, ivs)
    exp["chrom"] = [None if c == b"?" else c for c in exp["chrom"]]          # the array entry has no name for an unknown chrom
    return got, exp


# ---- intervals through nuc_intervals -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["plain", "bgzf"])
def test_every_column_offset_and_length_on_the_50_column_sequence(fa, kind):
    t = fa["names"].index(b"w50")
    ivs = [(t, 150 + c, 150 + c + n) for c in range(50) for n in range(131)]
    got, exp = run_intervals(fa, ivs, kind)
    assert exp["n_rows"] == 50 * 131
    same(got, exp)


@pytest.mark.parametrize("name", [b"w7", b"crlf", b"b1", b"w60", b"tail"])
def test_offsets_and_lengths_on_the_other_line_shapes(fa, name):
    t = fa["names"].index(name)
    ln, _, blen, _ = fa["tab"][name]
    ivs = [(t, c, c + n) for c in range(0, min(ln, 2 * blen + 3)) for n in range(0, 70, 3) if c + n <= ln + 5]
    got, exp = run_intervals(fa, ivs)
    same(got, exp)


def test_one_interval_over_each_whole_sequence(fa):
    ivs = [(t, 0, fa["tab"][n][0]) for t, n in enumerate(fa["names"])]
    for kind in ("plain", "bgzf"):
        got, exp = run_intervals(fa, ivs, kind)
        same(got, exp)
    assert got["seq_len"] == [s[1] for s in SEQS] and got["num_other"][3] > 100


def test_more_than_64_intervals_end_inside_one_wave(fa):
    t = fa["names"].index(b"w50")
    ivs = [(t, 1000 + i, 1001 + i) for i in range(5000)]
    ivs += [(t, 7 * i, 7 * i + (i % 5)) for i in range(3000)]                  # and runs of short ones of mixed lengths, some empty
    got, exp = run_intervals(fa, ivs)
    same(got, exp)


def test_clamping_and_rows_without_a_fetch(fa):
    t, o, x = fa["names"].index(b"w50"), fa["names"].index(b"one"), fa["names"].index(b"tail")
    ivs = [(t, -5, -1), (t, -5, 3), (t, 69990, 70010), (t, 70000, 70001), (t, 80000, 90000), (t, 5, 5), (t, 9, 2), (-1, 0, 5), (-1, 5, 5), (-1, 9, 2),
           (o, 0, 1), (o, 0, 2), (o, -1, 0), (o, 1, 2), (x, 100, 500), (x, 129, 130), (x, 130, 131), (99, 0, 4), (t, -(1 << 40), 1 << 40)]
    got, exp = run_intervals(fa, ivs)
    same(got, exp)
    assert got["seq_len"][:7] == [1, 3, 10, 0, 0, 0, -7] and got["seq"][3] == b"" and got["seq"][5] is None and got["chrom"][8] is None
    assert got["n_rows"] == len(ivs) - 2                                        # an unknown chrom with bases gives no row


def test_counts_equal_a_host_count_over_what_fasta_fetch_returns(fa):
    import duckhts_amd
    rng = random.Random(5)
    ivs = []
    for t, n in enumerate(fa["names"]):
        ln = fa["tab"][n][0]
        ivs.append((t, 0, ln))
        for _ in range(30):
            s = rng.randrange(ln)
            ivs.append((t, s, rng.randrange(s + 1, ln + 1)))
    for kind in ("plain", "bgzf"):
        ctx = open_ctx(fa, kind, include_seq=False)
        try:
            got = ctx.nuc_intervals([t for t, _, _ in ivs], [s for _, s, _ in ivs], [e for _, _, e in ivs])
            seqs = ctx.fasta_fetch(b",".join(b"%s:%d-%d" % (fa["names"][t], s + 1, e) for t, s, e in ivs))
        finally:
            ctx.close()
        assert got["n_rows"] == len(ivs) == len(seqs)
        for i, (_, seq) in enumerate(seqs):
            up = seq.upper()
            cnt = [up.count(c) for c in (b"A", b"C", b"G", b"T", b"N")]
            assert [got[k][i] for k in ("num_a", "num_c", "num_g", "num_t", "num_n")] == cnt and got["num_other"][i] == len(seq) - sum(cnt) and got["seq_len"][i] == len(seq)


def test_nuc_open_needs_the_index():
    import duckhts_amd
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(b">a\nACGT\n")
        with pytest.raises(duckhts_amd.DhtsError, match="FASTA index"):
            ctx.nuc_open()
        ctx.fasta_load_index(b"a\t4\t3\t4\t5\n")
        with pytest.raises(duckhts_amd.DhtsError, match="dhts_nuc_open"):
            ctx.nuc_intervals([0], [0], [4])
        ctx.nuc_open()
        with pytest.raises(duckhts_amd.DhtsError, match="projection"):
            ctx.nuc_set_projection(["seq"])
        assert ctx.nuc_intervals([0], [0], [4])["pct_gc"] == [0.5]
    finally:
        ctx.close()


def test_a_file_that_ends_early_drops_rows(fa):
    import duckhts_amd
    text, fai = M_FA_CUT, F.save(F.build(M_FA))
    bed = b"s1\t0\t5\ns1\t0\t7\ns1\t0\t8\ns1\t6\t7\ns1\t7\t8\ns2\t0\t1\ns2\t1\t1\n"
    exp = M.fasta_nuc(text, fai, bed_text=bed, include_seq=True)
    got = duckhts_amd.fasta_nuc(text, fai=fai, bed=bed, include_seq=True)
    same(got, exp)
    assert got["seq"] == [b"ACGTN", b"ACGTNac", b"c", None]
    same(duckhts_amd.fasta_nuc(text, fai=fai, bin_width=3), M.fasta_nuc(text, fai, bin_width=3))


M_FA = b">s1\nACGTN\nacgtn\nRY\n>s2 comment\nAAAA\n>s3\nGG"
M_FA_CUT = M_FA[:M_FA.index(b"acgtn") + 2]


# ---- bins ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def bins_ref(fa):
    return {bw: M.fasta_nuc(fa["text"], fa["fai"], bin_width=bw) for bw in (1, 7, 50, 1000000)}


@pytest.mark.parametrize("bw,max_rows", [(1, 30000), (7, 1000), (50, 333), (1000000, 4)])
@pytest.mark.parametrize("kind", ["plain", "bgzf"])
def test_bins_without_a_region(fa, bins_ref, kind, bw, max_rows):
    import duckhts_amd
    if kind == "bgzf" and bw == 1:
        max_rows = 0                                                           # one batch
    st = {}
    got = duckhts_amd.fasta_nuc(fa["paths"][kind], bin_width=bw, max_rows=max_rows, stats=st)
    exp = bins_ref[bw]
    assert exp["n_rows"] == sum((s[1] + bw - 1) // bw for s in SEQS)
    assert st["n_batches"] == (1 if max_rows == 0 else (exp["n_rows"] + max_rows - 1) // max_rows) and (max_rows == 0 or st["n_batches"] >= 3)
    same(got, exp)


@pytest.mark.parametrize("region", ["w7:4000", "crlf", "w50:69,951-", "tail:-70", "w50:20,001-20,350", "x51:51-51", "one:2"])
@pytest.mark.parametrize("bw", [1, 7, 50, 1000000])
def test_bins_of_a_region(fa, region, bw):
    import duckhts_amd
    exp = M.fasta_nuc(fa["text"], fa["fai"], bin_width=bw, region=region, include_seq=True)
    for kind in ("plain", "bgzf"):
        st = {}
        got = duckhts_amd.fasta_nuc(fa["paths"][kind], bin_width=bw, region=region, include_seq=True, max_rows=37, stats=st)
        same(got, exp)
        if kind == "plain":
            assert st["resident_bytes"] < 5000                                # only the region's window is staged
    assert (exp["n_rows"] == 0) == (region == "one:2")


@pytest.mark.parametrize("region", ["nope", "w7:0-5", "w7:4099", "w7:1-4098", "w7:9-3"])
def test_invalid_regions(fa, region):
    import duckhts_amd
    with pytest.raises(M.NucError, match=M.ERR_REGION):
        M.fasta_nuc(fa["text"], fa["fai"], bin_width=10, region=region)
    with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_REGION):
        duckhts_amd.fasta_nuc(fa["paths"]["plain"], bin_width=10, region=region)


def test_argument_errors(fa):
    import duckhts_amd
    for kw, msg in (({}, M.ERR_ONE_OF), ({"bed": b"x\t1\t2\n", "bin_width": 3}, M.ERR_ONE_OF), ({"bin_width": 0}, M.ERR_BIN_WIDTH), ({"bin_width": 5, "fai": "/nonexistent.fai"}, M.ERR_OPEN_INDEX),
                    ({"bed": "/nonexistent.bed"}, M.ERR_OPEN_BED)):
        with pytest.raises(duckhts_amd.DhtsError, match=msg):
            duckhts_amd.fasta_nuc(fa["paths"]["plain"], **kw)
    with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_PATH):
        duckhts_amd.fasta_nuc("", bin_width=5)


# ---- BED -----------------------------------------------------------------------------------------------------------------------------

def messy_bed(fa):
    """good rows on every sequence, the lines fasta_nuc passes over, unknown chroms, zero and negative lengths; no final newline"""
    rng = random.Random(11)
    L = [b"#header", b"track name=x", b"browser position w50:1-10", b""]
    names = fa["names"]
    for i in range(3000):
        nm = names[rng.randrange(len(names))]
        ln = fa["tab"][nm][0]
        s = rng.randrange(-3, ln + 3)
        e = s + rng.choice([0, 1, 2, 7, 48, 49, 50, 51, 97, 300, -4, 5000])
        pad = b"\tfeature_%d\t%d\t+\tsome more columns to make the lines long enough for several batches" % (i, i % 1000)
        k = i % 40
        if k == 3:
            L.append(b"%s\t%d" % (nm, s))                                      # fewer than three fields
        elif k == 7:
            L.append(b"%s\t%dx\t%d%s" % (nm, s, e, pad))                        # start not wholly a number
        elif k == 11:
            L.append(b"%s\t%d\t%s" % (nm, s, pad))                              # end not a number
        elif k == 13:
            L.append(b"chrUnknown\t%d\t%d%s" % (s, e, pad))
        elif k == 17:
            L.append(b"%s\t%d\t\t%s" % (nm, s, pad))                            # empty end
        elif k == 19:
            L.append(b"# comment %d" % i)
        elif k == 23:
            L.append(b"%s\t%d\t%d\tcr%s\r" % (nm, s, e, pad))
        elif k == 29:
            L.append(b"%s\t%d\t%d\0hidden\t%s" % (nm, s, e, pad))               # the C string ends at the NUL, inside the end field
        elif k == 31:
            L.append(nm)
        else:
            L.append(b"%s\t%d\t%d%s" % (nm, s, e, pad))
    return b"\n".join(L)


@pytest.fixture(scope="module")
def bed(fa):
    text = messy_bed(fa)
    assert 3 * 65280 < len(text) < 400_000
    files = {"plain": text, "bgzf": bgzf_of(text), "gzip": gzip.compress(text, 6)}
    exp = M.fasta_nuc(fa["text"], fa["fai"], bed_text=text, include_seq=True)
    assert 2000 < exp["n_rows"] < 2900 and None in exp["seq"] and b"chrUnknown" in exp["chrom"] and min(exp["seq_len"]) < 0
    return {"text": text, "files": files, "exp": exp}


@pytest.mark.parametrize("kind", ["plain", "bgzf", "gzip"])
def test_bed_rows_in_every_container(fa, bed, kind):
    import duckhts_amd
    st = {}
    got = duckhts_amd.fasta_nuc(fa["paths"]["bgzf" if kind == "bgzf" else "plain"], bed=bed["files"][kind], include_seq=True, max_rows=1, stats=st)
    assert st["n_batches"] >= 3                                                # batches cut lines
    same(got, bed["exp"])


@pytest.mark.parametrize("region", ["w50:30,001-40,000", "tail", "w7:2,001-"])
def test_bed_region_without_an_index_filters_the_whole_file(fa, bed, region):
    import duckhts_amd
    exp = M.fasta_nuc(fa["text"], fa["fai"], bed_text=bed["text"], region=region, include_seq=True)
    assert 0 < exp["n_rows"] < 600
    for kind in ("plain", "bgzf"):
        same(duckhts_amd.fasta_nuc(fa["paths"][kind], bed=bed["files"][kind], region=region, include_seq=True), exp)


def sorted_bed(fa):
    L = [b"#sorted"]
    for nm in (b"w7", b"w50", b"crlf"):
        ln = fa["tab"][nm][0]
        for i in range(0, ln + 200, 23 if nm != b"w50" else 31):
            L.append(b"%s\t%d\t%d\tr%d\t0\t+\tpadding so that the file has more than one block ....................................." % (nm, i, i + 10 + (i % 7) * 40, i))
    return b"\n".join(L) + b"\n"


def build_index(bgzf, conf):
    import duckhts_amd
    L = duckhts_amd.lib()
    L.dhts_tabix_build_index.restype = C.c_int64; L.dhts_tabix_build_index.argtypes = [C.c_void_p] + [C.c_int] * 7
    L.dhts_bgzf_wrap.restype = C.c_int64; L.dhts_bgzf_wrap.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(bgzf); ctx.bgzf_index()
        n = L.dhts_tabix_build_index(ctx.h, conf[0], conf[1], conf[2], conf[3], conf[4], conf[5], 0)
        assert n > 0, L.dhts_error(ctx.h)
        raw = np.zeros(n, np.uint8)
        assert L.dhts_bam_index_bytes(ctx.h, raw.ctypes.data, n) == 0
    finally:
        ctx.close()
    need = L.dhts_bgzf_wrap(raw.ctypes.data, n, None, 0)
    out = np.zeros(need, np.uint8)
    got = L.dhts_bgzf_wrap(raw.ctypes.data, n, out.ctypes.data, need)
    return out[:got].tobytes()


@pytest.fixture(scope="module")
def indexed_bed(fa):
    text = sorted_bed(fa)
    z = bgzf_of(text)
    assert len(text) > 2 * 65280
    path = os.path.join(fa["dir"], "sorted.bed.gz")
    open(path, "wb").write(z)
    open(path + ".tbi", "wb").write(build_index(z, M.R.CONF_BED))
    bare = os.path.join(fa["dir"], "bare.bed.gz")
    open(bare, "wb").write(z)
    return {"text": text, "path": path, "bare": bare, "size": len(z)}


@pytest.mark.parametrize("region", ["w50:30,001-40,000", "crlf", "w7:4,000", "w50:100-100"])
def test_bed_region_with_and_without_the_tabix_index(fa, indexed_bed, region):
    import duckhts_amd
    exp = M.fasta_nuc(fa["text"], fa["fai"], bed_text=indexed_bed["text"], region=region, bed_indexed=True, include_seq=True)
    assert exp == M.fasta_nuc(fa["text"], fa["fai"], bed_text=indexed_bed["text"], region=region, bed_indexed=False, include_seq=True) and exp["n_rows"] > 0
    for kind in ("plain", "bgzf"):
        same(duckhts_amd.fasta_nuc(fa["paths"][kind], bed=indexed_bed["path"], region=region, include_seq=True, max_rows=1), exp)
        same(duckhts_amd.fasta_nuc(fa["paths"][kind], bed=indexed_bed["bare"], region=region, include_seq=True, max_rows=1), exp)
        same(duckhts_amd.fasta_nuc(fa["paths"][kind], bed=indexed_bed["bare"], bed_index=indexed_bed["path"] + ".tbi", region=region, include_seq=True), exp)


def test_a_sequence_the_bed_index_does_not_know(fa, indexed_bed):
    import duckhts_amd
    with pytest.raises(M.NucError, match=M.ERR_BED_ITER):
        M.fasta_nuc(fa["text"], fa["fai"], bed_text=indexed_bed["text"], region="tail", bed_indexed=True)
    with pytest.raises(duckhts_amd.BedIteratorError, match=M.ERR_BED_ITER):
        duckhts_amd.fasta_nuc(fa["paths"]["plain"], bed=indexed_bed["path"], region="tail")
    assert duckhts_amd.fasta_nuc(fa["paths"]["plain"], bed=indexed_bed["bare"], region="tail")["n_rows"] == 0     # no index: silent, the scan finds nothing


# ---- projections ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cols", [[], ["chrom", "start", "end"], ["num_other"], ["seq", "pct_gc", "chrom", "seq_len", "num_n", "start"], None], ids=lambda c: "all" if c is None else "+".join(c) or "count")
def test_projections(fa, bed, cols):
    import duckhts_amd
    got = duckhts_amd.fasta_nuc(fa["paths"]["plain"], bed=bed["files"]["bgzf"], include_seq=True, columns=cols, max_rows=2)
    same(got, bed["exp"], M.COLUMNS if cols is None else cols)
    exp = M.fasta_nuc(fa["text"], fa["fai"], bin_width=11, include_seq=True)
    same(duckhts_amd.fasta_nuc(fa["paths"]["bgzf"], bin_width=11, include_seq=True, columns=cols, max_rows=2500), exp, M.COLUMNS if cols is None else cols)
    if cols is None:
        assert list(k for k in got if k != "n_rows") == M.COLUMNS
