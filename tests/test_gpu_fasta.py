"""fasta_index and read_fasta regions on the device (fasta_index.hip, dhts_fasta_index.inc), through the C ABI's ctypes mirror: device
bytes against tests/fasta_index_ref.py, the restatement of htslib's fai_build_core / fai_retrieve that tests/test_fasta_index_ref.py pins
on htslib's fixtures."""
import gzip
import os

import numpy as np
import pytest

import bamwriter as W
import duckhts_amd
import fasta_index_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "htslib_faidx")


def _g(name):
    return open(os.path.join(GOLD, name), "rb").read()


@pytest.fixture(scope="module")
def ce():
    text = R.ce_shaped()
    return text, W.bgzf_file(text)


def build(data, batch_blocks=None):
    """(.fai, .gzi, block table) of `data` on the device"""
    ctx = duckhts_amd.Context(0)
    old = os.environ.get("DHTS_BATCH_BLOCKS")
    try:
        if batch_blocks:
            os.environ["DHTS_BATCH_BLOCKS"] = str(batch_blocks)
        ctx.open(data)
        nb = ctx.bgzf_index()
        fai, gzi = ctx.fasta_build_index()
        coff, _, isize, _ = ctx.bgzf_table(nb)
        return fai, gzi, (coff, isize)
    finally:
        ctx.close()
        if batch_blocks:
            if old is None:
                del os.environ["DHTS_BATCH_BLOCKS"]
            else:
                os.environ["DHTS_BATCH_BLOCKS"] = old


def check(text, data=None, **kw):
    fai, gzi, (coff, isize) = build(text if data is None else data, **kw)
    assert fai == R.save(R.build(text))
    if data is None or data[:2] != b"\x1f\x8b":
        assert gzi == b""
    else:                                              # the .gzi by the restatement's rule on the context's own block table
        uoff = np.concatenate([np.zeros(1, np.uint64), np.cumsum(isize.astype(np.uint64))])[:-1]
        assert gzi == R.gzi(coff, uoff, isize)
        assert gzi == R.gzi(*R.bgzf_blocks(data))
    return fai


def test_faidx_fa():
    text = _g("faidx.fa")
    assert check(text) == _g("faidx.fa.expected.fai")
    assert check(text, W.bgzf_file(text, payload=61)) == _g("faidx.fa.expected.fai")


def test_ce_shaped(ce):
    text, bg = ce
    assert check(text) == _g("ce.fa.fai")
    assert check(text, bg) == _g("ce.fa.fai")


def test_ce_shaped_one_block_per_batch(ce):
    """the 1 Mbp record spans more than a dozen batches; block ends cut lines, and one cuts the header of CHROMOSOME_II (16 * 64,376 =
    1,030,016 lies inside the header line at [1,030,010, 1,030,024))"""
    text, _ = ce
    bg = W.bgzf_file(text, payload=64376)
    assert len(R.bgzf_blocks(bg)[0]) > 12 and text[1030010:1030024] == b">CHROMOSOME_II"
    assert check(text, bg, batch_blocks=1) == _g("ce.fa.fai")


@pytest.mark.parametrize("width", [1, 15, 16, 17, 63, 64, 65, 257])
@pytest.mark.parametrize("final_nl", [True, False])
def test_line_widths(width, final_nl):
    rng = np.random.default_rng(width)
    out = bytearray()
    for k, n in enumerate([width * 37 + width // 2 + (1 if width > 1 else 0), width * 3, width * 20 + max(width - 1, 1)]):
        seq = rng.choice(np.frombuffer(b"ACGTNacgt", np.uint8), n).tobytes()
        out += b">s%d some words\n" % k + b"".join(seq[i:i + width] + b"\n" for i in range(0, n, width))
    text = bytes(out) if final_nl else bytes(out[:-1])
    check(text)
    check(text, W.bgzf_file(text, payload=997), batch_blocks=2)


def test_duplicates_and_empty_records():
    check(b">a\nACGT\nAC\n>a\nGGGGGG\n>b\n>c d\n\n>e\nTT\n\n\r\n>f\r\nAC\r\nA\r\n")
    check(b"\n\r\n>a\nAC\n>")                          # blank lines in front; a bare '>' as the last byte
    check(b">a\n\r\n\r\n")                             # "\r\n" while IN_SEQ is a sequence line of no bases


ERRORS = [
    (b">a\nACGT\nACGT\nACGTA\nAC\n", "Different line length in sequence 'a' at line 4"),
    (b">a\nACGT\nAC\nACGT\n", 'Format error, unexpected "A" at line 4'),
    (b">a\nACGT\nAC\n\x01\n", "Format error, unexpected character at line 4"),
    (b">a\nACGT\nAC\n\rX\n", "Format error, carriage return not followed by new line at line 4"),
    (b">a\nACGT\nAC\n@b\n", "Found '@' in a FASTA file, error at line 4"),
    (b">a\nACGT\n>b\n", "File truncated at line 4"),
    (b">a\nACGT\n>b", "The last entry 'b' has no sequence at line 3"),
    (b">a\nACGT\n>b x", "File truncated at line 4"),
    (b"\n\n", "File truncated at line 3"),
    (b">a\nACGT\nAC\n@b\nACGTAA\n", "Found '@' in a FASTA file, error at line 4"),      # the first in file order
]


@pytest.mark.parametrize("text,msg", ERRORS)
def test_errors(text, msg):
    with pytest.raises(R.FaidxError) as e:
        R.build(text)
    assert str(e.value) == msg                         # (the restatement says the same)
    with pytest.raises(duckhts_amd.DhtsError) as d:
        build(text)
    assert str(d.value) == msg


def test_different_line_length_in_a_later_batch():
    lines = [b"ACGTACGTAC"] * 30000
    lines[25000] = b"ACGTACGTACG"
    text = b">chr one\n" + b"\n".join(lines) + b"\n"
    with pytest.raises(duckhts_amd.DhtsError) as d:
        build(W.bgzf_file(text), batch_blocks=1)      # line 25,002 lies in the fifth block
    assert str(d.value) == "Different line length in sequence 'chr' at line 25002"


def test_fastq_and_plain_gzip_are_refused():
    with pytest.raises(duckhts_amd.DhtsError) as d:
        build(b"@r1\nACGT\n+\nIIII\n")
    assert "FASTQ" in str(d.value)
    with pytest.raises(duckhts_amd.DhtsError) as d:
        build(gzip.compress(b">a\nACGTACGT\nACGT\n"))
    assert str(d.value) == "Cannot index files compressed with gzip, please use bgzip"


# ---- fetch ---------------------------------------------------------------------------------------------------------------------------
def fetch(data, fai, regions):
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(data)
        ctx.fasta_load_index(fai)
        return ctx.fasta_fetch(regions)
    finally:
        ctx.close()


def expect(text, fai, regions):
    _, tab = R.read(fai)
    return [(r.split(b":")[0], R.fetch(text, tab, r)) for r in R.split_regions(regions.encode())]


def test_fetch_regions(ce):
    text, bg = ce
    fai = _g("ce.fa.fai")
    regions = ("CHROMOSOME_I:7-23, CHROMOSOME_I:101-150,CHROMOSOME_II:51-100,CHROMOSOME_I:13-100012,CHROMOSOME_III,,CHROMOSOME_X:6000-7000,"
               "CHROMOSOME_MtDNA:4990,CHROMOSOME_V:-10,CHROMOSOME_I:1-10")
    want = expect(text, fai, regions)
    assert [len(s) for _, s in want] == [17, 50, 50, 100000, 5000, 0, 11, 10, 10]
    assert fetch(text, fai, regions) == want
    assert fetch(bg, fai, regions) == want


def test_fetch_faidx_fa():
    text = _g("faidx.fa")
    fai = _g("faidx.fa.expected.fai")
    regions = "trailingblank2:28-33,trailingblank3:4-5,bar:4-5,trailingblank3,foo,trailingblank1:12-14"
    want = expect(text, fai, regions)
    assert want[1] == (b"trailingblank3", b"TA") and want[0][1] == b"GGGCCC"
    assert fetch(text, fai, regions) == want
    assert fetch(W.bgzf_file(text, payload=61), fai, regions) == want


def test_fetch_errors(ce):
    text, _ = ce
    fai = _g("ce.fa.fai")
    for bad_fai, regions, msg in [
        (fai.replace(b"CHROMOSOME_II\t5000\t1030025\t50\t51", b"CHROMOSOME_II\t5000\t1030025\t0\t51"), "CHROMOSOME_II:1-10", "Invalid line length in index: 0"),
        (fai.replace(b"1055602", b"9055602"), "CHROMOSOME_MtDNA:1-10", "Failed to retrieve block: unexpected end of file"),
        (fai, "CHROMOSOME_I:1-10,nope:1-10", "Reference nope:1-10 not found in FASTA file"),
    ]:
        _, tab = R.read(bad_fai)
        with pytest.raises(R.FaidxError) as e:
            [R.fetch(text, tab, r) for r in R.split_regions(regions.encode())]
        assert str(e.value) == msg
        with pytest.raises(duckhts_amd.DhtsError) as d:
            fetch(text, bad_fai, regions)
        assert str(d.value) == msg


def test_fetch_stages_only_the_windows(tmp_path):
    """an uncompressed file of a few MB: the resident bytes are the regions' windows, not the file"""
    rng = np.random.default_rng(5)
    parts = []
    for k in range(4):
        seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), 1000000).tobytes()
        parts.append(b">c%d\n" % k + b"".join(seq[i:i + 60] + b"\n" for i in range(0, len(seq), 60)))
    text = b"".join(parts)
    path = tmp_path / "few_mb.fa"
    path.write_bytes(text)
    fai = R.save(R.build(text))
    regions = "c0:100-250,c3:999000-1000000,c1:5-6,c3:999990-1000100"
    ctx = duckhts_amd.Context(0)
    try:
        ctx.fasta_load_index(fai)
        ctx.fasta_open_regions(str(path), regions)
        staged = ctx.resident_bytes()
        got = ctx.fasta_fetch(regions)
    finally:
        ctx.close()
    assert got == expect(text, fai, regions)
    assert 0 < staged < 4096 and len(text) > 4000000
