"""DEFLATE conformance on the device: every hand-built stream of tests/deflate_cases.py through the BGZF inflate (phase A + phase B,
and every phase-A kernel on its own), through the knobs that pick other inflate paths (in child processes: they are read once per
process), and end to end: a BAM, a BCF and VCF text re-encoded in unusual shapes through read_bam / read_bcf, and malformed plain-gzip
members through the serial decoder.  The judge is CPython's zlib (the decoder htslib uses) and the oracle, which agrees with it on every
case (tests/test_deflate_conformance.py)."""
import os
import subprocess
import sys

import pytest

import deflate_cases as D
import deflate_writer as W
import duckhts_amd
import orc
from conftest import ROOT

pytestmark = pytest.mark.gpu


def _inflate_case(c):
    """the case's BGZF file (good block, case block, good block, EOF) through ctx.bgzf_inflate: per-block status and bytes"""
    f, blocks = D.bgzf_case_file(c)
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(f)
        nb = ctx.bgzf_index()
        assert nb == 4, (c.name, nb)
        out, bst = ctx.bgzf_inflate(0, nb, 4 * 65536 + 64)
        _, _, isize, st = ctx.bgzf_table(nb)
        assert st == 0
    finally:
        ctx.close()
    out, bst, isize = out.tobytes(), [int(x) for x in bst], [int(x) for x in isize]
    if blocks[1] is not None:
        assert bst == [0, 0, 0, 0], (c.name, c.note, bst)
        assert out == b"".join(blocks), (c.name, c.note)
    else:
        assert bst[0] == bst[2] == bst[3] == 0 and bst[1] != 0, (c.name, c.note, bst)
        assert out[:len(blocks[0])] == blocks[0]
        at = isize[0] + isize[1]
        assert out[at:at + len(blocks[2])] == blocks[2], c.name
        z = orc.bgzf_inflate_all(f)
        assert z["status"] == -3 and z["n_blocks"] == 1, (c.name, z["status"], z["n_blocks"])


def run_all_cases():
    for c in D.CASES:
        _inflate_case(c)


@pytest.mark.parametrize("name", [c.name for c in D.CASES])
def test_bgzf_inflate_every_case(name):
    """status 0 and zlib's bytes on valid cases; a non-zero status exactly on the case block of malformed ones (the blocks around it
    inflate), where the oracle's BGZF reader stops"""
    _inflate_case(D.by_name(name))


def test_phase_a_kernels_on_every_case():
    """phase-A kernels 0..3 (lane kernel with every symbol in LDS / the far table; wave kernel into fixed slots / the packed pool) emit
    the same words on every block; the case block fails in all of them when zlib rejects it, but where only a distance reaches in front
    of the block: the wave kernel leaves that to phase B, and its tokens must trip that test"""
    from test_gpu_bam import _huff_scratch, _replay_hits_bad_distance
    for c in D.CASES:
        f, blocks = D.bgzf_case_file(c)
        ctx = duckhts_amd.Context(0)
        try:
            ctx.open(f)
            nb = ctx.bgzf_index()
            ref = _huff_scratch(ctx, nb, 0)
            assert (ref[1] == ("failed",)) == (blocks[1] is None), (c.name, c.note)
            assert all(ref[b] != ("failed",) for b in (0, 2, 3)), c.name
            for kernel in (1, 2, 3):
                got = _huff_scratch(ctx, nb, kernel)
                for b, (x, y) in enumerate(zip(ref, got)):
                    if kernel >= 2 and x == ("failed",) and y != ("failed",):
                        assert c.far and _replay_hits_bad_distance(y), (c.name, b, kernel)
                        continue
                    assert x == y, f"{c.name}: block {b} differs between kernel 0 and kernel {kernel}"
        finally:
            ctx.close()


@pytest.mark.parametrize("knob", ["DHTS_PHASE_A=lane", "DHTS_INFLATE=fused", "DHTS_POOL_PER_BLOCK=2048", "DHTS_PHASE_A_NLO=196",
                                  "DHTS_PHASE_A_NLO=288"])
def test_every_case_under_inflate_knobs(knob):
    """the same per-case checks with another inflate path chosen (a child process: the knobs are read once per process)"""
    k, v = knob.split("=")
    env = dict(os.environ, **{k: v})
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_deflate_conformance as T\nT.run_all_cases()\nprint('cases ok')\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "cases ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


SHAPES = {"codes15": dict(maxlen=15, long_first=True), "farthest": dict(policy="farthest"),
          "smallblocks": dict(split=700, btypes=("dynamic", "fixed", "stored"), payload=20000)}


def _payloads():
    from test_deflate_conformance import reencode_payloads
    return reencode_payloads()


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_read_bam_on_reencoded_bam(shape):
    """a BAM whose BGZF blocks the writer made (15-bit codes / farthest matches / many small blocks): read_bam equals the oracle"""
    data = W.bgzf_reencode(_payloads()["bam"], **SHAPES[shape])
    exp = orc.bam_read(data)
    assert exp["status"] == 0 and exp["n_rows"] == 600
    got = duckhts_amd.read_bam(data, device=0)
    assert got["n_rows"] == exp["n_rows"]
    for k in duckhts_amd.BAM_COLUMNS:
        assert list(got[k]) == list(exp[k]), f"{shape}: column {k} differs"


@pytest.mark.parametrize("what", ["bcf", "vcf"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_read_bcf_on_reencoded_files(what, shape):
    """a BCF and BGZF-compressed VCF text made by the writer: read_bcf equals the oracle column for column"""
    raw = _payloads()[what]
    data = W.bgzf_reencode(raw, **SHAPES[shape])
    exp = orc.bcf_read(data)
    import bamwriter as bw
    assert exp["status"] == 0 and exp["n_rows"] > 0 and orc.bcf_cols_diff(orc.bcf_read(bw.bgzf_file(raw)), exp) is None
    got = duckhts_amd.read_bcf(data, device=0)
    assert orc.bcf_cols_diff(exp, got) is None


def test_plain_gzip_members_from_the_writer():
    """plain gzip (the serial decoder): VCF text in writer-made members is read as the text; a writer-made member behind it that zlib
    rejects ends the scan in an error with the rows in front of it (tests/test_plain_gzip.py's convention); the gap this pins: an
    incomplete code (one codeword of 2+ bits, several codewords short of the Kraft sum, an incomplete code-length code) is an error"""
    from test_plain_gzip import _expect, _text
    big = _text(6300, seed=11)
    # (the text ends 4,365 bytes into a 64 KiB chunk: what a bad member inflates before its error -- a prefix of what it means, at
    # most 32,867 bytes here -- stays inside that chunk, so the rows delivered are the ones in front of it, whatever a decoder emitted)
    assert len(big) % 65536 == 4365
    members = [W.gzip_member(W.encode(big[i:i + 60000], **kw), big[i:i + 60000])
               for i, kw in zip(range(0, len(big), 60000), [{k: v for k, v in SHAPES[s].items() if k != "payload"} for s in sorted(SHAPES)] * 100)]
    good = b"".join(members)
    assert gzip_all(good) == big
    _expect(good, big, False)
    delivered = big[:(len(big) // 65536) * 65536]
    rejected = []
    for c in D.CASES:
        if c.cls != "malformed":
            continue
        raw, intended = D.built(c)
        bad = good + W.gzip_member(raw, intended)
        if gzip_all(bad) is not None:
            continue                          # (malformed only as a BGZF block, e.g. more than 64 KiB of output)
        assert len(big) % 65536 + len(intended) < 65536, c.name
        _expect(bad, delivered, True)
        rejected.append(c.name)
    assert {"m_ll_single_2bit", "m_dist_single_2bit_used", "m_dist_single_15bit", "m_ll_incomplete", "m_cl_incomplete",
            "m_far_first_match", "m_fixed_dist_30"} <= set(rejected), rejected


def gzip_all(data):
    """zlib's reading of concatenated gzip members: the text, or None on any error"""
    import zlib
    out, rest = b"", data
    while rest:
        d = zlib.decompressobj(31)
        try:
            out += d.decompress(rest)
        except zlib.error:
            return None
        if not d.eof:
            return None
        rest = d.unused_data
    return out
