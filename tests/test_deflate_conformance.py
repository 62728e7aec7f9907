"""DEFLATE conformance on hand-built streams (tests/deflate_cases.py): shapes zlib's deflate never emits and headers zlib's inflate
rejects.  The judge is CPython's zlib, the decoder htslib uses; checked here on the CPU: the oracle's RFC 1951 restatement, libdeflate
(the other decoder htslib can be built with) where this machine has it, and the host build of the two phase-A kernel texts under
ASAN + UBSAN (tools/hostsim/run_wave.sh) -- the same kernel text meets every malformed input here before a GPU does."""
import ctypes as C
import ctypes.util
import os
import re
import shutil
import subprocess

import pytest

import deflate_cases as D
import deflate_writer as W
import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c.name for c in D.CASES]


def _payload(c):
    """the bytes a BGZF reader hands the inflater: the DEFLATE stream and the 8-byte trailer behind it"""
    raw, intended = D.built(c)
    return raw + W.bgzf_block(raw, intended, isize=min(len(intended), 65536))[-8:]


def test_catalogue_covers_both_classes():
    assert len(set(IDS)) == len(IDS)
    assert sum(c.cls == "valid" for c in D.CASES) >= 25 and sum(c.cls == "malformed" for c in D.CASES) >= 20
    assert all(c.cls in ("valid", "malformed") and len(c.note) > 20 for c in D.CASES)
    assert all(not c.far or c.cls == "malformed" for c in D.CASES)


@pytest.mark.parametrize("name", IDS)
def test_case_is_of_its_class(name):
    """zlib decides every case as it was written to be decided; a valid case inflates to the output its symbols mean"""
    c = D.by_name(name)
    z = D.zlib_inflate(_payload(c))
    if c.cls == "valid":
        assert z is not None and z == D.built(c)[1]
    else:
        assert z is None


@pytest.mark.parametrize("name", IDS)
def test_oracle_inflate_equals_zlib(name):
    """orc_inflate_raw (which judges every device decoder in the suite) makes zlib's bytes of every case, or rejects it as zlib does;
    its BGZF reader stops at the case block exactly when zlib rejects it"""
    c = D.by_name(name)
    z = D.zlib_inflate(_payload(c))
    r, out = orc.inflate_raw(_payload(c))
    assert (r == 0) == (z is not None), f"{name}: oracle {'accepts' if r == 0 else 'rejects'}, zlib {'rejects' if z is None else 'accepts'}"
    if z is not None:
        assert out == z
    f, blocks = D.bgzf_case_file(c)
    res = orc.bgzf_inflate_all(f)
    if z is not None:
        assert res["status"] == 0 and res["n_blocks"] == 4 and res["data"] == b"".join(blocks)
    else:
        assert res["status"] == -3 and res["n_blocks"] == 1 and res["data"] == blocks[0]


_LD = ctypes.util.find_library("deflate")


@pytest.mark.skipif(_LD is None, reason="libdeflate is not installed")
@pytest.mark.parametrize("name", IDS)
def test_libdeflate_agrees_with_zlib(name):
    """libdeflate decides every case as zlib does, but for the cases whose notes name where it is more lenient (it then accepts)"""
    L = C.CDLL(_LD)
    L.libdeflate_alloc_decompressor.restype = C.c_void_p
    L.libdeflate_free_decompressor.argtypes = [C.c_void_p]
    L.libdeflate_deflate_decompress_ex.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    c = D.by_name(name)
    p = _payload(c)
    d = L.libdeflate_alloc_decompressor()
    try:
        buf = C.create_string_buffer(65536)
        nin, nout = C.c_size_t(), C.c_size_t()
        r = L.libdeflate_deflate_decompress_ex(d, p, len(p), buf, 65536, C.byref(nin), C.byref(nout))
    finally:
        L.libdeflate_free_decompressor(d)
    got = buf.raw[:nout.value] if r == 0 else None
    z = D.zlib_inflate(p)
    if c.libdeflate is None:
        assert got == z, f"{name}: libdeflate status {r}"
    else:
        assert c.cls == "malformed" and c.libdeflate.startswith("accepts") and (got is None or r == 0)


def _reencoded_files(tmp_path):
    """a BAM, a BCF and VCF text, each re-encoded by the writer in three shapes"""
    out = []
    for name, raw in reencode_payloads().items():
        for shape, kw in SHAPES.items():
            p = tmp_path / f"{name}_{shape}.bgzf"
            p.write_bytes(W.bgzf_reencode(raw, **kw))
            out.append(str(p))
    return out


def reencode_payloads():
    """the uncompressed bytes of a BAM (cases.case_basic), a BCF (bcf_cases fuzz records) and VCF text"""
    import bcf_cases
    import bcfwriter
    import cases
    bam = orc.bgzf_inflate_all(cases.case_basic(n=600))["data"]
    bcf = orc.bgzf_inflate_all(bcfwriter.bcf_bytes(bcf_cases.std_header(), bcf_cases.fuzz_records(3, 300, 3)))["data"]
    vcf = open(os.path.join(ROOT, "tests", "golden", "vcf_file.vcf"), "rb").read()
    return {"bam": bam, "bcf": bcf, "vcf": vcf}


SHAPES = {"codes15": dict(maxlen=15, long_first=True), "farthest": dict(policy="farthest"),
          "smallblocks": dict(split=700, btypes=("dynamic", "fixed", "stored"), payload=20000)}


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_phase_a_kernel_texts_on_every_case(tmp_path):
    """the wave kernel and the lane kernel (host builds, ASAN + UBSAN) on every case as a BGZF file (good block, case block, good
    block, EOF): valid blocks replay to their CRC32 / ISIZE trailer and both kernels emit the same words; malformed blocks fail in
    both, but where a distance reaches in front of the block: the wave kernel leaves that test to phase B, so its tokens must trip it"""
    files = []
    for c in D.CASES:
        p = tmp_path / f"{c.name}.bgzf"
        p.write_bytes(D.bgzf_case_file(c)[0])
        files.append(str(p))
    shaped = _reencoded_files(tmp_path)
    r = subprocess.run([os.path.join(ROOT, "tools", "hostsim", "run_wave.sh"), "--per-block"] + files + shaped,
                       capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rows = {}
    for m in re.finditer(r"^(\S+): block (\d+) lane (-?\d+) wave (-?\d+) replay (-?\d+)$", r.stdout, re.M):
        rows.setdefault(os.path.basename(m.group(1)), []).append(tuple(int(m.group(k)) for k in range(2, 6)))
    for c in D.CASES:
        got = rows[f"{c.name}.bgzf"]
        assert len(got) == 4, (c.name, got)
        for b, lane, wave, rp in got:
            if b != 1 or c.cls == "valid":
                assert lane == 0 and wave == 0 and rp == 0, (c.name, b, lane, wave, rp)
            elif c.far:
                assert lane != 0 and (wave != 0 or rp == 2), (c.name, lane, wave, rp)
            else:
                assert lane != 0 and wave != 0, (c.name, c.note, lane, wave, rp)
    for f in shaped:
        got = rows[os.path.basename(f)]
        assert len(got) > 1 and all(x[1:] == (0, 0, 0) for x in got), (f, got)
