"""The synthetic workload made on the device must be the file the host generator writes.

The device deflates every BGZF payload with a restatement of zlib 1.2.11's level 6 (tools/zlib6_deflate.h); here the same code,
compiled for the host, is held to the system zlib byte for byte, and on the GPU whole segments are held to synth.bam_segment."""
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from duckhts_amd import synth  # noqa: E402


def zlib6(raw):
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY)
    z = c.compress(raw) + c.flush()
    return z if len(z) < 65536 - 26 else b""        # bgzf_block stores what level 6 cannot fit


def payloads():
    rng = np.random.default_rng(7)
    seg, _ = synth.bam_segment(3000, seed=11, total_n=92_000_000, rec0=45_000_000, with_header=False, with_eof=False, level=0)
    import gzip
    records = gzip.decompress(seg.tobytes())
    yield "records", records
    yield "random", rng.integers(0, 256, 200_000, dtype=np.uint8).tobytes()
    yield "zeros", bytes(150_000)
    parts = []
    for _ in range(120):
        k, n = int(rng.integers(0, 4)), int(rng.integers(1, 4000))
        if k == 0:
            parts.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        elif k == 1:
            parts.append(bytes([int(rng.integers(0, 256))]) * n)
        elif k == 2:
            parts.append(rng.integers(0, 4, n, dtype=np.uint8).tobytes())
        else:
            parts.append(b"".join(parts[-3:])[:n])
    yield "mixed", b"".join(parts)


@pytest.mark.parametrize("cut", [65280, 65279, 40000, 300, 3, 1])
def test_zlib6_restatement_equals_zlib(cut):
    for name, data in payloads():
        step = cut if cut > 1000 else 997
        for off in range(0, len(data), step):
            raw = data[off:off + cut]
            assert synth.zlib6_block(raw) == zlib6(raw), (name, off, len(raw))


def test_zlib6_restatement_empty_and_limit():
    assert synth.zlib6_block(b"") == zlib6(b"")
    with pytest.raises(ValueError):
        synth.zlib6_block(bytes(65281))


@pytest.mark.gpu
def test_gpu_segments_equal_host_generator():
    n, total = 30_000, 92_000_000
    got, sizes, raw = synth.bam_segments_gpu(n, 5, 3, seed=44, total_n=total, group=2)
    exp, exp_raw = [], 0
    for k in range(5, 8):
        a, st = synth.bam_segment(n, seed=44, total_n=total, rec0=k * n, with_header=False, with_eof=False)
        exp.append(a.tobytes())
        exp_raw += st["raw_bytes"]
    assert sizes == [len(e) for e in exp]
    assert raw == exp_raw
    assert got.tobytes() == b"".join(exp)
