"""Sanitizer pass over the record helpers of the row passes (tools/hostsim/run_rows.sh: the text of aux_size, find_nul_t, aux_skip_known,
aux_skip_t, aux_find_t and rec_check_t compiled for the host with ASAN + UBSAN).  aux_size is compared with the switch it replaced for all
256 type bytes; the 64-bit HBM accessor and the 32-bit window accessor run over every record of the streams of test_gpu_row_window_edges
and test_gpu_aux_walk -- on exact-size images of the stream and of each tile's staged window -- against a plain serial walk.
A check of the helpers' indexing and arithmetic, not a product path."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stream(data):
    """the records of a BAM file written by bamwriter.bam_bytes (the header sits in BGZF blocks of its own)"""
    import gzip
    import struct
    raw = gzip.decompress(data)
    l_text, = struct.unpack_from("<I", raw, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<I", raw, p); p += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<I", raw, p); p += 4 + l_name + 4
    return raw[p:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_row_helpers_are_sanitizer_clean_and_equal_a_serial_walk(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bamwriter as BW
    import test_gpu_aux_walk as A
    import test_gpu_row_window_edges as W
    streams = {"edges": _stream(W._file()[0])}
    for far in (False, True):
        streams["walk_far" if far else "walk_near"] = _stream(A._walk_file(far)[0])
        for k in range(len(A.BROKEN)):
            streams["broken%d_%d" % (k, far)] = _stream(A._broken_file(k, far)[0])
    files = []
    for name, s in streams.items():
        p = tmp_path / (name + ".bin"); p.write_bytes(s); files.append(str(p))
    r = subprocess.run([os.path.join(ROOT, "tools", "hostsim", "run_rows.sh")] + files, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "aux_size: 256 type bytes compared with the switch" in r.stdout and "MISMATCH" not in r.stdout
    lines = [l for l in r.stdout.splitlines() if l.startswith("records")]
    assert len(lines) == len(files) and all(" mismatching 0 " in l for l in lines), r.stdout[-3000:]
    got = {os.path.basename(l.split()[-1])[:-4]: (int(l.split()[1]), int(l.split()[3]), int(l.split()[5])) for l in lines}
    assert got["edges"][0] == W._file()[1]["n_rows"] and got["edges"][1] > got["edges"][0] // 2           # records, most of them inside a window
    assert got["walk_near"][1] >= got["walk_near"][0] - 4 and got["walk_far"][1] < got["walk_far"][0] - 400     # near: the window walk; far: the case records leave it
    assert all(got["broken%d_%d" % (k, far)][2] == 1 for k in range(len(A.BROKEN)) for far in (0, 1))           # the model too calls that record invalid
