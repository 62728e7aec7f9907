"""Sanitizer pass over bam_tile_scan_lanes' per-lane function (tools/hostsim/run_scan.sh: the text of tile_scan_lane -- line loads,
prefilter, rec_check_t<GSrc> three deep, light walk -- compiled for the host with ASAN + UBSAN) on the streams of tile_scan_cases.py and
the decoy files and the 3,000 synthetic records of test_gpu_tile_scan_lanes.py, tile by tile against a plain serial model, on images
that end where the stream's 16-byte padding ends.
A check of the function's indexing and arithmetic, not a product path."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _records(data):
    """(the record stream of a BAM file, the number of references its header names)"""
    import gzip
    import struct
    raw = gzip.decompress(data)
    l_text, = struct.unpack_from("<I", raw, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<I", raw, p); p += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<I", raw, p); p += 4 + l_name + 4
    return raw[p:], n_ref


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_lane_scan_is_sanitizer_clean_and_equals_a_serial_model(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import decoy_cases as D
    import tile_scan_cases as T
    from duckhts_amd import synth
    streams = {n: T.stream(n) for n in T.names()}
    for n in D.TILE_CASES:
        streams["decoy_" + n] = bytes(D.case("bam", n)["stream"])           # header and records, as the batch holds them: the decoys are placed by tile
    args = []
    for name, s in streams.items():
        p = tmp_path / (name + ".bin"); p.write_bytes(s); args.append(str(p))
    nonfinal = [n for n in T.names() if n.startswith("cut_") or n == "runs_past"]
    for name in nonfinal:                                                       # the same bytes as a batch that is not the file's last
        args += ["-t", str(tmp_path / (name + ".bin"))]
    # the GPU test's first stream: ordinary records (about 120 tiles), whole and cut inside its last record as a final and a non-final batch
    syn, n_ref = _records(synth.bam_file(3000, seed=7))
    assert len(syn) > 100 * T.TILE and n_ref >= 1
    (tmp_path / "synth3000.bin").write_bytes(syn); (tmp_path / "synth3000_cut.bin").write_bytes(syn[:len(syn) - 100])
    args += ["-r", str(n_ref), str(tmp_path / "synth3000.bin"), "-t", str(tmp_path / "synth3000.bin"),
             str(tmp_path / "synth3000_cut.bin"), "-t", str(tmp_path / "synth3000_cut.bin")]
    extra = 4
    r = subprocess.run([os.path.join(ROOT, "tools", "hostsim", "run_scan.sh")] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "MISMATCH" not in r.stdout
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith("tiles ")]
    assert len(lines) == len(streams) + len(nonfinal) + extra and all(l[3] == "0" for l in lines), r.stdout[-3000:]
    got = {}
    for l in lines:
        got[(os.path.basename(l[-1])[:-4], int(l[13]))] = {"tiles": int(l[1]), "with_first": int(l[5]), "without": int(l[7]), "records": int(l[9]), "err": int(l[11])}
    # the streams hold what they were built for (the model's numbers, which the function equalled)
    assert got[("long40k", 1)]["without"] >= 4                                  # tiles inside the long record
    assert got[("dense", 1)]["records"] >= 2 * 221                              # 221 starts in each of the two whole tiles behind tile 0
    assert all(got[(n, 1)]["err"] == 1 for n in ("bs31", "bs_minus1", "runs_past"))
    assert got[("runs_past", 0)]["err"] == 0                                    # incomplete is an error in the final batch only
    assert all(got[("cut_3_%d" % d, 1)]["err"] == 1 and got[("cut_3_%d" % d, 0)]["err"] == 0 for d in T.END_D)
    assert got[("decoy_every_tile_chain3", 1)]["tiles"] > 10
    for final in (0, 1):
        s = got[("synth3000", final)]
        assert s["tiles"] >= 100 and s["with_first"] == s["tiles"] and s["records"] > 2500 and s["err"] == 0
    assert got[("synth3000_cut", 1)]["err"] == 1 and got[("synth3000_cut", 0)]["err"] == 0
