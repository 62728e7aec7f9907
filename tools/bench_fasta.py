"""fasta_index / region fetch on a synthetic FASTA resident in HBM.

One sequence of --mbp million bases and --more further ones of --mbp2 million bases (slices of the first), 60 bases a line, each under its
own name (chr1, chr2, ...), are made on the host and uploaded once.  Prints WALL times of the build (all passes, copies and host round
trips) and of a fetch of the whole first sequence (host staging of offsets included); the kernel times come from running this under
`rocprofv3 --kernel-trace --stats -- python tools/bench_fasta.py`.  The host comparison (--ref) times tests/fasta_index_ref.py, a Python
restatement, on a small file: it is not htslib."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import duckhts_amd  # noqa: E402


def lines60(seq):
    n = len(seq)
    lines = np.full((n // 60, 61), 10, np.uint8)
    lines[:, :60] = seq[:n // 60 * 60].reshape(-1, 60)
    return lines.tobytes() + seq[n // 60 * 60:].tobytes() + (b"\n" if n % 60 else b"")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=int, default=250)
    ap.add_argument("--more", type=int, default=30)
    ap.add_argument("--mbp2", type=int, default=60)
    ap.add_argument("--ref", action="store_true", help="also time the Python restatement on 2 Mbp")
    a = ap.parse_args()
    seq = np.random.default_rng(1).choice(np.frombuffer(b"ACGT", np.uint8), a.mbp * 1000000)
    big, small = lines60(seq), lines60(seq[:a.mbp2 * 1000000])
    text = b">chr1\n" + big + b"".join(b">chr%d\n" % (k + 2) + small for k in range(a.more))
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(np.frombuffer(text, np.uint8))
        ctx.bgzf_index()
        out = {"text_bytes": len(text), "sequences": a.more + 1}
        for k in range(2):
            t0 = time.perf_counter()
            fai, _ = ctx.fasta_build_index()
            out["build_wall_s_run%d" % k] = round(time.perf_counter() - t0, 4)
        out["build_wall_GBps"] = round(out["text_bytes"] / out["build_wall_s_run1"] / 1e9, 2)
        ctx.fasta_load_index(fai)
        b = duckhts_amd.FastaBatch()
        for k in range(2):
            t0 = time.perf_counter()
            ctx._chk(ctx.L.dhts_fasta_fetch(ctx.h, b"chr1", b))
            out["fetch_wall_s_run%d" % k] = round(time.perf_counter() - t0, 4)
        out["fetch_bases"] = int(b.seq_nbytes)
        out["fai_lines"] = fai.decode().count("\n")
        out["fai_head"] = fai.decode().split("\n")[:3]
    finally:
        ctx.close()
    if a.ref:
        import fasta_index_ref as R
        small_text = b">s\n" + lines60(seq[:2000000])
        t0 = time.perf_counter()
        R.build(small_text)
        out["python_restatement_2mbp_s"] = round(time.perf_counter() - t0, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
