#!/usr/bin/env python3
"""read_bam on FASTQ TEXT (duckhts_amd/csrc/fastq_text.hip): full-scan throughput of the same reads in two forms on one MI355X.

The input is made at run time, nothing is committed: `--unique` four-line records of `--read-len` bases (seeded; every fourth quality
line begins with '@') are repeated until the text holds at least `--gb` GB, written uncompressed and as BGZF (the project's device
bgzip).  Each form is staged into HBM once; a step is one full scan (rewind, next_batch until the end) with the columns left in HBM.  One
JSON line per form -- records/s, text GB/s and the per-kernel times of the timed steps, from which the split between inflate, record
discovery + encoder (the text encoder's measure / write slots) and record stage is read -- printed and appended to
profiles/fastq/bench_fastq.jsonl."""
import argparse
import json
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import duckhts_amd  # noqa: E402
from bench_sam import GROUPS, scan  # noqa: E402


def render(n, read_len, seed):
    rng = np.random.default_rng(seed)
    seqs = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, read_len))]
    quals = np.frombuffer(b"#,:<@FIJ", np.uint8)[rng.integers(0, 8, (n, read_len))]
    quals[::4, 0] = ord("@")
    ys = rng.integers(0, 30000, n)
    out = []
    for i in range(n):
        out.append(b"@SIM:1:FCX:1:%d:%d:%d/%d\n%s\n+\n%s\n" % (i % 2000, ys[i], i, 1 + i % 2, seqs[i].tobytes(), quals[i].tobytes()))
    return b"".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--unique", type=int, default=100000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-blocks", type=int, default=0)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastq", "bench_fastq.jsonl"))
    a = ap.parse_args()
    block = render(a.unique, a.read_len, a.seed)
    reps = max(1, -(-int(a.gb * 1e9) // len(block)))
    d = tempfile.mkdtemp(prefix="bench_fastq_", dir=a.tmp)
    try:
        p_fq, p_gz = os.path.join(d, "t.fq"), os.path.join(d, "t.fq.gz")
        with open(p_fq, "wb") as f:
            for _ in range(reps):
                f.write(block)
        text_bytes = os.path.getsize(p_fq)
        ctx = duckhts_amd.Context(0)
        try:
            ctx.bgzip_file(p_fq, p_gz)
        finally:
            ctx.close()
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        for form, path in (("fq", p_fq), ("fq.gz", p_gz)):
            kind, rows, sec, kt = scan(path, a.steps, a.warmup, a.max_blocks)
            assert rows == a.unique * reps and kind in (3, 4), (form, rows, kind)
            split = {g: round(sum(kt.get(k, 0.0) for k in ks), 3) for g, ks in GROUPS.items()}
            line = json.dumps({"form": form, "is_text": kind, "file_bytes": os.path.getsize(path), "text_bytes": text_bytes, "records": rows, "read_len": a.read_len,
                               "ms_per_scan": round(sec * 1e3, 2), "records_per_s": round(rows / sec), "text_GBps": round(text_bytes / sec / 1e9, 3),
                               "kernel_ms": kt, "split_ms": split, "steps": a.steps, "max_blocks": a.max_blocks})
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
