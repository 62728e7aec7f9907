#!/usr/bin/env python3
"""Measures the seq_* / cigar_* functions and seq_kmers on read_bam batches kept in HBM (dhts_udf_*, duckhts_amd/csrc/seq_udf.hip).

A synthetic BAM from the project's generator (150-base reads) is scanned once; on every batch each function runs on the batch's own SEQ /
CIGAR column and its kernel time is read from the context's HIP-event timers.  Bytes = what the function has to move through HBM at least
(its input once, its output once), so bytes / time against the HBM peak says how far from the memory bound a kernel is.  Separately: the
time of ONE call on 2,048 host rows -- upload, launch, download -- which is what a per-chunk scalar call of a SQL host would pay.

Nothing here is a pass bar.  One JSON line on stdout; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_TBS = 8.0            # MI355X HBM3E, specification; a float4 copy reaches about 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=3_000_000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--kmers-cap", type=int, default=1 << 26, help="k-mers timed per seq_kmers variant")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import duckhts_amd
    from duckhts_amd import synth
    synth.build()
    arr, st = synth.bam_segment(a.records, seed=42, level=1, threads=min(os.cpu_count() or 1, 16))
    ctx = duckhts_amd.Context(a.device)
    res = {}

    def add(name, ms, nbytes, rows, items=None):
        r = res.setdefault(name, {"kernel_ms": 0.0, "bytes": 0, "rows": 0, "launches": 0})
        r["kernel_ms"] += ms; r["bytes"] += int(nbytes); r["rows"] += int(rows); r["launches"] += 1
        if items is not None:
            r["kmers"] = r.get("kmers", 0) + int(items)

    def timed(call):
        ctx.reset_times()
        out = call()
        ctx.L.dhts_sync(ctx.h)
        t = ctx.kernel_times()
        return out, t["string_write"][0] + t["core_unpack"][0]

    try:
        ctx.open(arr); ctx.bgzf_index(); ctx.bam_open()
        ctx.set_timing(True)
        kmers_done = {"hash": 0, "text": 0}
        while True:
            b = ctx.next_batch()
            n = int(b.n_rows)
            if n:
                L = int(ctx.d2h(b.seq.len, n, np.uint32).sum(dtype=np.uint64))
                Lc = int(ctx.d2h(b.cigar.len, n, np.uint32).sum(dtype=np.uint64))
                for fn, col, nbytes in (("seq_revcomp", b.seq, 2 * L + 17 * n), ("seq_canonical", b.seq, 2 * L + 17 * n), ("seq_gc_content", b.seq, L + 17 * n),
                                        ("cigar_reference_length", b.cigar, Lc + 17 * n)):
                    for rep in range(2):                          # the first call on a batch size allocates the result buffers
                        _, ms = timed(lambda: ctx.udf(fn, col, n_rows=n, fetch=False))
                    add(fn, ms, nbytes, n)
                # bytes written per k-mer: row 8 + pos 8 + validity 1, and the hash's 8 or the text's 31 + a 4-byte offset; read: a 150-base read
                # (once) per 120 k-mers.  The time is the whole call: the per-row counts, their scan over all rows, and the k-mers.
                for kind, text, hsh, per in (("hash", 0, 1, 8 + 8 + 1 + 8), ("text", 1, 0, 8 + 8 + 1 + 31 + 4)):
                    nxt = 0
                    while kmers_done[kind] < a.kmers_cap:
                        kb = duckhts_amd.UdfKmers()
                        arg = ctx._udf_arg(b.seq, 0, 0)
                        _, ms = timed(lambda: ctx._chk(ctx.L.dhts_udf_seq_kmers(ctx.h, arg, n, 31, 0, text, hsh, 0, nxt, kb)))
                        m = int(kb.n_rows)
                        if m == 0:
                            break
                        if nxt:                                   # (the first call of a batch allocates)
                            add("seq_kmers_k31_" + kind, ms, m * per + m * 150 // 120, 0, m)
                            kmers_done[kind] += m
                        nxt = int(kb.next)
                        if kb.status:
                            break
            if b.status != 0:
                break
        # one call on 2,048 host rows: upload, launch, download
        rng = np.random.default_rng(1)
        rows = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 150)) for _ in range(2048)]
        chunk = {}
        for fn in ("seq_revcomp", "seq_gc_content"):
            ctx.udf(fn, ctx.udf_upload(rows, 0))
            t0 = time.perf_counter()
            for _ in range(20):
                ctx.udf(fn, ctx.udf_upload(rows, 0))
            chunk[fn] = (time.perf_counter() - t0) / 20 * 1e3
        blob = np.frombuffer(b"".join(rows), np.uint8).copy()
        host = np.empty_like(blob)
        t0 = time.perf_counter()
        for _ in range(20):
            ctx.L.dhts_memcpy_d2h(ctx.h, host.ctypes.data, ctx.udf_upload(rows, 0).bytes, blob.nbytes)
        chunk["upload_and_copy_back_only"] = (time.perf_counter() - t0) / 20 * 1e3
    finally:
        ctx.close()
    for name, r in res.items():
        s = r["kernel_ms"] / 1e3
        r["gb_per_s"] = r["bytes"] / s / 1e9 if s else 0.0
        r["share_of_hbm_peak"] = r["gb_per_s"] / (HBM_PEAK_TBS * 1e3)
        if r["rows"]:
            r["rows_per_s"] = r["rows"] / s
        if r.get("kmers"):
            r["kmers_per_s"] = r["kmers"] / s
    out = {"tool": "bench_udf", "records": a.records, "file_bytes": int(arr.nbytes), "hbm_peak_tb_per_s": HBM_PEAK_TBS, "bound": "HBM bandwidth (input once + output once)",
           "functions": res, "chunk_of_2048_rows_ms": chunk}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
