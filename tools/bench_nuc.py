"""fasta_nuc on the synthetic FASTA of DESIGN.md §4d, resident in HBM.

The text is tools/bench_fasta.py's: one sequence of --mbp million bases and --more of --mbp2 million, 60 bases a line, uploaded once; the
.fai is built on the device.  Two questions: bin_width := 1000 over everything, and one interval over the whole first sequence.  For each:
WALL time of the batches with the columns left in HBM (all kernels and host round trips of a warm pass), and the device time of the
nuc_count launches (HIP events).  Run under `rocprofv3 --kernel-trace --stats -- python tools/bench_nuc.py` for the per-kernel table.
The comparison is what there was before for the same question: dhts_fasta_fetch of the same intervals plus the read-back of the bases
(--fetch; the counting a caller would then do on the host is timed separately and labelled host work).  One JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import duckhts_amd  # noqa: E402
from bench_fasta import lines60  # noqa: E402

HBM_PEAK = 8.0e12
COUNT_COLS = ["start", "end", "num_a", "num_c", "num_g", "num_t", "num_n", "num_other", "seq_len", "pct_gc"]


def timed(ctx, fn, reps=4):
    ts = []
    for _ in range(reps):
        ctx.L.dhts_sync(ctx.h)
        t0 = time.perf_counter()
        rows = fn()
        ctx.L.dhts_sync(ctx.h)
        ts.append(time.perf_counter() - t0)
    return rows, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=int, default=250)
    ap.add_argument("--more", type=int, default=30)
    ap.add_argument("--mbp2", type=int, default=60)
    ap.add_argument("--bin-width", type=int, default=1000)
    ap.add_argument("--fetch", action="store_true", help="also time dhts_fasta_fetch + read-back of the same intervals, and a host count")
    a = ap.parse_args()
    seq = np.random.default_rng(1).choice(np.frombuffer(b"ACGT", np.uint8), a.mbp * 1000000)
    big, small = lines60(seq), lines60(seq[:a.mbp2 * 1000000])
    text = b">chr1\n" + big + b"".join(b">chr%d\n" % (k + 2) + small for k in range(a.more))
    bases = a.mbp * 1000000 + a.more * a.mbp2 * 1000000
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(np.frombuffer(text, np.uint8))
        ctx.bgzf_index()
        fai, _ = ctx.fasta_build_index()
        ctx.fasta_load_index(fai)
        ctx.nuc_open(False)
        ctx.nuc_set_projection(COUNT_COLS)
        print(json.dumps({"text_bytes": len(text), "bases": bases, "sequences": a.more + 1, "resident": "uncompressed text in HBM"}), flush=True)

        def bins():
            ctx._chk(ctx.L.dhts_nuc_set_region(ctx.h, None))              # a new scan
            rows = 0
            while True:
                b = ctx.nuc_next_bins(a.bin_width, 0)
                rows += b.n_rows
                if b.status != 0:
                    return rows

        one_t, one_s, one_e = np.zeros(1, np.int32), np.zeros(1, np.int64), np.array([a.mbp * 1000000], np.int64)

        def whole():
            b = duckhts_amd.BedBatch()
            ctx._chk(ctx.L.dhts_nuc_intervals(ctx.h, one_t.ctypes.data, one_s.ctypes.data, one_e.ctypes.data, 1, C.byref(b)))
            return b.n_rows

        for label, fn, nb, nt in (("bin_width := %d over every sequence" % a.bin_width, bins, bases, len(text)), ("one interval over chr1", whole, a.mbp * 1000000, len(big))):
            rows, ts = timed(ctx, fn)
            warm = sorted(ts[1:])[len(ts[1:]) // 2]
            print(json.dumps({"what": "all batches, host clock, median of %d warm passes, columns left in HBM" % len(ts[1:]), "case": label, "rows": rows, "first_s": round(ts[0], 4), "warm_s": round(warm, 5),
                              "spread_s": [round(min(ts[1:]), 5), round(max(ts[1:]), 5)], "text_GBps": round(nt / warm / 1e9, 1), "of_hbm_peak": round(nt / warm / HBM_PEAK, 4)}), flush=True)
            ctx.set_timing(True); ctx.reset_times()
            fn()
            ctx.L.dhts_sync(ctx.h)                                        # collects the events
            ms, n = ctx.kernel_times()["core_unpack"]; ctx.set_timing(False)
            assert n > 0 and ms > 0, "no nuc_count launch was timed"
            print(json.dumps({"what": "device time, HIP events, one pass", "case": label, "kernels": "nuc_count", "launches": n, "ms": round(ms, 4), "bases": nb, "text_bytes_read": nt,
                              "text_GBps": round(nt / ms / 1e6, 1), "of_hbm_peak": round(nt / (ms * 1e-3) / HBM_PEAK, 4)}), flush=True)
        if a.fetch:
            b, hb = duckhts_amd.FastaBatch(), duckhts_amd.FastaBatch()
            ts, arena = [], None
            for _ in range(3):
                t0 = time.perf_counter()
                ctx._chk(ctx.L.dhts_fasta_fetch(ctx.h, b"chr1", b))
                t1 = time.perf_counter()
                need = int(ctx.L.dhts_fasta_batch_host_bytes(C.byref(b)))
                if arena is None:
                    arena = np.zeros(need, np.uint8)
                ctx._chk(ctx.L.dhts_fasta_batch_fetch(ctx.h, C.byref(b), arena.ctypes.data, need, C.byref(hb)))
                ts.append((t1 - t0, time.perf_counter() - t1))
            base = arena.ctypes.data
            got = arena[hb.seq_bytes - base: hb.seq_bytes - base + hb.seq_nbytes]
            t0 = time.perf_counter()
            cnt = np.bincount(got, minlength=256)
            host_s = time.perf_counter() - t0
            print(json.dumps({"what": "before fasta_nuc: dhts_fasta_fetch of chr1 + read-back to pageable host memory, host clock, last of 3", "fetch_s": round(ts[-1][0], 4), "readback_s": round(ts[-1][1], 4),
                              "bases": int(hb.seq_nbytes), "HOST WORK on top (numpy bincount of the bases, one thread)": round(host_s, 4), "A": int(cnt[65])}), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
