#!/usr/bin/env python3
"""read_bed on a resident synthetic BED12 text of about 1 GB: device time per kernel family (HIP events) and the whole scan (host clock
around scans that end in a synchronise), as GB/s of text and as a fraction of the HBM peak (8 TB/s), for all 13 columns and for
chrom, start, end alone; beside the three-column numbers the lane-per-line walk of the overlap join (vcf_line_* + bed_intervals) over
the same text.  Columns stay in HBM (no read-back).  One JSON line per measurement.

    python tools/bench_bed.py [gigabytes]
"""
import ctypes as C
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import duckhts_amd  # noqa: E402

HBM_PEAK = 8.0e12
FAMILIES = {"tiles": "delimiter table (bed_delim_count, scan, bed_delim_fill)", "core_unpack": "bed_classify", "scan": "row and offset scans",
            "bcf_check": "bed_ints", "bcf_measure": "bed_str_measure", "bcf_write": "bed_str_gather"}


def body(n_lines, seed=7):
    rnd = random.Random(seed)
    out = []
    pos = 0
    for i in range(n_lines):
        pos += rnd.randrange(1, 400)
        ln = rnd.randrange(50, 5000)
        nb = rnd.randrange(1, 6)
        out.append("chr%d\t%d\t%d\tfeature_%d\t%d\t%s\t%d\t%d\t%d,%d,%d\t%d\t%s\t%s\n" % (
            1 + i * 22 // n_lines, pos, pos + ln, i, rnd.randrange(1000), "+-"[i & 1], pos + 10, pos + ln - 10, rnd.randrange(256), rnd.randrange(256), rnd.randrange(256),
            nb, ",".join(str(ln // nb) for _ in range(nb)), ",".join(str(k * (ln // nb)) for k in range(nb))))
    return "".join(out).encode()


def scan(ctx, sc, reps=4):
    times = []
    rows = 0
    for _ in range(reps):
        sc.set_region(None)                                   # rewinds the scan
        ctx.L.dhts_sync(ctx.h)
        t0 = time.perf_counter()
        rows = 0
        while True:
            b = sc.next_batch(0)
            rows += b.n_rows
            if b.status != 0:
                assert b.status == 1, (b.status, sc.error)
                break
        ctx.L.dhts_sync(ctx.h)
        times.append(time.perf_counter() - t0)
    return rows, times


def main():
    gb = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    piece = body(16384)
    reps = max(1, int(gb * 1e9 / len(piece)))
    nbytes = len(piece) * reps
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open_tiled(b"", piece, reps, b"")
        ctx.L.dhts_bgzf_index(ctx.h)
        sc = duckhts_amd.BedScan(ctx)
        print(json.dumps({"text_bytes": nbytes, "lines": 16384 * reps, "bytes_per_line": round(len(piece) / 16384, 1), "resident": "uncompressed text in HBM"}), flush=True)
        for label, cols in (("all 13 columns", None), ("chrom,start,end", ["chrom", "start", "end"]), ("no column (count)", [])):
            sc.set_projection(list(range(13)) if cols is None else cols)
            rows, times = scan(ctx, sc)                       # warm-up included: the first scan allocates
            warm = sorted(times[1:])[len(times[1:]) // 2]
            print(json.dumps({"what": "whole scan, host clock, median of %d warm scans" % len(times[1:]), "columns": label, "rows": rows, "first_s": round(times[0], 4), "warm_s": round(warm, 4),
                              "spread_s": [round(min(times[1:]), 4), round(max(times[1:]), 4)], "text_GBps": round(nbytes / warm / 1e9, 1), "of_hbm_peak": round(nbytes / warm / HBM_PEAK, 4)}), flush=True)
            ctx.set_timing(True); ctx.reset_times()
            scan(ctx, sc, reps=1)
            kt = ctx.kernel_times(); ctx.set_timing(False)
            total = 0.0
            for fam, name in FAMILIES.items():
                ms, n = kt[fam]
                if n:
                    total += ms
                    print(json.dumps({"what": "device time, HIP events, one scan", "columns": label, "kernels": name, "launches": n, "ms": round(ms, 3),
                                      "text_GBps": round(nbytes / ms / 1e6, 1), "of_hbm_peak": round(nbytes / (ms * 1e-3) / HBM_PEAK, 4)}), flush=True)
            print(json.dumps({"what": "device time, HIP events, one scan", "columns": label, "kernels": "all read_bed kernels", "ms": round(total, 3),
                              "text_GBps": round(nbytes / total / 1e6, 1), "of_hbm_peak": round(nbytes / (total * 1e-3) / HBM_PEAK, 4)}), flush=True)
        f = ctx.L.dhts_debug_bed_walk
        f.restype = C.c_int64
        f.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        for rep in range(3):
            a, b = C.c_double(0), C.c_double(0)
            n = f(ctx.h, C.byref(a), C.byref(b))
            assert n > 0, ctx.L.dhts_error(ctx.h)
            if rep:
                print(json.dumps({"what": "device time, HIP events: the lane-per-line walk of the overlap join over the same text (chrom span, start, end per line; no row scan, no bytes gathered)",
                                  "lines": n, "line_table_ms": round(a.value, 3), "bed_intervals_ms": round(b.value, 3), "ms": round(a.value + b.value, 3),
                                  "text_GBps": round(nbytes / (a.value + b.value) / 1e6, 1), "of_hbm_peak": round(nbytes / ((a.value + b.value) * 1e-3) / HBM_PEAK, 4)}), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
