#!/usr/bin/env python3
"""read_gff on a resident synthetic GFF3 text of about 1 GB (a seeded piece repeated; nine fields, a numeric score on part of the lines,
attribute strings of 60 to 300 bytes): device time per kernel family (HIP events) and the whole scan (host clock around scans that end in a
synchronise, median of three warm scans), as GB/s of text and as a fraction of the HBM peak (8 TB/s), for count only, seqname / start / end,
all nine columns, and all nine plus attributes_map.  Also the share of score tokens the device handed to the host's strtod.  Columns stay
in HBM (no read-back).  One JSON line per measurement.

    python tools/bench_tabix.py [gigabytes]
"""
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import duckhts_amd  # noqa: E402

HBM_PEAK = 8.0e12
N_LINES = 16384
FAMILIES = {"tiles": "delimiter table (bed_delim_count, scan, bed_delim_fill)", "core_unpack": "tabix_classify", "scan": "row, offset and pair scans",
            "bcf_check": "tabix_fixed", "bcf_measure": "tabix_str_measure", "bcf_write": "tabix_str_gather", "string_write": "tabix_attr<measure>, tabix_attr<write>"}
CASES = (("no column (count)", []), ("seqname,start,end", [0, 3, 4]), ("all nine columns", list(range(9))), ("all nine + attributes_map", list(range(10))))


def body(n_lines, seed=11):
    rnd = random.Random(seed)
    out, pos = [], 0
    notes = ["".join(rnd.choice("abcdefghijklmnopqrstuvwxyz ") for _ in range(rnd.randrange(1, 216))).strip() or "n" for _ in range(64)]
    for i in range(n_lines):
        pos += rnd.randrange(1, 400)
        ln = rnd.randrange(50, 5000)
        feat = ("gene", "transcript", "exon", "CDS", "intron")[rnd.randrange(5)]
        score = "." if rnd.random() < 0.6 else ("%.*f" % (rnd.randrange(0, 4), rnd.random() * 1000)) if rnd.random() < 0.9 else "%.3e" % (rnd.random() * 1e-30)
        attrs = "ID=%s:%d;Parent=gene%06d;Name=%s_%d;biotype=protein_coding;Note=%s" % (feat, i, i // 9, feat, rnd.randrange(100000), notes[rnd.randrange(64)])
        out.append("chr%d\tsynth\t%s\t%d\t%d\t%s\t%s\t%s\t%s\n" % (1 + i * 22 // n_lines, feat, pos, pos + ln, score, "+-"[i & 1], ".012"[rnd.randrange(4)], attrs))
    return "".join(out).encode()


def scan(ctx, sc, reps=4):
    times, rows = [], 0
    for _ in range(reps):
        sc.set_region(None)                                   # rewinds the scan
        sc.n_double_fast = sc.n_double_patched = 0
        ctx.L.dhts_sync(ctx.h)
        t0 = time.perf_counter()
        rows = 0
        while True:
            b = sc.next_batch(0)
            rows += b.n_rows
            if b.status != 0:
                assert b.status == 1, b.status
                break
        ctx.L.dhts_sync(ctx.h)
        times.append(time.perf_counter() - t0)
    return rows, times


def main():
    gb = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    piece = body(N_LINES)
    attr_len = [len(ln.split(b"\t")[8]) for ln in piece.split(b"\n") if ln]
    reps = max(1, int(gb * 1e9 / len(piece)))
    nbytes = len(piece) * reps
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open_tiled(b"", piece, reps, b"")
        ctx.L.dhts_bgzf_index(ctx.h)
        sc = duckhts_amd.TabixScan(ctx, duckhts_amd.TABIX_GFF)
        print(json.dumps({"text_bytes": nbytes, "lines": N_LINES * reps, "bytes_per_line": round(len(piece) / N_LINES, 1), "attribute_bytes": [min(attr_len), max(attr_len)],
                          "resident": "uncompressed text in HBM"}), flush=True)
        for label, cols in CASES:
            sc.set_projection(cols)
            rows, times = scan(ctx, sc)                       # warm-up included: the first scan allocates
            warm = sorted(times[1:])[len(times[1:]) // 2]
            print(json.dumps({"what": "whole scan, host clock, median of %d warm scans" % len(times[1:]), "columns": label, "rows": rows, "first_s": round(times[0], 4), "warm_s": round(warm, 4),
                              "spread_s": [round(min(times[1:]), 4), round(max(times[1:]), 4)], "text_GBps": round(nbytes / warm / 1e9, 1), "of_hbm_peak": round(nbytes / warm / HBM_PEAK, 4)}), flush=True)
            if 5 in cols:
                tot = sc.n_double_fast + sc.n_double_patched
                print(json.dumps({"what": "score tokens of one scan", "columns": label, "converted_on_device": sc.n_double_fast, "patched_by_host_strtod": sc.n_double_patched,
                                  "host_share": round(sc.n_double_patched / max(tot, 1), 4)}), flush=True)
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
            print(json.dumps({"what": "device time, HIP events, one scan", "columns": label, "kernels": "all read_gff kernels", "ms": round(total, 3),
                              "text_GBps": round(nbytes / total / 1e6, 1), "of_hbm_peak": round(nbytes / (total * 1e-3) / HBM_PEAK, 4)}), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
