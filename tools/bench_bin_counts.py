"""bam_bin_counts on the benchmark's synthetic BAM, resident in HBM.

The file is bench.py's (its generator, seed 42): --unique-records records per segment, --reps segments, compressed bytes uploaded once.
Three legs over the same resident bytes, alternated pass by pass in one process after a warm-up pass of each:
  (a) scan     dhts_bam_next_batch to the end with the string-free column mask, nothing else
  (b) bins     dhts_bam_bins_open (the table is zeroed) + dhts_bam_bins_scan at --bin-width
  (c) fetch    the same scan + dhts_bam_batch_fetch of FLAG / POS / MAPQ / tid into pinned host memory + a numpy bincount of the bins:
               the SQL-first path (read_bam + GROUP BY) reduced to its unavoidable part
One JSON line per leg: records/s (median, min, max over the passes), and for (a) and (b) the device time of the record stage's row passes and
of the bin kernels (HIP events of one extra pass).  Run under `rocprofv3 --kernel-trace --stats -- python tools/bench_bin_counts.py` for the
per-kernel table."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import duckhts_amd  # noqa: E402
from duckhts_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--unique-records", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bin-width", type=int, default=5000)
    ap.add_argument("--max-blocks", type=int, default=24576)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--dedup", default="none")
    a = ap.parse_args()
    data, sizes, hdr_bytes, raw = bench.generate_file(None, synth, 42, a.unique_records, a.reps, min(16, os.cpu_count() or 1), 0)
    ctx = duckhts_amd.Context(0)
    L = ctx.L
    L.dhts_bam_batch_host_bytes.restype = C.c_uint64; L.dhts_bam_batch_host_bytes.argtypes = [C.c_void_p, C.c_uint32]
    L.dhts_host_alloc.restype = C.c_void_p; L.dhts_host_alloc.argtypes = [C.c_uint64]; L.dhts_host_free.argtypes = [C.c_void_p]
    L.dhts_bam_batch_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    mask = duckhts_amd.BINS_COLMASK
    fetch_mask = mask & ~(1 << 7)                                   # FLAG, RNAME (tid), POS, MAPQ
    arena = {"p": None, "cap": 0}
    try:
        ctx.open(data)
        file_bytes = int(data.nbytes)
        data = None
        ctx.bgzf_index()
        hdr = ctx.bam_open()
        base = np.concatenate([[0], np.cumsum([(n + a.bin_width - 1) // a.bin_width for n in hdr["ref_len"]])]).astype(np.int64)

        def scan():
            ctx.rewind()
            rows = 0
            while True:
                b = ctx.next_batch(a.max_blocks, mask)
                rows += b.n_rows
                if b.status != 0:
                    assert b.status == 1
                    return rows

        def bins():
            ctx.rewind()
            ctx.bam_bins_open(bin_width=a.bin_width, dedup=a.dedup)
            assert ctx.bam_bins_scan(a.max_blocks) == 1
            L.dhts_sync(ctx.h)
            return None

        def fetch():
            ctx.rewind()
            rows = 0
            table = np.zeros(2 * int(base[-1]), np.int64)
            hb = duckhts_amd.BamBatch()
            while True:
                b = ctx.next_batch(a.max_blocks, mask)
                n = int(b.n_rows)
                if n:
                    need = int(L.dhts_bam_batch_host_bytes(C.byref(b), fetch_mask))
                    if need > arena["cap"]:
                        if arena["p"]:
                            L.dhts_host_free(arena["p"])
                        arena["p"], arena["cap"] = L.dhts_host_alloc(need + need // 4), need + need // 4
                    ctx._chk(L.dhts_bam_batch_fetch(ctx.h, C.byref(b), fetch_mask, arena["p"], arena["cap"], C.byref(hb)))
                    flag = np.ctypeslib.as_array(C.cast(hb.flag, C.POINTER(C.c_uint16)), (n,))
                    pos = np.ctypeslib.as_array(C.cast(hb.pos, C.POINTER(C.c_int64)), (n,))
                    tid = np.ctypeslib.as_array(C.cast(hb.tid, C.POINTER(C.c_int32)), (n,))
                    ok = (tid >= 0) & (pos >= 1)
                    word = 2 * (base[tid[ok]] + (pos[ok] - 1) // a.bin_width) + ((flag[ok] >> 4) & 1)
                    table += np.bincount(word, minlength=table.size)
                    rows += n
                if b.status != 0:
                    return rows, table

        legs = [("scan", scan), ("bins", bins), ("fetch", fetch)]
        n_records = scan()
        bins()
        st = ctx.bam_bins_stats()
        _, host_table = fetch()
        assert st["n_rows"] == n_records and int(host_table.sum()) == st["n_counted"], (st, n_records, int(host_table.sum()))
        print(json.dumps({"records": n_records, "file_bytes": file_bytes, "bin_width": a.bin_width, "total_bins": st["total_bins"], "stats": st, "dedup": a.dedup,
                          "host_table_equals_n_counted": True, "resident": "compressed BAM in HBM", "max_blocks": a.max_blocks}), flush=True)
        times = {k: [] for k, _ in legs}
        for _ in range(a.passes):
            for k, fn in legs:
                L.dhts_sync(ctx.h)
                t0 = time.perf_counter()
                fn()
                L.dhts_sync(ctx.h)
                times[k].append(time.perf_counter() - t0)
        dev = {}
        for k, fn in legs[:2]:
            ctx.set_timing(True); ctx.reset_times()
            fn()
            L.dhts_sync(ctx.h)
            kt = ctx.kernel_times(); ctx.set_timing(False)
            dev[k] = {"row_passes_ms (core_unpack)": round(kt["core_unpack"][0], 3), "bin_kernels_ms (bcf_check)": round(kt["bcf_check"][0], 3), "bin_kernel_batches": kt["bcf_check"][1]}
        for k, _ in legs:
            ts = sorted(times[k])
            med = ts[len(ts) // 2]
            print(json.dumps({"leg": k, "passes": len(ts), "median_s": round(med, 4), "min_s": round(ts[0], 4), "max_s": round(ts[-1], 4), "records_per_s_median": round(n_records / med),
                              "records_per_s_min_max": [round(n_records / ts[-1]), round(n_records / ts[0])], **({"device_time_one_pass": dev[k]} if k in dev else {})}), flush=True)
    finally:
        if arena["p"]:
            L.dhts_host_free(arena["p"])
        ctx.close()


if __name__ == "__main__":
    main()
