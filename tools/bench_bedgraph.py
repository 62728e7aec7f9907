"""bam_bedgraph against bam_depth on the benchmark's synthetic BAM, resident in HBM.

The file is bench.py's (its generator, seed 42; the 25-contig header, so the depth table has 12.4 GB).  One context, the compressed bytes
uploaded once.  Legs over the same resident bytes, alternated pass by pass in one process after a warm-up pass of each:
  depth            dhts_bam_depth_open (mode 0) + _scan, the count (the first dhts_bam_depth_next, asked for one row with an empty column mask,
                   so that nothing is emitted), then the whole result page by page into one reused pinned buffer
  bedgraph         the same with dhts_bam_bedgraph_*: zero_runs 0 without breaks; zero_runs 1; breaks 1,5,15
Per leg: the device time of the count passes (the project's kernel timer DHTS_K_SCAN around them: HIP events on the stream), the host clock
around the count call and around the read-out, result rows, pages and the bytes fetched.  Medians of --passes passes.  Before the clock the
run checks that the runs of bam_bedgraph cover exactly bam_depth's positions with the same summed depth.  One JSON line per leg."""
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
import bench  # noqa: E402
import duckhts_amd  # noqa: E402
from bench_coverage import EXCLUDE  # noqa: E402
from duckhts_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--unique-records", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--max-blocks", type=int, default=24576)
    ap.add_argument("--max-rows", type=int, default=0, help="rows per page (0: the ABI's default)")
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    data, sizes, hdr_bytes, raw = bench.generate_file(None, synth, 42, a.unique_records, a.reps, min(16, os.cpu_count() or 1), 0)
    ctx = duckhts_amd.Context(0)
    L = ctx.L
    L.dhts_host_alloc.restype = C.c_void_p; L.dhts_host_alloc.argtypes = [C.c_uint64]; L.dhts_host_free.argtypes = [C.c_void_p]
    arena = {"p": None, "cap": 0}

    def reserve(need):
        if need > arena["cap"]:
            if arena["p"]:
                L.dhts_host_free(arena["p"])
            arena["p"], arena["cap"] = L.dhts_host_alloc(need + need // 4), need + need // 4

    legs = [("depth", "depth", duckhts_amd.DEPTH_DTYPES, dict(all_positions=0)),
            ("bedgraph", "bedgraph", duckhts_amd.BEDGRAPH_DTYPES, dict()),
            ("bedgraph_zero_runs", "bedgraph", duckhts_amd.BEDGRAPH_DTYPES, dict(zero_runs=1)),
            ("bedgraph_breaks_1_5_15", "bedgraph", duckhts_amd.BEDGRAPH_DTYPES, dict(breaks=[1, 5, 15]))]
    parts = {}

    def leg(key, fn, dtypes, kw, sink=None):
        """one pass; sink(columns): called with views of every page in the pinned buffer"""
        p = parts.setdefault(key, {"count_device_ms": [], "count_s": [], "readout_s": [], "open_scan_s": [], "rows": 0, "bytes": 0, "pages": 0})
        nxt, fetch, need_of = (getattr(L, "dhts_bam_%s_%s" % (fn, w)) for w in ("next", "batch_fetch", "batch_host_bytes"))
        ncol, full = len(dtypes), (1 << len(dtypes)) - 1
        ctx.rewind()
        t0 = time.perf_counter()
        getattr(ctx, "bam_%s_open" % fn)(exclude_flags=EXCLUDE, **kw)
        assert getattr(ctx, "bam_%s_scan" % fn)(a.max_blocks) == 1
        L.dhts_sync(ctx.h)
        t1 = time.perf_counter()
        b, host = duckhts_amd.BedBatch(), (duckhts_amd.BcfCol * ncol)()
        ctx.set_timing(True); ctx.reset_times()
        ctx._chk(nxt(ctx.h, 1, 0, C.byref(b)))                             # the count passes alone: no column, nothing emitted
        L.dhts_sync(ctx.h)
        t2 = time.perf_counter()
        dev_ms = ctx.kernel_times()["scan"][0]
        ctx.set_timing(False)
        rows, nbytes, pages, st = int(b.n_rows), 0, 0, int(b.status)        # (the one row of the count call is not fetched: it has no column)
        while st == 0:
            ctx._chk(nxt(ctx.h, a.max_rows, full, C.byref(b)))
            st, n = int(b.status), int(b.n_rows)
            need = int(need_of(C.byref(b)))
            reserve(need)
            ctx._chk(fetch(ctx.h, C.byref(b), arena["p"], arena["cap"], host))
            rows += n; nbytes += need; pages += 1
            if sink and n:
                sink([np.ctypeslib.as_array(C.cast(host[i].fixed, C.POINTER(C.c_uint8)), (n * np.dtype(dt).itemsize,)).view(dt) for i, dt in enumerate(dtypes)])
        t3 = time.perf_counter()
        p["open_scan_s"].append(t1 - t0); p["count_s"].append(t2 - t1); p["count_device_ms"].append(dev_ms); p["readout_s"].append(t3 - t2)
        p["rows"], p["bytes"], p["pages"] = rows, nbytes, pages
        return rows

    try:
        file_bytes = int(data.nbytes)
        ctx.open(data)
        ctx.bgzf_index()
        data = None
        hdr = ctx.bam_open()
        # ---- agreement, once: the runs cover bam_depth's positions, with the same summed depth (the first row went with the count call) ----
        seen = {"depth": [0, 0], "bedgraph": [0, 0]}

        def sink_depth(cols):
            seen["depth"][0] += len(cols[1]); seen["depth"][1] += int(cols[2].astype(np.int64).sum())

        def sink_runs(cols):
            n = cols[2] - cols[1]
            seen["bedgraph"][0] += int(n.sum()); seen["bedgraph"][1] += int((n * cols[3]).sum())

        leg("check_depth", "depth", duckhts_amd.DEPTH_DTYPES, dict(all_positions=0), sink=sink_depth)
        st_depth = ctx.bam_depth_stats()
        leg("check_bedgraph", "bedgraph", duckhts_amd.BEDGRAPH_DTYPES, dict(), sink=sink_runs)
        st = ctx.bam_bedgraph_stats()
        # the first row of each result left with the count call: one position of depth d, and the first run, n positions of that depth --
        # so the runs seen cover n - 1 positions fewer than the positions seen, and d (n - 1) less summed depth
        dpos, dsum = seen["depth"][0] - seen["bedgraph"][0], seen["depth"][1] - seen["bedgraph"][1]
        agree = {"positions": st_depth["n_positions"], "runs": st["n_runs"], "table_bytes": st["table_bytes"], "positions_seen": seen["depth"][0], "positions_in_the_runs_seen": seen["bedgraph"][0],
                 "summed_depth_seen": seen["depth"][1], "summed_depth_of_the_runs_seen": seen["bedgraph"][1]}
        print(json.dumps({"records": st["n_rows"], "counted": st["n_counted"], "file_bytes": file_bytes, "contigs": len(hdr["ref_len"]), "agreement": agree,
                          "resident": "compressed BAM in HBM", "max_blocks": a.max_blocks, "max_rows": a.max_rows or (1 << 20)}), flush=True)
        assert st_depth["table_bytes"] == st["table_bytes"] and seen["depth"][0] == st_depth["n_positions"] - 1 and parts["check_bedgraph"]["rows"] == st["n_runs"]
        assert dpos >= 0 and (dsum == 0 if dpos == 0 else dsum > 0 and dsum % dpos == 0), agree
        parts.clear()
        for k, fn, dt, kw in legs:                                          # warm-up
            leg(k, fn, dt, kw)
        parts.clear()
        for _ in range(a.passes):
            for k, fn, dt, kw in legs:
                leg(k, fn, dt, kw)
        med = lambda v: sorted(v)[len(v) // 2]
        base = med(parts["depth"]["count_device_ms"])
        for k, _, _, _ in legs:
            p = parts[k]
            ro = med(p["readout_s"])
            print(json.dumps({"leg": k, "passes": a.passes, "count_passes_device_ms_median": round(med(p["count_device_ms"]), 3), "count_passes_device_ms_all": [round(x, 3) for x in p["count_device_ms"]],
                              "count_against_bam_depth": round(med(p["count_device_ms"]) / base, 3), "count_call_s_median": round(med(p["count_s"]), 5),
                              "open_scan_s_median": round(med(p["open_scan_s"]), 4), "readout_s_median": round(ro, 4), "readout_s_all": [round(x, 4) for x in p["readout_s"]],
                              "result_rows": p["rows"], "pages": p["pages"], "fetched_bytes": p["bytes"], "readout_bytes_per_s": round(p["bytes"] / ro) if ro else None}), flush=True)
    finally:
        if arena["p"]:
            L.dhts_host_free(arena["p"])
        ctx.close()


if __name__ == "__main__":
    main()
