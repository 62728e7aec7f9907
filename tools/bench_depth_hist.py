"""bam_depth_hist against bam_coverage's table pass and bam_bedgraph on the benchmark's synthetic BAM, resident in HBM.

The file is bench.py's (its generator, seed 42; the 25-contig header, so the depth table has 12.4 GB).  One context, the compressed bytes
uploaded once.  Legs over the same resident bytes, alternated pass by pass in one process after a warm-up pass of each:
  hist, hist_contig   dhts_bam_hist_open (depth_cap 1000; per 'row' = one group per contig here, and per 'contig') + _scan; on the filled table the
                      histogram pass alone (dhi_hist) and bam_coverage's dep_tile_reduce alone, each between two HIP events
                      (dhts_debug_hist_pass_ms); then the result (the first dhts_bam_hist_next, asked for one row with an empty column mask: the
                      tile sums, their carry, the histogram pass, the group count and its carry), then the whole result page by page into one
                      reused pinned buffer
  bedgraph_zero_runs  the same with dhts_bam_bedgraph_* and zero_runs 1, the cheapest older route to the same answer (the host would still have
                      to group its rows): its count passes and its read-out
Per leg: the device time of the result's passes (the project's kernel timer DHTS_K_SCAN around them: HIP events on the stream), the host clock
around the result call and around the read-out, result rows, pages and the bytes fetched.  Medians of --passes passes.  Before the clock the
run checks that the histogram's positions per contig are the summed run lengths of bam_bedgraph per contig and depth.  One JSON line per leg."""
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

CAP = 1000


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

    # (key, the C entries' name, the Context methods' name, the columns' types, the parameters)
    legs = [("hist", "hist", "depth_hist", duckhts_amd.DEPTH_HIST_DTYPES, dict(depth_cap=CAP, per="row")),
            ("hist_contig", "hist", "depth_hist", duckhts_amd.DEPTH_HIST_DTYPES, dict(depth_cap=CAP, per="contig")),
            ("bedgraph_zero_runs", "bedgraph", "bedgraph", duckhts_amd.BEDGRAPH_DTYPES, dict(zero_runs=1))]
    parts = {}

    def leg(key, cfn, pfn, dtypes, kw, sink=None):
        """one pass; sink(columns): called with views of every page in the pinned buffer"""
        p = parts.setdefault(key, {"count_device_ms": [], "count_s": [], "readout_s": [], "open_scan_s": [], "hist_pass_ms": [], "tile_reduce_ms": [], "rows": 0, "bytes": 0, "pages": 0})
        nxt, fetch, need_of = (getattr(L, "dhts_bam_%s_%s" % (cfn, w)) for w in ("next", "batch_fetch", "batch_host_bytes"))
        ncol, full = len(dtypes), (1 << len(dtypes)) - 1
        ctx.rewind()
        t0 = time.perf_counter()
        getattr(ctx, "bam_%s_open" % pfn)(exclude_flags=EXCLUDE, **kw)
        assert getattr(ctx, "bam_%s_scan" % pfn)(a.max_blocks) == 1
        L.dhts_sync(ctx.h)
        t1 = t_scanned = time.perf_counter()
        if cfn == "hist":                                                  # the two table passes alone, on the table this leg filled
            for which, name in ((0, "tile_reduce_ms"), (1, "hist_pass_ms")):
                ms = L.dhts_debug_hist_pass_ms(ctx.h, which, 1)
                assert ms >= 0, L.dhts_error(ctx.h)
                p[name].append(ms)
            L.dhts_sync(ctx.h)
            t1 = time.perf_counter()
        b, host = duckhts_amd.BedBatch(), (duckhts_amd.BcfCol * ncol)()
        ctx.set_timing(True); ctx.reset_times()
        ctx._chk(nxt(ctx.h, 1, 0, C.byref(b)))                             # the result's passes alone: no column, nothing emitted
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
                sink([np.ctypeslib.as_array(C.cast(host[i].fixed, C.POINTER(C.c_uint8)), (n * np.dtype(dt).itemsize,)).view(dt).copy() for i, dt in enumerate(dtypes)])
        t3 = time.perf_counter()
        p["open_scan_s"].append(t_scanned - t0); p["count_s"].append(t2 - t1); p["count_device_ms"].append(dev_ms); p["readout_s"].append(t3 - t2)
        p["rows"], p["bytes"], p["pages"] = rows, nbytes, pages
        return rows

    try:
        file_bytes = int(data.nbytes)
        ctx.open(data)
        ctx.bgzf_index()
        data = None
        hdr = ctx.bam_open()
        n_ref = len(hdr["ref_len"])
        # ---- agreement, once: per contig and min(depth, CAP), the histogram's positions are the summed lengths of bam_bedgraph's runs.  The first
        # row of each result left with the count call, so the two are compared from the second row on, and the first by what is missing ----
        seen_hist, seen_runs = np.zeros((n_ref, CAP + 1), np.int64), np.zeros((n_ref, CAP + 1), np.int64)

        def sink_hist(cols):
            np.add.at(seen_hist, (cols[0], cols[3]), cols[4])

        def sink_runs(cols):
            np.add.at(seen_runs, (cols[0], np.minimum(cols[3], CAP)), cols[2] - cols[1])

        leg("check_hist", "hist", "depth_hist", duckhts_amd.DEPTH_HIST_DTYPES, dict(depth_cap=CAP, per="row"), sink=sink_hist)
        st = ctx.bam_depth_hist_stats()
        leg("check_bedgraph", "bedgraph", "bedgraph", duckhts_amd.BEDGRAPH_DTYPES, dict(zero_runs=1), sink=sink_runs)
        st_runs = ctx.bam_bedgraph_stats()
        diff = seen_runs - seen_hist                                        # the histogram's first row (one bin of contig 0) minus the first run's length
        lens = np.asarray(hdr["ref_len"], np.int64)
        agree = {"result_rows": st["n_result_rows"], "runs": st_runs["n_runs"], "table_bytes": st["table_bytes"], "hist_bytes": st["hist_bytes"], "groups": st["n_groups"],
                 "positions_in_the_bins_seen": int(seen_hist.sum()), "positions_in_the_runs_seen": int(seen_runs.sum()), "positions": int(lens.sum()),
                 "bins_that_differ": int(np.count_nonzero(diff))}
        print(json.dumps({"records": st["n_rows"], "counted": st["n_counted"], "file_bytes": file_bytes, "contigs": n_ref, "agreement": agree,
                          "resident": "compressed BAM in HBM", "max_blocks": a.max_blocks, "max_rows": a.max_rows or (1 << 20), "depth_cap": CAP}), flush=True)
        assert st["table_bytes"] == st_runs["table_bytes"] and parts["check_hist"]["rows"] == st["n_result_rows"] and parts["check_bedgraph"]["rows"] == st_runs["n_runs"]
        assert np.count_nonzero(diff[1:]) == 0 and np.count_nonzero(diff[0]) <= 1 and np.array_equal(seen_runs[1:].sum(axis=1), lens[1:]), agree
        parts.clear()
        for k, cfn, pfn, dt, kw in legs:                                    # warm-up
            leg(k, cfn, pfn, dt, kw)
        parts.clear()
        for _ in range(a.passes):
            for k, cfn, pfn, dt, kw in legs:
                leg(k, cfn, pfn, dt, kw)
        med = lambda v: sorted(v)[len(v) // 2]
        for k, _, _, _, _ in legs:
            p = parts[k]
            ro = med(p["readout_s"])
            line = {"leg": k, "passes": a.passes, "result_passes_device_ms_median": round(med(p["count_device_ms"]), 3), "result_passes_device_ms_all": [round(x, 3) for x in p["count_device_ms"]],
                    "result_call_s_median": round(med(p["count_s"]), 5), "open_scan_s_median": round(med(p["open_scan_s"]), 4), "readout_s_median": round(ro, 5),
                    "readout_s_all": [round(x, 5) for x in p["readout_s"]], "result_and_readout_s_median": round(med([x + y for x, y in zip(p["count_s"], p["readout_s"])]), 5),
                    "result_rows": p["rows"], "pages": p["pages"], "fetched_bytes": p["bytes"]}
            if p["hist_pass_ms"]:
                h, r = med(p["hist_pass_ms"]), med(p["tile_reduce_ms"])
                line.update({"hist_pass_device_ms_median": round(h, 3), "hist_pass_device_ms_all": [round(x, 3) for x in p["hist_pass_ms"]], "tile_reduce_device_ms_median": round(r, 3),
                             "tile_reduce_device_ms_all": [round(x, 3) for x in p["tile_reduce_ms"]], "hist_pass_against_tile_reduce": round(h / r, 3)})
            print(json.dumps(line), flush=True)
    finally:
        if arena["p"]:
            L.dhts_host_free(arena["p"])
        ctx.close()


if __name__ == "__main__":
    main()
