"""bam_coverage on the benchmark's synthetic BAM, resident in HBM.

The file is bench.py's (its generator, seed 42): --unique-records records per segment, --reps segments, compressed bytes uploaded once.
The target rows are the whole contigs of the header.  Three legs over the same resident bytes, alternated pass by pass in one process
after a warm-up pass of each, once per --min-baseq value (0: no quality decides anything; 20: runs are cut by the qualities):
  (a) scan      dhts_bam_next_batch to the end with the string-free column mask, nothing else
  (b) coverage  dhts_bam_coverage_open (the rows, the zeroed depth table) + dhts_bam_coverage_scan + the whole result read back
                (dhts_bam_coverage_next / _batch_fetch); the three parts are also timed one by one
  (c) fetch     the scan with dhts_bam_batch_fetch of FLAG / POS / MAPQ / tid / CIGAR / QUAL into pinned host memory + a numpy version of
                the model (CIGAR text -> M = X pieces, one entry per base, bincount into a depth array per contig): the SQL-first path
                reduced to its unavoidable part
One JSON line per leg: records/s (median, min, max over the passes), and for (a) and (b) the device time of the record stage's row passes,
of the coverage kernels (with the table's zeroing) and of the result's scan (HIP events of one extra pass).  Run under `rocprofv3
--kernel-trace --stats -- python tools/bench_coverage.py --skip-fetch` for the per-kernel table."""
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

EXCLUDE = 0x704
CHUNK = 250_000                                                      # reads expanded base by base at once on the host


def cigar_pieces(off, heap, n):
    """the M = X operations of a CIGAR text heap: (row, reference offset in the read, query offset in the read, length)"""
    digit = (heap >= 48) & (heap <= 57)
    ops = np.flatnonzero(~digit)
    code = heap[ops]
    val = np.zeros(ops.size, np.int64)
    alive = np.ones(ops.size, bool)
    for k in range(9):
        at = ops - 1 - k
        alive &= at >= 0
        alive[alive] &= digit[at[alive]]
        if not alive.any():
            break
        val[alive] += (heap[at[alive]].astype(np.int64) - 48) * 10 ** k
    row = np.searchsorted(off, ops, side="right") - 1
    keep = code != ord("*")
    row, code, val = row[keep], code[keep], val[keep]
    isin = lambda s: np.isin(code, np.frombuffer(s, np.uint8))
    m, ref, qry = isin(b"M=X"), isin(b"MDN=X"), isin(b"MIS=X")
    rstep, qstep = np.where(ref, val, 0), np.where(qry, val, 0)
    rcum, qcum = np.cumsum(rstep) - rstep, np.cumsum(qstep) - qstep           # exclusive, over the whole heap
    first = np.searchsorted(row, np.arange(n), side="left")
    r0, q0 = rcum[first[row]], qcum[first[row]]                               # what lies in front of the row's first operation
    return row[m], (rcum - r0)[m], (qcum - q0)[m], val[m]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--unique-records", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-blocks", type=int, default=24576)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--min-baseq", default="0,20")
    ap.add_argument("--fetch-passes", type=int, default=0, help="passes of leg (c), which takes seconds each (0: as --passes)")
    ap.add_argument("--skip-fetch", action="store_true", help="leave leg (c) out (a run under a profiler)")
    a = ap.parse_args()
    data, sizes, hdr_bytes, raw = bench.generate_file(None, synth, 42, a.unique_records, a.reps, min(16, os.cpu_count() or 1), 0)
    ctx = duckhts_amd.Context(0)
    L = ctx.L
    L.dhts_bam_batch_host_bytes.restype = C.c_uint64; L.dhts_bam_batch_host_bytes.argtypes = [C.c_void_p, C.c_uint32]
    L.dhts_host_alloc.restype = C.c_void_p; L.dhts_host_alloc.argtypes = [C.c_uint64]; L.dhts_host_free.argtypes = [C.c_void_p]
    L.dhts_bam_batch_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    mask = duckhts_amd.COVERAGE_COLMASK
    fetch_mask = mask | (1 << 5) | (1 << 10)                         # + CIGAR, QUAL
    arena = {"p": None, "cap": 0}
    try:
        ctx.open(data)
        file_bytes = int(data.nbytes)
        data = None
        ctx.bgzf_index()
        hdr = ctx.bam_open()
        lens = [int(x) for x in hdr["ref_len"]]

        def scan():
            ctx.rewind()
            rows = 0
            while True:
                b = ctx.next_batch(a.max_blocks, mask)
                rows += b.n_rows
                if b.status != 0:
                    assert b.status == 1
                    return rows

        n_records = scan()
        for bq in [int(x) for x in a.min_baseq.split(",")]:
            parts = {"open": [], "scan": [], "result": []}

            def coverage():
                ctx.rewind()
                t0 = time.perf_counter()
                ctx.bam_coverage_open(exclude_flags=EXCLUDE, min_baseq=bq)
                L.dhts_sync(ctx.h)
                t1 = time.perf_counter()
                assert ctx.bam_coverage_scan(a.max_blocks) == 1
                L.dhts_sync(ctx.h)
                t2 = time.perf_counter()
                got = []
                while True:
                    cols, st = ctx.bam_coverage_next(0)
                    got.append(cols)
                    if st != 0:
                        break
                t3 = time.perf_counter()
                parts["open"].append(t1 - t0); parts["scan"].append(t2 - t1); parts["result"].append(t3 - t2)
                return {k: np.concatenate([g[k] for g in got]) for k in duckhts_amd.COVERAGE_COLUMNS}

            def fetch():
                ctx.rewind()
                depth = [np.zeros(ln, np.int32) for ln in lens]
                numreads, sum_mapq, sum_baseq = np.zeros(len(lens), np.int64), np.zeros(len(lens), np.int64), np.zeros(len(lens), np.int64)
                hb = duckhts_amd.BamBatch()
                while True:
                    b = ctx.next_batch(a.max_blocks, fetch_mask)
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
                        mapq = np.ctypeslib.as_array(C.cast(hb.mapq, C.POINTER(C.c_int32)), (n,))
                        coff = np.ctypeslib.as_array(C.cast(hb.cigar.off, C.POINTER(C.c_uint32)), (n + 1,)).astype(np.int64)
                        cheap = np.ctypeslib.as_array(C.cast(hb.cigar.bytes, C.POINTER(C.c_uint8)), (max(int(hb.cigar.nbytes), 1),))[:int(hb.cigar.nbytes)]
                        qoff = np.ctypeslib.as_array(C.cast(hb.qual.off, C.POINTER(C.c_uint32)), (n + 1,)).astype(np.int64)
                        qheap = np.ctypeslib.as_array(C.cast(hb.qual.bytes, C.POINTER(C.c_uint8)), (max(int(hb.qual.nbytes), 1),))[:int(hb.qual.nbytes)]
                        ok = (tid >= 0) & (pos >= 1) & ((flag & EXCLUDE) == 0)
                        ok &= (pos - 1) < np.asarray(lens, np.int64)[np.maximum(tid, 0)]          # (a read that starts behind its contig overlaps no row)
                        numreads += np.bincount(tid[ok], minlength=len(lens))[:len(lens)]
                        sum_mapq += np.bincount(tid[ok], weights=mapq[ok], minlength=len(lens)).astype(np.int64)[:len(lens)]
                        for c0 in range(0, n, CHUNK):
                            c1 = min(n, c0 + CHUNK)
                            row, roff, qo, ln = cigar_pieces(coff[c0:c1 + 1] - coff[c0], cheap[coff[c0]:coff[c1]], c1 - c0)
                            row = row + c0
                            use = ok[row]
                            row, roff, qo, ln = row[use], roff[use], qo[use], ln[use]
                            # one entry per base: its piece, its offset inside the piece
                            piece = np.repeat(np.arange(row.size), ln)
                            inside = np.arange(piece.size) - np.repeat(np.cumsum(ln) - ln, ln)
                            x = (pos[row] - 1 + roff)[piece] + inside
                            q = qheap[(qoff[row] + qo)[piece] + inside].astype(np.int64) - 33
                            t = tid[row][piece]
                            keep = (q >= bq) & (x < np.asarray(lens, np.int64)[t])
                            for k in range(len(lens)):
                                sel = keep & (t == k)
                                if sel.any():
                                    xs = x[sel]
                                    lo = int(xs.min())                     # (a sorted file: a chunk's bases lie in a narrow window of the contig)
                                    cnt = np.bincount(xs - lo).astype(np.int32)
                                    depth[k][lo:lo + cnt.size] += cnt
                                    sum_baseq[k] += int(q[sel].sum())
                    if b.status != 0:
                        return {"numreads": numreads, "sum_mapq": sum_mapq, "sum_baseq": sum_baseq, "sum_depth": np.array([int(d.sum(dtype=np.int64)) for d in depth], np.int64),
                                "covbases": np.array([int((d >= 1).sum()) for d in depth], np.int64)}

            legs = [("scan", scan), ("coverage", coverage)] + ([] if a.skip_fetch else [("fetch", fetch)])
            dev = coverage()
            st = ctx.bam_coverage_stats()
            agree = None
            if not a.skip_fetch:
                host = fetch()
                agree = bool(all((host[k] == dev[k]).all() for k in host))
            assert st["n_rows"] == n_records
            print(json.dumps({"min_baseq": bq, "records": n_records, "file_bytes": file_bytes, "target_rows": st["n_target_rows"], "table_bytes": st["table_bytes"], "stats": st,
                              "sum_depth_total": int(dev["sum_depth"].sum()), "covbases_total": int(dev["covbases"].sum()), "numreads_total": int(dev["numreads"].sum()),
                              "host_model_equals_device": agree, "resident": "compressed BAM in HBM", "max_blocks": a.max_blocks}), flush=True)
            times = {k: [] for k, _ in legs}
            for v in parts.values():
                v.clear()
            for it in range(a.passes):
                for k, fn in legs:
                    if k == "fetch" and a.fetch_passes and it >= a.fetch_passes:
                        continue
                    L.dhts_sync(ctx.h)
                    t0 = time.perf_counter()
                    fn()
                    L.dhts_sync(ctx.h)
                    times[k].append(time.perf_counter() - t0)
            devt = {}
            for k, fn in legs[:2]:
                ctx.set_timing(True); ctx.reset_times()
                fn()
                L.dhts_sync(ctx.h)
                kt = ctx.kernel_times(); ctx.set_timing(False)
                devt[k] = {"row_passes_ms (core_unpack)": round(kt["core_unpack"][0], 3), "coverage_kernels_ms (bcf_check)": round(kt["bcf_check"][0], 3), "coverage_launch_groups": kt["bcf_check"][1],
                           "scans_ms (scan)": round(kt["scan"][0], 3)}
            for k, _ in legs:
                ts = sorted(times[k])
                med = ts[len(ts) // 2]
                print(json.dumps({"min_baseq": bq, "leg": k, "passes": len(ts), "median_s": round(med, 4), "min_s": round(ts[0], 4), "max_s": round(ts[-1], 4), "records_per_s_median": round(n_records / med),
                                  "records_per_s_min_max": [round(n_records / ts[-1]), round(n_records / ts[0])], **({"device_time_one_pass": devt[k]} if k in devt else {}),
                                  **({"median_s_of_open_scan_result": [round(sorted(parts[q][:a.passes])[a.passes // 2], 4) for q in ("open", "scan", "result")]} if k == "coverage" else {})}), flush=True)
    finally:
        if arena["p"]:
            L.dhts_host_free(arena["p"])
        ctx.close()


if __name__ == "__main__":
    main()
