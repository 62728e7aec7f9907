"""bam_bedcov on the benchmark's synthetic BAM, resident in HBM.

The file is bench.py's (its generator, seed 42): --unique-records records per segment, --reps segments, compressed bytes uploaded once.
Two BED files over the header's contigs, resident as text in a second context: "dense" tiles every contig with 1 kb intervals, "sparse"
spreads about 200,000 intervals of 150 bp evenly.  Per BED three legs over the same resident bytes, alternated pass by pass in one process
after a warm-up pass of each:
  (a) scan     dhts_bam_next_batch to the end with the string-free column mask, nothing else
  (b) bedcov   dhts_bam_bedcov_open (one pass over the BED, breakpoints, zeroed counters) + dhts_bam_bedcov_scan + the whole result read back
               (dhts_bam_bedcov_next / _batch_fetch, eight columns into pinned memory); the three parts are also timed one by one
  (c) fetch    the scan with dhts_bam_batch_fetch of FLAG / POS / MAPQ / tid / CIGAR into pinned host memory + a numpy version of the model
               (CIGAR text -> rlen, sorted starts and ends, searchsorted per BED row): the SQL-first path reduced to its unavoidable part
One JSON line per BED and leg: records/s (median, min, max over the passes), and for (a) and (b) the device time of the record stage's row
passes, of the bedcov kernels and of its scan (HIP events of one extra pass).  Run under `rocprofv3 --kernel-trace --stats -- python
tools/bench_bedcov.py` for the per-kernel table."""
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


def bed_text(names, lens, width, step):
    out = []
    for n, ln in zip(names, lens):
        n = n.decode() if isinstance(n, bytes) else n
        out.append("".join(f"{n}\t{s}\t{min(s + width, ln)}\n" for s in range(0, int(ln), step)))
    return "".join(out).encode()


def bed_arrays(names, lens, width, step):
    """(tid, start, end) of the rows bed_text writes"""
    t, s, e = [], [], []
    for k, ln in enumerate(lens):
        a = np.arange(0, int(ln), step, dtype=np.int64)
        t.append(np.full(a.size, k, np.int64)); s.append(a); e.append(np.minimum(a + width, int(ln)))
    return np.concatenate(t), np.concatenate(s), np.concatenate(e)


def cigar_rlen(off, heap, n):
    """reference length per row of a CIGAR text heap (numbers of at most 9 digits; '*' has none)"""
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
    ref = (code == ord("M")) | (code == ord("D")) | (code == ord("N")) | (code == ord("=")) | (code == ord("X"))
    row = np.searchsorted(off, ops, side="right") - 1
    return np.bincount(row[ref], weights=val[ref], minlength=n).astype(np.int64)[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--unique-records", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-blocks", type=int, default=24576)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--beds", default="dense,sparse")
    ap.add_argument("--skip-fetch", action="store_true", help="leave leg (c) out (a run under a profiler)")
    a = ap.parse_args()
    data, sizes, hdr_bytes, raw = bench.generate_file(None, synth, 42, a.unique_records, a.reps, min(16, os.cpu_count() or 1), 0)
    ctx, bctx = duckhts_amd.Context(0), duckhts_amd.Context(0)
    L = ctx.L
    L.dhts_bam_batch_host_bytes.restype = C.c_uint64; L.dhts_bam_batch_host_bytes.argtypes = [C.c_void_p, C.c_uint32]
    L.dhts_host_alloc.restype = C.c_void_p; L.dhts_host_alloc.argtypes = [C.c_uint64]; L.dhts_host_free.argtypes = [C.c_void_p]
    L.dhts_bam_batch_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    mask = duckhts_amd.BEDCOV_COLMASK
    fetch_mask = mask | (1 << 5)                                    # + CIGAR
    arena, res_arena = {"p": None, "cap": 0}, {"p": None, "cap": 0}
    try:
        ctx.open(data)
        file_bytes = int(data.nbytes)
        data = None
        ctx.bgzf_index()
        hdr = ctx.bam_open()
        names, lens = hdr["ref_names"], [int(x) for x in hdr["ref_len"]]
        genome = sum(lens)

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
        for which in a.beds.split(","):
            width, step = (1000, 1000) if which == "dense" else (150, max(150, genome // 200_000))
            text = bed_text(names, lens, width, step)
            btid, bs, be = bed_arrays(names, lens, width, step)
            bctx.open(text)
            bctx.L.dhts_bgzf_index(bctx.h)
            bctx._chk(bctx.L.dhts_bed_open(bctx.h))
            keys_s, keys_e = (btid << 32) + bs, (btid << 32) + be

            parts = {"open": [], "scan": [], "result": []}

            def bedcov():
                # the C ABI's calls; the result is read back whole (eight columns) into pinned memory, the two result columns are kept
                ctx.rewind()
                t0 = time.perf_counter()
                ctx.bam_bedcov_open(bctx, exclude_flags=EXCLUDE)
                t1 = time.perf_counter()
                assert ctx.bam_bedcov_scan(a.max_blocks) == 1
                L.dhts_sync(ctx.h)
                t2 = time.perf_counter()
                bases, reads = [], []
                rb, host = duckhts_amd.BedBatch(), (duckhts_amd.BcfCol * 8)()
                while True:
                    ctx._chk(L.dhts_bam_bedcov_next(ctx.h, bctx.h, 0, C.byref(rb)))
                    n = int(rb.n_rows)
                    need = int(L.dhts_bam_bedcov_batch_host_bytes(C.byref(rb)))
                    if need > res_arena["cap"]:
                        if res_arena["p"]:
                            L.dhts_host_free(res_arena["p"])
                        res_arena["p"], res_arena["cap"] = L.dhts_host_alloc(need + need // 4), need + need // 4
                    ctx._chk(L.dhts_bam_bedcov_batch_fetch(ctx.h, C.byref(rb), res_arena["p"], res_arena["cap"], host))
                    if n:
                        bases.append(np.ctypeslib.as_array(C.cast(host[6].fixed, C.POINTER(C.c_int64)), (n,)).copy())
                        reads.append(np.ctypeslib.as_array(C.cast(host[7].fixed, C.POINTER(C.c_int64)), (n,)).copy())
                    if rb.status != 0:
                        break
                t3 = time.perf_counter()
                parts["open"].append(t1 - t0); parts["scan"].append(t2 - t1); parts["result"].append(t3 - t2)
                return np.concatenate(bases), np.concatenate(reads)

            def fetch():
                ctx.rewind()
                bases, reads = np.zeros(bs.size, np.int64), np.zeros(bs.size, np.int64)
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
                        off = np.ctypeslib.as_array(C.cast(hb.cigar.off, C.POINTER(C.c_uint32)), (n + 1,))
                        heap = np.ctypeslib.as_array(C.cast(hb.cigar.bytes, C.POINTER(C.c_uint8)), (max(int(hb.cigar.nbytes), 1),))
                        rlen = cigar_rlen(off, heap[:int(hb.cigar.nbytes)], n)
                        ok = (tid >= 0) & (pos >= 1) & ((flag & EXCLUDE) == 0)
                        key = (tid[ok].astype(np.int64) << 32) + (pos[ok] - 1)
                        rl = np.where(flag[ok] & 4, 0, rlen[ok])
                        # depth: F(x) = sum max(0, x - a) - max(0, x - b) over the segments [a, b), from the sorted starts and ends
                        seg = rl > 0
                        sa, sb = np.sort(key[seg]), np.sort(key[seg] + rl[seg])
                        ca, cb = np.concatenate([[0], np.cumsum(sa)]), np.concatenate([[0], np.cumsum(sb)])

                        def F(x):
                            ia, ib = np.searchsorted(sa, x, side="left"), np.searchsorted(sb, x, side="left")
                            return (ia * x - ca[ia]) - (ib * x - cb[ib])
                        bases += F(keys_e) - F(keys_s)
                        p, q = np.sort(key), np.sort(key + np.maximum(rl, 1))
                        reads += np.searchsorted(p, keys_e, side="left") - np.searchsorted(q, keys_s, side="right")
                    if b.status != 0:
                        return bases, reads

            legs = [("scan", scan), ("bedcov", bedcov)] + ([] if a.skip_fetch else [("fetch", fetch)])
            dev_bases, dev_reads = bedcov()
            st = ctx.bam_bedcov_stats()
            agree = None
            if not a.skip_fetch:
                host_bases, host_reads = fetch()
                agree = bool((host_bases == dev_bases).all() and (host_reads == dev_reads).all())
                assert agree, (int((host_bases != dev_bases).sum()), int((host_reads != dev_reads).sum()))
            assert st["n_rows"] == n_records
            print(json.dumps({"bed": which, "records": n_records, "file_bytes": file_bytes, "bed_rows": st["n_bed_rows"], "bed_bytes": len(text), "breakpoints": st["n_breakpoints"],
                              "interval_width": width, "interval_step": step, "stats": st, "bases_covered_total": int(dev_bases.sum()), "read_count_total": int(dev_reads.sum()),
                              "host_model_equals_device": agree, "resident": "compressed BAM and BED text in HBM", "max_blocks": a.max_blocks}), flush=True)
            times = {k: [] for k, _ in legs}
            for v in parts.values():
                v.clear()
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
                dev[k] = {"row_passes_ms (core_unpack)": round(kt["core_unpack"][0], 3), "bedcov_kernels_ms (bcf_check)": round(kt["bcf_check"][0], 3), "bedcov_launch_groups": kt["bcf_check"][1],
                          "scans_ms (scan)": round(kt["scan"][0], 3)}
            for k, _ in legs:
                ts = sorted(times[k])
                med = ts[len(ts) // 2]
                print(json.dumps({"bed": which, "leg": k, "passes": len(ts), "median_s": round(med, 4), "min_s": round(ts[0], 4), "max_s": round(ts[-1], 4), "records_per_s_median": round(n_records / med),
                                  "records_per_s_min_max": [round(n_records / ts[-1]), round(n_records / ts[0])], **({"device_time_one_pass": dev[k]} if k in dev else {}),
                                  **({"median_s_of_open_scan_result": [round(sorted(parts[q][:a.passes])[a.passes // 2], 4) for q in ("open", "scan", "result")]} if k == "bedcov" else {})}), flush=True)
    finally:
        for ar in (arena, res_arena):
            if ar["p"]:
                L.dhts_host_free(ar["p"])
        bctx.close()
        ctx.close()


if __name__ == "__main__":
    main()
