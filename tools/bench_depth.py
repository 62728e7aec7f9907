"""bam_depth on the benchmark's synthetic BAM, resident in HBM.

The file is bench.py's (its generator, seed 42): --unique-records records per segment, --reps segments, compressed bytes uploaded once, on
two contexts: one for the whole file, one restricted by region to --contig.  Legs over the same resident bytes, alternated pass by pass in
one process after a warm-up pass of each:
  (a) scan         dhts_bam_next_batch to the end with the string-free column mask, nothing else
  (b) depth        dhts_bam_depth_open + _scan + the whole result taken page by page (dhts_bam_depth_next / _batch_fetch) into one reused
                   pinned buffer.  Three variants: mode 0; mode 0 with include_deletions; mode 2 (-aa) restricted by region to one contig, so
                   that the rows (the contig's length) and the bytes over PCIe (16 per row) are known in advance.  The parts are also timed
                   one by one: open, scan, count (the first dhts_bam_depth_next, asked for one row), emit + fetch (the remaining pages).
  (c) fetch        the only route the parent offers: the region's scan with dhts_bam_batch_fetch of FLAG / POS / MAPQ / tid / CIGAR / QUAL
                   into pinned host memory + a numpy expansion (bench_coverage.py's) into a depth array of that contig.  It must equal
                   (b)'s third variant exactly, and the first variant's rows on that contig.
  coverage         bam_coverage open + scan + result once per pass with the same min_baseq, so that bam_depth_add<false / true> runs on the
                   same batches as the nowords instantiations, and its result's carry in two levels over the same tile sums as bam_depth's
One JSON line per leg: the host clock around whole passes (median, min, max), for (b) the parts, rows/s and bytes/s of emit + fetch against
the rate of a plain device-to-host copy of the same bytes into the same buffer measured in the same run, and the device time of the add
passes (HIP events of one extra pass).  Run under `rocprofv3 --kernel-trace --stats -- python tools/bench_depth.py --skip-fetch --passes 2`
for the per-kernel table."""
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
from bench_coverage import CHUNK, EXCLUDE, cigar_pieces  # noqa: E402
from duckhts_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--unique-records", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-blocks", type=int, default=24576)
    ap.add_argument("--max-rows", type=int, default=0, help="rows per page (0: the ABI's default)")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--min-baseq", type=int, default=0)
    ap.add_argument("--contig", type=int, default=0, help="the contig of the region variant and of leg (c)")
    ap.add_argument("--skip-fetch", action="store_true", help="leave leg (c) out (a run under a profiler)")
    a = ap.parse_args()
    data, sizes, hdr_bytes, raw = bench.generate_file(None, synth, 42, a.unique_records, a.reps, min(16, os.cpu_count() or 1), 0)
    ctx, rctx = duckhts_amd.Context(0), duckhts_amd.Context(0)
    L = ctx.L
    L.dhts_bam_batch_host_bytes.restype = C.c_uint64; L.dhts_bam_batch_host_bytes.argtypes = [C.c_void_p, C.c_uint32]
    L.dhts_host_alloc.restype = C.c_void_p; L.dhts_host_alloc.argtypes = [C.c_uint64]; L.dhts_host_free.argtypes = [C.c_void_p]
    L.dhts_bam_batch_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    mask = duckhts_amd.DEPTH_COLMASK
    fetch_mask = mask | (1 << 5) | (1 << 10)                         # + CIGAR, QUAL
    arena = {"p": None, "cap": 0}

    def reserve(need):
        if need > arena["cap"]:
            if arena["p"]:
                L.dhts_host_free(arena["p"])
            arena["p"], arena["cap"] = L.dhts_host_alloc(need + need // 4), need + need // 4

    try:
        file_bytes = int(data.nbytes)
        for c in (ctx, rctx):
            c.open(data)
            c.bgzf_index()
        data = None
        hdr = ctx.bam_open()
        rctx.bam_open()
        lens = [int(x) for x in hdr["ref_len"]]
        name = hdr["ref_names"][a.contig]
        name = name.decode() if isinstance(name, bytes) else name
        assert rctx.set_regions(name)

        def scan():
            ctx.rewind()
            rows = 0
            while True:
                b = ctx.next_batch(a.max_blocks, mask)
                rows += b.n_rows
                if b.status != 0:
                    assert b.status == 1
                    return rows

        parts = {}

        def depth_leg(key, c, sink=None, **kw):
            """one pass of (b) on context c; sink(tid, pos, depth): called with views of every page in the pinned buffer"""
            p = parts.setdefault(key, {"open": [], "scan": [], "count": [], "emit_fetch": [], "rows": 0, "bytes": 0, "pages": 0, "copy_s": []})
            c.rewind()
            t0 = time.perf_counter()
            c.bam_depth_open(exclude_flags=EXCLUDE, min_baseq=a.min_baseq, **kw)
            L.dhts_sync(c.h)
            t1 = time.perf_counter()
            assert c.bam_depth_scan(a.max_blocks) == 1
            L.dhts_sync(c.h)
            t2 = time.perf_counter()
            b = duckhts_amd.BedBatch()
            host = (duckhts_amd.BcfCol * 3)()
            c._chk(L.dhts_bam_depth_next(c.h, 1, 7, C.byref(b)))          # the count, and one row
            t3 = time.perf_counter()
            rows, nbytes, pages, st, copy_s = int(b.n_rows), 0, 0, int(b.status), 0.0
            view = lambda n: [np.ctypeslib.as_array(C.cast(host[i].fixed, C.POINTER(t)), (n,)) for i, t in enumerate((C.c_int32, C.c_int64, C.c_int32))]
            if sink and b.n_rows:
                reserve(64)
                c._chk(L.dhts_bam_depth_batch_fetch(c.h, C.byref(b), arena["p"], arena["cap"], host))
                sink(*view(1))
            while st == 0:
                c._chk(L.dhts_bam_depth_next(c.h, a.max_rows, 7, C.byref(b)))
                st, n = int(b.status), int(b.n_rows)
                need = int(L.dhts_bam_depth_batch_host_bytes(C.byref(b)))
                reserve(need)
                c._chk(L.dhts_bam_depth_batch_fetch(c.h, C.byref(b), arena["p"], arena["cap"], host))
                rows += n; nbytes += need; pages += 1
                if sink and n:
                    sink(*view(n))
                if key.endswith("copy") and n:                           # the same bytes once more as a plain copy, outside the part's clock
                    tc = time.perf_counter()
                    c._chk(L.dhts_memcpy_d2h(c.h, arena["p"], b.cols[1].fixed, n * 8))
                    c._chk(L.dhts_memcpy_d2h(c.h, arena["p"] + n * 8, b.cols[0].fixed, n * 4))
                    c._chk(L.dhts_memcpy_d2h(c.h, arena["p"] + n * 12, b.cols[2].fixed, n * 4))
                    copy_s += time.perf_counter() - tc
            t4 = time.perf_counter()
            p["open"].append(t1 - t0); p["scan"].append(t2 - t1); p["count"].append(t3 - t2); p["emit_fetch"].append(t4 - t3 - copy_s)
            p["rows"], p["bytes"], p["pages"] = rows, nbytes, pages
            if copy_s:
                p["copy_s"].append(copy_s)
            return rows

        def coverage():
            ctx.rewind()
            ctx.bam_coverage_open(exclude_flags=EXCLUDE, min_baseq=a.min_baseq)
            assert ctx.bam_coverage_scan(a.max_blocks) == 1
            while ctx.bam_coverage_next(0)[1] == 0:
                pass

        def fetch():
            """leg (c): the depth array of the contig from the region's rows, expanded on the host"""
            rctx.rewind()
            k = a.contig
            depth = np.zeros(lens[k], np.int32)
            hb = duckhts_amd.BamBatch()
            while True:
                b = rctx.next_batch(a.max_blocks, fetch_mask)
                n = int(b.n_rows)
                if n:
                    reserve(int(L.dhts_bam_batch_host_bytes(C.byref(b), fetch_mask)))
                    rctx._chk(L.dhts_bam_batch_fetch(rctx.h, C.byref(b), fetch_mask, arena["p"], arena["cap"], C.byref(hb)))
                    flag = np.ctypeslib.as_array(C.cast(hb.flag, C.POINTER(C.c_uint16)), (n,))
                    pos = np.ctypeslib.as_array(C.cast(hb.pos, C.POINTER(C.c_int64)), (n,))
                    tid = np.ctypeslib.as_array(C.cast(hb.tid, C.POINTER(C.c_int32)), (n,))
                    coff = np.ctypeslib.as_array(C.cast(hb.cigar.off, C.POINTER(C.c_uint32)), (n + 1,)).astype(np.int64)
                    cheap = np.ctypeslib.as_array(C.cast(hb.cigar.bytes, C.POINTER(C.c_uint8)), (max(int(hb.cigar.nbytes), 1),))[:int(hb.cigar.nbytes)]
                    qoff = np.ctypeslib.as_array(C.cast(hb.qual.off, C.POINTER(C.c_uint32)), (n + 1,)).astype(np.int64)
                    qheap = np.ctypeslib.as_array(C.cast(hb.qual.bytes, C.POINTER(C.c_uint8)), (max(int(hb.qual.nbytes), 1),))[:int(hb.qual.nbytes)]
                    ok = (tid == k) & (pos >= 1) & ((flag & EXCLUDE) == 0) & ((pos - 1) < lens[k])
                    for c0 in range(0, n, CHUNK):
                        c1 = min(n, c0 + CHUNK)
                        row, roff, qo, ln = cigar_pieces(coff[c0:c1 + 1] - coff[c0], cheap[coff[c0]:coff[c1]], c1 - c0)
                        row = row + c0
                        use = ok[row]
                        row, roff, qo, ln = row[use], roff[use], qo[use], ln[use]
                        piece = np.repeat(np.arange(row.size), ln)
                        inside = np.arange(piece.size) - np.repeat(np.cumsum(ln) - ln, ln)
                        x = (pos[row] - 1 + roff)[piece] + inside
                        q = qheap[(qoff[row] + qo)[piece] + inside].astype(np.int64) - 33
                        sel = (q >= a.min_baseq) & (x < lens[k])
                        if sel.any():
                            xs = x[sel]
                            lo = int(xs.min())
                            cnt = np.bincount(xs - lo).astype(np.int32)
                            depth[lo:lo + cnt.size] += cnt
                if b.status != 0:
                    return depth

        n_records = scan()
        variants = [("depth", ctx, dict()), ("depth_deletions", ctx, dict(include_deletions=1)), ("depth_aa_one_contig", rctx, dict(all_positions=2))]
        # ---- agreement, once ----
        k, klen = a.contig, lens[a.contig]
        dense, seen = np.zeros(klen, np.int32), {"rows_on_k": 0, "positive": True, "ascending": True, "last": 0}

        def sink0(tid, pos, dep):                                        # mode 0, whole file: the rows on contig k into a dense array
            on_k = tid == k
            dense[pos[on_k] - 1] = dep[on_k]
            seen["rows_on_k"] += int(on_k.sum()); seen["positive"] &= bool((dep > 0).all())

        aa_dep, at = np.zeros(klen, np.int32), {"n": 0, "ok": True}

        def sink_aa(tid, pos, dep):                                      # mode 2 on the region: every position once, in order
            n = len(pos)
            at["ok"] &= bool((tid == k).all() and (pos == np.arange(at["n"] + 1, at["n"] + n + 1)).all())
            aa_dep[at["n"]:at["n"] + n] = dep
            at["n"] += n

        depth_leg("check", ctx, sink=sink0)
        st = ctx.bam_depth_stats()
        depth_leg("check_aa", rctx, sink=sink_aa, all_positions=2)
        assert st["n_rows"] == n_records and at["n"] == klen and at["ok"]
        agree = {"mode_0_rows_equal_aa_of_region": bool((dense == aa_dep).all()) and seen["rows_on_k"] == int((aa_dep > 0).sum()), "depths_positive_in_mode_0": seen["positive"]}
        if not a.skip_fetch:
            agree["host_expansion_equals_device"] = bool((fetch() == aa_dep).all())
        print(json.dumps({"records": n_records, "file_bytes": file_bytes, "min_baseq": a.min_baseq, "contig": name, "contig_len": lens[a.contig], "stats": st, "agreement": agree,
                          "resident": "compressed BAM in HBM", "max_blocks": a.max_blocks, "max_rows": a.max_rows or (1 << 20)}), flush=True)
        assert all(agree.values()), agree
        # ---- the copy rate of this run: the pages of the region variant once more as plain device-to-host copies ----
        depth_leg("aa_copy", rctx, all_positions=2)
        cp = parts["aa_copy"]
        copy_rate = cp["bytes"] / sum(cp["copy_s"]) if cp["copy_s"] else None
        parts.clear()
        # ---- the legs, alternated ----
        legs = [("scan", scan)] + [(k, (lambda k=k, c=c, kw=kw: depth_leg(k, c, **kw))) for k, c, kw in variants] + [("coverage", coverage)] + ([] if a.skip_fetch else [("fetch", fetch)])
        for _, fn in legs:
            fn()
        parts.clear()
        times = {k: [] for k, _ in legs}
        for _ in range(a.passes):
            for k, fn in legs:
                L.dhts_sync(ctx.h); L.dhts_sync(rctx.h)
                t0 = time.perf_counter()
                fn()
                L.dhts_sync(ctx.h); L.dhts_sync(rctx.h)
                times[k].append(time.perf_counter() - t0)
        devt = {}
        for k, fn in legs[:5]:
            c = rctx if k == "depth_aa_one_contig" else ctx
            c.set_timing(True); c.reset_times()
            fn()
            L.dhts_sync(c.h)
            kt = c.kernel_times(); c.set_timing(False)
            devt[k] = {"row_passes_ms (core_unpack)": round(kt["core_unpack"][0], 3), "classify_add_zero_ms (bcf_check)": round(kt["bcf_check"][0], 3), "result_ms (scan)": round(kt["scan"][0], 3)}
        med = lambda v: sorted(v)[len(v) // 2]
        for k, _ in legs:
            ts = sorted(times[k])
            line = {"leg": k, "passes": len(ts), "median_s": round(med(ts), 4), "min_s": round(ts[0], 4), "max_s": round(ts[-1], 4), "records_per_s_median": round(n_records / med(ts))}
            if k in devt:
                line["device_time_one_pass"] = devt[k]
            if k in parts:
                p = parts[k]
                ef = med(p["emit_fetch"])
                line.update({"median_s_of_open_scan_count_emitfetch": [round(med(p[q]), 4) for q in ("open", "scan", "count", "emit_fetch")], "result_rows": p["rows"], "pages": p["pages"],
                             "fetched_bytes": p["bytes"], "emit_fetch_rows_per_s": round(p["rows"] / ef) if ef else None, "emit_fetch_bytes_per_s": round(p["bytes"] / ef) if ef else None,
                             "plain_copy_bytes_per_s_same_run": round(copy_rate) if copy_rate else None})
            print(json.dumps(line), flush=True)
    finally:
        if arena["p"]:
            L.dhts_host_free(arena["p"])
        rctx.close()
        ctx.close()


if __name__ == "__main__":
    main()
