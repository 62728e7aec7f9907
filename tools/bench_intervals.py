#!/usr/bin/env python3
"""Times interval_merge / interval_overlap / interval_nearest on the device and prints ONE JSON line.

Seeded BED text is made in memory at every size of --sizes (default 10^6 and 10^7 rows) in five shapes:
    tiling       sorted, back to back on 6 chroms
    shuffled     the same rows shuffled within their chrom
    alternating  the chrom changes on every line
    right_span   tiling, and one right row that spans a whole chrom
    left_span    tiling, and one left row that spans a whole chrom
The right file of the join is the left one moved by half a row, so that every left row has about two pairs.  Per shape and size, after a
warm-up, --repeats repeats: the load (line table, bed_intervals, the append), every sort pass, the index, the merge, the overlap's count and
its write passes, all timed with device events (dhts_debug_ivl_ms), median and spread (min, max).  "sort_hbm_share": the sort moves 32 bytes
per pair and pass (the count reads the key, the scatter reads and writes key and row) -- that over the passes' time, as a share of the
8.0 TB/s HBM peak of MI355X_MICROARCH.md.  "host_build_ms": the index build the BAM join still uses (dhts_bam_set_overlap_intervals: a host
std::stable_sort and five uploads) for the same intervals, wall clock around the call, alternating with the device build in the same run;
"device_build_ms" is the sort plus the index on the device, by events, and "device_build_wall_ms" the wall clock around the whole load less
the load part.  The nearest legs run behind the overlap in the same repeat, at k = 1 and k = 8 (ties 'all', no max_distance), every page written
and none fetched: "nearest_k1" / "nearest_k8" hold n_pairs, n_unmatched, end_sort_passes and the end sort with its gather, the selection pass with its
carry and the write passes (dhts_debug_ivl_ms 6 / 7 / 8) -- to be read beside overlap_count_ms and overlap_write_ms of the same run.  The right
context is loaded anew in every repeat, so the k = 1 leg builds the end order and the k = 8 leg finds it there."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import duckhts_amd   # noqa: E402

HBM_PEAK = 8.0e12
SHAPES = ("tiling", "shuffled", "alternating", "right_span", "left_span")
N_CHROMS = 6
NEAREST_K = (1, 8)


def make_rows(shape, n, seed):
    """(chrom index, start, end) arrays of the left file, and of the right file"""
    rng = np.random.default_rng(seed)
    per = -(-n // N_CHROMS)
    idx = np.arange(n, dtype=np.int64)
    if shape == "alternating":
        chrom, k = idx % N_CHROMS, idx // N_CHROMS
    else:
        chrom, k = idx // per, idx % per
    start = k * 100
    end = start + 100
    if shape == "shuffled":
        perm = rng.permutation(n)
        o = perm[np.argsort(chrom[perm], kind="stable")]                       # the chroms in order, the rows of one chrom in random order
        chrom, start, end = chrom[o], start[o], end[o]
    rc, rs, re = chrom.copy(), start + 50, end + 50
    if shape == "right_span":
        rs[0], re[0] = 0, per * 100
    if shape == "left_span":
        start, end = start.copy(), end.copy()
        start[0], end[0] = 0, per * 100
    return (chrom, start, end), (rc, rs, re)


def bed_text(chrom, start, end):
    names = ["chr%d" % (c + 1) for c in range(N_CHROMS)]
    out = []
    for a in range(0, len(chrom), 1 << 20):
        out.append("".join("%s\t%d\t%d\n" % (names[c], s, e) for c, s, e in zip(chrom[a:a + (1 << 20)].tolist(), start[a:a + (1 << 20)].tolist(), end[a:a + (1 << 20)].tolist())))
    return "".join(out).encode()


def bed_ctx(text, device):
    ctx = duckhts_amd.Context(device)
    ctx.open(text)
    ctx.L.dhts_bgzf_index(ctx.h)
    ctx._chk(ctx.L.dhts_bed_open(ctx.h))
    return ctx


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def run(shape, n, repeats, device, bam):
    left, right = make_rows(shape, n, 17)
    lctx, rctx = bed_ctx(bed_text(*left), device), bed_ctx(bed_text(*right), device)
    tid, beg, end = right[0].astype(np.int32), right[1].astype(np.int64), right[2].astype(np.int64)
    t = {k: [] for k in ("load", "sort", "index", "merge", "overlap_count", "overlap_write", "device_build", "device_build_wall", "host_build")}
    near = {k: {"stats": None, "end_order": [], "select": [], "write": []} for k in NEAREST_K}
    passes = [[] for _ in range(duckhts_amd.IVL_SORT_MAX_PASSES)]
    st = pairs = runs = None
    try:
        for rep in range(repeats + 1):                                         # the first one warms up: buffers, code objects
            w0 = time.perf_counter()
            rctx.ivl_load()
            w1 = time.perf_counter()
            bam._chk(bam.L.dhts_bam_set_overlap_intervals(bam.h, tid.ctypes.data, beg.ctypes.data, end.ctypes.data, len(tid)))
            w2 = time.perf_counter()
            lctx.ivl_load()
            lctx.ivl_merge_open(0)
            runs = lctx.ivl_stats()["n_runs"]
            ms_merge = lctx.debug_ivl_ms(3)
            lctx.ivl_overlap_open(rctx, "any")
            b = duckhts_amd.BedBatch()
            while True:                                                        # every page written on the device, none fetched
                lctx._chk(lctx.L.dhts_ivl_overlap_next(lctx.h, 0, 0xff, C.byref(b)))
                if b.status != 0:
                    break
            st, pairs = rctx.ivl_stats(), lctx.ivl_stats()["n_pairs"]
            ms_overlap = (lctx.debug_ivl_ms(4), lctx.debug_ivl_ms(5))
            for k in NEAREST_K:
                lctx.ivl_nearest_open(rctx, k)
                while True:
                    lctx._chk(lctx.L.dhts_ivl_nearest_next(lctx.h, 0, 0x1ff, C.byref(b)))
                    if b.status != 0:
                        break
                near[k]["stats"] = lctx.ivl_nearest_stats()
                if rep:
                    near[k]["end_order"].append(lctx.debug_ivl_ms(6)); near[k]["select"].append(lctx.debug_ivl_ms(7)); near[k]["write"].append(lctx.debug_ivl_ms(8))
            if rep == 0:
                continue
            ms = [rctx.debug_ivl_ms(k) for k in range(3)]
            t["load"].append(ms[0]); t["sort"].append(ms[1]); t["index"].append(ms[2]); t["merge"].append(ms_merge)
            t["overlap_count"].append(ms_overlap[0]); t["overlap_write"].append(ms_overlap[1])
            t["device_build"].append(ms[1] + ms[2]); t["device_build_wall"].append((w1 - w0) * 1e3 - ms[0]); t["host_build"].append((w2 - w1) * 1e3)
            for p in range(duckhts_amd.IVL_SORT_MAX_PASSES):
                passes[p].append(rctx.debug_ivl_ms(16 + p))
    finally:
        lctx.close()
        rctx.close()
    ran = [p for p in range(len(passes)) if max(passes[p]) > 0]
    pass_ms = sum(statistics.median(passes[p]) for p in ran)
    out = {"shape": shape, "rows": n, "sort_passes": st["sort_passes"], "n_name_runs": st["n_name_runs"], "n_runs": runs, "n_pairs": pairs}
    out.update({k + "_ms": spread(v) for k, v in t.items()})
    out["sort_pass_ms"] = {str(p): spread(passes[p]) for p in ran}
    for k in NEAREST_K:
        out["nearest_k%d" % k] = dict({f: near[k]["stats"][f] for f in ("n_pairs", "n_unmatched", "end_sort_passes")},
                                      **{f + "_ms": spread(near[k][f]) for f in ("end_order", "select", "write")})
    out["sort_hbm_share"] = round(32.0 * st["n_rows"] * len(ran) / (pass_ms * 1e-3) / HBM_PEAK, 4) if pass_ms > 0 else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    bam = duckhts_amd.Context(a.device)                                        # the BAM join's context: its header gives the baseline its contigs
    try:
        bam.open(open(os.path.join(ROOT, "tests", "golden", "range.bam"), "rb").read())
        bam.bgzf_index()
        hdr = bam.bam_open()
        assert len(hdr["ref_names"]) >= N_CHROMS
        results = []
        for n in a.sizes.split(","):
            for shape in a.shapes.split(","):
                results.append(run(shape, int(n), a.repeats, a.device, bam))
                print("done: %s %s" % (shape, n), file=sys.stderr, flush=True)
    finally:
        bam.close()
    print(json.dumps({"bench": "intervals", "hbm_peak_bytes_per_s": HBM_PEAK, "repeats": a.repeats, "results": results}))


if __name__ == "__main__":
    main()
