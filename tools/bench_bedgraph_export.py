"""bam_bedgraph_export against the route it replaces, on the benchmark's synthetic BAM, resident in HBM.

The file is bench.py's (its generator, seed 42; the 25-contig header).  One context, the compressed bytes uploaded once; zero_runs = 1, so that the
result has a few rows per read.  Two routes to the same two files (x.bed.gz and its index), alternated pass by pass in one process after a warm-up
pass of each; every stage ends in a device synchronise or a closed file:
  export   dhts_bam_bedgraph_open + _scan | dhts_bedgraph_export with the index | the same without the index.  With the kernel timer on, the device
           time of the count and emit kernels (DHTS_K_SCAN), the encoder's lengths and carry (_BCF_MEASURE), its write pass (_BCF_WRITE) and the
           compressor (_HUFF).
  host     dhts_bam_bedgraph_open + _scan | every page fetched to a pinned buffer | formatted there by one thread (tools/format_rows.c, -O2) |
           the text written to a file | dhts_bgzip_file | the tabix index (dhts_tabix_build_index on the file, wrapped, written).
Before the clock the run checks that both routes leave the same bytes in both files.  Then the encoder's write pass alone, staged in LDS against one
lane per row (dhts_debug_rows_text_form), alternated over exports without an index at level 0.  Medians of --passes passes; one JSON line per leg."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
import duckhts_amd  # noqa: E402
from bench_coverage import EXCLUDE  # noqa: E402
from duckhts_amd import synth  # noqa: E402

CONF_BED = (0x10000, 1, 2, 3, ord("#"), 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--unique-records", type=int, default=5_500_000)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--max-blocks", type=int, default=24576)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--index", default="csi", choices=("tbi", "csi"))
    a = ap.parse_args()
    work = tempfile.mkdtemp(prefix="bedgraph_export_")
    so = os.path.join(work, "format_rows.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "format_rows.c")])
    F = C.CDLL(so)
    F.format_rows.restype = C.c_size_t
    F.format_rows.argtypes = [C.c_void_p] * 4 + [C.c_size_t, C.c_char_p, C.c_void_p, C.c_void_p]
    data, sizes, hdr_bytes, raw = bench.generate_file(None, synth, 42, a.unique_records, a.reps, min(16, os.cpu_count() or 1), 0)
    ctx = duckhts_amd.Context(0)
    L = ctx.L
    L.dhts_host_alloc.restype = C.c_void_p; L.dhts_host_alloc.argtypes = [C.c_uint64]; L.dhts_host_free.argtypes = [C.c_void_p]
    L.dhts_tabix_build_index.restype = C.c_int64; L.dhts_tabix_build_index.argtypes = [C.c_void_p] + [C.c_int] * 7
    L.dhts_bgzf_wrap.restype = C.c_int64; L.dhts_bgzf_wrap.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    arena = {"p": None, "cap": 0}
    min_shift = 0 if a.index == "tbi" else 14
    parts = {}

    def reserve(need):
        if need > arena["cap"]:
            if arena["p"]:
                L.dhts_host_free(arena["p"])
            arena["p"], arena["cap"] = L.dhts_host_alloc(need + need // 4), need + need // 4

    def scan():
        ctx.rewind()
        t0 = time.perf_counter()
        ctx.bam_bedgraph_open(exclude_flags=EXCLUDE, zero_runs=1)
        assert ctx.bam_bedgraph_scan(a.max_blocks) == 1
        L.dhts_sync(ctx.h)
        return time.perf_counter() - t0

    def leg_export(out, timed=True):
        p = parts.setdefault("export", {})
        s = scan()
        ctx.set_timing(True); ctx.reset_times()
        t0 = time.perf_counter()
        st = ctx.bam_bedgraph_export(out, index=a.index, min_shift=min_shift, overwrite=True)
        t1 = time.perf_counter()
        k = ctx.kernel_times()
        ctx.set_timing(False)
        t2 = time.perf_counter()
        ctx.bam_bedgraph_export(out + ".noindex", index="none", overwrite=True)
        t3 = time.perf_counter()
        if timed:
            for key, v in (("scan_accumulate_s", s), ("export_with_index_s", t1 - t0), ("export_without_index_s", t3 - t2), ("index_s", (t1 - t0) - (t3 - t2)),
                           ("count_emit_device_ms", k["scan"][0]), ("encoder_lengths_carry_device_ms", k["bcf_measure"][0]), ("encoder_write_device_ms", k["bcf_write"][0]),
                           ("compressor_device_ms", k["huff_decode"][0])):
                p.setdefault(key, []).append(v)
        return st

    def leg_host(out, names, name_off, longest, timed=True):
        p = parts.setdefault("host", {})
        s = scan()
        plain = out + ".txt"
        b, host = duckhts_amd.BedBatch(), (duckhts_amd.BcfCol * 4)()
        t_fetch = t_format = t_write = 0.0
        rows = fetched = 0
        buf = None
        with open(plain, "wb") as f:
            st = 0
            while st == 0:
                t0 = time.perf_counter()
                ctx._chk(L.dhts_bam_bedgraph_next(ctx.h, 0, 15, C.byref(b)))
                st, n = int(b.status), int(b.n_rows)
                need = int(L.dhts_bam_bedgraph_batch_host_bytes(C.byref(b)))
                reserve(need)
                ctx._chk(L.dhts_bam_bedgraph_batch_fetch(ctx.h, C.byref(b), arena["p"], arena["cap"], host))
                t1 = time.perf_counter()
                if n:
                    if buf is None or len(buf) < n * (longest + 64):
                        buf = np.empty(n * (longest + 64), np.uint8)
                    m = F.format_rows(host[0].fixed, host[1].fixed, host[2].fixed, host[3].fixed, n, names, name_off.ctypes.data, buf.ctypes.data)
                    t2 = time.perf_counter()
                    f.write(memoryview(buf[:m]))
                    t3 = time.perf_counter()
                    t_format += t2 - t1; t_write += t3 - t2
                t_fetch += t1 - t0; rows += n; fetched += need
        t0 = time.perf_counter()
        ctx2 = duckhts_amd.Context(0)
        try:
            ctx2.bgzip_file(plain, out, -1)
            t1 = time.perf_counter()
            ctx2.open(out); ctx2.bgzf_index()
            n = L.dhts_tabix_build_index(ctx2.h, *CONF_BED, min_shift)
            assert n > 0, L.dhts_error(ctx2.h)
            rawi = np.zeros(n, np.uint8)
            assert L.dhts_bam_index_bytes(ctx2.h, rawi.ctypes.data, n) == 0
            need = L.dhts_bgzf_wrap(rawi.ctypes.data, n, None, 0)
            z = np.zeros(need, np.uint8)
            z = z[:L.dhts_bgzf_wrap(rawi.ctypes.data, n, z.ctypes.data, need)]
            open(out + "." + a.index, "wb").write(z.tobytes())
            t2 = time.perf_counter()
        finally:
            ctx2.close()
        if timed:
            for key, v in (("scan_accumulate_s", s), ("fetch_pages_s", t_fetch), ("format_on_host_s", t_format), ("write_text_s", t_write), ("bgzip_file_s", t1 - t0), ("tabix_index_s", t2 - t1),
                           ("total_behind_the_scan_s", t_fetch + t_format + t_write + (t2 - t0))):
                p.setdefault(key, []).append(v)
        return rows, fetched, os.path.getsize(plain)

    def leg_form(form, out):
        ctx.debug_rows_text_form(form)
        try:
            ctx.set_timing(True); ctx.reset_times()
            t0 = time.perf_counter()
            ctx.bam_bedgraph_export(out, index="none", level=0, overwrite=True)
            dt = time.perf_counter() - t0
            k = ctx.kernel_times()
            ctx.set_timing(False)
        finally:
            ctx.debug_rows_text_form("staged")
        return k["bcf_write"][0], k["bcf_write"][1], dt

    try:
        file_bytes = int(data.nbytes)
        ctx.open(data)
        ctx.bgzf_index()
        data = None
        hdr = ctx.bam_open()
        nm = [n.encode() if isinstance(n, str) else bytes(n) for n in hdr["ref_names"]]
        names, name_off, longest = b"".join(nm), np.concatenate([[0], np.cumsum([len(x) for x in nm])]).astype(np.uint32), max(len(x) for x in nm)
        e_out, h_out = os.path.join(work, "export.bed.gz"), os.path.join(work, "host.bed.gz")
        # ---- agreement, once (and the warm-up pass of each route) ----
        st = leg_export(e_out, timed=False)
        rows, fetched, text_bytes = leg_host(h_out, names, name_off, longest, timed=False)
        same_file = open(e_out, "rb").read() == open(h_out, "rb").read()
        same_index = open(e_out + "." + a.index, "rb").read() == open(h_out + "." + a.index, "rb").read()
        stats = ctx.bam_bedgraph_stats()
        print(json.dumps({"records": stats["n_rows"], "counted": stats["n_counted"], "file_bytes": file_bytes, "contigs": len(nm), "result_rows": st["n_rows"], "text_bytes": st["bytes_text"],
                          "bed_gz_bytes": st["bytes_out"], "index": a.index, "index_bytes": st["bytes_index"], "fetched_column_bytes": fetched, "both_routes_same_bed_gz": same_file,
                          "both_routes_same_index": same_index, "resident": "compressed BAM in HBM", "max_blocks": a.max_blocks}), flush=True)
        assert same_file and same_index and rows == st["n_rows"] and text_bytes == st["bytes_text"]
        for _ in range(a.passes):
            leg_export(e_out)
            leg_host(h_out, names, name_off, longest)
        med = lambda v: sorted(v)[len(v) // 2]
        for leg in ("export", "host"):
            print(json.dumps(dict({"leg": leg, "passes": a.passes}, **{k: round(med(v), 4) for k, v in parts[leg].items()}, **{k + "_all": [round(x, 4) for x in v] for k, v in parts[leg].items()})), flush=True)
        # ---- the write pass: staged in LDS against one lane per row, on the result of the last scan ----
        forms = {"staged": [], "lane": []}
        for form in ("staged", "lane"):
            leg_form(form, e_out + ".form")                                 # warm-up
        for _ in range(a.passes):
            for form in ("staged", "lane"):
                forms[form].append(leg_form(form, e_out + ".form"))
        same_forms = True
        for form in ("staged", "lane"):
            leg_form(form, e_out + ".form." + form)
        same_forms = open(e_out + ".form.staged", "rb").read() == open(e_out + ".form.lane", "rb").read()
        for form in ("staged", "lane"):
            ms = [x[0] for x in forms[form]]
            print(json.dumps({"leg": "write_pass_" + form, "passes": a.passes, "device_ms_median": round(med(ms), 3), "device_ms_all": [round(x, 3) for x in ms], "launches": forms[form][0][1],
                              "text_bytes": st["bytes_text"], "bytes_per_s": round(st["bytes_text"] / (med(ms) * 1e-3)) if med(ms) else None,
                              "export_level0_s_median": round(med([x[2] for x in forms[form]]), 4), "same_bytes_as_the_other_form": same_forms}), flush=True)
    finally:
        if arena["p"]:
            L.dhts_host_free(arena["p"])
        ctx.close()
        for f in os.listdir(work):
            os.unlink(os.path.join(work, f))
        os.rmdir(work)


if __name__ == "__main__":
    main()
