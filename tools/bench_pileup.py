"""bam_pileup on two files resident in HBM.

  sparse   bench.py's synthetic BAM (its generator, seed 42; --unique-records x --reps records), restricted by region to --contig
  dense    400,000 sorted 150-base reads on one 2,000,000-base contig (30x): random bases and qualities, both strands, a third of the reads
           with a 2-base D, a third with a 3-base I; built here with numpy and compressed by the device BGZF writer (dhts_bgzf_compress)
Legs over the same resident bytes, alternated pass by pass in one process after a warm-up pass of each:
  (a) scan         dhts_bam_next_batch to the end with the string-free column mask, nothing else
  (b) pileup       dhts_bam_pileup_open + _scan + the count + every page emitted and fetched into one reused pinned buffer, once with every
                   add form (dhts_debug_pileup_add_form 1 direct, 2 window); the table function's defaults (deletions, strands)
  (c) fetch        the route without bam_pileup: the scan with dhts_bam_batch_fetch of FLAG / POS / MAPQ / tid / CIGAR / SEQ / QUAL into pinned
                   host memory + a numpy expansion into the same (position, strand, symbol) counts.  Before the clock this leg is the
                   agreement check: equal to (b) row for row, with every form.
One JSON line per file and leg: the host clock around whole passes (median, min, max), for (b) the parts (open, scan, count, emit + fetch) and
the device time of classify + add of one extra pass (HIP events).  Run under `rocprofv3 --kernel-trace --stats -- python tools/bench_pileup.py
--skip-fetch --passes 2` for the add kernel's own time per form and file."""
import argparse
import ctypes as C
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
import duckhts_amd  # noqa: E402
from bench_coverage import CHUNK, EXCLUDE  # noqa: E402
from duckhts_amd import synth  # noqa: E402

FORMS = {1: "direct", 2: "window"}
SYM_OF_TEXT = np.full(256, 4, np.int64)                                  # the symbol index of a SEQ character: A C G T, '=' 5, everything else N
for _i, _c in enumerate(b"ACGT"):
    SYM_OF_TEXT[_c] = _i
SYM_OF_TEXT[ord("=")] = 5


def dense_bam(n_reads=400_000, ref_len=2_000_000, read_len=150, seed=7):
    """the raw (uncompressed) BAM of the dense file: every record has three CIGAR operations and one size"""
    rng = np.random.default_rng(seed)
    text = f"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:dense\tLN:{ref_len}\n".encode()
    head = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", 1) + struct.pack("<i", 6) + b"dense\x00" + struct.pack("<i", ref_len)
    size = 32 + 8 + 12 + (read_len + 1) // 2 + read_len
    rec = np.zeros((n_reads, 4 + size), np.uint8)
    put32 = lambda col, v: rec.__setitem__((slice(None), slice(col, col + 4)), np.asarray(v, "<i4").reshape(-1, 1).view(np.uint8) if np.ndim(v) else np.tile(np.array([v], "<i4").view(np.uint8), (n_reads, 1)))
    pos = np.sort(rng.integers(0, ref_len - read_len - 2, n_reads)).astype("<i4")
    flag = (rng.integers(0, 2, n_reads) * 16).astype(np.int64)
    put32(0, size); put32(4, 0); put32(8, pos)
    put32(12, (30 << 8) | 8)                                              # bin 0, MAPQ 30, l_read_name 8
    put32(16, ((flag << 16) | 3).astype("<i4")); put32(20, read_len); put32(24, -1); put32(28, -1); put32(32, 0)
    names = np.char.add("r", np.char.zfill(np.arange(n_reads).astype(str), 6)).astype("S7")
    rec[:, 36:43] = np.frombuffer(names.tobytes(), np.uint8).reshape(n_reads, 7)
    kind = rng.integers(0, 3, n_reads)                                    # 0: 50M50M50M, 1: 70M2D80M, 2: 70M3I77M
    ops = np.array([[(50 << 4), (50 << 4), (50 << 4)], [(70 << 4), (2 << 4) | 2, (80 << 4)], [(70 << 4), (3 << 4) | 1, (77 << 4)]], "<u4")[kind]
    rec[:, 44:56] = ops.view(np.uint8).reshape(n_reads, 12)
    codes = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, (n_reads, read_len))]
    rec[:, 56:56 + read_len // 2] = (codes[:, 0::2] << 4) | codes[:, 1::2]
    rec[:, 56 + read_len // 2:] = rng.integers(2, 42, (n_reads, read_len), dtype=np.uint8)
    return head + rec.tobytes()


def cigar_all(off, heap, n):
    """every operation of a CIGAR text heap: (row, code, length, reference offset in the read, query offset in the read)"""
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
    rstep, qstep = np.where(isin(b"MDN=X"), val, 0), np.where(isin(b"MIS=X"), val, 0)
    rcum, qcum = np.cumsum(rstep) - rstep, np.cumsum(qstep) - qstep
    first = np.searchsorted(row, np.arange(n), side="left")
    return row, code, val, rcum - rcum[first[row]], qcum - qcum[first[row]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--unique-records", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--max-blocks", type=int, default=24576)
    ap.add_argument("--max-rows", type=int, default=0, help="rows per page (0: the ABI's default)")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--fetch-passes", type=int, default=2, help="passes of leg (c), which takes seconds each")
    ap.add_argument("--min-baseq", type=int, default=0)
    ap.add_argument("--contig", type=int, default=0, help="the contig of the sparse file's region")
    ap.add_argument("--files", default="sparse,dense")
    ap.add_argument("--skip-fetch", action="store_true", help="leave leg (c) and the agreement check out (a run under a profiler)")
    a = ap.parse_args()
    for which in a.files.split(","):
        run(a, which)


def run(a, which):
    ctx = duckhts_amd.Context(0)
    L = ctx.L
    L.dhts_bam_batch_host_bytes.restype = C.c_uint64; L.dhts_bam_batch_host_bytes.argtypes = [C.c_void_p, C.c_uint32]
    L.dhts_host_alloc.restype = C.c_void_p; L.dhts_host_alloc.argtypes = [C.c_uint64]; L.dhts_host_free.argtypes = [C.c_void_p]
    L.dhts_bam_batch_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    mask = duckhts_amd.PILEUP_COLMASK
    fetch_mask = mask | (1 << 5) | (1 << 9) | (1 << 10)                  # + CIGAR, SEQ, QUAL
    arena = {"p": None, "cap": 0}

    def reserve(need):
        if need > arena["cap"]:
            if arena["p"]:
                L.dhts_host_free(arena["p"])
            arena["p"], arena["cap"] = L.dhts_host_alloc(need + need // 4), need + need // 4

    try:
        if which == "dense":
            wctx = duckhts_amd.Context(0)
            try:
                data = wctx.bgzf_compress(dense_bam())
            finally:
                wctx.close()
        else:
            data = bench.generate_file(None, synth, 42, a.unique_records, a.reps, min(16, os.cpu_count() or 1), 0)[0]
        file_bytes = len(data) if isinstance(data, (bytes, bytearray)) else int(data.nbytes)
        ctx.open(data)
        ctx.bgzf_index()
        data = None
        hdr = ctx.bam_open()
        lens = [int(x) for x in hdr["ref_len"]]
        k = a.contig if which == "sparse" else 0
        name = hdr["ref_names"][k]
        name = name.decode() if isinstance(name, bytes) else name
        assert ctx.set_regions(name)
        S = 16

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

        def pileup_leg(form, sink=None):
            p = parts.setdefault(form, {"open": [], "scan": [], "count": [], "emit_fetch": [], "rows": 0, "bytes": 0, "pages": 0})
            ctx.rewind()
            ctx.bam_pileup_add_form(form)
            t0 = time.perf_counter()
            ctx.bam_pileup_open(exclude_flags=EXCLUDE, min_baseq=a.min_baseq, include_deletions=1, include_insertions=0, distinguish_strands=1, min_nucleotide_depth=1)
            L.dhts_sync(ctx.h)
            t1 = time.perf_counter()
            assert ctx.bam_pileup_scan(a.max_blocks) == 1
            L.dhts_sync(ctx.h)
            t2 = time.perf_counter()
            b = duckhts_amd.BedBatch()
            host = (duckhts_amd.BcfCol * 5)()
            view = lambda n: [np.ctypeslib.as_array(C.cast(host[i].fixed, C.POINTER(t)), (n,)) for i, t in enumerate((C.c_int32, C.c_int64, C.c_uint8, C.c_uint8, C.c_int32))]
            ctx._chk(L.dhts_bam_pileup_next(ctx.h, 1, 31, C.byref(b)))    # the count, and one row
            t3 = time.perf_counter()
            rows, nbytes, pages, st = int(b.n_rows), 0, 0, int(b.status)
            if sink and b.n_rows:
                reserve(64)
                ctx._chk(L.dhts_bam_pileup_batch_fetch(ctx.h, C.byref(b), arena["p"], arena["cap"], host))
                sink(*view(1))
            while st == 0:
                ctx._chk(L.dhts_bam_pileup_next(ctx.h, a.max_rows, 31, C.byref(b)))
                st, n = int(b.status), int(b.n_rows)
                need = int(L.dhts_bam_pileup_batch_host_bytes(C.byref(b)))
                reserve(max(need, 64))
                ctx._chk(L.dhts_bam_pileup_batch_fetch(ctx.h, C.byref(b), arena["p"], arena["cap"], host))
                rows += n; nbytes += need; pages += 1
                if sink and n:
                    sink(*view(n))
            t4 = time.perf_counter()
            p["open"].append(t1 - t0); p["scan"].append(t2 - t1); p["count"].append(t3 - t2); p["emit_fetch"].append(t4 - t3)
            p["rows"], p["bytes"], p["pages"] = rows, nbytes, pages
            return rows

        def fetch():
            """leg (c): the counts of the contig from the region's rows, expanded on the host: the sorted keys position * 16 + strand * 8 + symbol
            that occur, and their counts (a dense table of chr1 would take 16 GB on the host as well)"""
            ctx.rewind()
            keys, cnts = [], []
            hb = duckhts_amd.BamBatch()
            view = lambda p, t, n: np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), (max(n, 1),))[:n]
            while True:
                b = ctx.next_batch(a.max_blocks, fetch_mask)
                n = int(b.n_rows)
                if n:
                    reserve(int(L.dhts_bam_batch_host_bytes(C.byref(b), fetch_mask)))
                    ctx._chk(L.dhts_bam_batch_fetch(ctx.h, C.byref(b), fetch_mask, arena["p"], arena["cap"], C.byref(hb)))
                    flag, pos, tid = view(hb.flag, C.c_uint16, n), view(hb.pos, C.c_int64, n), view(hb.tid, C.c_int32, n)
                    coff, cheap = view(hb.cigar.off, C.c_uint32, n + 1).astype(np.int64), view(hb.cigar.bytes, C.c_uint8, int(hb.cigar.nbytes))
                    soff, sheap = view(hb.seq.off, C.c_uint32, n + 1).astype(np.int64), view(hb.seq.bytes, C.c_uint8, int(hb.seq.nbytes))
                    qoff, qheap = view(hb.qual.off, C.c_uint32, n + 1).astype(np.int64), view(hb.qual.bytes, C.c_uint8, int(hb.qual.nbytes))
                    ok = (tid == k) & (pos >= 1) & ((flag & EXCLUDE) == 0) & ((pos - 1) < lens[k])
                    strand = ((flag & 16) != 0).astype(np.int64) * 8
                    for c0 in range(0, n, CHUNK):
                        c1 = min(n, c0 + CHUNK)
                        row, code, ln, roff, qo = cigar_all(coff[c0:c1 + 1] - coff[c0], cheap[coff[c0]:coff[c1]], c1 - c0)
                        row = row + c0
                        use = ok[row] & (ln > 0)
                        for want, is_m in ((np.isin(code, np.frombuffer(b"M=X", np.uint8)), True), (code == ord("D"), False)):
                            w = use & want
                            r, rf, q0, l = row[w], roff[w], qo[w], ln[w]
                            piece = np.repeat(np.arange(r.size), l)
                            inside = np.arange(piece.size) - np.repeat(np.cumsum(l) - l, l)
                            x = (pos[r] - 1 + rf)[piece] + inside
                            if is_m:
                                at = (q0)[piece] + inside
                                q = qheap[qoff[r][piece] + at].astype(np.int64) - 33
                                sym = SYM_OF_TEXT[sheap[soff[r][piece] + at]]
                                sel = (q >= a.min_baseq) & (x < lens[k])
                            else:
                                sym = np.full(x.size, 6, np.int64)
                                sel = x < lens[k]
                            idx = (x * S + strand[r][piece] + sym)[sel]
                            if idx.size:
                                u, c = np.unique(idx, return_counts=True)
                                keys.append(u); cnts.append(c)
                if b.status != 0:
                    if not keys:
                        return np.zeros(0, np.int64), np.zeros(0, np.int64)
                    u, inv = np.unique(np.concatenate(keys), return_inverse=True)
                    return u, np.bincount(inv, weights=np.concatenate(cnts)).astype(np.int64)

        n_records = scan()
        # ---- agreement, once per form ----
        agree = {}
        if not a.skip_fetch:
            nz, want = fetch()
            for form, fname in FORMS.items():
                got = {"at": 0, "ok": True}

                def sink(tid, pos, strand, nuc, count):
                    n = len(pos)
                    w, wc = nz[got["at"]:got["at"] + n], want[got["at"]:got["at"] + n]
                    lut = np.full(256, -1, np.int64); lut[np.frombuffer(b"ACGTN=-+", np.uint8)] = np.arange(8)
                    idx = (pos - 1) * S + (strand == ord("-")) * 8 + lut[nuc]
                    got["ok"] &= len(w) == n and bool((tid == k).all() and (idx == w).all() and (count == wc).all())
                    got["at"] += n

                pileup_leg(form, sink=sink)
                agree[f"{fname}_equals_host_expansion_row_for_row"] = bool(got["ok"] and got["at"] == nz.size)
        st = ctx.bam_pileup_stats() if parts else {}
        print(json.dumps({"file": which, "records_in_region": n_records, "file_bytes": file_bytes, "min_baseq": a.min_baseq, "contig": name, "contig_len": lens[k], "stats": st,
                          "agreement": agree, "resident": "compressed BAM in HBM", "max_blocks": a.max_blocks, "max_rows": a.max_rows or (1 << 20)}), flush=True)
        assert all(agree.values()), agree
        parts.clear()
        # ---- the legs, alternated ----
        legs = [("scan", scan)] + [(f"pileup_{fname}", (lambda form=form: pileup_leg(form))) for form, fname in FORMS.items()] + ([] if a.skip_fetch else [("fetch", fetch)])
        for _, fn in legs:
            fn()
        parts.clear()
        times = {name_: [] for name_, _ in legs}
        for _ in range(a.passes):
            for name_, fn in legs:
                if name_ == "fetch" and len(times[name_]) >= a.fetch_passes:
                    continue
                L.dhts_sync(ctx.h)
                t0 = time.perf_counter()
                fn()
                L.dhts_sync(ctx.h)
                times[name_].append(time.perf_counter() - t0)
        devt = {}
        for name_, fn in legs[:1 + len(FORMS)]:
            ctx.set_timing(True); ctx.reset_times()
            fn()
            L.dhts_sync(ctx.h)
            kt = ctx.kernel_times(); ctx.set_timing(False)
            devt[name_] = {"row_passes_ms (core_unpack)": round(kt["core_unpack"][0], 3), "zero_classify_add_ms (bcf_check)": round(kt["bcf_check"][0], 3), "result_ms (scan)": round(kt["scan"][0], 3)}
        med = lambda v: sorted(v)[len(v) // 2]
        for name_, _ in legs:
            ts = sorted(times[name_])
            line = {"file": which, "leg": name_, "passes": len(ts), "median_s": round(med(ts), 4), "min_s": round(ts[0], 4), "max_s": round(ts[-1], 4), "records_per_s_median": round(n_records / med(ts))}
            if name_ in devt:
                line["device_time_one_pass"] = devt[name_]
            form = {f"pileup_{v}": f for f, v in FORMS.items()}.get(name_)
            if form in parts:
                p = parts[form]
                ef = med(p["emit_fetch"])
                line.update({"median_s_of_open_scan_count_emitfetch": [round(med(p[q]), 4) for q in ("open", "scan", "count", "emit_fetch")], "result_rows": p["rows"], "pages": p["pages"],
                             "fetched_bytes": p["bytes"], "emit_fetch_rows_per_s": round(p["rows"] / ef) if ef else None})
            print(json.dumps(line), flush=True)
    finally:
        if arena["p"]:
            L.dhts_host_free(arena["p"])
        ctx.close()


if __name__ == "__main__":
    main()
