// dhts_bam_bedgraph_export.inc -- part of dhts_api.hip (included there behind dhts_bam_bedgraph.inc, inside its extern "C" block; not a translation
// unit of its own): bam_bedgraph_export.  The result of an open and scanned bam_bedgraph leaves the device as a bgzipped bedGraph file with its
// tabix index: every page of the result (bedgraph_page: the windows and tiles dhts_bam_bedgraph_next walks) is printed by the row-text encoder
// (rows_text.hip) straight into the compressor's input z_in behind the tail the chunk before it left, all whole blocks of 0xff00 bytes go
// through bgzf_compress_device, their compressed bytes through a pinned buffer to the file, and the tail shorter than a block moves to the
// front.  The last tail is the last block; the EOF block closes the file.  No result row crosses PCIe.  The contract is in
// include/duckhts_amd.h.
#define EXPORT_DEFAULT_CHUNK_BLOCKS 4096ll                          /* blocks a launch of the compressor takes: dhts_bgzip_file's 267 MB of input */
enum { EXPORT_ERR = -1, EXPORT_ERR_OPEN = -3, EXPORT_ERR_WRITE = -5, EXPORT_ERR_EXISTS = -6, EXPORT_ERR_ORDER = -7, EXPORT_ERR_INDEX = -8 };

// rows [0, a.n) of the columns -> their text at dstbuf.p + at (dstbuf keeps its first `at` bytes when it has to grow, and has PAD_BYTES of
// room behind the text); *total = the bytes of the text.  off, part: scratch; which: the two 64-bit counters of the write paths, or null (not counted); form: 0 the
// write pass staged in LDS, 1 the lane-per-row form it is measured against.  The lengths and their carry are timed as DHTS_K_BCF_MEASURE, the
// write pass as DHTS_K_BCF_WRITE
static int rows_text_encode(dhts_ctx *c, const RtxCols &a, DevBuf &off, DevBuf &part, DevBuf *which, DevBuf &dstbuf, uint64_t at, uint64_t *total, int form = 0) {
    *total = 0;
    const uint64_t n = a.n;
    const size_t keep = dstbuf.cap >= at ? (size_t)at : 0;          // (a buffer that never held `at` bytes has nothing to keep)
    if (n == 0) return ensure_keep(c, dstbuf, (size_t)at + PAD_BYTES, keep);
    if (n > 0x7fffff00ull) return fail(c, "rows_text: too many rows in one page");
    ENSURE(c, off, (size_t)(n + 1) * 8 + 64);
    const unsigned grid = (unsigned)((n + 255) / 256);
    {
        KTimer tm(c, DHTS_K_BCF_MEASURE);
        hipLaunchKernelGGL(rtx_lengths, dim3(grid), dim3(256), 0, c->stream, a, (unsigned long long *)off.p);
        if (depth_carry<unsigned long long>(c, part, (unsigned long long *)off.p, n)) return -1;
    }
    HIPCHK(c, hipGetLastError());
    unsigned long long t = 0;
    HIPCHK(c, hipMemcpyAsync(&t, (const unsigned long long *)off.p + n, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (ensure_keep(c, dstbuf, (size_t)(at + t) + PAD_BYTES, keep)) return -1;
    {
        KTimer tm(c, DHTS_K_BCF_WRITE);
        if (form == 1) hipLaunchKernelGGL(rtx_write_lane, dim3(grid), dim3(256), 0, c->stream, a, (const unsigned long long *)off.p, (uint8_t *)dstbuf.p + at);
        else hipLaunchKernelGGL(rtx_write, dim3(grid), dim3(256), 0, c->stream, a, (const unsigned long long *)off.p, (uint8_t *)dstbuf.p + at, which ? (unsigned long long *)which->p : (unsigned long long *)nullptr);
    }
    HIPCHK(c, hipGetLastError());
    *total = t;
    return 0;
}

// tests: the encoder alone on host arrays -- a table of n_names names (names: the arena, name_offs: n_names + 1 offsets into it), n_rows rows of
// tid (int32), start, end (int64) and depth (int32) -> the text in out (cap bytes).  The text is written at an offset of 5 bytes into the
// device buffer, so that the write pass meets a span that is not 16-byte aligned.  Returns the bytes of the text (also when cap is smaller: nothing
// is copied then), or -1.  dhts_debug_rows_text_paths tells which write paths the call took.
int64_t dhts_debug_rows_text(dhts_ctx *c, const uint8_t *names, const uint32_t *name_offs, int32_t n_names, const int32_t *tid, const int64_t *start, const int64_t *end,
                             const int32_t *depth, int64_t n_rows, uint8_t *out, uint64_t cap) {
    if (!c) return -1;
    if (n_names < 0 || n_rows < 0 || (n_names && (!names || !name_offs)) || (n_rows && (!tid || !start || !end || !depth))) return fail(c, "debug_rows_text: arguments out of range");
    for (int32_t i = 0; i < n_names; i++) if (name_offs[i + 1] < name_offs[i]) return fail(c, "debug_rows_text: the name offsets decrease");
    HIPCHK(c, hipSetDevice(c->device));
    BedgraphState &S = c->bdg;
    const size_t n = (size_t)n_rows, nb = n_names ? name_offs[n_names] : 0;
    DevBuf d_tid, d_start, d_end, d_depth;
    ENSURE(c, S.x_names, nb + 64); ENSURE(c, S.x_noff, ((size_t)n_names + 1) * 4 + 64); ENSURE(c, S.x_which, 64);
    ENSURE(c, d_tid, n * 4 + 64); ENSURE(c, d_start, n * 8 + 64); ENSURE(c, d_end, n * 8 + 64); ENSURE(c, d_depth, n * 4 + 64);
    const std::vector<uint32_t> noff = n_names ? std::vector<uint32_t>(name_offs, name_offs + n_names + 1) : std::vector<uint32_t>(1, 0u);
    if (nb) HIPCHK(c, hipMemcpyAsync(S.x_names.p, names, nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(S.x_noff.p, noff.data(), noff.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (n) {
        HIPCHK(c, hipMemcpyAsync(d_tid.p, tid, n * 4, hipMemcpyHostToDevice, c->stream)); HIPCHK(c, hipMemcpyAsync(d_start.p, start, n * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_end.p, end, n * 8, hipMemcpyHostToDevice, c->stream)); HIPCHK(c, hipMemcpyAsync(d_depth.p, depth, n * 4, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipMemsetAsync(S.x_which.p, 0, 16, c->stream));
    RtxCols a; memset(&a, 0, sizeof(a));
    a.names = (const uint8_t *)S.x_names.p; a.name_off = (const uint32_t *)S.x_noff.p; a.n_names = (uint32_t)n_names; a.k = 3; a.name_id = (const int32_t *)d_tid.p;
    a.col[0] = d_start.p; a.width[0] = 8; a.col[1] = d_end.p; a.width[1] = 8; a.col[2] = d_depth.p; a.width[2] = 4; a.n = (unsigned long long)n;
    uint64_t total = 0; const uint64_t at = 5;
    if (rows_text_encode(c, a, S.x_off, S.part, &S.x_which, c->z_in, at, &total, S.x_form)) return -1;
    if (total && total <= cap) HIPCHK(c, hipMemcpyAsync(out, (const uint8_t *)c->z_in.p + at, total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                   // (the device columns and the offsets of this call are released behind it)
    return (int64_t)total;
}
// tests: the workgroups of the encoder's write pass that took the staged (out2[0]) and the fallback path (out2[1]) in the last
// dhts_debug_rows_text (an export does not count them)
int dhts_debug_rows_text_paths(dhts_ctx *c, uint64_t out2[2]) {
    if (!c || !out2) return -1;
    out2[0] = out2[1] = 0;
    if (!c->bdg.x_which.p) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out2, c->bdg.x_which.p, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// tests: the rows of a page and the blocks of a compressor launch of dhts_bedgraph_export on this context (0: the defaults), so that a
// small file crosses pages and chunks
int dhts_debug_export_limits(dhts_ctx *c, int64_t page_rows, int64_t chunk_blocks) {
    if (!c) return -1;
    if (page_rows < 0 || chunk_blocks < 0) return fail(c, "debug_export_limits: arguments out of range");
    c->bdg.x_page_rows = page_rows; c->bdg.x_chunk_blocks = chunk_blocks;
    return 0;
}

// tests, tools/bench_bedgraph_export.py: the form of the encoder's write pass on this context: 0 the default (rows staged in LDS, aligned
// 16-byte stores), 1 one lane per row storing byte by byte.  Any other value fails with a dhts_error
int dhts_debug_rows_text_form(dhts_ctx *c, int form) {
    if (!c) return -1;
    if (form < 0 || form > 1) return fail(c, "debug_rows_text_form: the form must be 0 (staged) or 1 (lane per row)");
    c->bdg.x_form = form;
    return 0;
}

// what dhts_bedgraph_export writes through: the file, the pinned buffer the compressed bytes reach the host in, and the bytes written
struct ExportOut {
    FILE *f = nullptr; uint8_t *pin = nullptr; uint64_t pin_cap = 0; int64_t written = 0;
    ~ExportOut() { if (pin) dhts_host_free(pin); if (f) fclose(f); }
};
// n bytes of z_in from `in` on (whole blocks, or the last tail) -> the file, at most chunk_blocks blocks a launch; 0 or an EXPORT_ERR_* code
static int export_compress(dhts_ctx *c, ExportOut &o, const uint8_t *in, uint64_t n, int level, int64_t chunk_blocks) {
    const uint64_t CH = (uint64_t)chunk_blocks * DFL_IN;
    for (uint64_t done = 0; done < n; done += CH) {
        const uint64_t m = n - done < CH ? n - done : CH;
        uint64_t ol = 0;
        {
            KTimer tm(c, DHTS_K_HUFF);                               // (the compressor's three kernels; the inflate stage does not run here)
            if (bgzf_compress_device(c, m, level, &ol, in + done)) return EXPORT_ERR;
        }
        if (ol > o.pin_cap) {
            if (o.pin) dhts_host_free(o.pin);
            o.pin_cap = ol + ol / 4 + (1u << 16); o.pin = (uint8_t *)dhts_host_alloc(o.pin_cap);
            if (!o.pin) { o.pin_cap = 0; fail(c, "bam_bedgraph_export: out of pinned memory"); return EXPORT_ERR; }
        }
        if (hipMemcpyAsync(o.pin, c->z_out.p, ol, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { fail(c, "bam_bedgraph_export: device error"); return EXPORT_ERR; }
        if (fwrite(o.pin, 1, ol, o.f) != ol) { fail(c, "bam_bedgraph_export: write error: %s", strerror(errno)); return EXPORT_ERR_WRITE; }
        o.written += (int64_t)ol;
    }
    return 0;
}

// the index of the written file by the tabix writer (the BED preset: 0-based half-open, columns 1 / 2 / 3) through a scratch context on the same
// device, wrapped as a BGZF file; 0 or EXPORT_ERR_INDEX with c's error set
static int export_index(dhts_ctx *c, const char *out_path, const std::string &index_path, int min_shift, uint64_t *bytes_index) {
    dhts_ctx *x = dhts_create(c->device);
    if (!x) { fail(c, "bam_bedgraph_export: no scratch context for the index"); return EXPORT_ERR_INDEX; }
    int rc = 0; int64_t n = -1; std::vector<uint8_t> raw, file;
    if (dhts_open_path(x, out_path) != 0 || dhts_bgzf_index(x) <= 0 || (n = dhts_tabix_build_index(x, 0x10000, 1, 2, 3, '#', 0, min_shift)) < 0) rc = EXPORT_ERR_INDEX;
    if (rc == 0) { raw.resize((size_t)n); if (n && dhts_bam_index_bytes(x, raw.data(), (uint64_t)n) != 0) rc = EXPORT_ERR_INDEX; }
    if (rc) fail(c, "bam_bedgraph_export: the index could not be built: %s", dhts_error(x));
    dhts_destroy(x);
    (void)hipSetDevice(c->device);
    if (rc) return rc;
    file.resize((size_t)dhts_bgzf_wrap(raw.data(), raw.size(), nullptr, 0));
    const int64_t z = dhts_bgzf_wrap(raw.data(), raw.size(), file.data(), file.size());
    FILE *f = fopen(index_path.c_str(), "wb");
    if (!f) { fail(c, "bam_bedgraph_export: cannot open output %s: %s", index_path.c_str(), strerror(errno)); return EXPORT_ERR_OPEN; }
    const bool ok = fwrite(file.data(), 1, (size_t)z, f) == (size_t)z;
    if (fclose(f) != 0 || !ok) { fail(c, "bam_bedgraph_export: write error: %s", index_path.c_str()); return EXPORT_ERR_WRITE; }
    *bytes_index = (uint64_t)z;
    return 0;
}

int dhts_bedgraph_export(dhts_ctx *c, const char *out_path, const dhts_bedgraph_export_params *p, dhts_bedgraph_export_stats *out) {
    if (!c) return EXPORT_ERR;
    if (out) memset(out, 0, sizeof(*out));
    if (!out_path || !*out_path || !p || !out) { fail(c, "bam_bedgraph_export: no output path, parameters or stats"); return EXPORT_ERR; }
    BedgraphState &S = c->bdg;
    if (!S.open) { fail(c, "bam_bedgraph_export: dhts_bam_bedgraph_open not called"); return EXPORT_ERR; }
    if (p->index < 0 || p->index > 2) { fail(c, "bam_bedgraph_export: index must be 0 (none), 1 (TBI) or 2 (CSI)"); return EXPORT_ERR; }
    if (p->overwrite < 0 || p->overwrite > 1) { fail(c, "bam_bedgraph_export: overwrite must be 0 or 1"); return EXPORT_ERR; }
    if (p->index && c->rg_active && !c->rg_given.empty()) {         // a tabix index wants every contig's lines together, ascending
        std::vector<char> seen(c->ref_len.size(), 0);
        for (size_t o = 0; o < S.o_tid.size(); o++) {
            const bool same = o && S.o_tid[o] == S.o_tid[o - 1];
            if ((same && S.o_beg[o] < S.o_beg[o - 1]) || (!same && seen[(size_t)S.o_tid[o]])) {
                fail(c, "bam_bedgraph_export: the regions are not in file order (an indexed file needs each contig's regions together and ascending)");
                return EXPORT_ERR_ORDER;
            }
            seen[(size_t)S.o_tid[o]] = 1;
        }
    }
    const std::string index_path = p->index ? std::string(out_path) + (p->index == 1 ? ".tbi" : ".csi") : std::string();
    struct stat st;
    if (!p->overwrite && stat(out_path, &st) == 0) { fail(c, "bam_bedgraph_export: output '%s' already exists (overwrite is off)", out_path); return EXPORT_ERR_EXISTS; }
    if (hipSetDevice(c->device) != hipSuccess) { fail(c, "bam_bedgraph_export: device error"); return EXPORT_ERR; }
    const int level = p->level == 0 ? 0 : 6;                        // as dhts_bgzip_file: 0 stores, every other level is the one compressing setting
    const int64_t page_rows = S.x_page_rows > 0 ? S.x_page_rows : 0, chunk_blocks = S.x_chunk_blocks > 0 ? S.x_chunk_blocks : EXPORT_DEFAULT_CHUNK_BLOCKS;
    int rc = 0; uint64_t n_rows = 0, bytes_text = 0, bytes_index = 0; int64_t bytes_out = 0;
    {
        ExportOut o;
        o.f = fopen(out_path, "wb");
        if (!o.f) { fail(c, "bam_bedgraph_export: cannot open output %s: %s", out_path, strerror(errno)); return EXPORT_ERR_OPEN; }
        auto body = [&]() -> int {
            // the contigs' names, once per export
            std::vector<uint32_t> noff(c->ref_name.size() + 1, 0); std::string arena;
            for (size_t t = 0; t < c->ref_name.size(); t++) { arena += c->ref_name[t]; noff[t + 1] = (uint32_t)arena.size(); }
            ENSURE(c, S.x_names, arena.size() + 64); ENSURE(c, S.x_noff, noff.size() * 4 + 64);
            if (!arena.empty()) HIPCHK(c, hipMemcpyAsync(S.x_names.p, arena.data(), arena.size(), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(S.x_noff.p, noff.data(), noff.size() * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));            // (the copies read vectors of this block)
            S.o_next = 0; S.o_within = 0;                           // the result starts over
            uint64_t tail = 0;
            for (bool last = false; !last;) {
                void *col[DHTS_BEDGRAPH_COL_COUNT]; int64_t n = 0;
                if (bedgraph_page(c, page_rows, (1u << DHTS_BEDGRAPH_COL_COUNT) - 1u, col, &n, &last)) return EXPORT_ERR;
                RtxCols a; memset(&a, 0, sizeof(a));
                a.names = (const uint8_t *)S.x_names.p; a.name_off = (const uint32_t *)S.x_noff.p; a.n_names = (uint32_t)c->ref_name.size(); a.k = 3;
                a.name_id = (const int32_t *)col[DHTS_BEDGRAPH_CHROM];
                a.col[0] = col[DHTS_BEDGRAPH_START]; a.width[0] = 8; a.col[1] = col[DHTS_BEDGRAPH_END]; a.width[1] = 8; a.col[2] = col[DHTS_BEDGRAPH_DEPTH]; a.width[2] = 4;
                a.n = (unsigned long long)n;
                uint64_t total = 0;
                if (rows_text_encode(c, a, S.x_off, S.part, nullptr, c->z_in, tail, &total, S.x_form)) return EXPORT_ERR;
                n_rows += (uint64_t)n; bytes_text += total;
                const uint64_t have = tail + total, whole = have / DFL_IN * DFL_IN;
                if (whole) {
                    if (const int e = export_compress(c, o, (const uint8_t *)c->z_in.p, whole, level, chunk_blocks)) return e;
                    tail = have - whole;                             // (shorter than a block, and the blocks in front of it are longer: the copy does not overlap)
                    if (tail) HIPCHK(c, hipMemcpyAsync(c->z_in.p, (const uint8_t *)c->z_in.p + whole, tail, hipMemcpyDeviceToDevice, c->stream));
                } else tail = have;
            }
            if (tail) {
                HIPCHK(c, hipMemsetAsync((uint8_t *)c->z_in.p + tail, 0, PAD_BYTES, c->stream));
                if (const int e = export_compress(c, o, (const uint8_t *)c->z_in.p, tail, level, chunk_blocks)) return e;
            }
            if (fwrite(BGZF_EOF_BLOCK, 1, 28, o.f) != 28) { fail(c, "bam_bedgraph_export: write error: %s", strerror(errno)); return EXPORT_ERR_WRITE; }
            o.written += 28;
            return 0;
        };
        rc = body();
        if (rc && c->err.compare(0, 20, "bam_bedgraph_export:") != 0 && c->err.compare(0, 13, "bam_bedgraph:") != 0) { const std::string m = c->err; fail(c, "bam_bedgraph_export: device error: %s", m.c_str()); }
        FILE *f = o.f; o.f = nullptr;
        if (fclose(f) != 0 && rc == 0) { rc = EXPORT_ERR_WRITE; fail(c, "bam_bedgraph_export: write error: %s", strerror(errno)); }
        bytes_out = o.written;
    }
    S.o_next = 0; S.o_within = 0;                                   // as after an accumulate: the next dhts_bam_bedgraph_next returns page one
    if (rc == 0 && p->index) rc = export_index(c, out_path, index_path, p->index == 1 ? 0 : (p->min_shift > 0 ? p->min_shift : 14), &bytes_index);
    if (rc) { unlink(out_path); if (p->index) unlink(index_path.c_str()); return rc; }
    out->n_rows = n_rows; out->bytes_text = bytes_text; out->bytes_out = (uint64_t)bytes_out; out->bytes_index = bytes_index; out->status = S.status;
    timing_collect(c);
    return 0;
}
