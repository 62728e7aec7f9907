// dhts_text_lines.inc -- part of dhts_api.hip (included there, inside its extern "C" block; not a translation unit of its own):
// the line table the text readers share (DESIGN.md 4s).  A text u[0, ulen) whose first line starts at t0 is cut into lines: newlines per
// 4 KiB chunk, a scan of the counts, every newline's successor at its rank (vcf_line_count / vcf_line_fill; with a tab part bed_delim_count /
// bed_delim_fill, which also give the tabs).  The host tail reads back where the last partial line starts, takes an unterminated last line
// when the caller says it counts, and drops the lines that start at or behind `lim`.  Line i is u[line_off[i], line_off[i + 1] - 1).

// the start of the scan's first line inside its first batch (0 in every later batch); false: it lies in front of the batch, which the
// caller reports as its own internal error
static bool first_line_t0(const dhts_ctx *c, uint64_t out_base, uint64_t &t0) {
    t0 = 0;
    if (!c->first_batch) return true;
    if (c->scan_first_uoff < out_base) return false;
    t0 = c->scan_first_uoff - out_base;
    return true;
}

// the start of line `i` of the last table in L (a record that is refused ends the scan in front of its line), and the
// first n starts on the host
static int line_start(dhts_ctx *c, const LineBufs &L, int64_t i, uint64_t &off) {
    uint32_t w = 0; HIPCHK(c, hipMemcpy(&w, (const uint32_t *)L.line_off.p + i, 4, hipMemcpyDeviceToHost)); off = w; return 0;
}
static int line_starts_fetch(dhts_ctx *c, const LineBufs &L, uint64_t n, std::vector<uint32_t> &v) {
    v.resize((size_t)n);
    if (n) HIPCHK(c, hipMemcpy(v.data(), L.line_off.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
}

struct LineTab {
    uint64_t nl = 0, ntabs = 0;         // newlines (and, with a tab part, tabs) at or behind t0
    int64_t nlines = 0;                 // the table's lines: the terminated ones, the open last line when it is taken, less those cut at lim
    uint64_t last_start = 0;            // where the text behind the last newline starts (line_off[nl])
    uint64_t carry_start = 0;           // the text offset behind the table's lines (lines_end): what the next batch carries starts here
    int last_open = 0;                  // the last of the nlines has no newline: it ends at ulen, and line_off[nl + 1] = ulen + 1 says so
    bool finished = false;              // a line starts at or behind lim, or the carry does: the scan range ends in this text
};
// timer: the kernel_times slot the two launches are timed in, < 0 for none
static int line_table(dhts_ctx *c, LineBufs &L, TabBufs *tabs, const uint8_t *u, uint64_t t0, uint64_t ulen, bool open_last_ok, uint64_t lim, int timer, LineTab &T) {
    T = LineTab(); T.last_start = T.carry_start = t0 < ulen ? t0 : ulen;
    if (t0 >= ulen) return 0;
    const int64_t nchunks = (int64_t)((ulen - (t0 & ~(uint64_t)15) + VCF_CHUNK - 1) / VCF_CHUNK);
    ENSURE(c, L.cnt, (size_t)nchunks * 4 + 64); ENSURE(c, L.base, (size_t)(nchunks + 1) * 4 + 64);
    if (tabs) { ENSURE(c, tabs->cnt, (size_t)nchunks * 4 + 64); ENSURE(c, tabs->base, (size_t)(nchunks + 1) * 4 + 64); }
    uint64_t tot[2] = {0, 0};
    {
        KTimer tm(c, timer);
        if (tabs) hipLaunchKernelGGL(bed_delim_count, dim3((unsigned)nchunks), dim3(256), 0, c->stream, u, t0, ulen, (uint32_t *)L.cnt.p, (uint32_t *)tabs->cnt.p);
        else hipLaunchKernelGGL(vcf_line_count, dim3((unsigned)nchunks), dim3(256), 0, c->stream, u, t0, ulen, (uint32_t *)L.cnt.p, nchunks);
        const uint32_t *kin[2] = {(const uint32_t *)L.cnt.p, tabs ? (const uint32_t *)tabs->cnt.p : nullptr}; uint32_t *kout[2] = {(uint32_t *)L.base.p, tabs ? (uint32_t *)tabs->base.p : nullptr};
        if (run_scan(c, tabs ? 2 : 1, kin, kout, nullptr, nchunks, tot)) return -1;
    }
    const uint64_t nl = tot[0], ntabs = tot[1];
    if (nl + 2 >= (1ull << 32)) return fail(c, "batch too large");
    ENSURE(c, L.line_off, (size_t)(nl + 2) * 4 + 64);
    if (tabs) {
        ENSURE(c, tabs->tab0, (size_t)(nl + 2) * 4 + 64); ENSURE(c, tabs->has_nul, (size_t)(nl + 2) * 4 + 64); ENSURE(c, tabs->tab_off, (size_t)(ntabs + 1) * 4 + 64);
        HIPCHK(c, hipMemsetAsync(tabs->has_nul.p, 0, (size_t)(nl + 2) * 4, c->stream));
    }
    {
        KTimer tm(c, timer);
        if (tabs) hipLaunchKernelGGL(bed_delim_fill, dim3((unsigned)nchunks), dim3(256), 0, c->stream, u, t0, ulen, (const uint32_t *)L.base.p, (const uint32_t *)tabs->base.p,
                                     (uint32_t *)L.line_off.p, (uint32_t *)tabs->tab_off.p, (uint32_t *)tabs->tab0.p, (uint32_t *)tabs->has_nul.p, (uint32_t)(nl + 2));
        else hipLaunchKernelGGL(vcf_line_fill, dim3((unsigned)nchunks), dim3(256), 0, c->stream, u, t0, ulen, (const uint32_t *)L.base.p, (uint32_t *)L.line_off.p, nchunks);
    }
    uint32_t last_start = 0;
    HIPCHK(c, hipMemcpyAsync(&last_start, (const uint32_t *)L.line_off.p + nl, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    T.nl = nl; T.ntabs = ntabs; T.nlines = (int64_t)nl; T.last_start = T.carry_start = last_start;
    if (open_last_ok && last_start < ulen) {                                    // a last line without a newline is a line
        const uint32_t end1 = (uint32_t)ulen + 1, nt32 = (uint32_t)ntabs;       // (line i ends at line_off[i + 1] - 1)
        HIPCHK(c, hipMemcpy((uint32_t *)L.line_off.p + nl + 1, &end1, 4, hipMemcpyHostToDevice));
        if (tabs) HIPCHK(c, hipMemcpy((uint32_t *)tabs->tab0.p + nl + 1, &nt32, 4, hipMemcpyHostToDevice));
        T.nlines++; T.last_open = 1; T.carry_start = ulen;
    }
    if (lim < ulen) {                                                           // lines that start at or behind lim are not this range's
        std::vector<uint32_t> lo_;
        if (line_starts_fetch(c, L, nl + 1, lo_)) return -1;
        int64_t lo = 0, hi = T.nlines;                                          // first line that starts at or behind lim
        while (lo < hi) { const int64_t mid = (lo + hi) / 2; if (lo_[(size_t)mid] < lim) lo = mid + 1; else hi = mid; }
        if (lo < T.nlines) { T.finished = true; T.carry_start = lo_[(size_t)lo]; T.nlines = lo; T.last_open = 0; }
        else if (T.carry_start >= lim) T.finished = true;
    }
    return 0;
}

// test hook (include/duckhts_amd_debug.h): line_table alone on a host text, staged with the 64 zero bytes behind it, in buffers of its own
int dhts_debug_line_table(dhts_ctx *c, const uint8_t *text, uint64_t n, uint64_t t0, int open_last_ok, uint64_t lim, int with_tabs, uint64_t out[7],
                          uint32_t *line_off, uint32_t *tab_off, uint32_t *tab0, uint32_t *has_nul) {
    if (!c) return -1;
    if (!out || !line_off || (n && !text) || n >= 0xfffffff0ull || (with_tabs && (!tab_off || !tab0 || !has_nul))) return fail(c, "debug_line_table: arguments out of range");
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf d_text; LineBufs L; TabBufs tb;
    ENSURE(c, d_text, n + 64);
    if (n) HIPCHK(c, hipMemcpyAsync(d_text.p, text, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync((uint8_t *)d_text.p + n, 0, 64, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    LineTab T;
    if (line_table(c, L, with_tabs ? &tb : nullptr, (const uint8_t *)d_text.p, t0, n, open_last_ok != 0, lim, -1, T)) return -1;
    const uint64_t w[7] = {T.nl, T.ntabs, (uint64_t)T.nlines, T.last_start, T.carry_start, (uint64_t)T.last_open, T.finished ? 1u : 0u};
    memcpy(out, w, sizeof(w));
    if (t0 >= n) return 0;                                                      // (no line starts in the text: no table was made)
    const size_t nw = (size_t)T.nlines + 1;
    HIPCHK(c, hipMemcpy(line_off, L.line_off.p, nw * 4, hipMemcpyDeviceToHost));
    if (with_tabs) {
        HIPCHK(c, hipMemcpy(tab0, tb.tab0.p, nw * 4, hipMemcpyDeviceToHost));
        if (T.nlines) HIPCHK(c, hipMemcpy(has_nul, tb.has_nul.p, (size_t)T.nlines * 4, hipMemcpyDeviceToHost));
        if (T.ntabs) HIPCHK(c, hipMemcpy(tab_off, tb.tab_off.p, (size_t)T.ntabs * 4, hipMemcpyDeviceToHost));
    }
    return 0;
}
