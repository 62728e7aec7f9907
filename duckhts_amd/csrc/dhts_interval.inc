// dhts_interval.inc -- part of dhts_api.hip (included there behind dhts_bam_depth_hist.inc, inside its extern "C" block; not a translation unit
// of its own): interval_merge and interval_overlap (the contract: include/duckhts_amd.h; the kernels: interval_sort.hip, interval_algebra.hip;
// DESIGN.md 4t).  dhts_ivl_load reads a BED context to its end -- line table, bed_intervals, the heads of name runs to the host, the rows
// appended to the table in HBM --, sorts the valid rows on the device and builds the index.  dhts_ivl_merge_open flags and numbers the runs,
// dhts_ivl_overlap_open counts every left row's pairs against the right context's index; the *_next calls write a page of the result.
#define IVL_DEFAULT_ROWS (1ll << 20)
#define IVL_MAX_ROWS 0xfffffff0ull           /* a file has fewer rows than this */
enum { IVL_MS_LOAD = 0, IVL_MS_SORT, IVL_MS_INDEX, IVL_MS_MERGE, IVL_MS_COUNT, IVL_MS_WRITE, IVL_MS_PASS0 = 16 };
static int ivl_col_kind(int col) { return col == 0 ? 4 : 8; }      // chrom is the int32 name id in both results, every other column an int64

// device time between two points of the context's stream, added to S.ms[what] by stop() (which waits for the stream)
struct IvlClock {
    dhts_ctx *c; hipEvent_t a = nullptr, b = nullptr;
    explicit IvlClock(dhts_ctx *c_) : c(c_) { a = ev_get(c); b = ev_get(c); (void)hipEventRecord(a, c->stream); }
    double stop() { float ms = 0; (void)hipEventRecord(b, c->stream); (void)hipEventSynchronize(b); (void)hipEventElapsedTime(&ms, a, b); return ms; }
    ~IvlClock() { c->ev_pool.push_back(a); c->ev_pool.push_back(b); }
};

// ---- the sort: S.key[0] / S.row[0] hold m pairs, S.rank_row every row's rank.  Returns the buffer (0 / 1) the sorted pairs lie in, < 0 on failure
static int ivl_sort(dhts_ctx *c, IvlState &S, uint64_t m) {
    S.sort_passes = 0;
    for (int p = 0; p < IVL_SORT_MAX_PASSES; p++) S.ms[IVL_MS_PASS0 + p] = 0;
    if (m == 0) return 0;
    const uint32_t ntiles = (uint32_t)((m + IVL_SORT_TILE - 1) / IVL_SORT_TILE);
    const uint64_t ncounts = 256ull * ntiles;
    ENSURE(c, S.bits, 64); ENSURE(c, S.counts, (size_t)(ncounts + 1) * 4 + 64);
    unsigned long long bits[4] = {0ull, ~0ull, 0ull, ~0ull};
    HIPCHK(c, hipMemcpyAsync(S.bits.p, bits, sizeof(bits), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(ivl_sort_bits, dim3(ntiles), dim3(256), 0, c->stream, (const unsigned long long *)S.key[0].p, (const uint32_t *)S.row[0].p, (const uint32_t *)S.rank_row.p, m, (unsigned long long *)S.bits.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(bits, S.bits.p, sizeof(bits), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const unsigned long long dk = bits[0] ^ bits[1], dr = (bits[2] ^ bits[3]) & 0xffffffffull;      // the bits in which the keys / the ranks differ
    int cur = 0;
    std::vector<hipEvent_t> ev; std::vector<int> ev_pass;
    ev.push_back(ev_get(c)); (void)hipEventRecord(ev.back(), c->stream);
    for (int p = 0; p < IVL_SORT_MAX_PASSES; p++) {
        const bool by_rank = p >= IVL_SORT_KEY_PASSES;
        const uint32_t shift = 8u * (uint32_t)(by_rank ? p - IVL_SORT_KEY_PASSES : p);
        if (!(((by_rank ? dr : dk) >> shift) & 255ull)) continue;               // the digit is the same in every pair: the pass would move nothing
        const unsigned long long *ki = (const unsigned long long *)S.key[cur].p; const uint32_t *ri = (const uint32_t *)S.row[cur].p, *rk = (const uint32_t *)S.rank_row.p;
        unsigned long long *ko = (unsigned long long *)S.key[cur ^ 1].p; uint32_t *ro = (uint32_t *)S.row[cur ^ 1].p;
        if (by_rank) hipLaunchKernelGGL(ivl_sort_count<true>, dim3(ntiles), dim3(256), 0, c->stream, ki, ri, rk, m, shift, ntiles, (uint32_t *)S.counts.p);
        else hipLaunchKernelGGL(ivl_sort_count<false>, dim3(ntiles), dim3(256), 0, c->stream, ki, ri, rk, m, shift, ntiles, (uint32_t *)S.counts.p);
        if (depth_carry<uint32_t>(c, S.part, (uint32_t *)S.counts.p, ncounts)) return -1;
        if (by_rank) hipLaunchKernelGGL(ivl_sort_scatter<true>, dim3(ntiles), dim3(256), 0, c->stream, ki, ri, rk, m, shift, ntiles, (const uint32_t *)S.counts.p, ko, ro);
        else hipLaunchKernelGGL(ivl_sort_scatter<false>, dim3(ntiles), dim3(256), 0, c->stream, ki, ri, rk, m, shift, ntiles, (const uint32_t *)S.counts.p, ko, ro);
        HIPCHK(c, hipGetLastError());
        ev.push_back(ev_get(c)); (void)hipEventRecord(ev.back(), c->stream); ev_pass.push_back(p);
        cur ^= 1; S.sort_passes++;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < ev_pass.size(); k++) { float ms = 0; if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) S.ms[IVL_MS_PASS0 + ev_pass[k]] = ms; }
    for (hipEvent_t e : ev) c->ev_pool.push_back(e);
    return cur;
}

int dhts_debug_ivl_sort(dhts_ctx *c, const uint64_t *keys, const uint32_t *rank, uint64_t n, uint32_t *rows_out, int32_t *passes) {
    if (!c) return -1;
    if (n > (1ull << 28) || (n && (!keys || !rank || !rows_out))) return fail(c, "debug_ivl_sort: arguments out of range");
    HIPCHK(c, hipSetDevice(c->device));
    IvlState &S = c->ivl;
    S.loaded = S.merge_open = S.ov_open = false;                                 // (the sort's buffers are the table's)
    if (passes) *passes = 0;
    if (n == 0) return 0;
    for (int k = 0; k < 2; k++) { ENSURE(c, S.key[k], (size_t)n * 8 + 64); ENSURE(c, S.row[k], (size_t)n * 4 + 64); }
    ENSURE(c, S.rank_row, (size_t)n * 4 + 64);
    std::vector<uint32_t> iota((size_t)n);
    for (uint64_t i = 0; i < n; i++) iota[(size_t)i] = (uint32_t)i;
    HIPCHK(c, hipMemcpyAsync(S.key[0].p, keys, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(S.row[0].p, iota.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(S.rank_row.p, rank, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int cur = ivl_sort(c, S, n);
    if (cur < 0) return -1;
    HIPCHK(c, hipMemcpyAsync(rows_out, S.row[cur].p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (passes) *passes = S.sort_passes;
    return 0;
}
double dhts_debug_ivl_ms(dhts_ctx *c, int what) { return c && what >= 0 && what < 32 ? c->ivl.ms[what] : 0.0; }

// ---- load ------------------------------------------------------------------------------------------------------------------------------
// one batch of the BED context: its rows behind the table's; *status as batch_end leaves it
static int ivl_load_batch(dhts_ctx *c, int64_t max_blocks, int32_t *status) {
    IvlState &S = c->ivl; BedState &B_ = c->bed;
    Batch B;
    if (batch_begin(c, max_blocks, B)) return -1;
    uint64_t t0 = 0;
    if (!first_line_t0(c, B.out_base, t0)) return fail(c, "internal: window start in front of its first batch");
    LineTab T;
    if (line_table(c, B_.lines, nullptr, B.u, t0, B.ulen, batch_clean_end(c, B), ~0ull, DHTS_K_TILES, T)) return -1;
    const int64_t nlines = T.nlines;
    if (nlines > 0) {
        const size_t ln = (size_t)(nlines + 2) * 4 + 64;
        const unsigned lgrid = (unsigned)((nlines + 255) / 256);
        ENSURE(c, B_.tbx, (size_t)nlines * sizeof(TbxLine) + 64); ENSURE(c, S.is_row, ln); ENSURE(c, S.head, ln); ENSURE(c, S.rpos, ln); ENSURE(c, S.hpos, ln);
        const TbxLine *tl = (const TbxLine *)B_.tbx.p;
        unsigned long long first_bad = ~0ull; uint64_t tot[2] = {0, 0};
        HIPCHK(c, hipMemsetAsync(S.ctr.p, 0xff, 8, c->stream));
        hipLaunchKernelGGL(bed_intervals, dim3(lgrid), dim3(256), 0, c->stream, (const uint8_t *)B.u, (const uint32_t *)B_.lines.line_off.p, nlines, B.ulen, (int32_t)T.last_open, (TbxLine *)B_.tbx.p);
        hipLaunchKernelGGL(ivl_lines, dim3(lgrid), dim3(256), 0, c->stream, tl, (uint32_t)nlines, (uint32_t *)S.is_row.p, (uint32_t *)S.head.p, (unsigned long long *)S.ctr.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&first_bad, S.ctr.p, 8, hipMemcpyDeviceToHost, c->stream));
        const uint32_t *kin[2] = {(const uint32_t *)S.is_row.p, (const uint32_t *)S.head.p}; uint32_t *kout[2] = {(uint32_t *)S.rpos.p, (uint32_t *)S.hpos.p};
        if (run_scan(c, 2, kin, kout, nullptr, nlines, tot)) return -1;         // (waits: first_bad has arrived as well)
        if (first_bad < (unsigned long long)nlines) return fail(c, "read_bed: BED line has fewer than 3 tab-delimited fields (line %lld)", (long long)(B_.lines_done + (int64_t)first_bad + 1));
        const uint64_t nrows = tot[0], nheads = tot[1];
        if (nheads) {
            // the heads' names, one after the other, to the host; the ids it gives them back to the device
            const size_t hn = (size_t)(nheads + 2) * 4 + 64;
            ENSURE(c, S.hoff, hn); ENSURE(c, S.hlen, hn); ENSURE(c, S.hdst, hn); ENSURE(c, S.head_id, hn);
            hipLaunchKernelGGL(ivl_head_meta, dim3(lgrid), dim3(256), 0, c->stream, tl, (uint32_t)nlines, (const uint32_t *)S.hpos.p, (uint32_t *)S.hoff.p, (uint32_t *)S.hlen.p);
            uint64_t nbytes = 0;
            const uint32_t *hin[1] = {(const uint32_t *)S.hlen.p}; uint32_t *hout[1] = {(uint32_t *)S.hdst.p};
            if (run_scan(c, 1, hin, hout, nullptr, (int64_t)nheads, &nbytes)) return -1;
            ENSURE(c, S.hnames, (size_t)nbytes + 64);
            hipLaunchKernelGGL(ivl_head_names, dim3((unsigned)((nheads + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t *)B.u, (uint32_t)nheads, (const uint32_t *)S.hoff.p, (const uint32_t *)S.hdst.p, (uint8_t *)S.hnames.p);
            HIPCHK(c, hipGetLastError());
            std::vector<uint32_t> dst((size_t)nheads + 1), ids((size_t)nheads); std::string bytes((size_t)nbytes, '\0');
            HIPCHK(c, hipMemcpyAsync(dst.data(), S.hdst.p, ((size_t)nheads + 1) * 4, hipMemcpyDeviceToHost, c->stream));
            if (nbytes) HIPCHK(c, hipMemcpyAsync(&bytes[0], S.hnames.p, (size_t)nbytes, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            std::string nm;
            for (uint64_t h = 0; h < nheads; h++) {                            // interned in order of first appearance
                nm.assign(bytes, dst[(size_t)h], dst[(size_t)h + 1] - dst[(size_t)h]);
                auto it = S.id_of.find(nm);
                if (it == S.id_of.end()) { it = S.id_of.emplace(nm, (int32_t)S.names.size()).first; S.names.push_back(nm); }
                ids[(size_t)h] = (uint32_t)it->second;
            }
            HIPCHK(c, hipMemcpy(S.head_id.p, ids.data(), (size_t)nheads * 4, hipMemcpyHostToDevice));
        }
        if (S.n_rows + nrows >= IVL_MAX_ROWS) { S.too_many = true; S.status = -2; *status = -2; return 0; }
        if (nrows) {
            const size_t have = (size_t)S.n_rows, need = (size_t)(S.n_rows + nrows) + 1;
            if (ensure_keep(c, S.name_id, need * 4 + 64, have * 4) || ensure_keep(c, S.start, need * 8 + 64, have * 8) || ensure_keep(c, S.end, need * 8 + 64, have * 8) ||
                ensure_keep(c, S.vpos, need * 4 + 64, have * 4)) return -1;
            IvlAppend a; memset(&a, 0, sizeof(a));
            a.t = tl; a.rpos = (const uint32_t *)S.rpos.p; a.hpos = (const uint32_t *)S.hpos.p; a.head_id = (const uint32_t *)S.head_id.p; a.nlines = (uint32_t)nlines; a.base = S.n_rows;
            a.name_id = (int32_t *)S.name_id.p; a.start = (long long *)S.start.p; a.end = (long long *)S.end.p; a.vflag = (uint32_t *)S.vpos.p; a.n_skipped = (unsigned long long *)S.ctr.p + 1;
            hipLaunchKernelGGL(ivl_append, dim3(lgrid), dim3(256), 0, c->stream, a);
            HIPCHK(c, hipGetLastError());
        }
        B_.lines_done += nlines; S.n_rows += nrows; S.n_name_runs += nheads;
    }
    return batch_end(c, B, T.carry_start, false, T.finished, status);
}

// the ranks of the names, the pairs of the valid rows, the sort and the index
static int ivl_build_index(dhts_ctx *c) {
    IvlState &S = c->ivl;
    const uint64_t n = S.n_rows; const uint32_t nch = (uint32_t)S.names.size();
    std::vector<uint32_t> order(nch);
    for (uint32_t i = 0; i < nch; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return S.names[x] < S.names[y]; });      // byte order: std::string compares as memcmp does, the shorter first
    S.rank_of.assign(nch, 0);
    for (uint32_t r = 0; r < nch; r++) S.rank_of[order[r]] = r;
    ENSURE(c, S.rank_of_id, (size_t)nch * 4 + 64); ENSURE(c, S.rank_first, ((size_t)nch + 1) * 4 + 64);
    if (nch) HIPCHK(c, hipMemcpy(S.rank_of_id.p, S.rank_of.data(), (size_t)nch * 4, hipMemcpyHostToDevice));
    uint32_t m32 = 0;
    if (n) {
        if (depth_carry<uint32_t>(c, S.part, (uint32_t *)S.vpos.p, n)) return -1;      // the validity flags become the valid rows in front of every row
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&m32, (const uint32_t *)S.vpos.p + n, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    const uint64_t m = m32;
    S.n_valid = m;
    for (int k = 0; k < 2; k++) { ENSURE(c, S.key[k], (size_t)m * 8 + 64); ENSURE(c, S.row[k], (size_t)m * 4 + 64); }
    ENSURE(c, S.rank_row, (size_t)n * 4 + 64);
    int cur = 0;
    {
        IvlClock clk(c);
        if (n) hipLaunchKernelGGL(ivl_sort_input, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const int32_t *)S.name_id.p, (const long long *)S.start.p, (const uint32_t *)S.vpos.p,
                                  (const uint32_t *)S.rank_of_id.p, n, (uint32_t *)S.rank_row.p, (unsigned long long *)S.key[0].p, (uint32_t *)S.row[0].p);
        HIPCHK(c, hipGetLastError());
        cur = ivl_sort(c, S, m);
        S.ms[IVL_MS_SORT] = clk.stop();
        if (cur < 0) return -1;
    }
    IvlClock clk(c);
    ENSURE(c, S.s_beg, (size_t)m * 8 + 64); ENSURE(c, S.s_end, (size_t)m * 8 + 64); ENSURE(c, S.s_id, (size_t)m * 4 + 64); ENSURE(c, S.s_rank, (size_t)m * 4 + 64);
    ENSURE(c, S.pair, ((size_t)m + 1) * sizeof(IvlPair) + 64); ENSURE(c, S.pmax, (size_t)m * 8 + 64); ENSURE(c, S.bmax, ((size_t)m / 64 + 1) * 8 + 64);
    IvlIndex a; memset(&a, 0, sizeof(a));
    a.row = (const uint32_t *)S.row[cur].p; a.rank_row = (const uint32_t *)S.rank_row.p; a.start = (const long long *)S.start.p; a.end = (const long long *)S.end.p; a.m = m; a.n_chroms = nch;
    a.s_beg = (long long *)S.s_beg.p; a.s_end = (long long *)S.s_end.p; a.s_id = (uint32_t *)S.s_id.p; a.s_rank = (uint32_t *)S.s_rank.p; a.rank_first = (uint32_t *)S.rank_first.p; a.pair = (IvlPair *)S.pair.p;
    hipLaunchKernelGGL(ivl_index_gather, dim3((unsigned)((m + 1 + 255) / 256)), dim3(256), 0, c->stream, a);
    if (m) {
        if (scan_carry<IvlPair, ScanMax, false>(c, S.part, (IvlPair *)S.pair.p, m, IvlPair::lowest())) return -1;
        hipLaunchKernelGGL(ivl_index_finish, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, (const IvlPair *)S.pair.p, (const long long *)S.s_end.p, (const uint32_t *)S.s_rank.p, m,
                           (long long *)S.pmax.p, (long long *)S.bmax.p);
    }
    HIPCHK(c, hipGetLastError());
    S.ms[IVL_MS_INDEX] = clk.stop();
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int dhts_ivl_load(dhts_ctx *c, int64_t max_blocks) {
    if (!c) return -1;
    IvlState &S = c->ivl;
    S.loaded = S.too_many = S.merge_open = S.ov_open = S.end_ready = S.near_open = false; S.status = 0; S.right = nullptr; S.end_sort_passes = 0;
    S.n_rows = S.n_valid = S.n_skipped = S.n_name_runs = S.n_runs = S.n_pairs = S.cursor = 0; S.sort_passes = 0;
    S.names.clear(); S.id_of.clear(); S.rank_of.clear();
    for (double &x : S.ms) x = 0;
    if (!c->bed.open) return fail(c, "dhts_ivl_load: dhts_bed_open not called");
    HIPCHK(c, hipSetDevice(c->device));
    if (dhts_bed_set_region(c, nullptr)) return -1;                              // the whole file, from its start
    ENSURE(c, S.ctr, 64);
    HIPCHK(c, hipMemsetAsync(S.ctr.p, 0, 64, c->stream));
    int32_t status = c->n_blocks > 0 ? 0 : 1;
    {
        IvlClock clk(c);
        while (status == 0 && !c->stream_done) if (ivl_load_batch(c, max_blocks, &status)) return -1;
        S.ms[IVL_MS_LOAD] = clk.stop();
    }
    if (S.too_many) return 0;
    S.status = status ? status : 1;
    unsigned long long skipped = 0;
    HIPCHK(c, hipMemcpyAsync(&skipped, (const unsigned long long *)S.ctr.p + 1, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    S.n_skipped = skipped;
    if (ivl_build_index(c)) return -1;
    S.loaded = true;
    return 0;
}

int dhts_ivl_stats_get(dhts_ctx *c, dhts_ivl_stats *out) {
    if (!c || !out) return c ? fail(c, "dhts_ivl_stats_get: no stats") : -1;
    memset(out, 0, sizeof(*out));
    const IvlState &S = c->ivl;
    if (!S.loaded && !S.too_many) return fail(c, "dhts_ivl_stats_get: dhts_ivl_load not called");
    out->n_rows = S.n_rows; out->n_skipped = S.n_skipped; out->n_chroms = S.names.size(); out->n_name_runs = S.n_name_runs;
    out->n_runs = S.merge_open ? S.n_runs : 0; out->n_pairs = S.ov_open ? S.n_pairs : 0; out->sort_passes = S.sort_passes; out->status = S.status;
    return 0;
}
const char *dhts_ivl_chrom_name(dhts_ctx *c, int32_t id, uint64_t *len) {
    if (len) *len = 0;
    if (!c || id < 0 || (size_t)id >= c->ivl.names.size()) return nullptr;
    if (len) *len = c->ivl.names[(size_t)id].size();
    return c->ivl.names[(size_t)id].data();
}

// what every open and next asks first
static int ivl_ready(dhts_ctx *c, const char *fn) {
    if (c->ivl.too_many) return fail(c, "%s: more than 4294967279 rows", fn);
    if (!c->ivl.loaded) return fail(c, "%s: dhts_ivl_load not called", fn);
    HIPCHK(c, hipSetDevice(c->device));
    return 0;
}
// a page's columns: room for nrows rows of the columns in colmask, dst[i] null for the others
static int ivl_page_cols(dhts_ctx *c, IvlState &S, int ncols, uint32_t colmask, uint64_t nrows, void **dst) {
    for (int i = 0; i < ncols; i++) {
        dst[i] = nullptr;
        if (nrows && ((colmask >> i) & 1u)) { ENSURE(c, S.out[i], (size_t)nrows * (size_t)ivl_col_kind(i) + 64); dst[i] = S.out[i].p; }
    }
    return 0;
}

// ---- merge -------------------------------------------------------------------------------------------------------------------------------
int dhts_ivl_merge_open(dhts_ctx *c, int64_t max_gap) {
    if (!c) return -1;
    IvlState &S = c->ivl;
    S.merge_open = false;
    if (ivl_ready(c, "interval_merge")) return -1;
    if (max_gap < 0 || max_gap > DHTS_IVL_MAX_GAP) return fail(c, "interval_merge: max_gap must be between 0 and 1099511627776");
    const uint64_t m = S.n_valid;
    uint32_t runs = 0;
    IvlClock clk(c);
    if (m) {
        ENSURE(c, S.hidx, ((size_t)m + 1) * 4 + 64);
        hipLaunchKernelGGL(ivl_merge_heads, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, (const long long *)S.s_beg.p, (const long long *)S.pmax.p, (const uint32_t *)S.s_rank.p, m,
                           (long long)max_gap, (uint32_t *)S.hidx.p);
        if (depth_carry<uint32_t>(c, S.part, (uint32_t *)S.hidx.p, m)) return -1;
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&runs, (const uint32_t *)S.hidx.p + m, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        ENSURE(c, S.run_head, ((size_t)runs + 1) * 4 + 64);
        hipLaunchKernelGGL(ivl_merge_runs, dim3((unsigned)((m + 1 + 255) / 256)), dim3(256), 0, c->stream, (const uint32_t *)S.hidx.p, m, (uint32_t *)S.run_head.p);
        HIPCHK(c, hipGetLastError());
    }
    S.ms[IVL_MS_MERGE] = clk.stop();
    S.n_runs = runs; S.cursor = 0; S.ov_open = S.near_open = false; S.merge_open = true;
    return 0;
}
int dhts_ivl_merge_next(dhts_ctx *c, int64_t max_rows, uint32_t colmask, dhts_ivl_batch *out) {
    if (!c || !out) return -1;
    memset(out, 0, sizeof(*out));
    IvlState &S = c->ivl;
    if (ivl_ready(c, "interval_merge")) return -1;
    if (!S.merge_open) return fail(c, "interval_merge: dhts_ivl_merge_open not called");
    if (max_rows <= 0) max_rows = IVL_DEFAULT_ROWS;
    colmask &= (1u << DHTS_IVL_MERGE_COL_COUNT) - 1u;
    cols_reset(S.cols, DHTS_IVL_MERGE_COL_COUNT);
    out->n_cols = DHTS_IVL_MERGE_COL_COUNT; out->cols = S.cols.data();
    const uint64_t r0 = S.cursor, left = S.n_runs - r0, take = left < (uint64_t)max_rows ? left : (uint64_t)max_rows;
    void *dst[DHTS_IVL_MERGE_COL_COUNT];
    if (ivl_page_cols(c, S, DHTS_IVL_MERGE_COL_COUNT, colmask, take, dst)) return -1;
    if (take && colmask) {
        IvlMergeEmit e; memset(&e, 0, sizeof(e));
        e.run_head = (const uint32_t *)S.run_head.p; e.s_id = (const uint32_t *)S.s_id.p; e.s_beg = (const long long *)S.s_beg.p; e.pmax = (const long long *)S.pmax.p; e.name_id = (const int32_t *)S.name_id.p;
        e.r0 = r0; e.n = take;
        e.out_chrom = (int32_t *)dst[DHTS_IVL_MERGE_CHROM]; e.out_start = (long long *)dst[DHTS_IVL_MERGE_START]; e.out_end = (long long *)dst[DHTS_IVL_MERGE_END]; e.out_n = (long long *)dst[DHTS_IVL_MERGE_N];
        hipLaunchKernelGGL(ivl_merge_emit, dim3((unsigned)((take + 255) / 256)), dim3(256), 0, c->stream, e);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    S.cursor = r0 + take;
    out->n_rows = (int64_t)take;
    for (int i = 0; i < DHTS_IVL_MERGE_COL_COUNT; i++) S.cols[(size_t)i].fixed = dst[i];
    out->status = S.cursor >= S.n_runs ? 1 : 0;
    return 0;
}

// ---- overlap -----------------------------------------------------------------------------------------------------------------------------
static void ivl_overlap_args(const IvlState &L, const IvlState &R, IvlOverlap &a) {
    memset(&a, 0, sizeof(a));
    a.R.beg = (const long long *)R.s_beg.p; a.R.end = (const long long *)R.s_end.p; a.R.pmax = (const long long *)R.pmax.p; a.R.bmax = (const long long *)R.bmax.p;
    a.R.id = (const uint32_t *)R.s_id.p; a.R.rank_first = (const uint32_t *)R.rank_first.p;
    a.mode = L.mode; a.name_id = (const int32_t *)L.name_id.p; a.start = (const long long *)L.start.p; a.end = (const long long *)L.end.p; a.vpos = (const uint32_t *)L.vpos.p;
    a.rank_of_left = (const int32_t *)L.rank_of_left.p;
}
int dhts_ivl_overlap_open(dhts_ctx *c, dhts_ctx *r, int32_t mode) {
    if (!c) return -1;
    IvlState &S = c->ivl;
    S.ov_open = false; S.right = nullptr;
    if (ivl_ready(c, "interval_overlap")) return -1;
    if (!r) return fail(c, "interval_overlap: no right context");
    if (r->device != c->device) return fail(c, "interval_overlap: the two contexts have to be on one device");
    if (r->ivl.too_many) return fail(c, "interval_overlap: more than 4294967279 rows");
    if (!r->ivl.loaded) return fail(c, "interval_overlap: dhts_ivl_load not called on the right context");
    if (mode != DHTS_IVL_ANY && mode != DHTS_IVL_CONTAIN && mode != DHTS_IVL_WITHIN) return fail(c, "interval_overlap: mode must be 'any', 'contain' or 'within'");
    HIPCHK(c, hipStreamSynchronize(r->stream));                                 // (the right index is read on this context's stream)
    const IvlState &R = r->ivl;
    const size_t nch = S.names.size();
    std::vector<int32_t> rl(nch, -1);                                           // the right rank of every left name: as many lookups as the left file has chroms
    for (size_t i = 0; i < nch; i++) { auto it = R.id_of.find(S.names[i]); if (it != R.id_of.end()) rl[i] = (int32_t)R.rank_of[(size_t)it->second]; }
    ENSURE(c, S.rank_of_left, nch * 4 + 64);
    if (nch) HIPCHK(c, hipMemcpy(S.rank_of_left.p, rl.data(), nch * 4, hipMemcpyHostToDevice));
    S.mode = mode;
    const uint64_t n = S.n_rows;
    unsigned long long pairs = 0;
    ENSURE(c, S.cnt, ((size_t)n + 1) * 8 + 64); ENSURE(c, S.cut, 64);
    IvlClock clk(c);
    if (n) {
        IvlOverlap a; ivl_overlap_args(S, R, a);
        a.i0 = 0; a.n = n; a.cnt = (unsigned long long *)S.cnt.p;
        hipLaunchKernelGGL(ivl_overlap_cells<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, a);
        if (depth_carry<unsigned long long>(c, S.part, (unsigned long long *)S.cnt.p, n)) return -1;
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&pairs, (const unsigned long long *)S.cnt.p + n, 8, hipMemcpyDeviceToHost, c->stream));
    }
    S.ms[IVL_MS_COUNT] = clk.stop();
    HIPCHK(c, hipStreamSynchronize(c->stream));
    S.ms[IVL_MS_WRITE] = 0;
    S.n_pairs = pairs; S.cursor = 0; S.right = r; S.merge_open = S.near_open = false; S.ov_open = true;
    return 0;
}
int dhts_ivl_overlap_next(dhts_ctx *c, int64_t max_rows, uint32_t colmask, dhts_ivl_batch *out) {
    if (!c || !out) return -1;
    memset(out, 0, sizeof(*out));
    IvlState &S = c->ivl;
    if (ivl_ready(c, "interval_overlap")) return -1;
    if (!S.ov_open || !S.right) return fail(c, "interval_overlap: dhts_ivl_overlap_open not called");
    if (!S.right->ivl.loaded) return fail(c, "interval_overlap: the right context was loaded anew or closed since dhts_ivl_overlap_open");
    if (max_rows <= 0) max_rows = IVL_DEFAULT_ROWS;
    colmask &= (1u << DHTS_IVL_OV_COL_COUNT) - 1u;
    cols_reset(S.cols, DHTS_IVL_OV_COL_COUNT);
    out->n_cols = DHTS_IVL_OV_COL_COUNT; out->cols = S.cols.data();
    const uint64_t n = S.n_rows, i0 = S.cursor;
    unsigned long long cut[3] = {i0, 0, 0};
    if (i0 < n) {                                                               // where the page ends: a search in the offsets on the device
        hipLaunchKernelGGL(ivl_page_cut, dim3(1), dim3(64), 0, c->stream, (const unsigned long long *)S.cnt.p, (unsigned long long)n, (unsigned long long)i0, (unsigned long long)max_rows, (unsigned long long *)S.cut.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(cut, S.cut.p, sizeof(cut), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (cut[0] <= i0 || cut[0] > n || cut[2] < cut[1]) return fail(c, "interval_overlap: internal error: the cut of a page is out of range");
    }
    const uint64_t i1 = cut[0], nrows = cut[2] - cut[1];
    void *dst[DHTS_IVL_OV_COL_COUNT];
    if (ivl_page_cols(c, S, DHTS_IVL_OV_COL_COUNT, colmask, nrows, dst)) return -1;
    if (nrows && colmask) {
        IvlOverlap a; ivl_overlap_args(S, S.right->ivl, a);
        a.i0 = i0; a.n = i1 - i0; a.off = (const unsigned long long *)S.cnt.p; a.off0 = cut[1];
        a.out_chrom = (int32_t *)dst[DHTS_IVL_OV_CHROM]; a.out_start = (long long *)dst[DHTS_IVL_OV_START]; a.out_end = (long long *)dst[DHTS_IVL_OV_END]; a.out_lrow = (long long *)dst[DHTS_IVL_OV_LEFT_ROW];
        a.out_rstart = (long long *)dst[DHTS_IVL_OV_RIGHT_START]; a.out_rend = (long long *)dst[DHTS_IVL_OV_RIGHT_END]; a.out_rrow = (long long *)dst[DHTS_IVL_OV_RIGHT_ROW]; a.out_ov = (long long *)dst[DHTS_IVL_OV_OVERLAP];
        IvlClock clk(c);
        hipLaunchKernelGGL(ivl_overlap_cells<true>, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, c->stream, a);
        HIPCHK(c, hipGetLastError());
        S.ms[IVL_MS_WRITE] += clk.stop();
    }
    S.cursor = i1;
    out->n_rows = (int64_t)nrows;
    for (int i = 0; i < DHTS_IVL_OV_COL_COUNT; i++) S.cols[(size_t)i].fixed = dst[i];
    out->status = i1 >= n ? 1 : 0;
    return 0;
}

// ---- read-back: out_cols[b->n_cols] = b->cols with HOST pointers into dst --------------------------------------------------------------
uint64_t dhts_ivl_batch_host_bytes(const dhts_ivl_batch *b) { return b ? cols_host_bytes(b->n_rows, b->n_cols, b->cols, ivl_col_kind) : 0; }
int dhts_ivl_batch_fetch(dhts_ctx *c, const dhts_ivl_batch *b, void *dst, uint64_t cap, dhts_col *out_cols) {
    return b ? cols_fetch(c, "interval", b->n_rows, b->n_cols, b->cols, ivl_col_kind, dst, cap, out_cols) : -1;
}
