// dhts_bam_depth_hist.inc -- part of dhts_api.hip (included there behind dhts_bam_bedgraph.inc, inside its extern "C" block; not a translation unit
// of its own): bam_depth_hist.  dhts_bam_hist_open makes bam_depth's target rows, hands them to dep_layout and puts them into groups (one per
// non-empty row in the order answered, or one per contig); a batch is classified and added by bam_depth's kernels, unchanged.  The result is not
// emitted out of the depth table: the table is read once into the histogram table (tile sums, their carry, dhi_hist), the non-empty bins of
// every group are counted and their carry goes to the host (one result index per group), and a page is a window of result indices emitted by
// the groups that hold it (dhi_emit).  Everything that carries none of the work is dhts_bam_accum.inc's.
static const AccumWho HIST_WHO = {"bam_depth_hist", "bam_depth_hist: dhts_bam_hist_open not called",
                                   "bam_depth_hist: a shard or block range of the file is not supported (the counts need the whole file on one device)"};
#define HIST_DEFAULT_ROWS (1ll << 20)
#define HIST_MAX_DEPTH_CAP 1048575
#define HIST_MAX_TABLE_BYTES (1ull << 30)
static uint64_t g_hist_max_table_bytes = HIST_MAX_TABLE_BYTES;
// tests: the most bytes the histogram table may take (0: the contract's 1 GiB)
void dhts_debug_hist_max_table_bytes(uint64_t n) { g_hist_max_table_bytes = n ? n : HIST_MAX_TABLE_BYTES; }
static int hist_col_kind(int col) { return col == DHTS_DEPTH_HIST_CHROM || col == DHTS_DEPTH_HIST_DEPTH ? 4 : 8; }
// the tiles of a workgroup's span in dhi_hist (bam_depth_hist.hip states the bound)
static uint64_t hist_span_tiles(uint64_t ntiles) {
    const uint64_t s = (ntiles + DHI_GRID_TARGET - 1) / DHI_GRID_TARGET;
    return s < DHI_SPAN_MIN_TILES ? DHI_SPAN_MIN_TILES : s;
}

int dhts_bam_hist_open(dhts_ctx *c, const dhts_depth_hist_params *p, dhts_ctx *b) {
    if (!c || !p) return c ? fail(c, "bam_depth_hist: no parameters") : -1;
    HistState &S = c->dhi;
    S.open = false;
    if (!c->bam_open) return fail(c, "bam_depth_hist: dhts_bam_open not called");
    if (b && (b == c || b->device != c->device)) return fail(c, "bam_depth_hist: the BED context has to be a second context on the BAM context's device");
    if (b && !b->bed.open) return fail(c, "bam_depth_hist: the BED context is not open (dhts_bed_open comes first)");
    if (c->range_cut) return fail(c, "%s", HIST_WHO.sharded);
    BamFilterMsg m;
    if (const char *bad = bam_filter_check(m, "bam_depth_hist", p->min_read_len, p->min_mapq, p->min_baseq, p->include_flags, p->require_flags, p->exclude_flags, true, true)) return fail(c, "%s", bad);
    if (p->include_deletions < 0 || p->include_deletions > 1) return fail(c, "bam_depth_hist: include_deletions must be 0 or 1");
    if (p->depth_cap < 1 || p->depth_cap > HIST_MAX_DEPTH_CAP) return fail(c, "bam_depth_hist: depth_cap must be between 1 and 1048575");
    if (p->per < 0 || p->per > 1) return fail(c, "bam_depth_hist: per must be 'row' or 'contig'");
    if (b && c->rg_active && !c->rg_given.empty()) return fail(c, "bam_depth_hist: a BED and regions cannot be combined (give the target rows one way)");
    // ---- the target rows, in the order they are answered in ----
    const size_t n_ref = c->ref_len.size();
    S.n_bed_skipped = 0;
    std::vector<size_t> o_given;
    if (!b) dep_target_rows(c, S, o_given);
    else if (dep_bed_target_rows(c, b, S, S.n_bed_skipped)) return -1;
    if (dep_layout(c, S, "bam_depth_hist", o_given)) return -1;
    const size_t R = (size_t)S.n_sorted;
    // ---- the groups: a non-empty row in the order answered, or the non-empty rows of a contig in header order (the sorted rows' order) ----
    std::vector<uint32_t> row_group(R + 1, 0);
    std::vector<int32_t> g_tid; std::vector<int64_t> g_beg, g_end, g_len;
    if (p->per == 0) {
        for (size_t o = 0; o < S.o_tid.size(); o++) {
            if (S.o_k[o] < 0) continue;
            row_group[(size_t)S.o_k[o]] = (uint32_t)g_tid.size();
            g_tid.push_back(S.o_tid[o]); g_beg.push_back(S.o_beg[o]); g_end.push_back(S.o_end[o]); g_len.push_back(S.o_end[o] - S.o_beg[o]);
        }
    } else {
        for (size_t k = 0; k < R; k++) {
            if (k == 0 || S.s_tid[k] != S.s_tid[k - 1]) { g_tid.push_back(S.s_tid[k]); g_beg.push_back(S.s_beg[k]); g_end.push_back(S.s_end[k]); g_len.push_back(0); }
            row_group[k] = (uint32_t)(g_tid.size() - 1);
            if (S.s_beg[k] < g_beg.back()) g_beg.back() = S.s_beg[k];
            if (S.s_end[k] > g_end.back()) g_end.back() = S.s_end[k];
            g_len.back() += S.s_end[k] - S.s_beg[k];
        }
    }
    const size_t G = g_tid.size();
    const uint64_t hist_bytes = (uint64_t)G * ((uint64_t)p->depth_cap + 1u) * 8u;
    if (hist_bytes > g_hist_max_table_bytes)
        return fail(c, "bam_depth_hist: the histogram needs %llu bytes (8 per bin of every group); at most %llu are supported (per := 'contig' or a smaller depth_cap)",
                    (unsigned long long)hist_bytes, (unsigned long long)g_hist_max_table_bytes);
    ENSURE(c, S.steps, 64); ENSURE(c, S.touched, (n_ref + 1) * 4 + 64); ENSURE(c, S.row_group, (R + 1) * 4 + 64); ENSURE(c, S.hist, (size_t)hist_bytes + 64);
    ENSURE(c, S.g_tid, (G + 1) * 4 + 64); ENSURE(c, S.g_beg, (G + 1) * 8 + 64); ENSURE(c, S.g_end, (G + 1) * 8 + 64); ENSURE(c, S.g_len, (G + 1) * 8 + 64);
    HIPCHK(c, hipMemsetAsync(S.steps.p, 0, 64, c->stream));
    HIPCHK(c, hipMemsetAsync(S.touched.p, 0, (n_ref + 1) * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(S.hist.p, 0, (size_t)hist_bytes, c->stream));
    HIPCHK(c, hipMemcpyAsync(S.row_group.p, row_group.data(), (R + 1) * 4, hipMemcpyHostToDevice, c->stream));
    if (G) {
        HIPCHK(c, hipMemcpyAsync(S.g_tid.p, g_tid.data(), G * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(S.g_beg.p, g_beg.data(), G * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(S.g_end.p, g_end.data(), G * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(S.g_len.p, g_len.data(), G * 8, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));                  // (the copies read vectors of this call)
    S.P = *p; S.n_ref = (int32_t)n_ref; S.status = 0; S.res_ready = false; S.n_groups = G; S.hist_bytes = hist_bytes; S.n_result_rows = 0; S.o_next = 0;
    S.goff.assign(G + 1, 0);
    S.open = true;
    return 0;
}

extern "C++" {
template <bool BQ, bool DEL> static void hist_launch_add(dhts_ctx *c, HistState &S, const DepArgs &a, unsigned grid) {
    hipLaunchKernelGGL((bam_depth_add_nowords<BQ, DEL>), dim3(grid), dim3(256), 0, c->stream, a, (int32_t *)S.diff.p, (uint32_t *)S.touched.p, (unsigned long long *)S.steps.p);
}
}

int dhts_bam_hist_accumulate(dhts_ctx *c, const dhts_bam_batch *b) {
    if (!c || !b) return c ? fail(c, "bam_depth_hist: no batch") : -1;
    HistState &S = c->dhi;
    const int go = accum_batch_ok(c, HIST_WHO, S, b, false, "CIGAR and QUAL are read where the scan left them");
    if (go <= 0) return go;
    const int64_t n = b->n_rows;
    DepArgs a;
    if (dep_args(c, S, b, a)) return -1;
    const unsigned grid = (unsigned)((n + 255) / 256), agrid0 = (unsigned)((n + 31) / 32), agrid = agrid0 < DEP_ADD_MAX_BLOCKS ? agrid0 : DEP_ADD_MAX_BLOCKS;
    const bool bq = S.P.min_baseq > 0, del = S.P.include_deletions != 0;
    KTimer tm(c, DHTS_K_BCF_CHECK);
    if (del) hipLaunchKernelGGL(bam_depth_classify_del, dim3(grid), dim3(256), 0, c->stream, a);
    else hipLaunchKernelGGL(bam_depth_classify, dim3(grid), dim3(256), 0, c->stream, a);
    if (bq) { if (del) hist_launch_add<true, true>(c, S, a, agrid); else hist_launch_add<true, false>(c, S, a, agrid); }
    else { if (del) hist_launch_add<false, true>(c, S, a, agrid); else hist_launch_add<false, false>(c, S, a, agrid); }
    HIPCHK(c, hipGetLastError());                          // (no wait: whatever reuses the batch's buffers is queued behind these kernels)
    S.res_ready = false; S.o_next = 0;                     // a result that was being paged out starts over: the histogram is made again from the table
    return 0;
}

int dhts_bam_hist_scan(dhts_ctx *c, int64_t max_blocks) {
    return c ? accum_scan(c, HIST_WHO, c->dhi.open, max_blocks, DEPTH_COLMASK, dhts_bam_hist_accumulate) : -1;
}

int dhts_bam_hist_stats(dhts_ctx *c, dhts_depth_hist_stats *out) {
    if (!c || !out) return c ? fail(c, "bam_depth_hist: no stats") : -1;
    memset(out, 0, sizeof(*out));
    HistState &S = c->dhi;
    uint64_t s[DEP_N_STEPS];
    if (accum_steps(c, HIST_WHO, S, s, DEP_N_STEPS)) return -1;
    dep_stats_common(out, s);
    out->n_target_rows = S.o_tid.size(); out->n_groups = S.n_groups; out->n_bed_skipped = S.n_bed_skipped; out->table_bytes = S.slots * 4; out->hist_bytes = S.hist_bytes;
    out->n_result_rows = S.res_ready ? S.n_result_rows : 0; out->status = S.status;
    return 0;
}

// the one pass over the depth table, queued: the histogram table zeroed, the depth in front of every tile, and dhi_hist on spans of tiles
static int hist_table_pass(dhts_ctx *c, HistState &S, uint64_t ntiles) {
    const uint64_t span = hist_span_tiles(ntiles), grid = (ntiles + span - 1) / span;
    if (span >= (1ull << 22) || grid > 0x7fffffffull) return fail(c, "bam_depth_hist: internal error: the spans of the table pass are out of range");
    HIPCHK(c, hipMemsetAsync(S.hist.p, 0, (size_t)S.hist_bytes, c->stream));
    hipLaunchKernelGGL(dep_tile_sum, dim3((unsigned)ntiles), dim3(256), 0, c->stream, (const int32_t *)S.diff.p, (uint32_t *)S.tsum.p);
    if (depth_carry<uint32_t>(c, S.part, (uint32_t *)S.tsum.p, ntiles)) return -1;
    hipLaunchKernelGGL(dhi_hist, dim3((unsigned)grid), dim3(256), 0, c->stream, (const int32_t *)S.diff.p, (const uint32_t *)S.tsum.p, (const uint32_t *)S.tile_row.p,
                       (const uint32_t *)S.row_group.p, (const unsigned long long *)S.rbase.p, (const long long *)S.rbeg.p, (const long long *)S.rend.p, ntiles, span,
                       (uint32_t)S.P.depth_cap, (unsigned long long *)S.hist.p);
    return 0;
}

// the histogram from the table as it is, and the result index in front of every group on the host
static int hist_result(dhts_ctx *c) {
    HistState &S = c->dhi;
    if (S.res_ready) return 0;
    const size_t G = (size_t)S.n_groups; const uint64_t ntiles = S.slots / DEP_TILE;
    S.goff.assign(G + 1, 0);
    if (G) {
        ENSURE(c, S.tsum, (size_t)(ntiles + 1) * 4 + 64); ENSURE(c, S.gcnt, (G + 1) * 8 + 64);
        {
            KTimer tm(c, DHTS_K_SCAN);
            if (hist_table_pass(c, S, ntiles)) return -1;
            hipLaunchKernelGGL(dhi_group_count, dim3((unsigned)G), dim3(256), 0, c->stream, (const unsigned long long *)S.hist.p, (uint32_t)S.P.depth_cap, (unsigned long long *)S.gcnt.p);
            if (depth_carry<unsigned long long>(c, S.part, (unsigned long long *)S.gcnt.p, G)) return -1;
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(S.goff.data(), S.gcnt.p, (G + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (size_t g = 0; g < G; g++)
            if (S.goff[g + 1] < S.goff[g] || S.goff[g + 1] - S.goff[g] > (uint64_t)S.P.depth_cap + 1u) return fail(c, "bam_depth_hist: internal error: the result indices of the groups are out of range");
    }
    S.n_result_rows = S.goff[G]; S.res_ready = true; S.o_next = 0;
    return 0;
}

int dhts_bam_hist_next(dhts_ctx *c, int64_t max_rows, uint32_t colmask, dhts_depth_hist_batch *out) {
    if (!c || !out) return -1;
    memset(out, 0, sizeof(*out));
    HistState &S = c->dhi;
    if (!S.open) return fail(c, "%s", HIST_WHO.not_open);
    HIPCHK(c, hipSetDevice(c->device));
    if (max_rows <= 0) max_rows = HIST_DEFAULT_ROWS;
    if (hist_result(c)) return -1;
    // the page: result indices [o_a, o_b), which the groups g_a .. g_b hold (the pager is the one index: the groups lie in answer order)
    const uint64_t total = S.n_result_rows, o_a = S.o_next, o_b = total - o_a < (uint64_t)max_rows ? total : o_a + (uint64_t)max_rows;
    const int64_t nrows = (int64_t)(o_b - o_a);
    DevBuf *const bufs[DHTS_DEPTH_HIST_COL_COUNT] = {&S.out_tid, &S.out_start, &S.out_end, &S.out_depth, &S.out_n, &S.out_at_least, &S.out_len};
    void *dst[DHTS_DEPTH_HIST_COL_COUNT] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    colmask &= (1u << DHTS_DEPTH_HIST_COL_COUNT) - 1u;
    cols_reset(S.out, DHTS_DEPTH_HIST_COL_COUNT);
    out->n_rows = nrows; out->n_cols = DHTS_DEPTH_HIST_COL_COUNT; out->cols = S.out.data();
    if (nrows > 0 && colmask) {
        for (int i = 0; i < DHTS_DEPTH_HIST_COL_COUNT; i++)
            if ((colmask >> i) & 1u) { ENSURE(c, *bufs[i], (size_t)nrows * (size_t)hist_col_kind(i) + 64); dst[i] = bufs[i]->p; }
        const uint64_t g_a = (uint64_t)(std::upper_bound(S.goff.begin(), S.goff.end(), o_a) - S.goff.begin()) - 1u;          // the last group that starts at or in front of o_a
        const uint64_t g_b = (uint64_t)(std::upper_bound(S.goff.begin(), S.goff.end(), o_b - 1u) - S.goff.begin()) - 1u;
        if (g_b < g_a || g_b >= S.n_groups) return fail(c, "bam_depth_hist: internal error: the groups of a page are out of range");
        {
            KTimer tm(c, DHTS_K_SCAN);
            DhiEmitArgs e; memset(&e, 0, sizeof(e));
            e.table = (const unsigned long long *)S.hist.p; e.goff = (const unsigned long long *)S.gcnt.p;
            e.g_tid = (const int32_t *)S.g_tid.p; e.g_beg = (const long long *)S.g_beg.p; e.g_end = (const long long *)S.g_end.p; e.g_len = (const long long *)S.g_len.p;
            e.cap = (uint32_t)S.P.depth_cap; e.g0 = g_a; e.o_a = o_a; e.o_b = o_b;
            e.out_tid = (int32_t *)dst[DHTS_DEPTH_HIST_CHROM]; e.out_start = (long long *)dst[DHTS_DEPTH_HIST_START]; e.out_end = (long long *)dst[DHTS_DEPTH_HIST_END];
            e.out_depth = (int32_t *)dst[DHTS_DEPTH_HIST_DEPTH]; e.out_n = (long long *)dst[DHTS_DEPTH_HIST_N_POSITIONS]; e.out_at_least = (long long *)dst[DHTS_DEPTH_HIST_N_AT_LEAST];
            e.out_len = (long long *)dst[DHTS_DEPTH_HIST_LENGTH];
            hipLaunchKernelGGL(dhi_emit, dim3((unsigned)(g_b - g_a + 1)), dim3(256), 0, c->stream, e);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int i = 0; i < DHTS_DEPTH_HIST_COL_COUNT; i++) S.out[(size_t)i].fixed = dst[i];
    }
    S.o_next = o_b;
    out->status = o_b >= total ? 1 : 0;
    return 0;
}

// tests, tools/bench_depth_hist.py: the device time in ms per launch of one pass over the open function's depth table, `reps` launches between two
// events: which 0 = dep_tile_reduce (bam_coverage's read of the table), 1 = dhi_hist.  The depth in front of every tile is made first.  The
// next dhts_bam_hist_next makes its result anew.  < 0 with dhts_error set when a call failed.
double dhts_debug_hist_pass_ms(dhts_ctx *c, int which, int reps) {
    if (!c) return -1.0;
    HistState &S = c->dhi;
    if (!S.open) { fail(c, "%s", HIST_WHO.not_open); return -1.0; }
    if (which < 0 || which > 1 || reps < 1 || !S.n_groups) { fail(c, "bam_depth_hist: nothing to time"); return -1.0; }
    if (hipSetDevice(c->device) != hipSuccess) { fail(c, "bam_depth_hist: hipSetDevice failed"); return -1.0; }
    const uint64_t ntiles = S.slots / DEP_TILE;
    if (S.scratch.ensure((size_t)ntiles * 12 + 64) || S.tsum.ensure((size_t)(ntiles + 1) * 4 + 64)) { fail(c, "bam_depth_hist: out of device memory"); return -1.0; }
    S.res_ready = false; S.o_next = 0;
    if (hist_table_pass(c, S, ntiles)) return -1.0;
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { fail(c, "bam_depth_hist: hipEventCreate failed"); return -1.0; }
    const uint64_t span = hist_span_tiles(ntiles), grid = (ntiles + span - 1) / span;
    (void)hipEventRecord(a, c->stream);
    for (int r = 0; r < reps; r++) {
        if (which == 0)
            hipLaunchKernelGGL(dep_tile_reduce, dim3((unsigned)ntiles), dim3(256), 0, c->stream, (const int32_t *)S.diff.p, (const uint32_t *)S.tsum.p, (const uint32_t *)S.tile_row.p,
                               (const unsigned long long *)S.rbase.p, (const long long *)S.rbeg.p, (const long long *)S.rend.p, 1ll, (uint32_t *)S.scratch.p,
                               (unsigned long long *)((uint8_t *)S.scratch.p + (((size_t)ntiles * 4 + 63) & ~(size_t)63)));
        else
            hipLaunchKernelGGL(dhi_hist, dim3((unsigned)grid), dim3(256), 0, c->stream, (const int32_t *)S.diff.p, (const uint32_t *)S.tsum.p, (const uint32_t *)S.tile_row.p,
                               (const uint32_t *)S.row_group.p, (const unsigned long long *)S.rbase.p, (const long long *)S.rbeg.p, (const long long *)S.rend.p, ntiles, span,
                               (uint32_t)S.P.depth_cap, (unsigned long long *)S.hist.p);
    }
    (void)hipEventRecord(b, c->stream);
    float ms = 0.f;
    const bool ok = hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&ms, a, b) == hipSuccess && hipGetLastError() == hipSuccess;
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    if (!ok) { fail(c, "bam_depth_hist: timing a pass failed"); return -1.0; }
    return (double)ms / reps;
}

// ---- read-back: out_cols[b->n_cols] = b->cols with HOST pointers into dst --------------------------------------------------------------
uint64_t dhts_bam_hist_batch_host_bytes(const dhts_depth_hist_batch *b) { return b ? cols_host_bytes(b->n_rows, b->n_cols, b->cols, hist_col_kind) : 0; }
int dhts_bam_hist_batch_fetch(dhts_ctx *c, const dhts_depth_hist_batch *b, void *dst, uint64_t cap, dhts_col *out_cols) {
    return b ? cols_fetch(c, "bam_depth_hist", b->n_rows, b->n_cols, b->cols, hist_col_kind, dst, cap, out_cols) : -1;
}
