// dhts_interval_nearest.inc -- part of dhts_api.hip (included there behind dhts_interval.inc, inside its extern "C" block; not a translation unit
// of its own): interval_nearest (the contract: include/duckhts_amd.h, "interval nearest"; the kernels: interval_nearest.hip; DESIGN.md 4u).
// dhts_ivl_nearest_open builds the right context's end order when it has none, selects every left row's count, D and tie quota with binary
// searches alone and takes the carry of the counts; dhts_ivl_nearest_next writes a page of whole left rows.  The table, the sort, the index, the
// page cut and the read-back are dhts_interval.inc's.
enum { IVL_MS_END_ORDER = 6, IVL_MS_SELECT = 7, IVL_MS_NEAR_WRITE = 8 };

// the ends of the right file's valid rows in (rank, end) order: the pairs, the index's sort, one gather.  The sort's buffers are free once the
// index is built; what dhts_ivl_stats_get reports of the start sort is kept
static int ivl_build_end_order(dhts_ctx *r) {
    IvlState &R = r->ivl;
    const uint64_t n = R.n_rows, m = R.n_valid;
    const int32_t passes = R.sort_passes;
    double pass_ms[IVL_SORT_MAX_PASSES];
    for (int p = 0; p < IVL_SORT_MAX_PASSES; p++) pass_ms[p] = R.ms[IVL_MS_PASS0 + p];
    IvlClock clk(r);
    ENSURE(r, R.e_end, (size_t)m * 8 + 64);
    if (n) hipLaunchKernelGGL(ivl_end_input, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, r->stream, (const long long *)R.end.p, (const uint32_t *)R.vpos.p, n,
                              (unsigned long long *)R.key[0].p, (uint32_t *)R.row[0].p);
    HIPCHK(r, hipGetLastError());
    const int cur = ivl_sort(r, R, m);
    R.end_sort_passes = R.sort_passes; R.sort_passes = passes;
    for (int p = 0; p < IVL_SORT_MAX_PASSES; p++) R.ms[IVL_MS_PASS0 + p] = pass_ms[p];
    if (cur < 0) return -1;
    if (m) hipLaunchKernelGGL(ivl_end_gather, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, r->stream, (const uint32_t *)R.row[cur].p, (const long long *)R.end.p, m, (long long *)R.e_end.p);
    HIPCHK(r, hipGetLastError());
    R.ms[IVL_MS_END_ORDER] = clk.stop();
    R.end_ready = true;
    return 0;
}

static void ivl_nearest_args(const IvlState &L, const IvlState &R, IvlNearest &a) {
    memset(&a, 0, sizeof(a));
    a.R.beg = (const long long *)R.s_beg.p; a.R.end = (const long long *)R.s_end.p; a.R.pmax = (const long long *)R.pmax.p; a.R.bmax = (const long long *)R.bmax.p;
    a.R.id = (const uint32_t *)R.s_id.p; a.R.rank_first = (const uint32_t *)R.rank_first.p; a.e_end = (const long long *)R.e_end.p;
    a.k = L.near_k; a.max_distance = L.near_max_distance; a.ties = L.near_ties;
    a.name_id = (const int32_t *)L.name_id.p; a.start = (const long long *)L.start.p; a.end = (const long long *)L.end.p; a.vpos = (const uint32_t *)L.vpos.p;
    a.rank_of_left = (const int32_t *)L.rank_of_left.p;
}
int dhts_ivl_nearest_open(dhts_ctx *c, dhts_ctx *r, int64_t k, int64_t max_distance, int32_t ties) {
    if (!c) return -1;
    IvlState &S = c->ivl;
    S.near_open = false; S.right = nullptr;
    if (c->ivl.too_many) return fail(c, "interval_nearest: more than 4294967279 rows");
    if (!c->ivl.loaded) return fail(c, "interval_nearest: dhts_ivl_load not called");
    HIPCHK(c, hipSetDevice(c->device));
    if (!r) return fail(c, "interval_nearest: no right context");
    if (r->device != c->device) return fail(c, "interval_nearest: the two contexts have to be on one device");
    if (r->ivl.too_many) return fail(c, "interval_nearest: more than 4294967279 rows");
    if (!r->ivl.loaded) return fail(c, "interval_nearest: dhts_ivl_load not called on the right context");
    if (k < 1 || k > DHTS_IVL_MAX_K) return fail(c, "interval_nearest: k must be between 1 and 1048576");
    if (max_distance < -1) return fail(c, "interval_nearest: max_distance must not be negative");
    if (ties != DHTS_IVL_TIES_ALL && ties != DHTS_IVL_TIES_FIRST) return fail(c, "interval_nearest: ties must be 'all' or 'first'");
    S.ms[IVL_MS_END_ORDER] = 0;
    if (!r->ivl.end_ready) {
        if (ivl_build_end_order(r)) return fail(c, "interval_nearest: the end order of the right context failed: %s", dhts_error(r));
        S.ms[IVL_MS_END_ORDER] = r->ivl.ms[IVL_MS_END_ORDER];
    }
    HIPCHK(c, hipStreamSynchronize(r->stream));                                 // (the right index is read on this context's stream)
    const IvlState &R = r->ivl;
    const size_t nch = S.names.size();
    std::vector<int32_t> rl(nch, -1);                                           // the right rank of every left name
    for (size_t i = 0; i < nch; i++) { auto it = R.id_of.find(S.names[i]); if (it != R.id_of.end()) rl[i] = (int32_t)R.rank_of[(size_t)it->second]; }
    ENSURE(c, S.rank_of_left, nch * 4 + 64);
    if (nch) HIPCHK(c, hipMemcpy(S.rank_of_left.p, rl.data(), nch * 4, hipMemcpyHostToDevice));
    S.near_k = k; S.near_max_distance = max_distance; S.near_ties = ties;
    const uint64_t n = S.n_rows;
    unsigned long long pairs = 0, unmatched = 0;
    ENSURE(c, S.cnt, ((size_t)n + 1) * 8 + 64); ENSURE(c, S.near_dist, ((size_t)n + 1) * 8 + 64); ENSURE(c, S.near_quota, ((size_t)n + 1) * 4 + 64); ENSURE(c, S.cut, 64);
    unsigned long long *ctr = (unsigned long long *)S.ctr.p + 2;               // (ctr[0], ctr[1]: the load's)
    HIPCHK(c, hipMemsetAsync(ctr, 0, 8, c->stream));
    IvlClock clk(c);
    if (n) {
        IvlNearest a; ivl_nearest_args(S, R, a);
        a.i0 = 0; a.n = n; a.cnt = (unsigned long long *)S.cnt.p; a.dist = (long long *)S.near_dist.p; a.quota = (uint32_t *)S.near_quota.p; a.n_unmatched = ctr;
        hipLaunchKernelGGL(ivl_nearest_cells<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, a);
        if (depth_carry<unsigned long long>(c, S.part, (unsigned long long *)S.cnt.p, n)) return -1;
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&pairs, (const unsigned long long *)S.cnt.p + n, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&unmatched, ctr, 8, hipMemcpyDeviceToHost, c->stream));
    }
    S.ms[IVL_MS_SELECT] = clk.stop();
    HIPCHK(c, hipStreamSynchronize(c->stream));
    S.ms[IVL_MS_NEAR_WRITE] = 0;
    S.near_pairs = pairs; S.near_unmatched = unmatched; S.cursor = 0; S.right = r; S.merge_open = S.ov_open = false; S.near_open = true;
    return 0;
}
int dhts_ivl_nearest_next(dhts_ctx *c, int64_t max_rows, uint32_t colmask, dhts_ivl_batch *out) {
    if (!c || !out) return -1;
    memset(out, 0, sizeof(*out));
    IvlState &S = c->ivl;
    if (c->ivl.too_many) return fail(c, "interval_nearest: more than 4294967279 rows");
    if (!c->ivl.loaded) return fail(c, "interval_nearest: dhts_ivl_load not called");
    HIPCHK(c, hipSetDevice(c->device));
    if (!S.near_open || !S.right) return fail(c, "interval_nearest: dhts_ivl_nearest_open not called");
    if (!S.right->ivl.loaded || !S.right->ivl.end_ready) return fail(c, "interval_nearest: the right context was loaded anew or closed since dhts_ivl_nearest_open");
    if (max_rows <= 0) max_rows = IVL_DEFAULT_ROWS;
    colmask &= (1u << DHTS_IVL_NEAR_COL_COUNT) - 1u;
    cols_reset(S.cols, DHTS_IVL_NEAR_COL_COUNT);
    out->n_cols = DHTS_IVL_NEAR_COL_COUNT; out->cols = S.cols.data();
    const uint64_t n = S.n_rows, i0 = S.cursor;
    unsigned long long cut[3] = {i0, 0, 0};
    if (i0 < n) {                                                               // where the page ends: a search in the offsets on the device
        hipLaunchKernelGGL(ivl_page_cut, dim3(1), dim3(64), 0, c->stream, (const unsigned long long *)S.cnt.p, (unsigned long long)n, (unsigned long long)i0, (unsigned long long)max_rows, (unsigned long long *)S.cut.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(cut, S.cut.p, sizeof(cut), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (cut[0] <= i0 || cut[0] > n || cut[2] < cut[1]) return fail(c, "interval_nearest: internal error: the cut of a page is out of range");
    }
    const uint64_t i1 = cut[0], nrows = cut[2] - cut[1];
    void *dst[DHTS_IVL_NEAR_COL_COUNT];
    if (ivl_page_cols(c, S, DHTS_IVL_NEAR_COL_COUNT, colmask, nrows, dst)) return -1;
    if (nrows && colmask) {
        IvlNearest a; ivl_nearest_args(S, S.right->ivl, a);
        a.i0 = i0; a.n = i1 - i0; a.off = (const unsigned long long *)S.cnt.p; a.off0 = cut[1]; a.dist = (long long *)S.near_dist.p; a.quota = (uint32_t *)S.near_quota.p;
        a.out_chrom = (int32_t *)dst[DHTS_IVL_NEAR_CHROM]; a.out_start = (long long *)dst[DHTS_IVL_NEAR_START]; a.out_end = (long long *)dst[DHTS_IVL_NEAR_END]; a.out_lrow = (long long *)dst[DHTS_IVL_NEAR_LEFT_ROW];
        a.out_rstart = (long long *)dst[DHTS_IVL_NEAR_RIGHT_START]; a.out_rend = (long long *)dst[DHTS_IVL_NEAR_RIGHT_END]; a.out_rrow = (long long *)dst[DHTS_IVL_NEAR_RIGHT_ROW];
        a.out_ov = (long long *)dst[DHTS_IVL_NEAR_OVERLAP]; a.out_dist = (long long *)dst[DHTS_IVL_NEAR_DISTANCE];
        IvlClock clk(c);
        hipLaunchKernelGGL(ivl_nearest_cells<true>, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, c->stream, a);
        HIPCHK(c, hipGetLastError());
        S.ms[IVL_MS_NEAR_WRITE] += clk.stop();
    }
    S.cursor = i1;
    out->n_rows = (int64_t)nrows;
    for (int i = 0; i < DHTS_IVL_NEAR_COL_COUNT; i++) S.cols[(size_t)i].fixed = dst[i];
    out->status = i1 >= n ? 1 : 0;
    return 0;
}
int dhts_ivl_nearest_stats_get(dhts_ctx *c, dhts_ivl_nearest_stats *out) {
    if (!c || !out) return c ? fail(c, "interval_nearest: no stats") : -1;
    memset(out, 0, sizeof(*out));
    const IvlState &S = c->ivl;
    if (!S.loaded && !S.too_many) return fail(c, "interval_nearest: dhts_ivl_load not called");
    if (!S.near_open || !S.right) return fail(c, "interval_nearest: dhts_ivl_nearest_open not called");
    out->n_pairs = S.near_pairs; out->n_unmatched = S.near_unmatched; out->end_sort_passes = (uint32_t)S.right->ivl.end_sort_passes; out->status = S.status;
    return 0;
}
