// dhts_bam_bedgraph.inc -- part of dhts_api.hip (included there behind dhts_bam_pileup.inc, inside its extern "C" block; not a translation unit
// of its own): bam_bedgraph.  dhts_bam_bedgraph_open makes bam_depth's target rows and hands them to dep_layout; a batch is classified and added
// by bam_depth's kernels, unchanged.  The result is counted once (tile sums, their carry, the emitted boundaries and the first boundary of every
// tile, the suffix minimum of the latter, the carry of the former, one result index per row to the host) and then emitted page by page: the
// next max_rows runs become windows of result indices (dep_page_windows), and bdg_emit is launched on the tiles that hold each window
// (dep_page_tiles_of).  Everything that carries none of the work is dhts_bam_accum.inc's.
static const AccumWho BEDGRAPH_WHO = {"bam_bedgraph", "bam_bedgraph: dhts_bam_bedgraph_open not called",
                                       "bam_bedgraph: a shard or block range of the file is not supported (the counts need the whole file on one device)"};
#define BEDGRAPH_DEFAULT_ROWS (1ll << 20)
static int bedgraph_col_kind(int col) { return col == DHTS_BEDGRAPH_START || col == DHTS_BEDGRAPH_END ? 8 : 4; }

int dhts_bam_bedgraph_open(dhts_ctx *c, const dhts_bedgraph_params *p, dhts_ctx *b) {
    if (!c || !p) return c ? fail(c, "bam_bedgraph: no parameters") : -1;
    BedgraphState &S = c->bdg;
    S.open = false;
    if (!c->bam_open) return fail(c, "bam_bedgraph: dhts_bam_open not called");
    if (b && (b == c || b->device != c->device)) return fail(c, "bam_bedgraph: the BED context has to be a second context on the BAM context's device");
    if (b && !b->bed.open) return fail(c, "bam_bedgraph: the BED context is not open (dhts_bed_open comes first)");
    if (c->range_cut) return fail(c, "%s", BEDGRAPH_WHO.sharded);
    BamFilterMsg m;
    if (const char *bad = bam_filter_check(m, "bam_bedgraph", p->min_read_len, p->min_mapq, p->min_baseq, p->include_flags, p->require_flags, p->exclude_flags, true, true)) return fail(c, "%s", bad);
    if (p->zero_runs < 0 || p->zero_runs > 1) return fail(c, "bam_bedgraph: zero_runs must be 0 or 1");
    if (p->include_deletions < 0 || p->include_deletions > 1) return fail(c, "bam_bedgraph: include_deletions must be 0 or 1");
    if (p->n_breaks < 0 || p->n_breaks > (int32_t)BDG_MAX_BREAKS) return fail(c, "bam_bedgraph: at most 16 breaks are supported");
    for (int32_t j = 0; j < p->n_breaks; j++)
        if (p->breaks[j] < 1 || (j && p->breaks[j] <= p->breaks[j - 1])) return fail(c, "bam_bedgraph: breaks must be strictly increasing integers between 1 and 2147483647");
    if (b && c->rg_active && !c->rg_given.empty()) return fail(c, "bam_bedgraph: a BED and regions cannot be combined (give the target rows one way)");
    // ---- the target rows, in the order they are answered in ----
    const size_t n_ref = c->ref_len.size();
    S.n_bed_skipped = 0;
    std::vector<size_t> o_given;
    if (!b) dep_target_rows(c, S, o_given);
    else if (dep_bed_target_rows(c, b, S, S.n_bed_skipped)) return -1;
    if (dep_layout(c, S, "bam_bedgraph", o_given)) return -1;
    const size_t R = (size_t)S.n_sorted;
    ENSURE(c, S.steps, 64); ENSURE(c, S.touched, (n_ref + 1) * 4 + 64); ENSURE(c, S.row_tid, (R + 1) * 4 + 64);
    HIPCHK(c, hipMemsetAsync(S.steps.p, 0, 64, c->stream));
    HIPCHK(c, hipMemsetAsync(S.touched.p, 0, (n_ref + 1) * 4, c->stream));
    HIPCHK(c, hipMemcpyAsync(S.row_tid.p, S.s_tid.data(), (R + 1) * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    S.P = *p; S.n_ref = (int32_t)n_ref; S.status = 0; S.res_ready = false; S.n_runs = 0; S.o_next = 0; S.o_within = 0;
    S.open = true;
    return 0;
}

extern "C++" {
template <bool BQ, bool DEL> static void bedgraph_launch_add(dhts_ctx *c, BedgraphState &S, const DepArgs &a, unsigned grid) {
    hipLaunchKernelGGL((bam_depth_add_nowords<BQ, DEL>), dim3(grid), dim3(256), 0, c->stream, a, (int32_t *)S.diff.p, (uint32_t *)S.touched.p, (unsigned long long *)S.steps.p);
}
}

int dhts_bam_bedgraph_accumulate(dhts_ctx *c, const dhts_bam_batch *b) {
    if (!c || !b) return c ? fail(c, "bam_bedgraph: no batch") : -1;
    BedgraphState &S = c->bdg;
    const int go = accum_batch_ok(c, BEDGRAPH_WHO, S, b, false, "CIGAR and QUAL are read where the scan left them");
    if (go <= 0) return go;
    const int64_t n = b->n_rows;
    DepArgs a;
    if (dep_args(c, S, b, a)) return -1;
    const unsigned grid = (unsigned)((n + 255) / 256), agrid0 = (unsigned)((n + 31) / 32), agrid = agrid0 < DEP_ADD_MAX_BLOCKS ? agrid0 : DEP_ADD_MAX_BLOCKS;
    const bool bq = S.P.min_baseq > 0, del = S.P.include_deletions != 0;
    KTimer tm(c, DHTS_K_BCF_CHECK);
    if (del) hipLaunchKernelGGL(bam_depth_classify_del, dim3(grid), dim3(256), 0, c->stream, a);
    else hipLaunchKernelGGL(bam_depth_classify, dim3(grid), dim3(256), 0, c->stream, a);
    if (bq) { if (del) bedgraph_launch_add<true, true>(c, S, a, agrid); else bedgraph_launch_add<true, false>(c, S, a, agrid); }
    else { if (del) bedgraph_launch_add<false, true>(c, S, a, agrid); else bedgraph_launch_add<false, false>(c, S, a, agrid); }
    HIPCHK(c, hipGetLastError());                          // (no wait: whatever reuses the batch's buffers is queued behind these kernels)
    S.res_ready = false; S.o_next = 0; S.o_within = 0;     // a result that was being paged out starts over
    return 0;
}

int dhts_bam_bedgraph_scan(dhts_ctx *c, int64_t max_blocks) {
    return c ? accum_scan(c, BEDGRAPH_WHO, c->bdg.open, max_blocks, DEPTH_COLMASK, dhts_bam_bedgraph_accumulate) : -1;
}

int dhts_bam_bedgraph_stats(dhts_ctx *c, dhts_bedgraph_stats *out) {
    if (!c || !out) return c ? fail(c, "bam_bedgraph: no stats") : -1;
    memset(out, 0, sizeof(*out));
    BedgraphState &S = c->bdg;
    uint64_t s[DEP_N_STEPS];
    if (accum_steps(c, BEDGRAPH_WHO, S, s, DEP_N_STEPS)) return -1;
    dep_stats_common(out, s);
    out->n_target_rows = S.o_tid.size(); out->n_bed_skipped = S.n_bed_skipped; out->table_bytes = S.slots * 4;
    out->n_runs = S.res_ready ? S.n_runs : 0; out->status = S.status;
    return 0;
}

static BdgClasses bedgraph_classes(const dhts_bedgraph_params &P) {
    BdgClasses k;
    k.n = (uint32_t)P.n_breaks; k.zero_runs = (uint32_t)P.zero_runs;
    for (uint32_t j = 0; j < BDG_MAX_BREAKS; j++) k.br[j] = j < k.n ? (uint32_t)P.breaks[j] : 0u;
    return k;
}

// the count: the depth, the result index and the next boundary around every tile, and the result index in front of every sorted row on the host
static int bedgraph_result(dhts_ctx *c) {
    BedgraphState &S = c->bdg;
    if (S.res_ready) return 0;
    const size_t R = (size_t)S.n_sorted; const uint64_t ntiles = S.slots / DEP_TILE;
    S.row_off.assign(R + 1, 0);
    if (R) {
        ENSURE(c, S.tsum, (size_t)(ntiles + 1) * 4 + 64); ENSURE(c, S.toff, (size_t)(ntiles + 1) * 8 + 64); ENSURE(c, S.tnext, (size_t)(ntiles + 1) * 8 + 64);
        ENSURE(c, S.rowres, (R + 1) * 8 + 64);
        {
            KTimer tm(c, DHTS_K_SCAN);
            hipLaunchKernelGGL(dep_tile_sum, dim3((unsigned)ntiles), dim3(256), 0, c->stream, (const int32_t *)S.diff.p, (uint32_t *)S.tsum.p);
            if (depth_carry<uint32_t>(c, S.part, (uint32_t *)S.tsum.p, ntiles)) return -1;
            hipLaunchKernelGGL(bdg_tile_count, dim3((unsigned)ntiles), dim3(256), 0, c->stream, (const int32_t *)S.diff.p, (const uint32_t *)S.tsum.p, (const uint32_t *)S.tile_row.p,
                               (const unsigned long long *)S.rbase.p, (const long long *)S.rbeg.p, (const long long *)S.rend.p, bedgraph_classes(S.P), (unsigned long long)S.slots,
                               (unsigned long long *)S.toff.p, (unsigned long long *)S.tnext.p);
            // the suffix minimum in place: tnext[t] = the least tfirst behind t, `none` (the slots of the table) where there is none
            if (scan_carry<unsigned long long, ScanMin, true>(c, S.part, (unsigned long long *)S.tnext.p, ntiles, (unsigned long long)S.slots)) return -1;
            if (depth_carry<unsigned long long>(c, S.part, (unsigned long long *)S.toff.p, ntiles)) return -1;
            hipLaunchKernelGGL(dep_row_offsets, dim3((unsigned)((R + 1 + 255) / 256)), dim3(256), 0, c->stream, (const unsigned long long *)S.toff.p, (const unsigned long long *)S.rbase.p,
                               (uint64_t)R, ntiles, (unsigned long long *)S.rowres.p);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(S.row_off.data(), S.rowres.p, (R + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    S.n_runs = S.row_off[R]; S.res_ready = true; S.o_next = 0; S.o_within = 0;
    return 0;
}

// the next <= max_rows rows of the result as a page of device columns (dst[i]: null for a column colmask leaves out), emitted and waited for;
// *n_rows its rows, *last whether it ends the result.  dhts_bam_bedgraph_next hands the page out, dhts_bedgraph_export prints it
static int bedgraph_page(dhts_ctx *c, int64_t max_rows, uint32_t colmask, void *dst[DHTS_BEDGRAPH_COL_COUNT], int64_t *n_rows, bool *last) {
    BedgraphState &S = c->bdg;
    if (max_rows <= 0) max_rows = BEDGRAPH_DEFAULT_ROWS;
    if (bedgraph_result(c)) return -1;
    DepPage pg;
    dep_page_windows(S, S, max_rows, pg);
    const int64_t nrows = (int64_t)pg.rows;
    DevBuf *const bufs[DHTS_BEDGRAPH_COL_COUNT] = {&S.out_tid, &S.out_start, &S.out_end, &S.out_depth};
    for (int i = 0; i < DHTS_BEDGRAPH_COL_COUNT; i++) dst[i] = nullptr;
    if (nrows > 0 && colmask) {
        for (int i = 0; i < DHTS_BEDGRAPH_COL_COUNT; i++)
            if ((colmask >> i) & 1u) { ENSURE(c, *bufs[i], (size_t)nrows * (size_t)bedgraph_col_kind(i) + 64); dst[i] = bufs[i]->p; }
        const uint64_t ntiles = S.slots / DEP_TILE;
        if (dep_page_tiles_of(c, "bam_bedgraph", S, ntiles, pg)) return -1;
        {
            KTimer tm(c, DHTS_K_SCAN);
            for (size_t w = 0; w < pg.wins.size(); w++) {
                const uint64_t t0 = pg.tiles[2 * w], t1 = pg.tiles[2 * w + 1];
                BdgEmitArgs e; memset(&e, 0, sizeof(e));
                e.diff = (const int32_t *)S.diff.p; e.tcarry = (const uint32_t *)S.tsum.p; e.toff = (const unsigned long long *)S.toff.p; e.tnext = (const unsigned long long *)S.tnext.p;
                e.tile_row = (const uint32_t *)S.tile_row.p; e.rbase = (const unsigned long long *)S.rbase.p; e.rbeg = (const long long *)S.rbeg.p; e.rend = (const long long *)S.rend.p;
                e.row_tid = (const int32_t *)S.row_tid.p; e.c = bedgraph_classes(S.P);
                e.t0 = t0; e.o_a = pg.wins[w].o_a; e.o_b = pg.wins[w].o_b; e.dst0 = pg.wins[w].dst0;
                e.out_tid = (int32_t *)dst[DHTS_BEDGRAPH_CHROM]; e.out_start = (long long *)dst[DHTS_BEDGRAPH_START]; e.out_end = (long long *)dst[DHTS_BEDGRAPH_END];
                e.out_depth = (int32_t *)dst[DHTS_BEDGRAPH_DEPTH];
                hipLaunchKernelGGL(bdg_emit, dim3((unsigned)(t1 - t0 + 1)), dim3(256), 0, c->stream, e);
            }
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    S.o_next = pg.o; S.o_within = pg.within;
    *n_rows = nrows; *last = pg.o >= S.o_tid.size();
    return 0;
}

int dhts_bam_bedgraph_next(dhts_ctx *c, int64_t max_rows, uint32_t colmask, dhts_bedgraph_batch *out) {
    if (!c || !out) return -1;
    memset(out, 0, sizeof(*out));
    BedgraphState &S = c->bdg;
    if (!S.open) return fail(c, "%s", BEDGRAPH_WHO.not_open);
    HIPCHK(c, hipSetDevice(c->device));
    void *dst[DHTS_BEDGRAPH_COL_COUNT]; int64_t nrows = 0; bool last = false;
    colmask &= (1u << DHTS_BEDGRAPH_COL_COUNT) - 1u;
    cols_reset(S.out, DHTS_BEDGRAPH_COL_COUNT);
    out->n_cols = DHTS_BEDGRAPH_COL_COUNT; out->cols = S.out.data();
    if (bedgraph_page(c, max_rows, colmask, dst, &nrows, &last)) return -1;
    out->n_rows = nrows;
    for (int i = 0; i < DHTS_BEDGRAPH_COL_COUNT; i++) S.out[(size_t)i].fixed = dst[i];
    out->status = last ? 1 : 0;
    return 0;
}

// ---- read-back: out_cols[b->n_cols] = b->cols with HOST pointers into dst --------------------------------------------------------------
uint64_t dhts_bam_bedgraph_batch_host_bytes(const dhts_bedgraph_batch *b) { return b ? cols_host_bytes(b->n_rows, b->n_cols, b->cols, bedgraph_col_kind) : 0; }
int dhts_bam_bedgraph_batch_fetch(dhts_ctx *c, const dhts_bedgraph_batch *b, void *dst, uint64_t cap, dhts_col *out_cols) {
    return b ? cols_fetch(c, "bam_bedgraph", b->n_rows, b->n_cols, b->cols, bedgraph_col_kind, dst, cap, out_cols) : -1;
}
