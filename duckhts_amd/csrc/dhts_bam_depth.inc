// dhts_bam_depth.inc -- part of dhts_api.hip (included there behind dhts_bam_coverage.inc, inside its extern "C" block; not a translation unit
// of its own): bam_depth.  dhts_bam_depth_open makes the target rows -- bam_coverage's, or the merged intervals of a BED -- and hands them to
// dep_layout, the layout both functions share.  A batch is classified and added where it lies, as in bam_coverage, by the add kernel's form
// without per-row words.  The result is counted once (tile sums, their carry, the positions every tile emits, their carry, one result index per
// row to the host) and then emitted page by page: the next max_rows positions become windows of result indices (dep_page_windows), and dep_emit
// is launched on the tiles that hold each window (dep_page_tiles_of).  Those two, dep_bed_target_rows, dep_target_rows, dep_layout, dep_args,
// depth_carry, the checks in front of a batch, the scan loop, the step counters and the read-back are dhts_bam_accum.inc's.
static const uint32_t DEPTH_COLMASK = (1u << DHTS_BAM_FLAG) | (1u << DHTS_BAM_RNAME) | (1u << DHTS_BAM_POS) | (1u << DHTS_BAM_MAPQ);   // no string column
static const AccumWho DEPTH_WHO = {"bam_depth", "bam_depth: dhts_bam_depth_open not called",
                                    "bam_depth: a shard or block range of the file is not supported (the counts need the whole file on one device)"};
#define DEPTH_DEFAULT_ROWS (1ll << 20)

int dhts_bam_depth_open(dhts_ctx *c, const dhts_depth_params *p, dhts_ctx *b) {
    if (!c || !p) return c ? fail(c, "bam_depth: no parameters") : -1;
    DepthState &S = c->dpt;
    S.open = false;
    if (!c->bam_open) return fail(c, "bam_depth: dhts_bam_open not called");
    if (b && (b == c || b->device != c->device)) return fail(c, "bam_depth: the BED context has to be a second context on the BAM context's device");
    if (b && !b->bed.open) return fail(c, "bam_depth: the BED context is not open (dhts_bed_open comes first)");
    if (c->range_cut) return fail(c, "%s", DEPTH_WHO.sharded);
    BamFilterMsg m;
    if (const char *bad = bam_filter_check(m, "bam_depth", p->min_read_len, p->min_mapq, p->min_baseq, p->include_flags, p->require_flags, p->exclude_flags, true, true)) return fail(c, "%s", bad);
    if (p->include_deletions < 0 || p->include_deletions > 1) return fail(c, "bam_depth: include_deletions must be 0 or 1");
    if (p->all_positions < 0 || p->all_positions > 2) return fail(c, "bam_depth: all_positions must be between 0 and 2");
    const bool regions = c->rg_active && !c->rg_given.empty();
    if (b && regions) return fail(c, "bam_depth: a BED and regions cannot be combined (give the target rows one way)");
    // ---- the target rows, in the order they are answered in ----
    const size_t n_ref = c->ref_len.size();
    S.n_bed_skipped = 0;
    std::vector<size_t> o_given;
    if (!b) dep_target_rows(c, S, o_given);
    else if (dep_bed_target_rows(c, b, S, S.n_bed_skipped)) return -1;
    if (dep_layout(c, S, "bam_depth", o_given)) return -1;
    const size_t R = (size_t)S.n_sorted;
    ENSURE(c, S.steps, 64); ENSURE(c, S.touched, (n_ref + 1) * 4 + 64); ENSURE(c, S.row_tid, (R + 1) * 4 + 64);
    HIPCHK(c, hipMemsetAsync(S.steps.p, 0, 64, c->stream));
    HIPCHK(c, hipMemsetAsync(S.touched.p, 0, (n_ref + 1) * 4, c->stream));
    HIPCHK(c, hipMemcpyAsync(S.row_tid.p, S.s_tid.data(), (R + 1) * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    S.P = *p; S.n_ref = (int32_t)n_ref; S.status = 0; S.res_ready = false; S.n_positions = 0; S.o_next = 0; S.o_within = 0;
    S.open = true;
    return 0;
}

extern "C++" {
template <bool BQ, bool DEL> static void depth_launch_add(dhts_ctx *c, DepthState &S, const DepArgs &a, unsigned grid) {
    hipLaunchKernelGGL((bam_depth_add_nowords<BQ, DEL>), dim3(grid), dim3(256), 0, c->stream, a, (int32_t *)S.diff.p, (uint32_t *)S.touched.p, (unsigned long long *)S.steps.p);
}
}

int dhts_bam_depth_accumulate(dhts_ctx *c, const dhts_bam_batch *b) {
    if (!c || !b) return c ? fail(c, "bam_depth: no batch") : -1;
    DepthState &S = c->dpt;
    const int go = accum_batch_ok(c, DEPTH_WHO, S, b, false, "CIGAR and QUAL are read where the scan left them");
    if (go <= 0) return go;
    const int64_t n = b->n_rows;
    DepArgs a;
    if (dep_args(c, S, b, a)) return -1;
    const unsigned grid = (unsigned)((n + 255) / 256), agrid0 = (unsigned)((n + 31) / 32), agrid = agrid0 < DEP_ADD_MAX_BLOCKS ? agrid0 : DEP_ADD_MAX_BLOCKS;
    const bool bq = S.P.min_baseq > 0, del = S.P.include_deletions != 0;
    KTimer tm(c, DHTS_K_BCF_CHECK);
    if (del) hipLaunchKernelGGL(bam_depth_classify_del, dim3(grid), dim3(256), 0, c->stream, a);
    else hipLaunchKernelGGL(bam_depth_classify, dim3(grid), dim3(256), 0, c->stream, a);
    if (bq) { if (del) depth_launch_add<true, true>(c, S, a, agrid); else depth_launch_add<true, false>(c, S, a, agrid); }
    else { if (del) depth_launch_add<false, true>(c, S, a, agrid); else depth_launch_add<false, false>(c, S, a, agrid); }
    HIPCHK(c, hipGetLastError());                          // (no wait: whatever reuses the batch's buffers is queued behind these kernels)
    S.res_ready = false; S.o_next = 0; S.o_within = 0;     // a result that was being paged out starts over
    return 0;
}

int dhts_bam_depth_scan(dhts_ctx *c, int64_t max_blocks) {
    return c ? accum_scan(c, DEPTH_WHO, c->dpt.open, max_blocks, DEPTH_COLMASK, dhts_bam_depth_accumulate) : -1;
}

int dhts_bam_depth_stats(dhts_ctx *c, dhts_depth_stats *out) {
    if (!c || !out) return c ? fail(c, "bam_depth: no stats") : -1;
    memset(out, 0, sizeof(*out));
    DepthState &S = c->dpt;
    uint64_t s[DEP_N_STEPS];
    if (accum_steps(c, DEPTH_WHO, S, s, DEP_N_STEPS)) return -1;
    dep_stats_common(out, s);
    out->n_target_rows = S.o_tid.size(); out->n_bed_skipped = S.n_bed_skipped; out->table_bytes = S.slots * 4;
    out->n_positions = S.res_ready ? S.n_positions : 0; out->status = S.status;
    return 0;
}

// the count: the depth and the result index in front of every tile, and the result index in front of every sorted row on the host
static int depth_result(dhts_ctx *c) {
    DepthState &S = c->dpt;
    if (S.res_ready) return 0;
    const size_t R = (size_t)S.n_sorted; const uint64_t ntiles = S.slots / DEP_TILE;
    S.row_off.assign(R + 1, 0);
    if (R) {
        ENSURE(c, S.tsum, (size_t)(ntiles + 1) * 4 + 64); ENSURE(c, S.toff, (size_t)(ntiles + 1) * 8 + 64); ENSURE(c, S.rowres, (R + 1) * 8 + 64);
        {
            KTimer tm(c, DHTS_K_SCAN);
            hipLaunchKernelGGL(dep_tile_sum, dim3((unsigned)ntiles), dim3(256), 0, c->stream, (const int32_t *)S.diff.p, (uint32_t *)S.tsum.p);
            if (depth_carry<uint32_t>(c, S.part, (uint32_t *)S.tsum.p, ntiles)) return -1;
            hipLaunchKernelGGL(dep_tile_count, dim3((unsigned)ntiles), dim3(256), 0, c->stream, (const int32_t *)S.diff.p, (const uint32_t *)S.tsum.p, (const uint32_t *)S.tile_row.p,
                               (const unsigned long long *)S.rbase.p, (const long long *)S.rbeg.p, (const long long *)S.rend.p, (const int32_t *)S.row_tid.p, (const uint32_t *)S.touched.p,
                               (uint32_t)S.P.all_positions, (unsigned long long *)S.toff.p);
            if (depth_carry<unsigned long long>(c, S.part, (unsigned long long *)S.toff.p, ntiles)) return -1;
            hipLaunchKernelGGL(dep_row_offsets, dim3((unsigned)((R + 1 + 255) / 256)), dim3(256), 0, c->stream, (const unsigned long long *)S.toff.p, (const unsigned long long *)S.rbase.p,
                               (uint64_t)R, ntiles, (unsigned long long *)S.rowres.p);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(S.row_off.data(), S.rowres.p, (R + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    S.n_positions = S.row_off[R]; S.res_ready = true; S.o_next = 0; S.o_within = 0;
    return 0;
}

int dhts_bam_depth_next(dhts_ctx *c, int64_t max_rows, uint32_t colmask, dhts_depth_batch *out) {
    if (!c || !out) return -1;
    memset(out, 0, sizeof(*out));
    DepthState &S = c->dpt;
    if (!S.open) return fail(c, "%s", DEPTH_WHO.not_open);
    HIPCHK(c, hipSetDevice(c->device));
    if (max_rows <= 0) max_rows = DEPTH_DEFAULT_ROWS;
    if (depth_result(c)) return -1;
    DepPage pg;
    dep_page_windows(S, S, max_rows, pg);
    const int64_t nrows = (int64_t)pg.rows;
    const bool w_tid = (colmask >> DHTS_DEPTH_CHROM) & 1u, w_pos = (colmask >> DHTS_DEPTH_POS) & 1u, w_dep = (colmask >> DHTS_DEPTH_DEPTH) & 1u;
    cols_reset(S.out, DHTS_DEPTH_COL_COUNT);
    out->n_rows = nrows; out->n_cols = DHTS_DEPTH_COL_COUNT; out->cols = S.out.data();
    if (nrows > 0) {
        if (w_tid) ENSURE(c, S.out_tid, (size_t)nrows * 4 + 64);
        if (w_pos) ENSURE(c, S.out_pos, (size_t)nrows * 8 + 64);
        if (w_dep) ENSURE(c, S.out_depth, (size_t)nrows * 4 + 64);
        if (w_tid || w_pos || w_dep) {
            const uint64_t ntiles = S.slots / DEP_TILE;
            if (dep_page_tiles_of(c, "bam_depth", S, ntiles, pg)) return -1;
            KTimer tm(c, DHTS_K_SCAN);
            for (size_t w = 0; w < pg.wins.size(); w++) {
                const uint64_t t0 = pg.tiles[2 * w], t1 = pg.tiles[2 * w + 1];
                DepEmitArgs e; memset(&e, 0, sizeof(e));
                e.diff = (const int32_t *)S.diff.p; e.tcarry = (const uint32_t *)S.tsum.p; e.toff = (const unsigned long long *)S.toff.p; e.tile_row = (const uint32_t *)S.tile_row.p;
                e.rbase = (const unsigned long long *)S.rbase.p; e.rbeg = (const long long *)S.rbeg.p; e.rend = (const long long *)S.rend.p;
                e.row_tid = (const int32_t *)S.row_tid.p; e.touched = (const uint32_t *)S.touched.p; e.mode = (uint32_t)S.P.all_positions;
                e.t0 = t0; e.o_a = pg.wins[w].o_a; e.o_b = pg.wins[w].o_b; e.dst0 = pg.wins[w].dst0;
                e.out_tid = w_tid ? (int32_t *)S.out_tid.p : nullptr; e.out_pos = w_pos ? (long long *)S.out_pos.p : nullptr; e.out_depth = w_dep ? (int32_t *)S.out_depth.p : nullptr;
                hipLaunchKernelGGL(dep_emit, dim3((unsigned)(t1 - t0 + 1)), dim3(256), 0, c->stream, e);
            }
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        if (w_tid) S.out[DHTS_DEPTH_CHROM].fixed = S.out_tid.p;
        if (w_pos) S.out[DHTS_DEPTH_POS].fixed = S.out_pos.p;
        if (w_dep) S.out[DHTS_DEPTH_DEPTH].fixed = S.out_depth.p;
    }
    S.o_next = pg.o; S.o_within = pg.within;
    out->status = pg.o >= S.o_tid.size() ? 1 : 0;
    return 0;
}

// ---- read-back: out_cols[b->n_cols] = b->cols with HOST pointers into dst --------------------------------------------------------------
static int depth_col_kind(int col) { return col == DHTS_DEPTH_POS ? 8 : 4; }
uint64_t dhts_bam_depth_batch_host_bytes(const dhts_depth_batch *b) { return b ? cols_host_bytes(b->n_rows, b->n_cols, b->cols, depth_col_kind) : 0; }
int dhts_bam_depth_batch_fetch(dhts_ctx *c, const dhts_depth_batch *b, void *dst, uint64_t cap, dhts_col *out_cols) {
    return b ? cols_fetch(c, "bam_depth", b->n_rows, b->n_cols, b->cols, depth_col_kind, dst, cap, out_cols) : -1;
}
