// dhts_bam_depth.inc -- part of dhts_api.hip (included there behind dhts_bam_coverage.inc, inside its extern "C" block; not a translation unit
// of its own): bam_depth.  dhts_bam_depth_open makes the target rows -- bam_coverage's, or the merged intervals of a BED -- and hands them to
// dep_layout, the layout both functions share.  A batch is classified and added where it lies, as in bam_coverage, by the add kernel's form
// without per-row words.  The result is counted once (tile sums, their carry, the positions every tile emits, their carry, one result index per
// row to the host) and then emitted page by page: the host walks the rows in the order they are answered in, turns the next max_rows
// positions into windows of result indices -- one per run of rows that follow each other in both orders -- and launches dep_emit on the tiles
// that hold each window.
static const uint32_t DEPTH_COLMASK = (1u << DHTS_BAM_FLAG) | (1u << DHTS_BAM_RNAME) | (1u << DHTS_BAM_POS) | (1u << DHTS_BAM_MAPQ);   // no string column
#define DEPTH_SHARDED "bam_depth: a shard or block range of the file is not supported (the counts need the whole file on one device)"
#define DEPTH_NOT_OPEN "bam_depth: dhts_bam_depth_open not called"
#define DEPTH_DEFAULT_ROWS (1ll << 20)

int dhts_bam_depth_open(dhts_ctx *c, const dhts_depth_params *p, dhts_ctx *b) {
    if (!c || !p) return c ? fail(c, "bam_depth: no parameters") : -1;
    DepthState &S = c->dpt;
    S.open = false;
    if (!c->bam_open) return fail(c, "bam_depth: dhts_bam_open not called");
    if (b && (b == c || b->device != c->device)) return fail(c, "bam_depth: the BED context has to be a second context on the BAM context's device");
    if (b && !b->bed.open) return fail(c, "bam_depth: the BED context is not open (dhts_bed_open comes first)");
    if (c->range_cut) return fail(c, DEPTH_SHARDED);
    if (p->min_read_len < 0) return fail(c, "bam_depth: min_read_len must be >= 0");
    if (p->min_mapq < 0 || p->min_mapq > 255) return fail(c, "bam_depth: min_mapq must be between 0 and 255");
    if (p->min_baseq < 0 || p->min_baseq > 255) return fail(c, "bam_depth: min_baseq must be between 0 and 255");
    if (p->include_flags < 0 || p->include_flags > 65535) return fail(c, "bam_depth: include_flags must be between 0 and 65535");
    if (p->require_flags < 0 || p->require_flags > 65535) return fail(c, "bam_depth: require_flags must be between 0 and 65535");
    if (p->exclude_flags < 0 || p->exclude_flags > 65535) return fail(c, "bam_depth: exclude_flags must be between 0 and 65535");
    if (p->include_deletions < 0 || p->include_deletions > 1) return fail(c, "bam_depth: include_deletions must be 0 or 1");
    if (p->all_positions < 0 || p->all_positions > 2) return fail(c, "bam_depth: all_positions must be between 0 and 2");
    const bool regions = c->rg_active && !c->rg_given.empty();
    if (b && regions) return fail(c, "bam_depth: a BED and regions cannot be combined (give the target rows one way)");
    // ---- the target rows, in the order they are answered in ----
    const size_t n_ref = c->ref_len.size();
    S.o_tid.clear(); S.o_beg.clear(); S.o_end.clear(); S.o_k.clear(); S.n_bed_skipped = 0;
    std::vector<size_t> o_given;
    if (b) {
        // the union of the BED's rows: per contig sorted by start, rows that overlap or touch merged, clipped to the contig, empty ones dropped
        std::vector<int32_t> tid; std::vector<int64_t> beg, end; uint64_t n_bed = 0;
        if (bed_rows_read(c, b, ~0ull, tid, beg, end, n_bed)) return -1;
        std::vector<uint32_t> order;
        for (size_t i = 0; i < tid.size(); i++) {
            if (tid[i] < 0) { S.n_bed_skipped++; continue; }
            const int64_t L = (int64_t)c->ref_len[(size_t)tid[i]];
            if (beg[i] < 0) beg[i] = 0;
            if (end[i] > L) end[i] = L;
            if (end[i] > beg[i]) order.push_back((uint32_t)i);
        }
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return tid[x] != tid[y] ? tid[x] < tid[y] : beg[x] < beg[y]; });
        for (const uint32_t i : order) {
            if (!S.o_tid.empty() && S.o_tid.back() == tid[i] && beg[i] <= S.o_end.back()) { if (end[i] > S.o_end.back()) S.o_end.back() = end[i]; }
            else { S.o_tid.push_back(tid[i]); S.o_beg.push_back(beg[i]); S.o_end.push_back(end[i]); }
        }
    } else if (regions) {
        for (size_t g = 0; g < c->rg_given.size(); g++) {
            const auto &r = c->rg_given[g];
            const int64_t L = (int64_t)c->ref_len[(size_t)r.tid];
            S.o_tid.push_back(r.tid); S.o_beg.push_back(r.beg < L ? r.beg : L); S.o_end.push_back(r.end < L ? r.end : L); o_given.push_back(g);
        }
    } else for (size_t t = 0; t < n_ref; t++) { S.o_tid.push_back((int32_t)t); S.o_beg.push_back(0); S.o_end.push_back((int64_t)c->ref_len[t]); }
    if (dep_layout(c, S, "bam_depth", [&](size_t i) { return c->rg_given[o_given[i]].tok.c_str(); })) return -1;
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
    if (!S.open) return fail(c, DEPTH_NOT_OPEN);
    if (c->range_cut) return fail(c, DEPTH_SHARDED);
    if (b->status != 0) S.status = b->status;
    const int64_t n = b->n_rows;
    if (n <= 0) return 0;
    if (n > 0x7fffff00ll || !b->flag || !b->tid || !b->pos || !b->mapq) return fail(c, "bam_depth: the batch lacks FLAG, tid, POS or MAPQ");
    if (n != c->last_batch_rows || b->first_rec_uoff != c->last_batch_first || !c->last_stream.u || !c->rec_off.p || !c->cig_rel.p || !c->ncig_eff.p)
        return fail(c, "bam_depth: the batch is not the one dhts_bam_next_batch returned last on this context (CIGAR and QUAL are read where the scan left them)");
    HIPCHK(c, hipSetDevice(c->device));
    ENSURE(c, S.step, (size_t)n + 64); ENSURE(c, S.rlen, (size_t)n * 8 + 64); ENSURE(c, S.k0, (size_t)n * 4 + 64); ENSURE(c, S.k1, (size_t)n * 4 + 64);
    DepArgs a; memset(&a, 0, sizeof(a));
    a.u = c->last_stream.u; a.rec_off = (const uint32_t *)c->rec_off.p; a.cig_rel = (const uint32_t *)c->cig_rel.p; a.ncig_eff = (const uint32_t *)c->ncig_eff.p;
    a.flag = b->flag; a.tid = b->tid; a.pos = (const int64_t *)b->pos; a.mapq = b->mapq; a.n = (uint32_t)n; a.n_ref = S.n_ref;
    a.require = (uint32_t)S.P.require_flags; a.exclude = (uint32_t)S.P.exclude_flags; a.include = (uint32_t)S.P.include_flags; a.min_mapq = (uint32_t)S.P.min_mapq;
    a.min_baseq = (uint32_t)S.P.min_baseq; a.min_read_len = (long long)S.P.min_read_len;
    a.tid_first = (const uint32_t *)S.tid_first.p; a.rbeg = (const long long *)S.rbeg.p; a.rend = (const long long *)S.rend.p; a.rbase = (const unsigned long long *)S.rbase.p;
    a.step = (uint8_t *)S.step.p; a.rlen = (long long *)S.rlen.p; a.k0 = (uint32_t *)S.k0.p; a.k1 = (uint32_t *)S.k1.p;
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
    if (!c) return -1;
    if (!c->dpt.open) return fail(c, DEPTH_NOT_OPEN);
    if (c->range_cut) return fail(c, DEPTH_SHARDED);
    for (;;) {
        dhts_bam_batch b;
        if (dhts_bam_next_batch(c, max_blocks, DEPTH_COLMASK, &b) != 0) return -1;
        if (dhts_bam_depth_accumulate(c, &b) != 0) return -1;
        if (b.status != 0) return b.status;
    }
}

int dhts_bam_depth_stats(dhts_ctx *c, dhts_depth_stats *out) {
    if (!c || !out) return c ? fail(c, "bam_depth: no stats") : -1;
    memset(out, 0, sizeof(*out));
    DepthState &S = c->dpt;
    if (!S.open) return fail(c, DEPTH_NOT_OPEN);
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t s[DEP_N_STEPS];
    HIPCHK(c, hipMemcpyAsync(s, S.steps.p, sizeof(s), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out->n_flag_filtered = s[DEP_STEP_FLAG]; out->n_unplaced = s[DEP_STEP_UNPLACED]; out->n_short = s[DEP_STEP_SHORT]; out->n_low_mapq = s[DEP_STEP_MAPQ];
    out->n_outside = s[DEP_STEP_OUTSIDE]; out->n_counted = s[DEP_STEP_COUNTED];
    for (int k = 0; k < DEP_N_STEPS; k++) out->n_rows += s[k];
    out->n_target_rows = S.o_tid.size(); out->n_bed_skipped = S.n_bed_skipped; out->table_bytes = S.slots * 4;
    out->n_positions = S.res_ready ? S.n_positions : 0; out->status = S.status;
    return 0;
}

// an exclusive scan of v[0 .. n) in place, the total in v[n]: the carry in two levels (part: scratch)
extern "C++" {
template <typename T> static int depth_carry(dhts_ctx *c, DevBuf &part, T *v, uint64_t n) {
    const uint64_t np = (n + DEPC_CHUNK - 1) / DEPC_CHUNK;
    ENSURE(c, part, (size_t)(np + 1) * sizeof(T) + 64);
    hipLaunchKernelGGL(dep_carry_reduce<T>, dim3((unsigned)np), dim3(256), 0, c->stream, (const T *)v, n, (T *)part.p);
    hipLaunchKernelGGL(dep_carry_scan<T>, dim3(1), dim3(256), 0, c->stream, (T *)part.p, np);
    hipLaunchKernelGGL(dep_carry_apply<T>, dim3((unsigned)np), dim3(256), 0, c->stream, v, n, (const T *)part.p, np);
    return 0;
}
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
    if (!S.open) return fail(c, DEPTH_NOT_OPEN);
    HIPCHK(c, hipSetDevice(c->device));
    if (max_rows <= 0) max_rows = DEPTH_DEFAULT_ROWS;
    if (depth_result(c)) return -1;
    // ---- the windows of this page: runs of rows that follow each other in the answer and in the table ----
    struct Win { uint64_t o_a, o_b, dst0; };
    std::vector<Win> wins;
    const size_t n_out = S.o_tid.size();
    uint64_t taken = 0; size_t o = (size_t)S.o_next; uint64_t within = S.o_within;
    while (o < n_out && taken < (uint64_t)max_rows) {
        const int64_t k = S.o_k[o];
        const uint64_t cnt = k < 0 ? 0 : S.row_off[(size_t)k + 1] - S.row_off[(size_t)k];
        if (within >= cnt) { o++; within = 0; continue; }
        const uint64_t a = S.row_off[(size_t)k] + within, room = (uint64_t)max_rows - taken, m = cnt - within < room ? cnt - within : room;
        if (!wins.empty() && wins.back().o_b == a) wins.back().o_b = a + m;            // (the row before it in the answer is the row before it in the table)
        else wins.push_back({a, a + m, taken});
        taken += m; within += m;
    }
    while (o < n_out && (S.o_k[o] < 0 || within >= S.row_off[(size_t)S.o_k[o] + 1] - S.row_off[(size_t)S.o_k[o]])) { o++; within = 0; }      // (rows that have nothing left)
    const int64_t nrows = (int64_t)taken;
    const bool w_tid = (colmask >> DHTS_DEPTH_CHROM) & 1u, w_pos = (colmask >> DHTS_DEPTH_POS) & 1u, w_dep = (colmask >> DHTS_DEPTH_DEPTH) & 1u;
    S.out.assign(DHTS_DEPTH_COL_COUNT, dhts_col());
    for (int i = 0; i < DHTS_DEPTH_COL_COUNT; i++) { memset(&S.out[(size_t)i], 0, sizeof(dhts_col)); S.out[(size_t)i].col = i; }
    out->n_rows = nrows; out->n_cols = DHTS_DEPTH_COL_COUNT; out->cols = S.out.data();
    if (nrows > 0) {
        if (w_tid) ENSURE(c, S.out_tid, (size_t)nrows * 4 + 64);
        if (w_pos) ENSURE(c, S.out_pos, (size_t)nrows * 8 + 64);
        if (w_dep) ENSURE(c, S.out_depth, (size_t)nrows * 4 + 64);
        if (w_tid || w_pos || w_dep) {
            const uint64_t ntiles = S.slots / DEP_TILE;
            ENSURE(c, S.pagetiles, wins.size() * 16 + 64);
            std::vector<uint64_t> tiles(wins.size() * 2, 0);
            for (size_t w = 0; w < wins.size(); w++)
                hipLaunchKernelGGL(dep_page_tiles, dim3(1), dim3(64), 0, c->stream, (const unsigned long long *)S.toff.p, ntiles, (unsigned long long)wins[w].o_a, (unsigned long long)wins[w].o_b,
                                   (unsigned long long *)S.pagetiles.p + 2 * w);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(tiles.data(), S.pagetiles.p, wins.size() * 16, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            KTimer tm(c, DHTS_K_SCAN);
            for (size_t w = 0; w < wins.size(); w++) {
                const uint64_t t0 = tiles[2 * w], t1 = tiles[2 * w + 1];
                if (t1 < t0 || t1 >= ntiles) return fail(c, "bam_depth: internal error: the tiles of a page are out of range");
                DepEmitArgs e; memset(&e, 0, sizeof(e));
                e.diff = (const int32_t *)S.diff.p; e.tcarry = (const uint32_t *)S.tsum.p; e.toff = (const unsigned long long *)S.toff.p; e.tile_row = (const uint32_t *)S.tile_row.p;
                e.rbase = (const unsigned long long *)S.rbase.p; e.rbeg = (const long long *)S.rbeg.p; e.rend = (const long long *)S.rend.p;
                e.row_tid = (const int32_t *)S.row_tid.p; e.touched = (const uint32_t *)S.touched.p; e.mode = (uint32_t)S.P.all_positions;
                e.t0 = t0; e.o_a = wins[w].o_a; e.o_b = wins[w].o_b; e.dst0 = wins[w].dst0;
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
    S.o_next = o; S.o_within = within;
    out->status = o >= n_out ? 1 : 0;
    return 0;
}

// ---- read-back: out_cols[b->n_cols] = b->cols with HOST pointers into dst --------------------------------------------------------------
static uint64_t depth_col_bytes(int col, uint64_t n) { return ((col == DHTS_DEPTH_POS ? n * 8 : n * 4) + 7) & ~7ull; }
uint64_t dhts_bam_depth_batch_host_bytes(const dhts_depth_batch *b) {
    if (!b) return 0;
    uint64_t need = 0;
    for (int i = 0; i < b->n_cols; i++) if (b->cols[i].fixed) need += depth_col_bytes(b->cols[i].col, (uint64_t)b->n_rows);
    return need;
}
int dhts_bam_depth_batch_fetch(dhts_ctx *c, const dhts_depth_batch *b, void *dst, uint64_t cap, dhts_col *out_cols) {
    if (!c || !b || !out_cols || (!dst && cap)) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    if (cap < dhts_bam_depth_batch_host_bytes(b)) return fail(c, "bam_depth: fetch buffer too small");
    uint8_t *p = (uint8_t *)dst; const uint64_t n = (uint64_t)b->n_rows;
    for (int i = 0; i < b->n_cols; i++) {
        const dhts_col &s = b->cols[i]; dhts_col &o = out_cols[i];
        memset(&o, 0, sizeof(o)); o.col = s.col;
        if (n == 0 || !s.fixed) continue;
        HIPCHK(c, hipMemcpyAsync(p, s.fixed, s.col == DHTS_DEPTH_POS ? n * 8 : n * 4, hipMemcpyDeviceToHost, c->stream)); o.fixed = p; p += depth_col_bytes(s.col, n);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
