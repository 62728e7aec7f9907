// dhts_bam_bins.inc -- part of dhts_api.hip (included there, inside its extern "C" block; not a translation unit of its own):
// bam_bin_counts.  The table of 64-bit counters (two per bin) and the step counters live in HBM from dhts_bam_bins_open on; every batch of
// the context's read_bam scan is classified and added by the kernels of bam_bins.hip without a visit to the host; the result rows are
// cut out of the table window by window (mark, scan, emit) and paged out.  The checks in front of a batch, the scan loop, the step counters
// and the read-back are dhts_bam_accum.inc's.
#define BINS_MAX_TOTAL (1ull << 28)
#define BINS_WINDOW (1u << 22)                 /* bins marked and scanned at once when the result is paged out */
static const uint32_t BINS_COLMASK = (1u << DHTS_BAM_FLAG) | (1u << DHTS_BAM_RNAME) | (1u << DHTS_BAM_POS) | (1u << DHTS_BAM_MAPQ) | (1u << DHTS_BAM_PNEXT);   // no string column

// (a shard or a block range of the file is refused; the windows of a region query are the whole answer of that query, not a shard)
static const AccumWho BINS_WHO = {"bam_bin_counts", "bam_bin_counts: dhts_bam_bins_open not called",
                                  "bam_bin_counts: a shard or block range of the file is not supported (the duplicate rule and the counts need the whole file on one device)"};

int dhts_bam_bins_open(dhts_ctx *c, const dhts_bins_params *p) {
    if (!c || !p) return c ? fail(c, "bam_bin_counts: no parameters") : -1;
    BinsState &S = c->bins;
    S.open = false;
    if (!c->bam_open) return fail(c, "bam_bin_counts: dhts_bam_open not called");
    if (c->range_cut) return fail(c, "%s", BINS_WHO.sharded);
    if (p->bin_width <= 0) return fail(c, "bam_bin_counts: bin_width must be > 0");
    BamFilterMsg m;
    if (const char *bad = bam_filter_check(m, "bam_bin_counts", 0, p->min_mapq, 0, p->include_flags, p->require_flags, p->exclude_flags, false, false)) return fail(c, "%s", bad);
    if (p->dedup != DHTS_BINS_DEDUP_NONE && p->dedup != DHTS_BINS_DEDUP_ADJACENT) return fail(c, "bam_bin_counts: dedup must be one of: none, adjacent");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n_ref = c->ref_len.size();
    const uint64_t bw = (uint64_t)p->bin_width;
    std::vector<uint32_t> base(n_ref + 1, 0); uint64_t total = 0;
    for (size_t t = 0; t < n_ref; t++) { base[t] = (uint32_t)total; total += ((uint64_t)c->ref_len[t] + bw - 1) / bw; if (total > BINS_MAX_TOTAL) { for (size_t k = t + 1; k < n_ref; k++) total += ((uint64_t)c->ref_len[k] + bw - 1) / bw; break; } }
    if (total > BINS_MAX_TOTAL) return fail(c, "bam_bin_counts: bin_width %lld gives %llu bins; at most %llu are supported (a wider bin_width)", (long long)p->bin_width, (unsigned long long)total, (unsigned long long)BINS_MAX_TOTAL);
    base[n_ref] = (uint32_t)total;
    // emit_zero_bins: every bin of every contig the scan names -- all of them without regions, or with '.'
    std::vector<uint8_t> zero_ok(n_ref + 1, 1);
    if (c->rg_active && !c->rg_all) for (size_t t = 0; t < n_ref; t++) zero_ok[t] = t + 1 < c->rg_tid_first.size() && c->rg_tid_first[t + 1] > c->rg_tid_first[t] ? 1 : 0;
    ENSURE(c, S.steps, 64); ENSURE(c, S.carry, 2 * sizeof(BinCarry)); ENSURE(c, S.bin_base, (n_ref + 1) * 4 + 64); ENSURE(c, S.ref_len, n_ref * 4 + 64); ENSURE(c, S.zero_ok, n_ref + 64);
    HIPCHK(c, hipMemsetAsync(S.steps.p, 0, 64, c->stream));
    HIPCHK(c, hipMemsetAsync(S.carry.p, 0, 2 * sizeof(BinCarry), c->stream));
    HIPCHK(c, hipMemcpyAsync(S.bin_base.p, base.data(), (n_ref + 1) * 4, hipMemcpyHostToDevice, c->stream));
    if (n_ref) HIPCHK(c, hipMemcpyAsync(S.ref_len.p, c->ref_len.data(), n_ref * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(S.zero_ok.p, zero_ok.data(), n_ref + 1, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    S.P = *p; S.total_bins = total; S.n_ref = (int32_t)n_ref; S.status = 0; S.carry_cur = 0; S.win_b0 = 0; S.win_n = 0; S.win_rows = 0; S.win_done = 0;
    S.table_ready = false;                                 // the table itself is made by the first call that touches it: a bind that only asks "how many bins" allocates nothing
    S.open = true;
    return 0;
}
static int bins_table(dhts_ctx *c) {
    BinsState &S = c->bins;
    if (S.table_ready) return 0;
    ENSURE(c, S.counts, (size_t)S.total_bins * 16 + 64);
    HIPCHK(c, hipMemsetAsync(S.counts.p, 0, (size_t)S.total_bins * 16 + 64, c->stream));
    S.table_ready = true;
    return 0;
}

int dhts_bam_bins_accumulate(dhts_ctx *c, const dhts_bam_batch *b) {
    if (!c || !b) return c ? fail(c, "bam_bin_counts: no batch") : -1;
    BinsState &S = c->bins;
    const int go = accum_batch_ok(c, BINS_WHO, S, b, true, nullptr);
    if (go <= 0) return go;
    const int64_t n = b->n_rows;
    if (bins_table(c)) return -1;
    const bool dedup = S.P.dedup == DHTS_BINS_DEDUP_ADJACENT;
    ENSURE(c, S.step, (size_t)n + 64); ENSURE(c, S.word, (size_t)n * 4 + 64);
    BinArgs a; memset(&a, 0, sizeof(a));
    a.flag = b->flag; a.tid = b->tid; a.pos = (const int64_t *)b->pos; a.mapq = b->mapq; a.pnext = (const int64_t *)b->pnext; a.n = (uint32_t)n;
    a.ref_len = (const uint32_t *)S.ref_len.p; a.bin_base = (const uint32_t *)S.bin_base.p; a.n_ref = S.n_ref;
    a.bin_width = S.P.bin_width >= (1ll << 31) ? 0u : (uint32_t)S.P.bin_width;
    a.require = (uint32_t)S.P.require_flags; a.exclude = (uint32_t)S.P.exclude_flags; a.include = (uint32_t)S.P.include_flags; a.min_mapq = (uint32_t)S.P.min_mapq;
    a.step = (uint8_t *)S.step.p; a.word = (uint32_t *)S.word.p;
    if (dedup) { ENSURE(c, S.vis, (size_t)(n + 2) * 4 + 64); ENSURE(c, S.rank, (size_t)(n + 2) * 4 + 64); ENSURE(c, S.src, (size_t)n * 4 + 64); a.vis = (uint32_t *)S.vis.p; }
    const unsigned grid = (unsigned)((n + 255) / 256);
    KTimer tm(c, DHTS_K_BCF_CHECK);
    hipLaunchKernelGGL(bam_bin_classify, dim3(grid), dim3(256), 0, c->stream, a);
    if (dedup) {
        // the rows the rule sees, compacted: a row's predecessor is its neighbour there; the last one stays on the device for the next batch
        const uint32_t *kin[1] = {(const uint32_t *)S.vis.p}; uint32_t *kout[1] = {(uint32_t *)S.rank.p};
        if (run_scan(c, 1, kin, kout, nullptr, n, nullptr)) return -1;
        hipLaunchKernelGGL(fq_compact, dim3(grid), dim3(256), 0, c->stream, (const uint32_t *)S.vis.p, (const uint32_t *)S.rank.p, (uint32_t)n, (uint32_t *)S.src.p);
        BinCarry *cy = (BinCarry *)S.carry.p;
        hipLaunchKernelGGL(bam_bin_dedup, dim3(grid), dim3(256), 0, c->stream, a, (const uint32_t *)S.rank.p, (const uint32_t *)S.src.p, (const BinCarry *)(cy + S.carry_cur), cy + (S.carry_cur ^ 1));
        S.carry_cur ^= 1;
    }
    hipLaunchKernelGGL(bam_bin_add, dim3(grid < BIN_ADD_MAX_BLOCKS ? grid : BIN_ADD_MAX_BLOCKS), dim3(256), 0, c->stream, (const uint8_t *)S.step.p, (const uint32_t *)S.word.p, (uint32_t)n, (unsigned long long *)S.counts.p, (unsigned long long *)S.steps.p);
    HIPCHK(c, hipGetLastError());                          // (no wait: whatever reuses the batch's columns is queued behind these kernels)
    S.win_n = 0; S.win_rows = S.win_done = 0; S.win_b0 = 0;  // a result that was being paged out starts over
    return 0;
}

int dhts_bam_bins_scan(dhts_ctx *c, int64_t max_blocks) {
    return c ? accum_scan(c, BINS_WHO, c->bins.open, max_blocks, BINS_COLMASK, dhts_bam_bins_accumulate) : -1;
}

int dhts_bam_bins_stats(dhts_ctx *c, dhts_bins_stats *out) {
    if (!c || !out) return c ? fail(c, "bam_bin_counts: no stats") : -1;
    memset(out, 0, sizeof(*out));
    BinsState &S = c->bins;
    uint64_t s[BIN_N_STEPS];
    if (accum_steps(c, BINS_WHO, S, s, BIN_N_STEPS)) return -1;
    out->n_flag_filtered = s[BIN_STEP_FLAG]; out->n_unplaced = s[BIN_STEP_UNPLACED]; out->n_out_of_range = s[BIN_STEP_RANGE]; out->n_duplicate = s[BIN_STEP_DUP];
    out->n_low_mapq = s[BIN_STEP_MAPQ]; out->n_counted = s[BIN_STEP_COUNTED];
    for (int k = 0; k < BIN_N_STEPS; k++) out->n_rows += s[k];
    out->total_bins = S.total_bins; out->status = S.status;
    return 0;
}

// the next <= max_rows result rows (0 = default): contigs in header order, bins ascending
int dhts_bam_bins_next(dhts_ctx *c, int64_t max_rows, dhts_bins_batch *out) {
    if (!c || !out) return -1;
    memset(out, 0, sizeof(*out));
    BinsState &S = c->bins;
    if (!S.open) return fail(c, "%s", BINS_WHO.not_open);
    HIPCHK(c, hipSetDevice(c->device));
    if (max_rows <= 0) max_rows = 1 << 20;
    if (max_rows > BINS_WINDOW) max_rows = BINS_WINDOW;
    if (bins_table(c)) return -1;
    const uint8_t *zero_ok = S.P.emit_zero_bins ? (const uint8_t *)S.zero_ok.p : nullptr;
    // the window that still has rows to hand out: mark and scan the next ones until one has
    while (S.win_done >= S.win_rows && S.win_b0 + S.win_n < S.total_bins) {
        S.win_b0 += S.win_n;
        const uint64_t left = S.total_bins - S.win_b0;
        S.win_n = left < BINS_WINDOW ? (uint32_t)left : BINS_WINDOW;
        ENSURE(c, S.keep, (size_t)(S.win_n + 2) * 4 + 64); ENSURE(c, S.krank, (size_t)(S.win_n + 2) * 4 + 64);
        hipLaunchKernelGGL(bam_bin_mark, dim3((S.win_n + 255) / 256), dim3(256), 0, c->stream, (const unsigned long long *)S.counts.p, (const uint32_t *)S.bin_base.p, S.n_ref, zero_ok, (uint32_t)S.win_b0, S.win_n, (uint32_t *)S.keep.p);
        const uint32_t *kin[1] = {(const uint32_t *)S.keep.p}; uint32_t *kout[1] = {(uint32_t *)S.krank.p}; uint64_t rows = 0;
        if (run_scan(c, 1, kin, kout, nullptr, S.win_n, &rows)) return -1;
        S.win_rows = rows; S.win_done = 0;
    }
    const uint64_t avail = S.win_rows - S.win_done;
    const int64_t nrows = avail < (uint64_t)max_rows ? (int64_t)avail : max_rows;
    cols_reset(S.out, DHTS_BINS_COL_COUNT);
    out->n_rows = nrows; out->n_cols = DHTS_BINS_COL_COUNT; out->cols = S.out.data();
    if (nrows > 0) {
        BinCols o; long long **op[DHTS_BINS_COL_COUNT] = {&o.chrom, &o.start, &o.end, &o.bin_id, &o.total, &o.fwd, &o.rev};
        for (int i = 0; i < DHTS_BINS_COL_COUNT; i++) { ENSURE(c, S.cols[i], (size_t)nrows * 8 + 64); *op[i] = (long long *)S.cols[i].p; }
        ENSURE(c, S.ones, (size_t)nrows + 64);
        HIPCHK(c, hipMemsetAsync(S.ones.p, 1, (size_t)nrows, c->stream));
        hipLaunchKernelGGL(bam_bin_emit, dim3((S.win_n + 255) / 256), dim3(256), 0, c->stream, (const unsigned long long *)S.counts.p, (const uint32_t *)S.bin_base.p, (const uint32_t *)S.ref_len.p, S.n_ref, (uint64_t)S.P.bin_width,
                           (uint32_t)S.win_b0, S.win_n, (const uint32_t *)S.keep.p, (const uint32_t *)S.krank.p, (uint32_t)S.win_done, (uint32_t)nrows, o);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int i = 0; i < DHTS_BINS_COL_COUNT; i++) { S.out[(size_t)i].fixed = S.cols[i].p; S.out[(size_t)i].valid = (const uint8_t *)S.ones.p; }
        S.win_done += (uint64_t)nrows;
    }
    out->status = (S.win_done >= S.win_rows && S.win_b0 + S.win_n >= S.total_bins) ? 1 : 0;
    return 0;
}

// ---- read-back: out_cols[b->n_cols] = b->cols with HOST pointers into dst (every column eight bytes wide) ----------------------------
uint64_t dhts_bam_bins_batch_host_bytes(const dhts_bins_batch *b) { return b ? cols_host_bytes(b->n_rows, b->n_cols, b->cols, col_kind_int64) : 0; }
int dhts_bam_bins_batch_fetch(dhts_ctx *c, const dhts_bins_batch *b, void *dst, uint64_t cap, dhts_col *out_cols) {
    return b ? cols_fetch(c, "bam_bin_counts", b->n_rows, b->n_cols, b->cols, col_kind_int64, dst, cap, out_cols) : -1;
}
