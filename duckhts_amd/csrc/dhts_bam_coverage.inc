// dhts_bam_coverage.inc -- part of dhts_api.hip (included there, inside its extern "C" block; not a translation unit of its own):
// bam_coverage.  dhts_bam_coverage_open lays out the target rows (one per @SQ, or one per region given), sorts them per contig, refuses
// overlaps, and leaves the zeroed difference table, the per-row words and the step counters in HBM.  Every batch of the context's read_bam
// scan is classified and added by the kernels of bam_coverage.hip where it lies: CIGAR and QUAL are read out of the inflated stream, which
// stays in HBM with the record offsets and the CIGAR locations of the unpack pass until the next batch is made, so the pass runs behind
// dhts_bam_next_batch and the scan projects no string column.  The result is four kernels over the table and one small copy to the host,
// where the four doubles are divided (one IEEE division each) and the rows are put back into the order they were asked for in.
#define COVERAGE_MAX_TABLE_BYTES (16ull << 30)
static uint64_t g_coverage_max_table_bytes = COVERAGE_MAX_TABLE_BYTES;
static const uint32_t COVERAGE_COLMASK = (1u << DHTS_BAM_FLAG) | (1u << DHTS_BAM_RNAME) | (1u << DHTS_BAM_POS) | (1u << DHTS_BAM_MAPQ);   // no string column
#define COVERAGE_SHARDED "bam_coverage: a shard or block range of the file is not supported (the counts need the whole file on one device)"
#define COVERAGE_NOT_OPEN "bam_coverage: dhts_bam_coverage_open not called"

// tests: the most bytes the difference table may take (0: the contract's 16 GiB)
void dhts_debug_coverage_max_table_bytes(uint64_t n) { g_coverage_max_table_bytes = n ? n : COVERAGE_MAX_TABLE_BYTES; }

// The layout bam_coverage and bam_depth share.  S.o_tid / o_beg / o_end hold the target rows in the order they are answered in, clipped.  They
// are sorted by (contig, start) with the empty ones left out (o_k: a row's index among the sorted ones, -1 for an empty one), neighbours on one
// contig must not overlap (tok(i): what row i was given as, for the error), every sorted row gets a span of (end - beg) + 1 slots of the
// difference table rounded up to the tile, and the rows, tid_first, tile_row and the zeroed table go to the device (queued on the stream).
// bpp / noun: the table's bytes per slot and what the cap's error calls it (bam_pileup's count table has 32 or 64 bytes per position).
static int dep_layout(dhts_ctx *c, DepLayout &S, const char *fn, const std::function<const char *(size_t)> &tok, uint64_t bpp = 4, const char *noun = "depth table") {
    const size_t n_ref = c->ref_len.size(), n_out = S.o_tid.size();
    std::vector<uint32_t> order;
    for (size_t i = 0; i < n_out; i++) if (S.o_end[i] > S.o_beg[i]) order.push_back((uint32_t)i);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return S.o_tid[x] != S.o_tid[y] ? S.o_tid[x] < S.o_tid[y] : S.o_beg[x] < S.o_beg[y]; });
    for (size_t j = 1; j < order.size(); j++) {
        const uint32_t x = order[j - 1], y = order[j];
        if (S.o_tid[x] == S.o_tid[y] && S.o_beg[y] < S.o_end[x]) {
            const uint32_t first = x < y ? x : y, second = x < y ? y : x;
            return fail(c, "%s: the regions '%s' and '%s' overlap (one row is answered per region: give disjoint regions)", fn, tok(first), tok(second));
        }
    }
    const size_t R = order.size();
    S.o_k.assign(n_out, -1);
    std::vector<uint32_t> tid_first(n_ref + 1, 0);
    S.s_beg.assign(R + 1, 0); S.s_end.assign(R + 1, 0); S.s_base.assign(R + 1, 0); S.s_tid.assign(R + 1, 0);
    uint64_t slots = 0;
    for (size_t k = 0; k < R; k++) {
        const uint32_t i = order[k];
        S.o_k[i] = (int64_t)k; S.s_beg[k] = S.o_beg[i]; S.s_end[k] = S.o_end[i]; S.s_base[k] = slots; S.s_tid[k] = S.o_tid[i];
        tid_first[(size_t)S.o_tid[i] + 1]++;
        slots += ((uint64_t)(S.s_end[k] - S.s_beg[k]) + 1u + DEP_TILE - 1u) / DEP_TILE * DEP_TILE;
    }
    S.s_base[R] = slots;
    for (size_t t = 0; t < n_ref; t++) tid_first[t + 1] += tid_first[t];
    if (slots * bpp > g_coverage_max_table_bytes)
        return fail(c, "%s: the %s needs %llu bytes (%llu per position of every row); at most %llu are supported (fewer or shorter regions)",
                    fn, noun, (unsigned long long)(slots * bpp), (unsigned long long)bpp, (unsigned long long)g_coverage_max_table_bytes);
    const uint64_t ntiles = slots / DEP_TILE;
    std::vector<uint32_t> tile_row((size_t)ntiles + 1, 0);
    for (size_t k = 0; k < R; k++) for (uint64_t t = S.s_base[k] / DEP_TILE; t < S.s_base[k + 1] / DEP_TILE; t++) tile_row[(size_t)t] = (uint32_t)k;
    HIPCHK(c, hipSetDevice(c->device));
    ENSURE(c, S.tid_first, (n_ref + 1) * 4 + 64); ENSURE(c, S.rbeg, (R + 1) * 8 + 64); ENSURE(c, S.rend, (R + 1) * 8 + 64); ENSURE(c, S.rbase, (R + 1) * 8 + 64);
    ENSURE(c, S.tile_row, (size_t)(ntiles + 1) * 4 + 64); ENSURE(c, S.diff, (size_t)(slots * bpp) + 64);
    {
        KTimer tm(c, DHTS_K_BCF_CHECK);
        HIPCHK(c, hipMemsetAsync(S.diff.p, 0, (size_t)(slots * bpp) + 64, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(S.tid_first.p, tid_first.data(), (n_ref + 1) * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(S.rbeg.p, S.s_beg.data(), (R + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(S.rend.p, S.s_end.data(), (R + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(S.rbase.p, S.s_base.data(), (R + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(S.tile_row.p, tile_row.data(), (size_t)(ntiles + 1) * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                  // (the copies read vectors of this call)
    S.n_sorted = R; S.slots = slots;
    return 0;
}

int dhts_bam_coverage_open(dhts_ctx *c, const dhts_coverage_params *p) {
    if (!c || !p) return c ? fail(c, "bam_coverage: no parameters") : -1;
    CoverageState &S = c->dep;
    S.open = false;
    if (!c->bam_open) return fail(c, "bam_coverage: dhts_bam_open not called");
    if (c->range_cut) return fail(c, COVERAGE_SHARDED);
    if (p->min_read_len < 0) return fail(c, "bam_coverage: min_read_len must be >= 0");
    if (p->min_mapq < 0 || p->min_mapq > 255) return fail(c, "bam_coverage: min_mapq must be between 0 and 255");
    if (p->min_baseq < 0 || p->min_baseq > 255) return fail(c, "bam_coverage: min_baseq must be between 0 and 255");
    if (p->include_flags < 0 || p->include_flags > 65535) return fail(c, "bam_coverage: include_flags must be between 0 and 65535");
    if (p->require_flags < 0 || p->require_flags > 65535) return fail(c, "bam_coverage: require_flags must be between 0 and 65535");
    if (p->exclude_flags < 0 || p->exclude_flags > 65535) return fail(c, "bam_coverage: exclude_flags must be between 0 and 65535");
    if (p->min_depth < 1) return fail(c, "bam_coverage: min_depth must be >= 1");
    // ---- the target rows, in the order they are answered in: the regions that name a contig, or every @SQ ('.' and '*' name no row) ----
    const size_t n_ref = c->ref_len.size();
    S.o_tid.clear(); S.o_beg.clear(); S.o_end.clear(); S.o_k.clear();
    std::vector<size_t> o_given;
    if (c->rg_active && !c->rg_given.empty()) {
        for (size_t g = 0; g < c->rg_given.size(); g++) {
            const auto &r = c->rg_given[g];
            const int64_t L = (int64_t)c->ref_len[(size_t)r.tid];
            S.o_tid.push_back(r.tid); S.o_beg.push_back(r.beg < L ? r.beg : L); S.o_end.push_back(r.end < L ? r.end : L); o_given.push_back(g);
        }
    } else for (size_t t = 0; t < n_ref; t++) { S.o_tid.push_back((int32_t)t); S.o_beg.push_back(0); S.o_end.push_back((int64_t)c->ref_len[t]); }
    if (dep_layout(c, S, "bam_coverage", [&](size_t i) { return c->rg_given[o_given[i]].tok.c_str(); })) return -1;
    const size_t R = (size_t)S.n_sorted;
    ENSURE(c, S.steps, 64); ENSURE(c, S.words, (R + 1) * DEP_REPLICAS * 64 + 64);
    HIPCHK(c, hipMemsetAsync(S.steps.p, 0, 64, c->stream));
    HIPCHK(c, hipMemsetAsync(S.words.p, 0, (R + 1) * DEP_REPLICAS * 64, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    S.P = *p; S.n_ref = (int32_t)n_ref; S.status = 0; S.res_ready = false; S.row_next = 0;
    S.open = true;
    return 0;
}

int dhts_bam_coverage_accumulate(dhts_ctx *c, const dhts_bam_batch *b) {
    if (!c || !b) return c ? fail(c, "bam_coverage: no batch") : -1;
    CoverageState &S = c->dep;
    if (!S.open) return fail(c, COVERAGE_NOT_OPEN);
    if (c->range_cut) return fail(c, COVERAGE_SHARDED);
    if (b->status != 0) S.status = b->status;
    const int64_t n = b->n_rows;
    if (n <= 0) return 0;
    if (n > 0x7fffff00ll || !b->flag || !b->tid || !b->pos || !b->mapq) return fail(c, "bam_coverage: the batch lacks FLAG, tid, POS or MAPQ");
    if (n != c->last_batch_rows || b->first_rec_uoff != c->last_batch_first || !c->last_stream.u || !c->rec_off.p || !c->cig_rel.p || !c->ncig_eff.p)
        return fail(c, "bam_coverage: the batch is not the one dhts_bam_next_batch returned last on this context (CIGAR and QUAL are read where the scan left them)");
    HIPCHK(c, hipSetDevice(c->device));
    ENSURE(c, S.step, (size_t)n + 64); ENSURE(c, S.rlen, (size_t)n * 8 + 64); ENSURE(c, S.k0, (size_t)n * 4 + 64); ENSURE(c, S.k1, (size_t)n * 4 + 64);
    DepArgs a; memset(&a, 0, sizeof(a));
    a.u = c->last_stream.u; a.rec_off = (const uint32_t *)c->rec_off.p; a.cig_rel = (const uint32_t *)c->cig_rel.p; a.ncig_eff = (const uint32_t *)c->ncig_eff.p;
    a.flag = b->flag; a.tid = b->tid; a.pos = (const int64_t *)b->pos; a.mapq = b->mapq; a.n = (uint32_t)n; a.n_ref = S.n_ref;
    a.require = (uint32_t)S.P.require_flags; a.exclude = (uint32_t)S.P.exclude_flags; a.include = (uint32_t)S.P.include_flags; a.min_mapq = (uint32_t)S.P.min_mapq;
    a.min_baseq = (uint32_t)S.P.min_baseq; a.min_read_len = (long long)S.P.min_read_len;
    a.tid_first = (const uint32_t *)S.tid_first.p; a.rbeg = (const long long *)S.rbeg.p; a.rend = (const long long *)S.rend.p; a.rbase = (const unsigned long long *)S.rbase.p;
    a.step = (uint8_t *)S.step.p; a.rlen = (long long *)S.rlen.p; a.k0 = (uint32_t *)S.k0.p; a.k1 = (uint32_t *)S.k1.p;
    const unsigned grid = (unsigned)((n + 255) / 256), agrid = (unsigned)((n + 31) / 32);
    KTimer tm(c, DHTS_K_BCF_CHECK);
    hipLaunchKernelGGL(bam_depth_classify, dim3(grid), dim3(256), 0, c->stream, a);
    if (S.P.min_baseq > 0) hipLaunchKernelGGL(bam_depth_add<true>, dim3(agrid < DEP_ADD_MAX_BLOCKS ? agrid : DEP_ADD_MAX_BLOCKS), dim3(256), 0, c->stream, a, (int32_t *)S.diff.p, (unsigned long long *)S.words.p, (unsigned long long *)S.steps.p);
    else hipLaunchKernelGGL(bam_depth_add<false>, dim3(agrid < DEP_ADD_MAX_BLOCKS ? agrid : DEP_ADD_MAX_BLOCKS), dim3(256), 0, c->stream, a, (int32_t *)S.diff.p, (unsigned long long *)S.words.p, (unsigned long long *)S.steps.p);
    HIPCHK(c, hipGetLastError());                          // (no wait: whatever reuses the batch's buffers is queued behind these kernels)
    S.res_ready = false; S.row_next = 0;                   // a result that was being paged out starts over
    return 0;
}

// the context's scan to the end of the stream; returns the status it ended on (1, or the negative status of a stream that ended on an error:
// its rows are counted), < 0 with dhts_error set when a call failed (dhts_coverage_stats.status stays 0 then)
int dhts_bam_coverage_scan(dhts_ctx *c, int64_t max_blocks) {
    if (!c) return -1;
    if (!c->dep.open) return fail(c, COVERAGE_NOT_OPEN);
    if (c->range_cut) return fail(c, COVERAGE_SHARDED);
    for (;;) {
        dhts_bam_batch b;
        if (dhts_bam_next_batch(c, max_blocks, COVERAGE_COLMASK, &b) != 0) return -1;
        if (dhts_bam_coverage_accumulate(c, &b) != 0) return -1;
        if (b.status != 0) return b.status;
    }
}

int dhts_bam_coverage_stats(dhts_ctx *c, dhts_coverage_stats *out) {
    if (!c || !out) return c ? fail(c, "bam_coverage: no stats") : -1;
    memset(out, 0, sizeof(*out));
    CoverageState &S = c->dep;
    if (!S.open) return fail(c, COVERAGE_NOT_OPEN);
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t s[DEP_N_STEPS];
    HIPCHK(c, hipMemcpyAsync(s, S.steps.p, sizeof(s), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out->n_flag_filtered = s[DEP_STEP_FLAG]; out->n_unplaced = s[DEP_STEP_UNPLACED]; out->n_short = s[DEP_STEP_SHORT]; out->n_low_mapq = s[DEP_STEP_MAPQ];
    out->n_outside = s[DEP_STEP_OUTSIDE]; out->n_counted = s[DEP_STEP_COUNTED];
    for (int k = 0; k < DEP_N_STEPS; k++) out->n_rows += s[k];
    out->n_target_rows = S.o_tid.size(); out->table_bytes = S.slots * 4; out->status = S.status;
    return 0;
}

// the twelve columns of every row on the host (the counters and the table stay: a later batch adds to them)
static int coverage_result(dhts_ctx *c) {
    CoverageState &S = c->dep;
    if (S.res_ready) return 0;
    const size_t R = (size_t)S.n_sorted, n_out = S.o_tid.size(); const uint64_t ntiles = S.slots / DEP_TILE;
    std::vector<uint64_t> res(R * DEP_RES_WORDS + 1, 0);
    if (R) {
        ENSURE(c, S.tsum, (size_t)ntiles * 4 + 64); ENSURE(c, S.tcov, (size_t)ntiles * 4 + 64); ENSURE(c, S.tdepth, (size_t)ntiles * 8 + 64); ENSURE(c, S.res, R * DEP_RES_WORDS * 8 + 64);
        {
            KTimer tm(c, DHTS_K_SCAN);
            hipLaunchKernelGGL(dep_tile_sum, dim3((unsigned)ntiles), dim3(256), 0, c->stream, (const int32_t *)S.diff.p, (uint32_t *)S.tsum.p);
            hipLaunchKernelGGL(dep_tile_carry, dim3(1), dim3(256), 0, c->stream, (uint32_t *)S.tsum.p, ntiles);
            hipLaunchKernelGGL(dep_tile_reduce, dim3((unsigned)ntiles), dim3(256), 0, c->stream, (const int32_t *)S.diff.p, (const uint32_t *)S.tsum.p, (const uint32_t *)S.tile_row.p,
                               (const unsigned long long *)S.rbase.p, (const long long *)S.rbeg.p, (const long long *)S.rend.p, (long long)S.P.min_depth, (uint32_t *)S.tcov.p, (unsigned long long *)S.tdepth.p);
            hipLaunchKernelGGL(dep_row_sum, dim3((unsigned)R), dim3(256), 0, c->stream, (const uint32_t *)S.tcov.p, (const unsigned long long *)S.tdepth.p, (const unsigned long long *)S.rbase.p,
                               (const long long *)S.rbeg.p, (const long long *)S.rend.p, (const unsigned long long *)S.words.p, (unsigned long long *)S.res.p);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(res.data(), S.res.p, R * DEP_RES_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    for (int i = 0; i < DHTS_COVERAGE_COL_COUNT; i++) S.h_cols[i].assign(n_out, 0);
    auto div = [](double a, double b) -> int64_t { const double d = b == 0.0 ? 0.0 : a / b; int64_t bits; memcpy(&bits, &d, 8); return bits; };    // one IEEE division
    for (size_t i = 0; i < n_out; i++) {
        uint64_t numreads = 0, covbases = 0, sum_depth = 0, sum_baseq = 0, sum_mapq = 0;
        if (S.o_k[i] >= 0) { const size_t k = (size_t)S.o_k[i]; const uint64_t *w = res.data() + k * DEP_RES_WORDS; covbases = w[0]; sum_depth = w[1]; numreads = w[2]; sum_mapq = w[3]; sum_baseq = w[4]; }
        const double len = (double)(S.o_end[i] - S.o_beg[i]);
        S.h_cols[DHTS_COVERAGE_CHROM][i] = S.o_tid[i]; S.h_cols[DHTS_COVERAGE_START][i] = S.o_beg[i]; S.h_cols[DHTS_COVERAGE_END][i] = S.o_end[i];
        S.h_cols[DHTS_COVERAGE_NUMREADS][i] = (int64_t)numreads; S.h_cols[DHTS_COVERAGE_COVBASES][i] = (int64_t)covbases;
        S.h_cols[DHTS_COVERAGE_COVERAGE][i] = div((double)(100ull * covbases), len);
        S.h_cols[DHTS_COVERAGE_MEANDEPTH][i] = div((double)sum_depth, len);
        S.h_cols[DHTS_COVERAGE_MEANBASEQ][i] = div((double)sum_baseq, (double)sum_depth);
        S.h_cols[DHTS_COVERAGE_MEANMAPQ][i] = div((double)sum_mapq, (double)numreads);
        S.h_cols[DHTS_COVERAGE_SUM_DEPTH][i] = (int64_t)sum_depth; S.h_cols[DHTS_COVERAGE_SUM_BASEQ][i] = (int64_t)sum_baseq; S.h_cols[DHTS_COVERAGE_SUM_MAPQ][i] = (int64_t)sum_mapq;
    }
    S.res_ready = true; S.row_next = 0;
    return 0;
}

// the next <= max_rows result rows (0 = default), in the order of the contract
int dhts_bam_coverage_next(dhts_ctx *c, int64_t max_rows, dhts_coverage_batch *out) {
    if (!c || !out) return -1;
    memset(out, 0, sizeof(*out));
    CoverageState &S = c->dep;
    if (!S.open) return fail(c, COVERAGE_NOT_OPEN);
    HIPCHK(c, hipSetDevice(c->device));
    if (max_rows <= 0) max_rows = 1 << 20;
    if (coverage_result(c)) return -1;
    const uint64_t n_out = S.o_tid.size(), avail = n_out - S.row_next;
    const int64_t nrows = avail < (uint64_t)max_rows ? (int64_t)avail : max_rows;
    S.out.assign(DHTS_COVERAGE_COL_COUNT, dhts_col());
    for (int i = 0; i < DHTS_COVERAGE_COL_COUNT; i++) { memset(&S.out[(size_t)i], 0, sizeof(dhts_col)); S.out[(size_t)i].col = i; }
    out->n_rows = nrows; out->n_cols = DHTS_COVERAGE_COL_COUNT; out->cols = S.out.data();
    if (nrows > 0) {
        ENSURE(c, S.ones, (size_t)nrows + 64);
        HIPCHK(c, hipMemsetAsync(S.ones.p, 1, (size_t)nrows, c->stream));
        for (int i = 0; i < DHTS_COVERAGE_COL_COUNT; i++) {
            ENSURE(c, S.cols[i], (size_t)nrows * 8 + 64);
            HIPCHK(c, hipMemcpyAsync(S.cols[i].p, S.h_cols[i].data() + S.row_next, (size_t)nrows * 8, hipMemcpyHostToDevice, c->stream));
            S.out[(size_t)i].fixed = S.cols[i].p; S.out[(size_t)i].valid = (const uint8_t *)S.ones.p;
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        S.row_next += (uint64_t)nrows;
    }
    out->status = S.row_next >= n_out ? 1 : 0;
    return 0;
}

// ---- read-back: out_cols[b->n_cols] = b->cols with HOST pointers into dst (every column eight bytes wide) ----------------------------
uint64_t dhts_bam_coverage_batch_host_bytes(const dhts_coverage_batch *b) {
    if (!b) return 0;
    const uint64_t n = (uint64_t)b->n_rows;
    return (uint64_t)b->n_cols * (((n + 7) & ~7ull) + n * 8);
}
int dhts_bam_coverage_batch_fetch(dhts_ctx *c, const dhts_coverage_batch *b, void *dst, uint64_t cap, dhts_col *out_cols) {
    if (!c || !b || !out_cols || (!dst && cap)) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    if (cap < dhts_bam_coverage_batch_host_bytes(b)) return fail(c, "bam_coverage: fetch buffer too small");
    uint8_t *p = (uint8_t *)dst; const uint64_t n = (uint64_t)b->n_rows;
    for (int i = 0; i < b->n_cols; i++) {
        const dhts_col &s = b->cols[i]; dhts_col &o = out_cols[i];
        memset(&o, 0, sizeof(o)); o.col = s.col;
        if (n == 0) continue;
        HIPCHK(c, hipMemcpyAsync(p, s.valid, n, hipMemcpyDeviceToHost, c->stream)); o.valid = p; p += (n + 7) & ~7ull;
        HIPCHK(c, hipMemcpyAsync(p, s.fixed, n * 8, hipMemcpyDeviceToHost, c->stream)); o.fixed = p; p += n * 8;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
