// dhts_bam_coverage.inc -- part of dhts_api.hip (included there, inside its extern "C" block; not a translation unit of its own):
// bam_coverage.  dhts_bam_coverage_open lays out the target rows (one per @SQ, or one per region given), sorts them per contig, refuses
// overlaps, and leaves the zeroed difference table, the per-row words and the step counters in HBM.  Every batch of the context's read_bam
// scan is classified and added by the kernels of bam_coverage.hip where it lies: CIGAR and QUAL are read out of the inflated stream, which
// stays in HBM with the record offsets and the CIGAR locations of the unpack pass until the next batch is made, so the pass runs behind
// dhts_bam_next_batch and the scan projects no string column.  The result is four kernels over the table and one small copy to the host,
// where the four doubles are divided (one IEEE division each) and the rows are put back into the order they were asked for in.  The target
// rows and their layout (dep_target_rows, dep_layout, with the table's cap and its debug hook), the checks in front of a batch, the kernels'
// arguments (dep_args), the scan loop, the step counters and the read-back are dhts_bam_accum.inc's.
static const uint32_t COVERAGE_COLMASK = (1u << DHTS_BAM_FLAG) | (1u << DHTS_BAM_RNAME) | (1u << DHTS_BAM_POS) | (1u << DHTS_BAM_MAPQ);   // no string column
static const AccumWho COVERAGE_WHO = {"bam_coverage", "bam_coverage: dhts_bam_coverage_open not called",
                                      "bam_coverage: a shard or block range of the file is not supported (the counts need the whole file on one device)"};

int dhts_bam_coverage_open(dhts_ctx *c, const dhts_coverage_params *p) {
    if (!c || !p) return c ? fail(c, "bam_coverage: no parameters") : -1;
    CoverageState &S = c->dep;
    S.open = false;
    if (!c->bam_open) return fail(c, "bam_coverage: dhts_bam_open not called");
    if (c->range_cut) return fail(c, "%s", COVERAGE_WHO.sharded);
    BamFilterMsg m;
    if (const char *bad = bam_filter_check(m, "bam_coverage", p->min_read_len, p->min_mapq, p->min_baseq, p->include_flags, p->require_flags, p->exclude_flags, true, true)) return fail(c, "%s", bad);
    if (p->min_depth < 1) return fail(c, "bam_coverage: min_depth must be >= 1");
    const size_t n_ref = c->ref_len.size();
    std::vector<size_t> o_given;
    dep_target_rows(c, S, o_given);
    if (dep_layout(c, S, "bam_coverage", o_given)) return -1;
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
    const int go = accum_batch_ok(c, COVERAGE_WHO, S, b, false, "CIGAR and QUAL are read where the scan left them");
    if (go <= 0) return go;
    const int64_t n = b->n_rows;
    DepArgs a;
    if (dep_args(c, S, b, a)) return -1;
    const unsigned grid = (unsigned)((n + 255) / 256), agrid = (unsigned)((n + 31) / 32);
    KTimer tm(c, DHTS_K_BCF_CHECK);
    hipLaunchKernelGGL(bam_depth_classify, dim3(grid), dim3(256), 0, c->stream, a);
    if (S.P.min_baseq > 0) hipLaunchKernelGGL(bam_depth_add<true>, dim3(agrid < DEP_ADD_MAX_BLOCKS ? agrid : DEP_ADD_MAX_BLOCKS), dim3(256), 0, c->stream, a, (int32_t *)S.diff.p, (unsigned long long *)S.words.p, (unsigned long long *)S.steps.p);
    else hipLaunchKernelGGL(bam_depth_add<false>, dim3(agrid < DEP_ADD_MAX_BLOCKS ? agrid : DEP_ADD_MAX_BLOCKS), dim3(256), 0, c->stream, a, (int32_t *)S.diff.p, (unsigned long long *)S.words.p, (unsigned long long *)S.steps.p);
    HIPCHK(c, hipGetLastError());                          // (no wait: whatever reuses the batch's buffers is queued behind these kernels)
    S.res_ready = false; S.row_next = 0;                   // a result that was being paged out starts over
    return 0;
}

int dhts_bam_coverage_scan(dhts_ctx *c, int64_t max_blocks) {
    return c ? accum_scan(c, COVERAGE_WHO, c->dep.open, max_blocks, COVERAGE_COLMASK, dhts_bam_coverage_accumulate) : -1;
}

int dhts_bam_coverage_stats(dhts_ctx *c, dhts_coverage_stats *out) {
    if (!c || !out) return c ? fail(c, "bam_coverage: no stats") : -1;
    memset(out, 0, sizeof(*out));
    CoverageState &S = c->dep;
    uint64_t s[DEP_N_STEPS];
    if (accum_steps(c, COVERAGE_WHO, S, s, DEP_N_STEPS)) return -1;
    dep_stats_common(out, s);
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
        ENSURE(c, S.tsum, (size_t)(ntiles + 1) * 4 + 64); ENSURE(c, S.tcov, (size_t)ntiles * 4 + 64); ENSURE(c, S.tdepth, (size_t)ntiles * 8 + 64); ENSURE(c, S.res, R * DEP_RES_WORDS * 8 + 64);
        {
            KTimer tm(c, DHTS_K_SCAN);
            hipLaunchKernelGGL(dep_tile_sum, dim3((unsigned)ntiles), dim3(256), 0, c->stream, (const int32_t *)S.diff.p, (uint32_t *)S.tsum.p);
            if (depth_carry<uint32_t>(c, S.part, (uint32_t *)S.tsum.p, ntiles)) return -1;
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
    if (!S.open) return fail(c, "%s", COVERAGE_WHO.not_open);
    HIPCHK(c, hipSetDevice(c->device));
    if (max_rows <= 0) max_rows = 1 << 20;
    if (coverage_result(c)) return -1;
    const uint64_t n_out = S.o_tid.size(), avail = n_out - S.row_next;
    const int64_t nrows = avail < (uint64_t)max_rows ? (int64_t)avail : max_rows;
    cols_reset(S.out, DHTS_COVERAGE_COL_COUNT);
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
uint64_t dhts_bam_coverage_batch_host_bytes(const dhts_coverage_batch *b) { return b ? cols_host_bytes(b->n_rows, b->n_cols, b->cols, col_kind_int64) : 0; }
int dhts_bam_coverage_batch_fetch(dhts_ctx *c, const dhts_coverage_batch *b, void *dst, uint64_t cap, dhts_col *out_cols) {
    return b ? cols_fetch(c, "bam_coverage", b->n_rows, b->n_cols, b->cols, col_kind_int64, dst, cap, out_cols) : -1;
}
