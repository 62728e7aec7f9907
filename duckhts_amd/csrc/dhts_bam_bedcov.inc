// dhts_bam_bedcov.inc -- part of dhts_api.hip (included there, inside its extern "C" block; not a translation unit of its own):
// bam_bedcov.  dhts_bam_bedcov_open reads contig, start and end of every row of the BED context once, builds the breakpoints on the host
// (sorting 2 n numbers belongs there, like bin_base) and leaves them, the rows' breakpoint indices and the zeroed counters in HBM.  Every
// batch of the context's read_bam scan is classified and added by the kernels of bam_bedcov.hip where it lies: the binary CIGARs are read out
// of the inflated stream, which stays in HBM with the record offsets and the CIGAR locations of the unpack pass until the next batch is
// made, so the pass runs behind dhts_bam_next_batch and the scan projects no string column.  The result is a second pass over the BED
// context: its six passthrough columns, and two columns emitted from the prefix sums for the same rows.  The pass over the BED's rows
// (bed_rows_read), the checks in front of a batch, the scan loop, the step counters and the read-back are dhts_bam_accum.inc's.
#define BEDCOV_MAX_ROWS (1ull << 27)
static uint64_t g_bedcov_max_rows = BEDCOV_MAX_ROWS;
static const uint32_t BEDCOV_COLMASK = (1u << DHTS_BAM_FLAG) | (1u << DHTS_BAM_RNAME) | (1u << DHTS_BAM_POS) | (1u << DHTS_BAM_MAPQ);   // no string column
static const AccumWho BEDCOV_WHO = {"bam_bedcov", "bam_bedcov: dhts_bam_bedcov_open not called",
                                    "bam_bedcov: a shard or block range of the file is not supported (the counts need the whole file on one device)"};

// tests: the most BED rows dhts_bam_bedcov_open takes (0: the contract's 2^27)
void dhts_debug_bedcov_max_rows(uint64_t n) { g_bedcov_max_rows = n ? n : BEDCOV_MAX_ROWS; }

static int bedcov_bed_ok(dhts_ctx *c, dhts_ctx *b) {
    if (b && (b == c || b->device != c->device)) return fail(c, "bam_bedcov: the BED context has to be a second context on the BAM context's device");
    if (!b || !b->bed.open) return fail(c, "bam_bedcov: the BED context is not open (dhts_bed_open comes first)");
    return 0;
}

int dhts_bam_bedcov_open(dhts_ctx *c, dhts_ctx *b, const dhts_bedcov_params *p) {
    if (!c || !p) return c ? fail(c, "bam_bedcov: no parameters") : -1;
    BedcovState &S = c->cov;
    S.open = false;
    if (!c->bam_open) return fail(c, "bam_bedcov: dhts_bam_open not called");
    if (bedcov_bed_ok(c, b)) return -1;
    if (c->range_cut) return fail(c, "%s", BEDCOV_WHO.sharded);
    BamFilterMsg m;
    if (const char *bad = bam_filter_check(m, "bam_bedcov", 0, p->min_mapq, 0, p->include_flags, p->require_flags, p->exclude_flags, false, false)) return fail(c, "%s", bad);
    if ((p->count_deletions != 0 && p->count_deletions != 1) || (p->count_ref_skips != 0 && p->count_ref_skips != 1)) return fail(c, "bam_bedcov: count_deletions and count_ref_skips must be 0 or 1");
    // ---- the first pass over the BED: contig, start and end of every row; a row without a contig of the header or with end <= start takes no part ----
    std::vector<int32_t> tid; std::vector<int64_t> beg, end; uint64_t n_bed = 0;
    if (bed_rows_read(c, b, g_bedcov_max_rows, tid, beg, end, n_bed)) return -1;
    for (size_t i = 0; i < tid.size(); i++) if (tid[i] < 0 || end[i] <= beg[i]) { tid[i] = -1; beg[i] = 0; end[i] = 0; }
    if (n_bed > g_bedcov_max_rows) return fail(c, "bam_bedcov: the BED file has %llu rows; at most %llu are supported", (unsigned long long)n_bed, (unsigned long long)g_bedcov_max_rows);
    // ---- breakpoints: per contig the sorted distinct starts and ends of its valid rows, concatenated ----
    const size_t n_ref = c->ref_name.size();
    std::vector<uint32_t> per(n_ref + 1, 0);
    for (uint64_t i = 0; i < n_bed; i++) if (tid[i] >= 0) per[(size_t)tid[i] + 1] += 2;
    for (size_t t = 0; t < n_ref; t++) per[t + 1] += per[t];
    std::vector<int64_t> pts(per[n_ref]);
    { std::vector<uint32_t> at(per.begin(), per.end() - 1); for (uint64_t i = 0; i < n_bed; i++) if (tid[i] >= 0) { uint32_t &w = at[(size_t)tid[i]]; pts[w++] = beg[i]; pts[w++] = end[i]; } }
    std::vector<uint32_t> base(n_ref + 1, 0); std::vector<int64_t> X; X.reserve(pts.size());
    for (size_t t = 0; t < n_ref; t++) {
        base[t] = (uint32_t)X.size();
        if (!std::is_sorted(pts.begin() + per[t], pts.begin() + per[t + 1])) std::sort(pts.begin() + per[t], pts.begin() + per[t + 1]);     // (a tiling BED arrives sorted)
        for (uint32_t k = per[t]; k < per[t + 1]; k++) if (k == per[t] || pts[k] != pts[k - 1]) X.push_back(pts[k]);
    }
    base[n_ref] = (uint32_t)X.size();
    const uint64_t M = X.size();
    std::vector<uint32_t> ks(n_bed ? n_bed : 1, COV_NO_IDX), ke(n_bed ? n_bed : 1, COV_NO_IDX);
    for (uint64_t i = 0; i < n_bed; i++) if (tid[i] >= 0) {
        const int64_t *x0 = X.data() + base[(size_t)tid[i]], *x1 = X.data() + base[(size_t)tid[i] + 1];
        ks[i] = (uint32_t)(std::lower_bound(x0, x1, beg[i]) - X.data()); ke[i] = (uint32_t)(std::lower_bound(x0, x1, end[i]) - X.data());
    }
    HIPCHK(c, hipSetDevice(c->device));
    ENSURE(c, S.steps, 64); ENSURE(c, S.base, (n_ref + 1) * 4 + 64); ENSURE(c, S.X, M * 8 + 64); ENSURE(c, S.ks, n_bed * 4 + 64); ENSURE(c, S.ke, n_bed * 4 + 64);
    ENSURE(c, S.cnt, (size_t)(M + 1) * COV_WORDS * 8 + 64);
    HIPCHK(c, hipMemsetAsync(S.steps.p, 0, 64, c->stream));
    HIPCHK(c, hipMemsetAsync(S.cnt.p, 0, (size_t)(M + 1) * COV_WORDS * 8, c->stream));
    HIPCHK(c, hipMemcpyAsync(S.base.p, base.data(), (n_ref + 1) * 4, hipMemcpyHostToDevice, c->stream));
    if (M) HIPCHK(c, hipMemcpyAsync(S.X.p, X.data(), M * 8, hipMemcpyHostToDevice, c->stream));
    if (n_bed) { HIPCHK(c, hipMemcpyAsync(S.ks.p, ks.data(), n_bed * 4, hipMemcpyHostToDevice, c->stream)); HIPCHK(c, hipMemcpyAsync(S.ke.p, ke.data(), n_bed * 4, hipMemcpyHostToDevice, c->stream)); }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    S.P = *p; S.n_ref = (int32_t)n_ref; S.status = 0; S.n_points = M; S.n_bed = n_bed; S.sums_ready = false; S.started = false; S.row_next = 0;
    S.open = true;
    return 0;
}

int dhts_bam_bedcov_accumulate(dhts_ctx *c, const dhts_bam_batch *b) {
    if (!c || !b) return c ? fail(c, "bam_bedcov: no batch") : -1;
    BedcovState &S = c->cov;
    const int go = accum_batch_ok(c, BEDCOV_WHO, S, b, false, "the CIGARs are read where the scan left them");
    if (go <= 0) return go;
    const int64_t n = b->n_rows;
    ENSURE(c, S.step, (size_t)n + 64); ENSURE(c, S.rlen, (size_t)n * 8 + 64); ENSURE(c, S.nseg, (size_t)n * 4 + 64);
    CovArgs a; memset(&a, 0, sizeof(a));
    a.u = c->last_stream.u; a.rec_off = (const uint32_t *)c->rec_off.p; a.cig_rel = (const uint32_t *)c->cig_rel.p; a.ncig_eff = (const uint32_t *)c->ncig_eff.p;
    a.flag = b->flag; a.tid = b->tid; a.pos = (const int64_t *)b->pos; a.mapq = b->mapq; a.n = (uint32_t)n; a.n_ref = S.n_ref;
    a.require = (uint32_t)S.P.require_flags; a.exclude = (uint32_t)S.P.exclude_flags; a.include = (uint32_t)S.P.include_flags; a.min_mapq = (uint32_t)S.P.min_mapq;
    a.cover_ops = (1u << 0) | (1u << 7) | (1u << 8) | (S.P.count_deletions ? 1u << 2 : 0u) | (S.P.count_ref_skips ? 1u << 3 : 0u);
    a.base = (const uint32_t *)S.base.p; a.X = (const long long *)S.X.p;
    a.step = (uint8_t *)S.step.p; a.rlen = (long long *)S.rlen.p; a.nseg = (uint32_t *)S.nseg.p;
    const unsigned grid = (unsigned)((n + 255) / 256);
    KTimer tm(c, DHTS_K_BCF_CHECK);
    hipLaunchKernelGGL(bam_cov_classify, dim3(grid), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(bam_cov_add, dim3(grid < COV_ADD_MAX_BLOCKS ? grid : COV_ADD_MAX_BLOCKS), dim3(256), 0, c->stream, a, (unsigned long long *)S.cnt.p, (unsigned long long *)S.steps.p);
    HIPCHK(c, hipGetLastError());                          // (no wait: whatever reuses the batch's buffers is queued behind these kernels)
    S.sums_ready = false; S.started = false;               // a result that was being paged out starts over
    return 0;
}

int dhts_bam_bedcov_scan(dhts_ctx *c, int64_t max_blocks) {
    return c ? accum_scan(c, BEDCOV_WHO, c->cov.open, max_blocks, BEDCOV_COLMASK, dhts_bam_bedcov_accumulate) : -1;
}

int dhts_bam_bedcov_stats(dhts_ctx *c, dhts_bedcov_stats *out) {
    if (!c || !out) return c ? fail(c, "bam_bedcov: no stats") : -1;
    memset(out, 0, sizeof(*out));
    BedcovState &S = c->cov;
    uint64_t s[COV_N_STEPS];
    if (accum_steps(c, BEDCOV_WHO, S, s, COV_N_STEPS)) return -1;
    out->n_flag_filtered = s[COV_STEP_FLAG]; out->n_unplaced = s[COV_STEP_UNPLACED]; out->n_low_mapq = s[COV_STEP_MAPQ]; out->n_counted = s[COV_STEP_COUNTED];
    for (int k = 0; k < COV_N_STEPS; k++) out->n_rows += s[k];
    out->n_bed_rows = S.n_bed; out->n_breakpoints = S.n_points; out->status = S.status;
    return 0;
}

// prefix sums of the four counter words over the whole concatenation, in S.sums: a copy of the counters (they stay: a later batch adds to
// them) scanned in place, so sums[i] = the sum in front of i and the inclusive sums of i lie in sums[i + 1]
static int bedcov_sums(dhts_ctx *c) {
    BedcovState &S = c->cov;
    if (S.sums_ready) return 0;
    const uint64_t n = S.n_points + 1;
    ENSURE(c, S.sums, (size_t)(n + 1) * sizeof(CovVec) + 64);
    KTimer tm(c, DHTS_K_SCAN);
    HIPCHK(c, hipMemcpyAsync(S.sums.p, S.cnt.p, (size_t)n * sizeof(CovVec), hipMemcpyDeviceToDevice, c->stream));
    if (scan_carry<CovVec, ScanSum, false, 4u>(c, S.partial, (CovVec *)S.sums.p, n, CovVec{})) return -1;
    HIPCHK(c, hipGetLastError());
    S.sums_ready = true;
    return 0;
}

int dhts_bam_bedcov_next(dhts_ctx *c, dhts_ctx *b, int64_t max_blocks, dhts_bedcov_batch *out) {
    if (!c || !out) return -1;
    memset(out, 0, sizeof(*out));
    BedcovState &S = c->cov;
    if (!S.open) return fail(c, "%s", BEDCOV_WHO.not_open);
    if (bedcov_bed_ok(c, b)) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    if (!S.started) {
        const int32_t proj[6] = {DHTS_BED_CHROM, DHTS_BED_START, DHTS_BED_END, DHTS_BED_NAME, DHTS_BED_SCORE, DHTS_BED_STRAND};
        if (dhts_bed_set_projection(b, proj, 6) || bed_rewind(b)) return fail(c, "%s", dhts_error(b));
        S.row_next = 0; S.started = true;
    }
    if (bedcov_sums(c)) return -1;
    dhts_bed_batch bb;
    if (dhts_bed_next_batch(b, max_blocks, &bb)) return fail(c, "%s", dhts_error(b));
    if (bb.status < 0) return fail(c, "%s", dhts_error(b));
    HIPCHK(c, hipStreamSynchronize(b->stream));             // the passthrough columns were made on the BED context's stream
    const uint64_t n = (uint64_t)bb.n_rows;
    if (bb.n_cols != 6 || S.row_next + n > S.n_bed || (bb.status == 1 && S.row_next + n != S.n_bed))
        return fail(c, "bam_bedcov: the BED context does not return the rows dhts_bam_bedcov_open read (it was used in between)");
    cols_reset(S.out, DHTS_BEDCOV_COL_COUNT);
    for (int i = 0; i < 6; i++) { S.out[(size_t)i] = bb.cols[i]; S.out[(size_t)i].col = i; }     // (DHTS_BEDCOV_CHROM .. _STRAND are DHTS_BED_CHROM .. _STRAND)
    out->n_rows = (int64_t)n; out->n_cols = DHTS_BEDCOV_COL_COUNT; out->cols = S.out.data(); out->status = bb.status;
    if (n > 0) {
        ENSURE(c, S.bases, (size_t)n * 8 + 64); ENSURE(c, S.reads, (size_t)n * 8 + 64); ENSURE(c, S.ones, (size_t)n + 64);
        HIPCHK(c, hipMemsetAsync(S.ones.p, 1, (size_t)n, c->stream));
        {
            KTimer tm(c, DHTS_K_BCF_CHECK);
            hipLaunchKernelGGL(bam_cov_emit, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const unsigned long long *)S.sums.p, (const long long *)S.X.p, (const uint32_t *)S.ks.p, (const uint32_t *)S.ke.p,
                               S.row_next, (uint32_t)n, (long long *)S.bases.p, (long long *)S.reads.p);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        S.out[DHTS_BEDCOV_BASES_COVERED].fixed = S.bases.p; S.out[DHTS_BEDCOV_BASES_COVERED].valid = (const uint8_t *)S.ones.p;
        S.out[DHTS_BEDCOV_READ_COUNT].fixed = S.reads.p; S.out[DHTS_BEDCOV_READ_COUNT].valid = (const uint8_t *)S.ones.p;
        S.row_next += n;
    }
    return 0;
}

// ---- read-back: out_cols[b->n_cols] = b->cols with HOST pointers into dst -------------------------------------------------------------
static int bedcov_col_kind(int col) { return col == DHTS_BEDCOV_START || col == DHTS_BEDCOV_END || col == DHTS_BEDCOV_BASES_COVERED || col == DHTS_BEDCOV_READ_COUNT ? COL_INT64 : COL_STRING; }
uint64_t dhts_bam_bedcov_batch_host_bytes(const dhts_bedcov_batch *b) { return b ? cols_host_bytes(b->n_rows, b->n_cols, b->cols, bedcov_col_kind) : 0; }
int dhts_bam_bedcov_batch_fetch(dhts_ctx *c, const dhts_bedcov_batch *b, void *dst, uint64_t cap, dhts_col *out_cols) {
    return b ? cols_fetch(c, "bam_bedcov", b->n_rows, b->n_cols, b->cols, bedcov_col_kind, dst, cap, out_cols) : -1;
}
