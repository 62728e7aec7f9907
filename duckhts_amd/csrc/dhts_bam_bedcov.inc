// dhts_bam_bedcov.inc -- part of dhts_api.hip (included there, inside its extern "C" block; not a translation unit of its own):
// bam_bedcov.  dhts_bam_bedcov_open reads contig, start and end of every row of the BED context once, builds the breakpoints on the host
// (sorting 2 n numbers belongs there, like bin_base) and leaves them, the rows' breakpoint indices and the zeroed counters in HBM.  Every
// batch of the context's read_bam scan is classified and added by the kernels of bam_bedcov.hip where it lies: the binary CIGARs are read out
// of the inflated stream, which stays in HBM with the record offsets and the CIGAR locations of the unpack pass until the next batch is
// made, so the pass runs behind dhts_bam_next_batch and the scan projects no string column.  The result is a second pass over the BED
// context: its six passthrough columns, and two columns emitted from the prefix sums for the same rows.
#define BEDCOV_MAX_ROWS (1ull << 27)
static uint64_t g_bedcov_max_rows = BEDCOV_MAX_ROWS;
static const uint32_t BEDCOV_COLMASK = (1u << DHTS_BAM_FLAG) | (1u << DHTS_BAM_RNAME) | (1u << DHTS_BAM_POS) | (1u << DHTS_BAM_MAPQ);   // no string column
#define BEDCOV_SHARDED "bam_bedcov: a shard or block range of the file is not supported (the counts need the whole file on one device)"

// tests: the most BED rows dhts_bam_bedcov_open takes (0: the contract's 2^27)
void dhts_debug_bedcov_max_rows(uint64_t n) { g_bedcov_max_rows = n ? n : BEDCOV_MAX_ROWS; }

static int bedcov_bed_ok(dhts_ctx *c, dhts_ctx *b) {
    if (b && (b == c || b->device != c->device)) return fail(c, "bam_bedcov: the BED context has to be a second context on the BAM context's device");
    if (!b || !b->bed.open) return fail(c, "bam_bedcov: the BED context is not open (dhts_bed_open comes first)");
    return 0;
}

// One pass over the BED context b (after dhts_bed_open): contig, start and end of every row, for bam_bedcov and bam_depth.  tid[i] = the
// contig's id in c's header (the first @SQ of a name listed twice), -1 for a name it lacks or a NULL chrom; a row whose start or end is NULL has
// beg = end = 0.  Rows behind max_rows are counted in n_bed and not kept.  Errors of b become c's.
static int bed_rows_read(dhts_ctx *c, dhts_ctx *b, uint64_t max_rows, std::vector<int32_t> &tid, std::vector<int64_t> &beg, std::vector<int64_t> &end, uint64_t &n_bed) {
    const int32_t proj[3] = {DHTS_BED_CHROM, DHTS_BED_START, DHTS_BED_END};
    if (dhts_bed_set_projection(b, proj, 3) || bed_rewind(b)) return fail(c, "%s", dhts_error(b));
    std::map<std::string, int32_t> tid_of;
    for (size_t t = 0; t < c->ref_name.size(); t++) tid_of.emplace(c->ref_name[t], (int32_t)t);   // (a name listed twice: the first @SQ, as sam_hdr_name2tid's hash keeps)
    n_bed = 0; std::string last_name; int32_t last_tid = -1; bool have_last = false;
    std::vector<uint8_t> arena;
    for (;;) {
        dhts_bed_batch bb;
        if (dhts_bed_next_batch(b, 0, &bb)) return fail(c, "%s", dhts_error(b));
        const uint64_t n = (uint64_t)bb.n_rows;
        if (n && n_bed + n <= max_rows) {
            dhts_col hc[3];
            arena.resize((size_t)dhts_bed_batch_host_bytes(&bb) + 8);
            if (dhts_bed_batch_fetch(b, &bb, arena.data(), arena.size(), hc)) return fail(c, "%s", dhts_error(b));
            const int64_t *hs = (const int64_t *)hc[1].fixed, *he = (const int64_t *)hc[2].fixed;
            for (uint64_t r = 0; r < n; r++) {
                int32_t t = -1;
                if (hc[0].valid[r]) {
                    const char *nm = (const char *)hc[0].bytes + hc[0].off[r]; const size_t nl = hc[0].off[r + 1] - hc[0].off[r];
                    if (!have_last || last_name.size() != nl || memcmp(last_name.data(), nm, nl) != 0) {
                        last_name.assign(nm, nl); have_last = true;
                        auto it = tid_of.find(last_name); last_tid = it == tid_of.end() ? -1 : it->second;
                    }
                    t = last_tid;
                }
                const bool have = hc[1].valid[r] && hc[2].valid[r];
                tid.push_back(t); beg.push_back(have ? hs[r] : 0); end.push_back(have ? he[r] : 0);
            }
        }
        n_bed += n;
        if (bb.status < 0) return fail(c, "%s", dhts_error(b));
        if (bb.status != 0) break;
    }
    return 0;
}

int dhts_bam_bedcov_open(dhts_ctx *c, dhts_ctx *b, const dhts_bedcov_params *p) {
    if (!c || !p) return c ? fail(c, "bam_bedcov: no parameters") : -1;
    BedcovState &S = c->cov;
    S.open = false;
    if (!c->bam_open) return fail(c, "bam_bedcov: dhts_bam_open not called");
    if (bedcov_bed_ok(c, b)) return -1;
    if (c->range_cut) return fail(c, BEDCOV_SHARDED);
    if (p->min_mapq < 0 || p->min_mapq > 255) return fail(c, "bam_bedcov: min_mapq must be between 0 and 255");
    if (p->include_flags < 0 || p->include_flags > 65535) return fail(c, "bam_bedcov: include_flags must be between 0 and 65535");
    if (p->require_flags < 0 || p->require_flags > 65535) return fail(c, "bam_bedcov: require_flags must be between 0 and 65535");
    if (p->exclude_flags < 0 || p->exclude_flags > 65535) return fail(c, "bam_bedcov: exclude_flags must be between 0 and 65535");
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
    if (!S.open) return fail(c, "bam_bedcov: dhts_bam_bedcov_open not called");
    if (c->range_cut) return fail(c, BEDCOV_SHARDED);
    if (b->status != 0) S.status = b->status;
    const int64_t n = b->n_rows;
    if (n <= 0) return 0;
    if (n > 0x7fffff00ll || !b->flag || !b->tid || !b->pos || !b->mapq) return fail(c, "bam_bedcov: the batch lacks FLAG, tid, POS or MAPQ");
    if (n != c->last_batch_rows || b->first_rec_uoff != c->last_batch_first || !c->last_stream.u || !c->rec_off.p || !c->cig_rel.p || !c->ncig_eff.p)
        return fail(c, "bam_bedcov: the batch is not the one dhts_bam_next_batch returned last on this context (the CIGARs are read where the scan left them)");
    HIPCHK(c, hipSetDevice(c->device));
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

// the context's scan to the end of the stream; returns the status it ended on (1, or the negative status of a stream that ended on an error:
// its rows are counted), < 0 with dhts_error set when a call failed (dhts_bedcov_stats.status stays 0 then)
int dhts_bam_bedcov_scan(dhts_ctx *c, int64_t max_blocks) {
    if (!c) return -1;
    if (!c->cov.open) return fail(c, "bam_bedcov: dhts_bam_bedcov_open not called");
    if (c->range_cut) return fail(c, BEDCOV_SHARDED);
    for (;;) {
        dhts_bam_batch b;
        if (dhts_bam_next_batch(c, max_blocks, BEDCOV_COLMASK, &b) != 0) return -1;
        if (dhts_bam_bedcov_accumulate(c, &b) != 0) return -1;
        if (b.status != 0) return b.status;
    }
}

int dhts_bam_bedcov_stats(dhts_ctx *c, dhts_bedcov_stats *out) {
    if (!c || !out) return c ? fail(c, "bam_bedcov: no stats") : -1;
    memset(out, 0, sizeof(*out));
    BedcovState &S = c->cov;
    if (!S.open) return fail(c, "bam_bedcov: dhts_bam_bedcov_open not called");
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t s[COV_N_STEPS];
    HIPCHK(c, hipMemcpyAsync(s, S.steps.p, sizeof(s), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out->n_flag_filtered = s[COV_STEP_FLAG]; out->n_unplaced = s[COV_STEP_UNPLACED]; out->n_low_mapq = s[COV_STEP_MAPQ]; out->n_counted = s[COV_STEP_COUNTED];
    for (int k = 0; k < COV_N_STEPS; k++) out->n_rows += s[k];
    out->n_bed_rows = S.n_bed; out->n_breakpoints = S.n_points; out->status = S.status;
    return 0;
}

// inclusive prefix sums of the four counter words over the whole concatenation, into S.sums (the counters stay: a later batch adds to them)
static int bedcov_sums(dhts_ctx *c) {
    BedcovState &S = c->cov;
    if (S.sums_ready) return 0;
    const uint64_t n = S.n_points + 1, ntiles = (n + COV_TILE - 1) / COV_TILE;
    ENSURE(c, S.sums, (size_t)n * COV_WORDS * 8 + 64); ENSURE(c, S.partial, (size_t)ntiles * COV_WORDS * 8 + 64);
    KTimer tm(c, DHTS_K_SCAN);
    hipLaunchKernelGGL(cov_scan_reduce, dim3((unsigned)ntiles), dim3(256), 0, c->stream, (const unsigned long long *)S.cnt.p, n, (unsigned long long *)S.partial.p);
    hipLaunchKernelGGL(cov_scan_partials, dim3(1), dim3(256), 0, c->stream, (unsigned long long *)S.partial.p, ntiles);
    hipLaunchKernelGGL(cov_scan_apply, dim3((unsigned)ntiles), dim3(256), 0, c->stream, (const unsigned long long *)S.cnt.p, n, (const unsigned long long *)S.partial.p, (unsigned long long *)S.sums.p);
    HIPCHK(c, hipGetLastError());
    S.sums_ready = true;
    return 0;
}

int dhts_bam_bedcov_next(dhts_ctx *c, dhts_ctx *b, int64_t max_blocks, dhts_bedcov_batch *out) {
    if (!c || !out) return -1;
    memset(out, 0, sizeof(*out));
    BedcovState &S = c->cov;
    if (!S.open) return fail(c, "bam_bedcov: dhts_bam_bedcov_open not called");
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
    S.out.assign(DHTS_BEDCOV_COL_COUNT, dhts_col());
    for (int i = 0; i < DHTS_BEDCOV_COL_COUNT; i++) { memset(&S.out[(size_t)i], 0, sizeof(dhts_col)); S.out[(size_t)i].col = i; }
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
static bool bedcov_col_is_int(int col) { return col == DHTS_BEDCOV_START || col == DHTS_BEDCOV_END || col == DHTS_BEDCOV_BASES_COVERED || col == DHTS_BEDCOV_READ_COUNT; }
uint64_t dhts_bam_bedcov_batch_host_bytes(const dhts_bedcov_batch *b) {
    if (!b) return 0;
    uint64_t need = 0; const uint64_t n = (uint64_t)b->n_rows;
    for (int i = 0; i < b->n_cols; i++) {
        need += (n + 7) & ~7ull;
        if (bedcov_col_is_int(b->cols[i].col)) need += n * 8; else need += (((n + 1) * 4 + 7) & ~7ull) + ((b->cols[i].nbytes + 7) & ~7ull);
    }
    return need;
}
int dhts_bam_bedcov_batch_fetch(dhts_ctx *c, const dhts_bedcov_batch *b, void *dst, uint64_t cap, dhts_col *out_cols) {
    if (!c || !b || !out_cols || (!dst && cap)) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    if (cap < dhts_bam_bedcov_batch_host_bytes(b)) return fail(c, "bam_bedcov: fetch buffer too small");
    uint8_t *p = (uint8_t *)dst; const uint64_t n = (uint64_t)b->n_rows;
    for (int i = 0; i < b->n_cols; i++) {
        const dhts_col &s = b->cols[i]; dhts_col &o = out_cols[i];
        memset(&o, 0, sizeof(o)); o.col = s.col;
        if (n == 0) continue;
        HIPCHK(c, hipMemcpyAsync(p, s.valid, n, hipMemcpyDeviceToHost, c->stream)); o.valid = p; p += (n + 7) & ~7ull;
        if (bedcov_col_is_int(s.col)) { HIPCHK(c, hipMemcpyAsync(p, s.fixed, n * 8, hipMemcpyDeviceToHost, c->stream)); o.fixed = p; p += n * 8; }
        else {
            HIPCHK(c, hipMemcpyAsync(p, s.off, (n + 1) * 4, hipMemcpyDeviceToHost, c->stream)); o.off = (const uint32_t *)p; p += ((n + 1) * 4 + 7) & ~7ull;
            if (s.nbytes) HIPCHK(c, hipMemcpyAsync(p, s.bytes, s.nbytes, hipMemcpyDeviceToHost, c->stream));
            o.bytes = p; o.nbytes = s.nbytes; p += (s.nbytes + 7) & ~7ull;
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
