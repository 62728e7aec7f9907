// dhts_bam_pileup.inc -- part of dhts_api.hip (included there behind dhts_bam_depth.inc, inside its extern "C" block; not a translation unit
// of its own): bam_pileup.  dhts_bam_pileup_open makes bam_coverage's target rows and hands them to dep_layout with the count table's bytes
// per position (32, or 64 with strands).  A batch is classified (bam_depth_classify_del) and counted where it lies by bam_pileup_add.  The
// result is counted once (per tile of words the words that emit, their 64-bit carry, one result index per row to the host) and then emitted
// page by page as in bam_depth: the host turns the next max_rows result rows into windows of result indices and launches pil_emit on the
// tiles that hold each window.
static const uint32_t PILEUP_COLMASK = (1u << DHTS_BAM_FLAG) | (1u << DHTS_BAM_RNAME) | (1u << DHTS_BAM_POS) | (1u << DHTS_BAM_MAPQ);   // no string column
#define PILEUP_SHARDED "bam_pileup: a shard or block range of the file is not supported (the counts need the whole file on one device)"
#define PILEUP_NOT_OPEN "bam_pileup: dhts_bam_pileup_open not called"
#define PILEUP_DEFAULT_ROWS (1ll << 20)

// the form dhts_debug_pileup_add_form's 0 stands for (DESIGN.md 4m has the rule and the measurements)
#define PILEUP_DEFAULT_FORM 2
// tests, tools/bench_pileup.py: the add kernel's form from the next accumulate on this context (0: the default; 1: direct; 2: window)
int dhts_debug_pileup_add_form(dhts_ctx *c, int form) {
    if (!c) return -1;
    if (form < 0 || form > 2) return fail(c, "bam_pileup: add form %d is not built (0: the default, 1: direct, 2: window)", form);
    c->pil.form = form;
    return 0;
}

int dhts_bam_pileup_open(dhts_ctx *c, const dhts_pileup_params *p) {
    if (!c || !p) return c ? fail(c, "bam_pileup: no parameters") : -1;
    PileupState &S = c->pil;
    S.open = false;
    if (!c->bam_open) return fail(c, "bam_pileup: dhts_bam_open not called");
    if (c->range_cut) return fail(c, PILEUP_SHARDED);
    if (p->min_read_len < 0) return fail(c, "bam_pileup: min_read_len must be >= 0");
    if (p->min_mapq < 0 || p->min_mapq > 255) return fail(c, "bam_pileup: min_mapq must be between 0 and 255");
    if (p->min_baseq < 0 || p->min_baseq > 255) return fail(c, "bam_pileup: min_baseq must be between 0 and 255");
    if (p->include_flags < 0 || p->include_flags > 65535) return fail(c, "bam_pileup: include_flags must be between 0 and 65535");
    if (p->require_flags < 0 || p->require_flags > 65535) return fail(c, "bam_pileup: require_flags must be between 0 and 65535");
    if (p->exclude_flags < 0 || p->exclude_flags > 65535) return fail(c, "bam_pileup: exclude_flags must be between 0 and 65535");
    if (p->include_deletions < 0 || p->include_deletions > 1) return fail(c, "bam_pileup: include_deletions must be 0 or 1");
    if (p->include_insertions < 0 || p->include_insertions > 1) return fail(c, "bam_pileup: include_insertions must be 0 or 1");
    if (p->distinguish_strands < 0 || p->distinguish_strands > 1) return fail(c, "bam_pileup: distinguish_strands must be 0 or 1");
    if (p->min_nucleotide_depth < 1) return fail(c, "bam_pileup: min_nucleotide_depth must be >= 1");
    // ---- the target rows, in the order they are answered in: bam_coverage's ----
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
    const uint64_t words = p->distinguish_strands ? 2u * PIL_SYMBOLS : PIL_SYMBOLS;
    if (dep_layout(c, S, "bam_pileup", [&](size_t i) { return c->rg_given[o_given[i]].tok.c_str(); }, 4 * words, "count table")) return -1;
    const size_t R = (size_t)S.n_sorted;
    ENSURE(c, S.steps, 64); ENSURE(c, S.row_tid, (R + 1) * 4 + 64);
    HIPCHK(c, hipMemsetAsync(S.steps.p, 0, 64, c->stream));
    HIPCHK(c, hipMemcpyAsync(S.row_tid.p, S.s_tid.data(), (R + 1) * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    S.P = *p; S.n_ref = (int32_t)n_ref; S.status = 0; S.res_ready = false; S.n_result_rows = 0; S.o_next = 0; S.o_within = 0;
    S.open = true;
    return 0;
}

extern "C++" {
template <bool BQ, bool DEL, bool INS, bool STRANDS> static void pileup_launch_form(dhts_ctx *c, PileupState &S, const DepArgs &a, unsigned grid) {
    if ((S.form ? S.form : PILEUP_DEFAULT_FORM) == 2) hipLaunchKernelGGL((bam_pileup_add<BQ, DEL, INS, STRANDS, true>), dim3(grid), dim3(256), 0, c->stream, a, (uint32_t *)S.diff.p, (unsigned long long *)S.steps.p);
    else hipLaunchKernelGGL((bam_pileup_add<BQ, DEL, INS, STRANDS, false>), dim3(grid), dim3(256), 0, c->stream, a, (uint32_t *)S.diff.p, (unsigned long long *)S.steps.p);
}
template <bool BQ, bool DEL, bool INS> static void pileup_launch_add(dhts_ctx *c, PileupState &S, const DepArgs &a, unsigned grid) {
    if (S.P.distinguish_strands) pileup_launch_form<BQ, DEL, INS, true>(c, S, a, grid); else pileup_launch_form<BQ, DEL, INS, false>(c, S, a, grid);
}
template <bool BQ> static void pileup_launch_add_bq(dhts_ctx *c, PileupState &S, const DepArgs &a, unsigned grid) {
    const bool del = S.P.include_deletions != 0, ins = S.P.include_insertions != 0;
    if (del) { if (ins) pileup_launch_add<BQ, true, true>(c, S, a, grid); else pileup_launch_add<BQ, true, false>(c, S, a, grid); }
    else { if (ins) pileup_launch_add<BQ, false, true>(c, S, a, grid); else pileup_launch_add<BQ, false, false>(c, S, a, grid); }
}
}

int dhts_bam_pileup_accumulate(dhts_ctx *c, const dhts_bam_batch *b) {
    if (!c || !b) return c ? fail(c, "bam_pileup: no batch") : -1;
    PileupState &S = c->pil;
    if (!S.open) return fail(c, PILEUP_NOT_OPEN);
    if (c->range_cut) return fail(c, PILEUP_SHARDED);
    if (b->status != 0) S.status = b->status;
    const int64_t n = b->n_rows;
    if (n <= 0) return 0;
    if (n > 0x7fffff00ll || !b->flag || !b->tid || !b->pos || !b->mapq) return fail(c, "bam_pileup: the batch lacks FLAG, tid, POS or MAPQ");
    if (n != c->last_batch_rows || b->first_rec_uoff != c->last_batch_first || !c->last_stream.u || !c->rec_off.p || !c->cig_rel.p || !c->ncig_eff.p)
        return fail(c, "bam_pileup: the batch is not the one dhts_bam_next_batch returned last on this context (CIGAR, SEQ and QUAL are read where the scan left them)");
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
    KTimer tm(c, DHTS_K_BCF_CHECK);
    hipLaunchKernelGGL(bam_depth_classify_del, dim3(grid), dim3(256), 0, c->stream, a);            // (a superset of what must be walked: M = X and D)
    if (S.P.min_baseq > 0) pileup_launch_add_bq<true>(c, S, a, agrid); else pileup_launch_add_bq<false>(c, S, a, agrid);
    HIPCHK(c, hipGetLastError());                          // (no wait: whatever reuses the batch's buffers is queued behind these kernels)
    S.res_ready = false; S.o_next = 0; S.o_within = 0;     // a result that was being paged out starts over
    return 0;
}

int dhts_bam_pileup_scan(dhts_ctx *c, int64_t max_blocks) {
    if (!c) return -1;
    if (!c->pil.open) return fail(c, PILEUP_NOT_OPEN);
    if (c->range_cut) return fail(c, PILEUP_SHARDED);
    for (;;) {
        dhts_bam_batch b;
        if (dhts_bam_next_batch(c, max_blocks, PILEUP_COLMASK, &b) != 0) return -1;
        if (dhts_bam_pileup_accumulate(c, &b) != 0) return -1;
        if (b.status != 0) return b.status;
    }
}

static uint32_t pileup_sshift(const PileupState &S) { return S.P.distinguish_strands ? 4u : 3u; }

int dhts_bam_pileup_stats(dhts_ctx *c, dhts_pileup_stats *out) {
    if (!c || !out) return c ? fail(c, "bam_pileup: no stats") : -1;
    memset(out, 0, sizeof(*out));
    PileupState &S = c->pil;
    if (!S.open) return fail(c, PILEUP_NOT_OPEN);
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t s[DEP_N_STEPS];
    HIPCHK(c, hipMemcpyAsync(s, S.steps.p, sizeof(s), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out->n_flag_filtered = s[DEP_STEP_FLAG]; out->n_unplaced = s[DEP_STEP_UNPLACED]; out->n_short = s[DEP_STEP_SHORT]; out->n_low_mapq = s[DEP_STEP_MAPQ];
    out->n_outside = s[DEP_STEP_OUTSIDE]; out->n_counted = s[DEP_STEP_COUNTED];
    for (int k = 0; k < DEP_N_STEPS; k++) out->n_rows += s[k];
    out->n_target_rows = S.o_tid.size(); out->table_bytes = (S.slots << pileup_sshift(S)) * 4;
    out->n_result_rows = S.res_ready ? S.n_result_rows : 0; out->status = S.status;
    return 0;
}

// the count: the result index in front of every tile of words, and in front of every sorted row on the host
static int pileup_result(dhts_ctx *c) {
    PileupState &S = c->pil;
    if (S.res_ready) return 0;
    const size_t R = (size_t)S.n_sorted; const uint32_t sh = pileup_sshift(S); const uint64_t ntiles = (S.slots << sh) / PIL_TILE;
    S.row_off.assign(R + 1, 0);
    if (R) {
        ENSURE(c, S.toff, (size_t)(ntiles + 1) * 8 + 64); ENSURE(c, S.rowres, (R + 1) * 8 + 64);
        {
            KTimer tm(c, DHTS_K_SCAN);
            hipLaunchKernelGGL(pil_tile_count, dim3((unsigned)ntiles), dim3(256), 0, c->stream, (const uint32_t *)S.diff.p, (const uint32_t *)S.tile_row.p, (const unsigned long long *)S.rbase.p,
                               (const long long *)S.rbeg.p, (const long long *)S.rend.p, sh, (uint32_t)S.P.min_nucleotide_depth, (unsigned long long *)S.toff.p);
            if (depth_carry<unsigned long long>(c, S.part, (unsigned long long *)S.toff.p, ntiles)) return -1;
            hipLaunchKernelGGL(pil_row_offsets, dim3((unsigned)((R + 1 + 255) / 256)), dim3(256), 0, c->stream, (const unsigned long long *)S.toff.p, (const unsigned long long *)S.rbase.p,
                               sh, (uint64_t)R, ntiles, (unsigned long long *)S.rowres.p);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(S.row_off.data(), S.rowres.p, (R + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    S.n_result_rows = S.row_off[R]; S.res_ready = true; S.o_next = 0; S.o_within = 0;
    return 0;
}

int dhts_bam_pileup_next(dhts_ctx *c, int64_t max_rows, uint32_t colmask, dhts_pileup_batch *out) {
    if (!c || !out) return -1;
    memset(out, 0, sizeof(*out));
    PileupState &S = c->pil;
    if (!S.open) return fail(c, PILEUP_NOT_OPEN);
    HIPCHK(c, hipSetDevice(c->device));
    if (max_rows <= 0) max_rows = PILEUP_DEFAULT_ROWS;
    if (pileup_result(c)) return -1;
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
    DevBuf *bufs[DHTS_PILEUP_COL_COUNT] = {&S.out_tid, &S.out_pos, &S.out_strand, &S.out_nuc, &S.out_count};
    static const size_t width[DHTS_PILEUP_COL_COUNT] = {4, 8, 1, 1, 4};
    S.out.assign(DHTS_PILEUP_COL_COUNT, dhts_col());
    for (int i = 0; i < DHTS_PILEUP_COL_COUNT; i++) { memset(&S.out[(size_t)i], 0, sizeof(dhts_col)); S.out[(size_t)i].col = i; }
    out->n_rows = nrows; out->n_cols = DHTS_PILEUP_COL_COUNT; out->cols = S.out.data();
    colmask &= (1u << DHTS_PILEUP_COL_COUNT) - 1u;
    if (nrows > 0 && colmask) {
        for (int i = 0; i < DHTS_PILEUP_COL_COUNT; i++) if ((colmask >> i) & 1u) ENSURE(c, *bufs[i], (size_t)nrows * width[i] + 64);
        const uint32_t sh = pileup_sshift(S); const uint64_t ntiles = (S.slots << sh) / PIL_TILE;
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
            if (t1 < t0 || t1 >= ntiles) return fail(c, "bam_pileup: internal error: the tiles of a page are out of range");
            PilEmitArgs e; memset(&e, 0, sizeof(e));
            e.table = (const uint32_t *)S.diff.p; e.toff = (const unsigned long long *)S.toff.p; e.tile_row = (const uint32_t *)S.tile_row.p;
            e.rbase = (const unsigned long long *)S.rbase.p; e.rbeg = (const long long *)S.rbeg.p; e.rend = (const long long *)S.rend.p;
            e.row_tid = (const int32_t *)S.row_tid.p; e.sshift = sh; e.min_count = (uint32_t)S.P.min_nucleotide_depth;
            e.t0 = t0; e.o_a = wins[w].o_a; e.o_b = wins[w].o_b; e.dst0 = wins[w].dst0;
            e.out_tid = (colmask >> DHTS_PILEUP_CHROM) & 1u ? (int32_t *)S.out_tid.p : nullptr; e.out_pos = (colmask >> DHTS_PILEUP_POS) & 1u ? (long long *)S.out_pos.p : nullptr;
            e.out_strand = (colmask >> DHTS_PILEUP_STRAND) & 1u ? (uint8_t *)S.out_strand.p : nullptr; e.out_nuc = (colmask >> DHTS_PILEUP_NUCLEOTIDE) & 1u ? (uint8_t *)S.out_nuc.p : nullptr;
            e.out_count = (colmask >> DHTS_PILEUP_COUNT) & 1u ? (int32_t *)S.out_count.p : nullptr;
            hipLaunchKernelGGL(pil_emit, dim3((unsigned)(t1 - t0 + 1)), dim3(256), 0, c->stream, e);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int i = 0; i < DHTS_PILEUP_COL_COUNT; i++) if ((colmask >> i) & 1u) S.out[(size_t)i].fixed = bufs[i]->p;
    }
    S.o_next = o; S.o_within = within;
    out->status = o >= n_out ? 1 : 0;
    return 0;
}

// ---- read-back: out_cols[b->n_cols] = b->cols with HOST pointers into dst --------------------------------------------------------------
static uint64_t pileup_col_width(int col) { return col == DHTS_PILEUP_POS ? 8 : col == DHTS_PILEUP_STRAND || col == DHTS_PILEUP_NUCLEOTIDE ? 1 : 4; }
static uint64_t pileup_col_bytes(int col, uint64_t n) { return (n * pileup_col_width(col) + 7) & ~7ull; }
uint64_t dhts_bam_pileup_batch_host_bytes(const dhts_pileup_batch *b) {
    if (!b) return 0;
    uint64_t need = 0;
    for (int i = 0; i < b->n_cols; i++) if (b->cols[i].fixed) need += pileup_col_bytes(b->cols[i].col, (uint64_t)b->n_rows);
    return need;
}
int dhts_bam_pileup_batch_fetch(dhts_ctx *c, const dhts_pileup_batch *b, void *dst, uint64_t cap, dhts_col *out_cols) {
    if (!c || !b || !out_cols || (!dst && cap)) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    if (cap < dhts_bam_pileup_batch_host_bytes(b)) return fail(c, "bam_pileup: fetch buffer too small");
    uint8_t *p = (uint8_t *)dst; const uint64_t n = (uint64_t)b->n_rows;
    for (int i = 0; i < b->n_cols; i++) {
        const dhts_col &s = b->cols[i]; dhts_col &o = out_cols[i];
        memset(&o, 0, sizeof(o)); o.col = s.col;
        if (n == 0 || !s.fixed) continue;
        HIPCHK(c, hipMemcpyAsync(p, s.fixed, n * pileup_col_width(s.col), hipMemcpyDeviceToHost, c->stream)); o.fixed = p; p += pileup_col_bytes(s.col, n);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
