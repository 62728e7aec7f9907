// dhts_bam_pileup.inc -- part of dhts_api.hip (included there behind dhts_bam_depth.inc, inside its extern "C" block; not a translation unit
// of its own): bam_pileup.  dhts_bam_pileup_open makes bam_coverage's target rows and hands them to dep_layout with the count table's bytes
// per position (32, or 64 with strands).  A batch is classified (bam_depth_classify_del) and counted where it lies by bam_pileup_add.  The
// result is counted once (per tile of words the words that emit, their 64-bit carry, one result index per row to the host) and then emitted
// page by page as in bam_depth: the host turns the next max_rows result rows into windows of result indices and launches pil_emit on the
// tiles that hold each window.  dep_target_rows, dep_layout, dep_args, depth_carry, the page's windows and tiles (dep_page_windows,
// dep_page_tiles_of), the checks in front of a batch, the scan loop, the step counters and the read-back are dhts_bam_accum.inc's.
static const uint32_t PILEUP_COLMASK = (1u << DHTS_BAM_FLAG) | (1u << DHTS_BAM_RNAME) | (1u << DHTS_BAM_POS) | (1u << DHTS_BAM_MAPQ);   // no string column
static const AccumWho PILEUP_WHO = {"bam_pileup", "bam_pileup: dhts_bam_pileup_open not called",
                                     "bam_pileup: a shard or block range of the file is not supported (the counts need the whole file on one device)"};
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
    if (c->range_cut) return fail(c, "%s", PILEUP_WHO.sharded);
    BamFilterMsg m;
    if (const char *bad = bam_filter_check(m, "bam_pileup", p->min_read_len, p->min_mapq, p->min_baseq, p->include_flags, p->require_flags, p->exclude_flags, true, true)) return fail(c, "%s", bad);
    if (p->include_deletions < 0 || p->include_deletions > 1) return fail(c, "bam_pileup: include_deletions must be 0 or 1");
    if (p->include_insertions < 0 || p->include_insertions > 1) return fail(c, "bam_pileup: include_insertions must be 0 or 1");
    if (p->distinguish_strands < 0 || p->distinguish_strands > 1) return fail(c, "bam_pileup: distinguish_strands must be 0 or 1");
    if (p->min_nucleotide_depth < 1) return fail(c, "bam_pileup: min_nucleotide_depth must be >= 1");
    const size_t n_ref = c->ref_len.size();
    std::vector<size_t> o_given;
    dep_target_rows(c, S, o_given);                        // (bam_coverage's)
    const uint64_t words = p->distinguish_strands ? 2u * PIL_SYMBOLS : PIL_SYMBOLS;
    if (dep_layout(c, S, "bam_pileup", o_given, 4 * words, "count table")) return -1;
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
    const int go = accum_batch_ok(c, PILEUP_WHO, S, b, false, "CIGAR, SEQ and QUAL are read where the scan left them");
    if (go <= 0) return go;
    const int64_t n = b->n_rows;
    DepArgs a;
    if (dep_args(c, S, b, a)) return -1;
    const unsigned grid = (unsigned)((n + 255) / 256), agrid0 = (unsigned)((n + 31) / 32), agrid = agrid0 < DEP_ADD_MAX_BLOCKS ? agrid0 : DEP_ADD_MAX_BLOCKS;
    KTimer tm(c, DHTS_K_BCF_CHECK);
    hipLaunchKernelGGL(bam_depth_classify_del, dim3(grid), dim3(256), 0, c->stream, a);            // (a superset of what must be walked: M = X and D)
    if (S.P.min_baseq > 0) pileup_launch_add_bq<true>(c, S, a, agrid); else pileup_launch_add_bq<false>(c, S, a, agrid);
    HIPCHK(c, hipGetLastError());                          // (no wait: whatever reuses the batch's buffers is queued behind these kernels)
    S.res_ready = false; S.o_next = 0; S.o_within = 0;     // a result that was being paged out starts over
    return 0;
}

int dhts_bam_pileup_scan(dhts_ctx *c, int64_t max_blocks) {
    return c ? accum_scan(c, PILEUP_WHO, c->pil.open, max_blocks, PILEUP_COLMASK, dhts_bam_pileup_accumulate) : -1;
}

static uint32_t pileup_sshift(const PileupState &S) { return S.P.distinguish_strands ? 4u : 3u; }

int dhts_bam_pileup_stats(dhts_ctx *c, dhts_pileup_stats *out) {
    if (!c || !out) return c ? fail(c, "bam_pileup: no stats") : -1;
    memset(out, 0, sizeof(*out));
    PileupState &S = c->pil;
    uint64_t s[DEP_N_STEPS];
    if (accum_steps(c, PILEUP_WHO, S, s, DEP_N_STEPS)) return -1;
    dep_stats_common(out, s);
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
    if (!S.open) return fail(c, "%s", PILEUP_WHO.not_open);
    HIPCHK(c, hipSetDevice(c->device));
    if (max_rows <= 0) max_rows = PILEUP_DEFAULT_ROWS;
    if (pileup_result(c)) return -1;
    DepPage pg;
    dep_page_windows(S, S, max_rows, pg);
    const int64_t nrows = (int64_t)pg.rows;
    DevBuf *bufs[DHTS_PILEUP_COL_COUNT] = {&S.out_tid, &S.out_pos, &S.out_strand, &S.out_nuc, &S.out_count};
    static const size_t width[DHTS_PILEUP_COL_COUNT] = {4, 8, 1, 1, 4};
    cols_reset(S.out, DHTS_PILEUP_COL_COUNT);
    out->n_rows = nrows; out->n_cols = DHTS_PILEUP_COL_COUNT; out->cols = S.out.data();
    colmask &= (1u << DHTS_PILEUP_COL_COUNT) - 1u;
    if (nrows > 0 && colmask) {
        for (int i = 0; i < DHTS_PILEUP_COL_COUNT; i++) if ((colmask >> i) & 1u) ENSURE(c, *bufs[i], (size_t)nrows * width[i] + 64);
        const uint32_t sh = pileup_sshift(S); const uint64_t ntiles = (S.slots << sh) / PIL_TILE;
        if (dep_page_tiles_of(c, "bam_pileup", S, ntiles, pg)) return -1;
        KTimer tm(c, DHTS_K_SCAN);
        for (size_t w = 0; w < pg.wins.size(); w++) {
            const uint64_t t0 = pg.tiles[2 * w], t1 = pg.tiles[2 * w + 1];
            PilEmitArgs e; memset(&e, 0, sizeof(e));
            e.table = (const uint32_t *)S.diff.p; e.toff = (const unsigned long long *)S.toff.p; e.tile_row = (const uint32_t *)S.tile_row.p;
            e.rbase = (const unsigned long long *)S.rbase.p; e.rbeg = (const long long *)S.rbeg.p; e.rend = (const long long *)S.rend.p;
            e.row_tid = (const int32_t *)S.row_tid.p; e.sshift = sh; e.min_count = (uint32_t)S.P.min_nucleotide_depth;
            e.t0 = t0; e.o_a = pg.wins[w].o_a; e.o_b = pg.wins[w].o_b; e.dst0 = pg.wins[w].dst0;
            e.out_tid = (colmask >> DHTS_PILEUP_CHROM) & 1u ? (int32_t *)S.out_tid.p : nullptr; e.out_pos = (colmask >> DHTS_PILEUP_POS) & 1u ? (long long *)S.out_pos.p : nullptr;
            e.out_strand = (colmask >> DHTS_PILEUP_STRAND) & 1u ? (uint8_t *)S.out_strand.p : nullptr; e.out_nuc = (colmask >> DHTS_PILEUP_NUCLEOTIDE) & 1u ? (uint8_t *)S.out_nuc.p : nullptr;
            e.out_count = (colmask >> DHTS_PILEUP_COUNT) & 1u ? (int32_t *)S.out_count.p : nullptr;
            hipLaunchKernelGGL(pil_emit, dim3((unsigned)(t1 - t0 + 1)), dim3(256), 0, c->stream, e);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int i = 0; i < DHTS_PILEUP_COL_COUNT; i++) if ((colmask >> i) & 1u) S.out[(size_t)i].fixed = bufs[i]->p;
    }
    S.o_next = pg.o; S.o_within = pg.within;
    out->status = pg.o >= S.o_tid.size() ? 1 : 0;
    return 0;
}

// ---- read-back: out_cols[b->n_cols] = b->cols with HOST pointers into dst --------------------------------------------------------------
static int pileup_col_kind(int col) { return col == DHTS_PILEUP_POS ? 8 : col == DHTS_PILEUP_STRAND || col == DHTS_PILEUP_NUCLEOTIDE ? 1 : 4; }
uint64_t dhts_bam_pileup_batch_host_bytes(const dhts_pileup_batch *b) { return b ? cols_host_bytes(b->n_rows, b->n_cols, b->cols, pileup_col_kind) : 0; }
int dhts_bam_pileup_batch_fetch(dhts_ctx *c, const dhts_pileup_batch *b, void *dst, uint64_t cap, dhts_col *out_cols) {
    return b ? cols_fetch(c, "bam_pileup", b->n_rows, b->n_cols, b->cols, pileup_col_kind, dst, cap, out_cols) : -1;
}
