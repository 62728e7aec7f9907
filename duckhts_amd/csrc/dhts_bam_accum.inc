// dhts_bam_accum.inc -- part of dhts_api.hip (included there in front of dhts_bam_bins.inc, inside its extern "C" block; not a translation unit
// of its own): the host scaffold of the seven bam_* count functions (bam_bin_counts, bam_bedcov, bam_coverage, bam_depth, bam_pileup, bam_bedgraph, bam_depth_hist).  It owns
// what carries none of the work and was the same in all of them: the checks in front of an accumulate, the scan loop, the read-out of the step
// counters, the target rows and their layout in the table (dep_layout), the arguments of the depth kernels, the windows and tiles of a result
// page, the reset of a result batch's columns, and the read-back of dhts_col columns.  A function keeps its own extern "C" entry points, its
// parameters' own checks, its kernels and their launches, and its result.  Plain functions and small structs: the states derive from
// AccumBase / DepLayout / DepPager (dhts_api.hip).

// who is asking: the function's name as the errors' prefix, and its two standing errors
struct AccumWho { const char *fn, *not_open, *sharded; };

// ---- accumulate, scan, stats ------------------------------------------------------------------------------------------------------------
// The checks in front of an accumulate (c and b are not null): -1 with the error set, 0 when the batch has no rows (its status is latched),
// 1 to go on.  stream_tail: what the function reads where the scan left it -- the parenthesis of the stale-batch error -- or nullptr for a
// function that reads the batch's columns only (bam_bin_counts: no such check, and PNEXT is needed).
static int accum_batch_ok(dhts_ctx *c, const AccumWho &w, AccumBase &S, const dhts_bam_batch *b, bool need_pnext, const char *stream_tail) {
    if (!S.open) return fail(c, "%s", w.not_open);
    if (c->range_cut) return fail(c, "%s", w.sharded);
    if (b->status != 0) S.status = b->status;
    const int64_t n = b->n_rows;
    if (n <= 0) return 0;
    if (n > 0x7fffff00ll || !b->flag || !b->tid || !b->pos || !b->mapq || (need_pnext && !b->pnext)) return fail(c, "%s: the batch lacks %s", w.fn, need_pnext ? "FLAG, tid, POS, MAPQ or PNEXT" : "FLAG, tid, POS or MAPQ");
    if (stream_tail && (n != c->last_batch_rows || b->first_rec_uoff != c->last_batch_first || !c->last_stream.u || !c->rec_off.p || !c->cig_rel.p || !c->ncig_eff.p))
        return fail(c, "%s: the batch is not the one dhts_bam_next_batch returned last on this context (%s)", w.fn, stream_tail);
    HIPCHK(c, hipSetDevice(c->device));
    return 1;
}

// the context's scan to the end of the stream; returns the status it ended on (1, or the negative status of a stream that ended on an error:
// its rows are counted), < 0 with dhts_error set when a call failed (the stats' status stays 0 then)
static int accum_scan(dhts_ctx *c, const AccumWho &w, bool open, int64_t max_blocks, uint32_t colmask, int (*accumulate)(dhts_ctx *, const dhts_bam_batch *)) {
    if (!open) return fail(c, "%s", w.not_open);
    if (c->range_cut) return fail(c, "%s", w.sharded);
    for (;;) {
        dhts_bam_batch b;
        if (dhts_bam_next_batch(c, max_blocks, colmask, &b) != 0) return -1;
        if (accumulate(c, &b) != 0) return -1;
        if (b.status != 0) return b.status;
    }
}

// the n step counters on the host (one copy, one wait)
static int accum_steps(dhts_ctx *c, const AccumWho &w, AccumBase &S, uint64_t *s, int n) {
    if (!S.open) return fail(c, "%s", w.not_open);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(s, S.steps.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// a result batch's columns, all absent
static void cols_reset(std::vector<dhts_col> &out, int n) {
    out.assign((size_t)n, dhts_col());
    for (int i = 0; i < n; i++) { memset(&out[(size_t)i], 0, sizeof(dhts_col)); out[(size_t)i].col = i; }
}

// ---- the rows of a BED context ------------------------------------------------------------------------------------------------------------
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

// ---- the layout bam_coverage, bam_depth, bam_pileup, bam_bedgraph and bam_depth_hist share ------------------------------------------------------------------------------
#define COVERAGE_MAX_TABLE_BYTES (16ull << 30)
static uint64_t g_coverage_max_table_bytes = COVERAGE_MAX_TABLE_BYTES;
// tests: the most bytes the table may take (0: the contract's 16 GiB)
void dhts_debug_coverage_max_table_bytes(uint64_t n) { g_coverage_max_table_bytes = n ? n : COVERAGE_MAX_TABLE_BYTES; }

// the target rows, in the order they are answered in: the regions that name a contig, clipped to it, or every @SQ ('.' and '*' name no row).
// o_given[i]: the region row i was given as
static void dep_target_rows(const dhts_ctx *c, DepLayout &L, std::vector<size_t> &o_given) {
    L.o_tid.clear(); L.o_beg.clear(); L.o_end.clear(); L.o_k.clear();
    if (c->rg_active && !c->rg_given.empty()) {
        for (size_t g = 0; g < c->rg_given.size(); g++) {
            const auto &r = c->rg_given[g];
            const int64_t len = (int64_t)c->ref_len[(size_t)r.tid];
            L.o_tid.push_back(r.tid); L.o_beg.push_back(r.beg < len ? r.beg : len); L.o_end.push_back(r.end < len ? r.end : len); o_given.push_back(g);
        }
    } else for (size_t t = 0; t < c->ref_len.size(); t++) { L.o_tid.push_back((int32_t)t); L.o_beg.push_back(0); L.o_end.push_back((int64_t)c->ref_len[t]); }
}

// the target rows of a BED context b (bam_depth, bam_bedgraph, bam_depth_hist): the union of its rows -- per contig in header order, sorted by start, rows that
// overlap or touch merged, clipped to the contig, empty ones dropped.  n_skipped: the rows that name a contig the header lacks
static int dep_bed_target_rows(dhts_ctx *c, dhts_ctx *b, DepLayout &L, uint64_t &n_skipped) {
    L.o_tid.clear(); L.o_beg.clear(); L.o_end.clear(); L.o_k.clear();
    n_skipped = 0;
    std::vector<int32_t> tid; std::vector<int64_t> beg, end; uint64_t n_bed = 0;
    if (bed_rows_read(c, b, ~0ull, tid, beg, end, n_bed)) return -1;
    std::vector<uint32_t> order;
    for (size_t i = 0; i < tid.size(); i++) {
        if (tid[i] < 0) { n_skipped++; continue; }
        const int64_t len = (int64_t)c->ref_len[(size_t)tid[i]];
        if (beg[i] < 0) beg[i] = 0;
        if (end[i] > len) end[i] = len;
        if (end[i] > beg[i]) order.push_back((uint32_t)i);
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return tid[x] != tid[y] ? tid[x] < tid[y] : beg[x] < beg[y]; });
    for (const uint32_t i : order) {
        if (!L.o_tid.empty() && L.o_tid.back() == tid[i] && beg[i] <= L.o_end.back()) { if (end[i] > L.o_end.back()) L.o_end.back() = end[i]; }
        else { L.o_tid.push_back(tid[i]); L.o_beg.push_back(beg[i]); L.o_end.push_back(end[i]); }
    }
    return 0;
}

// S.o_tid / o_beg / o_end hold the target rows in the order they are answered in, clipped.  They are sorted by (contig, start) with the empty
// ones left out (o_k: a row's index among the sorted ones, -1 for an empty one), neighbours on one contig must not overlap (o_given: what the
// rows were given as, for the error), every sorted row gets a span of (end - beg) + 1 slots of the table rounded up to the tile, and the rows,
// tid_first, tile_row and the zeroed table go to the device (queued on the stream).
// bpp / noun: the table's bytes per slot and what the cap's error calls it (bam_pileup's count table has 32 or 64 bytes per position).
static int dep_layout(dhts_ctx *c, DepLayout &S, const char *fn, const std::vector<size_t> &o_given, uint64_t bpp = 4, const char *noun = "depth table") {
    const size_t n_ref = c->ref_len.size(), n_out = S.o_tid.size();
    std::vector<uint32_t> order;
    for (size_t i = 0; i < n_out; i++) if (S.o_end[i] > S.o_beg[i]) order.push_back((uint32_t)i);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return S.o_tid[x] != S.o_tid[y] ? S.o_tid[x] < S.o_tid[y] : S.o_beg[x] < S.o_beg[y]; });
    for (size_t j = 1; j < order.size(); j++) {
        const uint32_t x = order[j - 1], y = order[j];
        if (S.o_tid[x] == S.o_tid[y] && S.o_beg[y] < S.o_end[x]) {
            const uint32_t first = x < y ? x : y, second = x < y ? y : x;
            return fail(c, "%s: the regions '%s' and '%s' overlap (one row is answered per region: give disjoint regions)", fn,
                        c->rg_given[o_given[first]].tok.c_str(), c->rg_given[o_given[second]].tok.c_str());
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

extern "C++" {
// the per-batch scratch and the arguments of the depth kernels (bam_depth_classify* and the add kernels of bam_coverage, bam_depth and
// bam_pileup; bam_bedgraph and bam_depth_hist launch bam_depth's) from the batch, the scan's stream, the layout and the function's filter; S: CoverageState, DepthState,
// PileupState, BedgraphState or HistState
template <typename State> static int dep_args(dhts_ctx *c, State &S, const dhts_bam_batch *b, DepArgs &a) {
    const int64_t n = b->n_rows;
    ENSURE(c, S.step, (size_t)n + 64); ENSURE(c, S.rlen, (size_t)n * 8 + 64); ENSURE(c, S.k0, (size_t)n * 4 + 64); ENSURE(c, S.k1, (size_t)n * 4 + 64);
    memset(&a, 0, sizeof(a));
    a.u = c->last_stream.u; a.rec_off = (const uint32_t *)c->rec_off.p; a.cig_rel = (const uint32_t *)c->cig_rel.p; a.ncig_eff = (const uint32_t *)c->ncig_eff.p;
    a.flag = b->flag; a.tid = b->tid; a.pos = (const int64_t *)b->pos; a.mapq = b->mapq; a.n = (uint32_t)n; a.n_ref = S.n_ref;
    a.require = (uint32_t)S.P.require_flags; a.exclude = (uint32_t)S.P.exclude_flags; a.include = (uint32_t)S.P.include_flags; a.min_mapq = (uint32_t)S.P.min_mapq;
    a.min_baseq = (uint32_t)S.P.min_baseq; a.min_read_len = (long long)S.P.min_read_len;
    a.tid_first = (const uint32_t *)S.tid_first.p; a.rbeg = (const long long *)S.rbeg.p; a.rend = (const long long *)S.rend.p; a.rbase = (const unsigned long long *)S.rbase.p;
    a.step = (uint8_t *)S.step.p; a.rlen = (long long *)S.rlen.p; a.k0 = (uint32_t *)S.k0.p; a.k1 = (uint32_t *)S.k1.p;
    return 0;
}

// the seven counters dhts_coverage_stats, dhts_depth_stats, dhts_pileup_stats, dhts_bedgraph_stats and dhts_depth_hist_stats share, from the DEP_N_STEPS step counters
template <typename Stats> static void dep_stats_common(Stats *out, const uint64_t *s) {
    out->n_flag_filtered = s[DEP_STEP_FLAG]; out->n_unplaced = s[DEP_STEP_UNPLACED]; out->n_short = s[DEP_STEP_SHORT]; out->n_low_mapq = s[DEP_STEP_MAPQ];
    out->n_outside = s[DEP_STEP_OUTSIDE]; out->n_counted = s[DEP_STEP_COUNTED];
    for (int k = 0; k < DEP_N_STEPS; k++) out->n_rows += s[k];
}

// the carry in two levels (dev_scan.hip) over v[0 .. n) in place: v[i] = seed combined with the elements in front of i, the total in v[n]
// (the buffer has n + 1 elements); REV: with the elements behind i, and no total.  part: scratch
template <typename T, typename Op, bool REV, uint32_t PER = 16u> static int scan_carry(dhts_ctx *c, DevBuf &part, T *v, uint64_t n, T seed) {
    const uint64_t np = (n + 256u * PER - 1) / (256u * PER);
    ENSURE(c, part, (size_t)(np + 1) * sizeof(T) + 64);
    hipLaunchKernelGGL((carry_reduce<T, Op, PER>), dim3((unsigned)np), dim3(256), 0, c->stream, (const T *)v, n, (T *)part.p);
    hipLaunchKernelGGL((carry_scan<T, Op, REV, PER>), dim3(1), dim3(256), 0, c->stream, (T *)part.p, np, seed);
    hipLaunchKernelGGL((carry_apply<T, Op, REV, PER>), dim3((unsigned)np), dim3(256), 0, c->stream, v, n, (const T *)part.p, np);
    return 0;
}
// an exclusive sum of v[0 .. n) in place, the total in v[n]
template <typename T> static int depth_carry(dhts_ctx *c, DevBuf &part, T *v, uint64_t n) { return scan_carry<T, ScanSum, false>(c, part, v, n, (T)0); }
}

// tests: the carry alone, through the launcher the count functions call, on host_v (n elements in; the forward kinds return n + 1, the total
// last).  kind 0: uint32_t sum; 1: uint64 sum; 2: uint64 suffix minimum, seeded; 3: CovVec sum, four elements per thread.  The data and the
// chunk values lie in the context's compressor scratch (z_in, z_tok).  host_v has room for n + 1 elements and element n goes to the device
// as it is: the carry must not read it, so the caller puts a value there that would show.
int dhts_debug_carry(dhts_ctx *c, int kind, void *host_v, uint64_t n, uint64_t seed) {
    if (!c) return -1;
    if (kind < 0 || kind > 3 || !host_v || n == 0 || n > (1ull << 28)) return fail(c, "debug_carry: arguments out of range");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t esz = kind == 0 ? 4 : kind == 3 ? sizeof(CovVec) : 8, n_out = (size_t)n + (kind == 2 ? 0 : 1);
    ENSURE(c, c->z_in, ((size_t)n + 1) * esz + 64);
    HIPCHK(c, hipMemcpyAsync(c->z_in.p, host_v, ((size_t)n + 1) * esz, hipMemcpyHostToDevice, c->stream));
    int rc;
    if (kind == 0) rc = depth_carry<uint32_t>(c, c->z_tok, (uint32_t *)c->z_in.p, n);
    else if (kind == 1) rc = depth_carry<unsigned long long>(c, c->z_tok, (unsigned long long *)c->z_in.p, n);
    else if (kind == 2) rc = scan_carry<unsigned long long, ScanMin, true>(c, c->z_tok, (unsigned long long *)c->z_in.p, n, (unsigned long long)seed);
    else rc = scan_carry<CovVec, ScanSum, false, 4u>(c, c->z_tok, (CovVec *)c->z_in.p, n, CovVec{});
    if (rc) return -1;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(host_v, c->z_in.p, n_out * esz, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- a page of a result that is emitted out of the table (bam_depth, bam_pileup, bam_bedgraph) ----------------------------------------------------------
// The host walks the rows in the order they are answered in and turns the next max_rows result rows into windows of result indices -- one per
// run of rows that follow each other in both orders.  rows: the page's rows; o / within: where the page behind it starts (the caller stores
// them in the pager once the page is made); tiles[2 w], tiles[2 w + 1]: the first and the last tile that holds window w.
struct DepWin { uint64_t o_a, o_b, dst0; };
struct DepPage { std::vector<DepWin> wins; std::vector<uint64_t> tiles; uint64_t rows = 0, o = 0, within = 0; };
static void dep_page_windows(const DepLayout &L, const DepPager &P, int64_t max_rows, DepPage &pg) {
    const size_t n_out = L.o_tid.size();
    uint64_t taken = 0; size_t o = (size_t)P.o_next; uint64_t within = P.o_within;
    while (o < n_out && taken < (uint64_t)max_rows) {
        const int64_t k = L.o_k[o];
        const uint64_t cnt = k < 0 ? 0 : P.row_off[(size_t)k + 1] - P.row_off[(size_t)k];
        if (within >= cnt) { o++; within = 0; continue; }
        const uint64_t a = P.row_off[(size_t)k] + within, room = (uint64_t)max_rows - taken, m = cnt - within < room ? cnt - within : room;
        if (!pg.wins.empty() && pg.wins.back().o_b == a) pg.wins.back().o_b = a + m;            // (the row before it in the answer is the row before it in the table)
        else pg.wins.push_back({a, a + m, taken});
        taken += m; within += m;
    }
    while (o < n_out && (L.o_k[o] < 0 || within >= P.row_off[(size_t)L.o_k[o] + 1] - P.row_off[(size_t)L.o_k[o]])) { o++; within = 0; }      // (rows that have nothing left)
    pg.rows = taken; pg.o = o; pg.within = within;
}
// the tiles of the page's windows: one dep_page_tiles launch per window, one copy, one wait; every pair is checked against the ntiles of the table
static int dep_page_tiles_of(dhts_ctx *c, const char *fn, DepPager &P, uint64_t ntiles, DepPage &pg) {
    const size_t nw = pg.wins.size();
    ENSURE(c, P.pagetiles, nw * 16 + 64);
    pg.tiles.assign(nw * 2, 0);
    for (size_t w = 0; w < nw; w++)
        hipLaunchKernelGGL(dep_page_tiles, dim3(1), dim3(64), 0, c->stream, (const unsigned long long *)P.toff.p, ntiles, (unsigned long long)pg.wins[w].o_a, (unsigned long long)pg.wins[w].o_b,
                           (unsigned long long *)P.pagetiles.p + 2 * w);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(pg.tiles.data(), P.pagetiles.p, nw * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t w = 0; w < nw; w++)
        if (pg.tiles[2 * w + 1] < pg.tiles[2 * w] || pg.tiles[2 * w + 1] >= ntiles) return fail(c, "%s: internal error: the tiles of a page are out of range", fn);
    return 0;
}

// ---- read-back: out_cols[n_cols] = cols with HOST pointers into dst (every part 8-byte aligned, every copy queued, one wait) ------------------
static uint64_t cols_host_bytes(int64_t n_rows, int n_cols, const dhts_col *cols, ColKind kind) {
    uint64_t need = 0; const uint64_t n = (uint64_t)n_rows;
    for (int i = 0; i < n_cols; i++) {
        const int k = kind(cols[i].col);
        if (k > 0) { if (cols[i].fixed) need += (n * (uint64_t)k + 7) & ~7ull; continue; }
        need += (n + 7) & ~7ull;
        if (k == COL_INT64) need += n * 8; else need += (((n + 1) * 4 + 7) & ~7ull) + ((cols[i].nbytes + 7) & ~7ull);
    }
    return need;
}
static int cols_fetch(dhts_ctx *c, const char *fn, int64_t n_rows, int n_cols, const dhts_col *cols, ColKind kind, void *dst, uint64_t cap, dhts_col *out_cols) {
    if (!c || !out_cols || (!dst && cap)) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    if (cap < cols_host_bytes(n_rows, n_cols, cols, kind)) return fail(c, "%s: fetch buffer too small", fn);
    uint8_t *p = (uint8_t *)dst; const uint64_t n = (uint64_t)n_rows;
    for (int i = 0; i < n_cols; i++) {
        const dhts_col &s = cols[i]; dhts_col &o = out_cols[i];
        memset(&o, 0, sizeof(o)); o.col = s.col;
        if (n == 0) continue;
        const int k = kind(s.col);
        if (k > 0) {
            if (!s.fixed) continue;
            HIPCHK(c, hipMemcpyAsync(p, s.fixed, n * (uint64_t)k, hipMemcpyDeviceToHost, c->stream)); o.fixed = p; p += (n * (uint64_t)k + 7) & ~7ull;
            continue;
        }
        HIPCHK(c, hipMemcpyAsync(p, s.valid, n, hipMemcpyDeviceToHost, c->stream)); o.valid = p; p += (n + 7) & ~7ull;
        if (k == COL_INT64) { HIPCHK(c, hipMemcpyAsync(p, s.fixed, n * 8, hipMemcpyDeviceToHost, c->stream)); o.fixed = p; p += n * 8; }
        else {
            HIPCHK(c, hipMemcpyAsync(p, s.off, (n + 1) * 4, hipMemcpyDeviceToHost, c->stream)); o.off = (const uint32_t *)p; p += ((n + 1) * 4 + 7) & ~7ull;
            if (s.nbytes) HIPCHK(c, hipMemcpyAsync(p, s.bytes, s.nbytes, hipMemcpyDeviceToHost, c->stream));
            o.bytes = p; o.nbytes = s.nbytes; p += (s.nbytes + 7) & ~7ull;
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
static int col_kind_int64(int) { return COL_INT64; }
