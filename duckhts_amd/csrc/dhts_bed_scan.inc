// dhts_bed_scan.inc -- part of dhts_api.hip (included there, inside its extern "C" block; not a translation unit of its own):
// read_bed.  A batch of text (carry + blocks, batch_begin) gets its delimiter table (bed_text.hip), its lines are classified, the rows are
// numbered by a scan and the projected columns are parsed / gathered, one lane per row.  The carry is the text from the first line that is
// not whole.  A region query (dhts_bed_set_region + dhts_bed_load_index) walks the index windows as read_bcf does on VCF text and keeps
// the rows by the interval tabix_intervals gives a line under the index's own configuration.
static const char *bed_container(const dhts_ctx *c) { return c->gz_plain ? "plain (non-BGZF) gzip" : "uncompressed text"; }

// hts_open for a reader of lines (read_bed, read_tabix): BGZF stays BGZF, everything else is text
static int text_open(dhts_ctx *c, const char *who) {
    HIPCHK(c, hipSetDevice(c->device));
    c->bed.open = false; c->tbx.open = false;
    if (c->comp_len > 0 && !c->plain_text) {
        // anything that is not BGZF is text, whatever it looks like (hts_getline reads every file): uncompressed, or the members of a plain gzip
        uint8_t head[18] = {0};
        HIPCHK(c, hipMemcpy(head, c->comp.p, c->comp_len < 18 ? (size_t)c->comp_len : 18, hipMemcpyDeviceToHost));
        const bool bgzf = c->comp_len >= 18 && head[0] == 0x1f && head[1] == 0x8b && head[2] == 8 && (head[3] & 4) && head[10] == 6 && head[11] == 0 && head[12] == 'B' && head[13] == 'C' && head[14] == 2 && head[15] == 0;
        if (!bgzf) { c->text_any = true; if (index_impl(c, false) < 0) return -1; if (!c->plain_text) return fail(c, "%s: failed to open file", who); }
        else if (c->n_blocks <= 0) return fail(c, "%s: failed to open file (no BGZF block)", who);
    }
    c->bam_open = false; c->bcf_open = false; c->sam_text = false; c->vcf_text = false; c->fastq = 0;
    c->first_rec_uoff = 0;
    return 0;
}

int dhts_bed_open(dhts_ctx *c) {
    if (!c) return -1;
    if (text_open(c, "read_bed")) return -1;
    BedState &S = c->bed;
    S.proj.clear(); for (int i = 0; i < BED_N_COLS; i++) S.proj.push_back(i);
    S.open = true;
    return dhts_bed_set_region(c, nullptr);
}

int dhts_bed_set_projection(dhts_ctx *c, const int32_t *col_ids, int32_t n) {
    if (!c || !c->bed.open) return c ? fail(c, "dhts_bed_open not called") : -1;
    if (n < 0 || (n > 0 && !col_ids)) return fail(c, "read_bed: bad projection");
    std::vector<int32_t> p; uint32_t seen = 0;
    for (int32_t i = 0; i < n; i++) {
        if (col_ids[i] < 0 || col_ids[i] >= BED_N_COLS || ((seen >> col_ids[i]) & 1u)) return fail(c, "read_bed: bad projection (column %d)", (int)col_ids[i]);
        seen |= 1u << col_ids[i]; p.push_back(col_ids[i]);
    }
    c->bed.proj.swap(p);
    return 0;
}

// (the scan position of a text context: read_bed's line count and error, read_tabix's remaining line_skip / header line)
static int bed_rewind(dhts_ctx *c) { c->bed.lines_done = 0; c->bed.status = 0; c->tbx.skip_left = c->tbx.line_skip; c->tbx.hdr_left = c->tbx.skip_header ? 1 : 0; return dhts_bam_rewind(c); }

// ONE region, as tbx_itr_querys takes it (commas are thousands separators of its numbers); "." = every record; NULL / "" clears.  The name is
// one of the INDEX's sequences, so it is resolved by dhts_bed_load_index, which has to follow (except for ".").
// The three region entries are shared with read_tabix (dhts_tabix_scan.inc): `who` names the table function in the messages, the region
// state lives in c->bed for both.
static int text_set_region(dhts_ctx *c, const char *who, const char *region) {
    BedState &S = c->bed;
    S.rg_active = S.rg_all = S.rg_pending = false; c->rg_empty_window = false;
    c->wins.clear(); c->win_cur = 0; c->scan_end_uoff = ~0ull;
    c->shard_b0 = 0; c->shard_b1 = c->n_blocks; c->shard_rank = 0; c->shard_world = 1; c->scan_first_uoff = 0;
    if (!region || !*region) return bed_rewind(c);
    if (c->plain_text) return fail(c, "%s: region queries need a BGZF file with a tabix index; this file is %s", who, bed_container(c));
    S.rg_active = true; S.rg_tok = region;
    if (S.rg_tok == ".") S.rg_all = true; else S.rg_pending = true;
    return bed_rewind(c);
}
int dhts_bed_set_region(dhts_ctx *c, const char *region) {
    if (!c || !c->bed.open) return c ? fail(c, "dhts_bed_open not called") : -1;
    return text_set_region(c, "read_bed", region);
}

// the region of `tok` among the sequences of the index `d` (already plain): 0, 1 = no iterator (unknown sequence, malformed region)
static int bed_resolve(dhts_ctx *c, const char *who, const uint8_t *d, uint64_t n, const std::string &tok, TbxConf &cf, std::string &name, int &tid, int64_t &b, int64_t &e) {
    int32_t preset = 0; std::vector<std::string> names;
    const int rc = tabix_header(c, d, n, preset, names);
    if (rc < 0) return -1;
    if (rc == 1) return fail(c, "%s: the index has no tabix header", who);
    const uint8_t *m = memcmp(d, "TBI\1", 4) == 0 ? d + 8 : d + 16;
    cf.preset = (int32_t)hle32(m); cf.sc = (int32_t)hle32(m + 4); cf.bc = (int32_t)hle32(m + 8); cf.ec = (int32_t)hle32(m + 12); cf.meta = (int32_t)hle32(m + 16); cf.skip = (int32_t)hle32(m + 20);
    if ((cf.preset & 0xffff) > 1) return fail(c, "%s: the tabix index was built with the VCF preset", who);
    if (!parse_region_token(names, tok, tid, b, e)) return 1;
    name = names[(size_t)tid];
    return 0;
}

// .tbi, or .csi with the tabix header.  0, 1 = the index does not know the region's sequence ("failed to create region iterator"), < 0 error.
static int text_load_index(dhts_ctx *c, const char *who, const void *bytes, uint64_t n) {
    BedState &S = c->bed;
    if (c->plain_text) return fail(c, "%s: %s has no index", who, bed_container(c));
    if (!S.rg_active) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    const uint8_t *d = (const uint8_t *)bytes; std::vector<uint8_t> inflated;
    if (index_plain(c, d, n, inflated)) return -1;
    std::vector<QIv> q;
    if (!S.rg_all) {
        int tid = -1; int64_t b = 0, e = 0;
        const int rc = bed_resolve(c, who, d, n, S.rg_tok, S.conf, S.rg_name, tid, b, e);
        if (rc < 0) return -1;
        if (rc == 1) { S.rg_pending = false; c->rg_empty_window = true; (void)bed_rewind(c); return 1; }
        S.rg_pending = false; S.rg_beg = b; S.rg_end = e;
        ENSURE(c, S.rg_name_dev, S.rg_name.size() + 64);
        if (!S.rg_name.empty()) HIPCHK(c, hipMemcpy(S.rg_name_dev.p, S.rg_name.data(), S.rg_name.size(), hipMemcpyHostToDevice));
        q.push_back({tid, b, e});
    }
    IdxWindow w;
    if (index_window(c, d, n, q, S.rg_all, w)) return -1;
    if (apply_window(c, w, S.rg_all, false, true)) return -1;
    return bed_rewind(c);
}
int dhts_bed_load_index(dhts_ctx *c, const void *bytes, uint64_t n) {
    if (!c || !c->bed.open) return c ? fail(c, "dhts_bed_open not called") : -1;
    return text_load_index(c, "read_bed", bytes, n);
}

// The file ranges a region query stages instead of the file (conventions of dhts_bam_region_segments; *count = -1: the whole file).  BED text
// has no header and the names are the index's, so the context need not hold the file.  Returns 1 when the index does not know the sequence.
static int text_region_segments(dhts_ctx *c, const char *who, const char *region, const void *index_bytes, uint64_t n, uint64_t *beg, uint64_t *end, int64_t cap, int64_t *count) {
    if (!c || !count || !region) return -1;
    *count = -1;
    if (!*region || !strcmp(region, ".")) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    const uint8_t *d = (const uint8_t *)index_bytes; std::vector<uint8_t> inflated;
    if (index_plain(c, d, n, inflated)) return -1;
    TbxConf cf; std::string name; int tid = -1; int64_t b = 0, e = 0;
    const int rc = bed_resolve(c, who, d, n, region, cf, name, tid, b, e);
    if (rc) { if (rc == 1) *count = 0; return rc; }
    std::vector<QIv> q; q.push_back({tid, b, e});
    IdxWindow w;
    if (index_window(c, d, n, q, false, w)) return -1;
    const std::vector<std::pair<uint64_t, uint64_t>> mg = merged_windows(w, true);
    if ((int64_t)mg.size() > cap) return 0;                                    // too many ranges for the caller's room: the whole file
    *count = (int64_t)mg.size();
    for (size_t k = 0; k < mg.size(); k++) { beg[k] = mg[k].first >> 16; end[k] = mg[k].second >> 16; }
    return 0;
}
int dhts_bed_region_segments(dhts_ctx *c, const char *region, const void *index_bytes, uint64_t n, uint64_t *beg, uint64_t *end, int64_t cap, int64_t *count) {
    return text_region_segments(c, "read_bed", region, index_bytes, n, beg, end, cap, count);
}

// The delimiter table of a batch (line_table with the tab part, dhts_text_lines.inc) in c->bed's buffers, for read_bed and read_tabix: the
// lines that belong to this batch's scan range (a window of a region query ends inside a block), where the carry begins, whether the range
// ends here.
static int text_line_table(dhts_ctx *c, const Batch &B, LineTab &T) {
    BedState &S = c->bed;
    const uint64_t ulen = B.ulen, out_base = B.out_base;
    uint64_t t0 = 0;
    if (!first_line_t0(c, out_base, t0)) return fail(c, "internal: window start in front of its first batch");
    // the scan range ends with its last block or, for an index window, exactly at the window's end (windows are disjoint)
    uint64_t end_abs = B.sharded_tail ? c->h_uoff[c->shard_b1] : ~0ull;
    if (c->scan_end_uoff < end_abs) end_abs = c->scan_end_uoff;
    const uint64_t lim = (end_abs != ~0ull && out_base + ulen > end_abs) ? end_abs - out_base : ~0ull;
    if (c->first_batch && out_base + t0 >= end_abs) { T = LineTab(); T.carry_start = t0 < ulen ? t0 : ulen; T.finished = true; return 0; }
    return line_table(c, S.lines, &S.tabs, B.u, t0, ulen, batch_clean_end(c, B), lim, DHTS_K_TILES, T);
}

static int bed_next_batch_one(dhts_ctx *c, int64_t max_blocks, dhts_bed_batch *out) {
    memset(out, 0, sizeof(*out));
    BedState &S = c->bed;
    if (!S.open) return fail(c, "dhts_bed_open not called");
    HIPCHK(c, hipSetDevice(c->device));
    const int ncols = (int)S.proj.size();
    S.out.assign((size_t)ncols, dhts_col());
    for (int i = 0; i < ncols; i++) { memset(&S.out[(size_t)i], 0, sizeof(dhts_col)); S.out[(size_t)i].col = S.proj[(size_t)i]; }
    out->n_cols = ncols; out->cols = S.out.data();
    if (c->stream_done || c->n_blocks <= 0) { out->status = S.status ? S.status : 1; return 0; }
    if (S.rg_pending) return fail(c, "read_bed: a region query needs the tabix index (dhts_bed_load_index) before the scan");
    Batch B;
    if (batch_begin(c, max_blocks, B)) return -1;
    const uint8_t *u = B.u; const uint64_t ulen = B.ulen;
    LineTab T;
    if (text_line_table(c, B, T)) return -1;
    bool finished = T.finished, rec_err = false; uint64_t carry_start = T.carry_start; int64_t nlines = T.nlines, nrows = 0; int last_open = T.last_open;
    BedRows R; memset(&R, 0, sizeof(R));
    if (nlines > 0) {
        const size_t ln = (size_t)(nlines + 2) * 4 + 64;
        ENSURE(c, S.lend, ln); ENSURE(c, S.ntab, ln); ENSURE(c, S.is_row, ln); ENSURE(c, S.rank, ln); ENSURE(c, S.ctr, 64);
        const bool by_region = S.rg_active && !S.rg_all;
        BedLines a; memset(&a, 0, sizeof(a));
        a.u = u; a.line_off = (const uint32_t *)S.lines.line_off.p; a.tab_off = (const uint32_t *)S.tabs.tab_off.p; a.tab0 = (const uint32_t *)S.tabs.tab0.p; a.has_nul = (const uint32_t *)S.tabs.has_nul.p;
        a.nlines = (uint32_t)nlines; a.text_end = (uint32_t)ulen; a.last_open = last_open; a.report_bad = by_region ? 0 : 1;
        a.lend = (uint32_t *)S.lend.p; a.ntab = (uint32_t *)S.ntab.p; a.is_row = (uint32_t *)S.is_row.p; a.first_bad = (unsigned long long *)S.ctr.p;
        const unsigned lgrid = (unsigned)((nlines + 255) / 256);
        unsigned long long first_bad = ~0ull;
        {
            KTimer tm(c, DHTS_K_CORE);
            HIPCHK(c, hipMemsetAsync(S.ctr.p, 0xff, 8, c->stream));
            hipLaunchKernelGGL(bed_classify, dim3(lgrid), dim3(256), 0, c->stream, a);
            if (by_region) {
                // hts_itr_next's test on the interval tbx_parse1 gives the line under the index's configuration; a line tabix passes over or
                // cannot parse is no row of the query
                ENSURE(c, S.tbx, (size_t)nlines * sizeof(TbxLine) + 64);
                hipLaunchKernelGGL(tabix_intervals, dim3(lgrid), dim3(256), 0, c->stream, u, (const uint32_t *)S.lines.line_off.p, nlines, ulen, (int32_t)last_open, S.conf, (TbxLine *)S.tbx.p);
                hipLaunchKernelGGL(bed_region_keep, dim3(lgrid), dim3(256), 0, c->stream, u, (const TbxLine *)S.tbx.p, (uint32_t)nlines, (const uint8_t *)S.rg_name_dev.p, (uint32_t)S.rg_name.size(),
                                   (long long)S.rg_beg, (long long)S.rg_end, (uint32_t *)S.is_row.p, (unsigned long long *)S.ctr.p);
            }
            HIPCHK(c, hipMemcpyAsync(&first_bad, S.ctr.p, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        int64_t nl_eff = nlines;
        if (first_bad < (unsigned long long)nlines) {                          // the first short line ends the scan in front of it
            nl_eff = (int64_t)first_bad; rec_err = true;
            if (!S.rg_active) fail(c, "read_bed: BED line has fewer than 3 tab-delimited fields (line %lld)", (long long)(S.lines_done + nl_eff + 1));
            else fail(c, "read_bed: BED line has fewer than 3 tab-delimited fields");
        }
        S.lines_done += nl_eff;
        uint64_t nr = 0;
        if (nl_eff > 0) {
            KTimer tm(c, DHTS_K_SCAN);
            const uint32_t *kin[1] = {(const uint32_t *)S.is_row.p}; uint32_t *kout[1] = {(uint32_t *)S.rank.p};
            if (run_scan(c, 1, kin, kout, nullptr, nl_eff, &nr)) return -1;
        }
        nrows = (int64_t)nr;
        if (nrows > 0 && ncols > 0) {
            ENSURE(c, S.row_line, (size_t)nrows * 4 + 64);
            hipLaunchKernelGGL(fq_compact, dim3((unsigned)((nl_eff + 255) / 256)), dim3(256), 0, c->stream, (const uint32_t *)S.is_row.p, (const uint32_t *)S.rank.p, (uint32_t)nl_eff, (uint32_t *)S.row_line.p);
            R.u = u; R.line_off = a.line_off; R.tab_off = a.tab_off; R.tab0 = a.tab0; R.lend = a.lend; R.ntab = a.ntab; R.row_line = (const uint32_t *)S.row_line.p; R.nrows = (uint32_t)nrows;
        }
    }
    if (nrows > 0 && ncols > 0) {
        const unsigned rgrid = (unsigned)((nrows + 255) / 256);
        BedIntArgs gi; memset(&gi, 0, sizeof(gi)); BedStrArgs gs; memset(&gs, 0, sizeof(gs));
        int slot_of[BED_N_COLS];
        for (int i = 0; i < ncols; i++) {
            const int col = S.proj[(size_t)i];
            if (bed_col_is_int(col)) {
                const int k = gi.n++; slot_of[i] = k;
                ENSURE(c, S.ival[k], (size_t)nrows * 8 + 64); ENSURE(c, S.ivalid[k], (size_t)nrows + 64);
                gi.field[k] = col; gi.val[k] = (long long *)S.ival[k].p; gi.valid[k] = (uint8_t *)S.ivalid[k].p;
            } else {
                const int k = gs.n++; slot_of[i] = k;
                ENSURE(c, S.slen[k], (size_t)(nrows + 1) * 4 + 64); ENSURE(c, S.soff[k], (size_t)(nrows + 1) * 4 + 64); ENSURE(c, S.svalid[k], (size_t)nrows + 64);
                gs.col[k] = col; gs.len[k] = (uint32_t *)S.slen[k].p; gs.off[k] = (const uint32_t *)S.soff[k].p; gs.valid[k] = (uint8_t *)S.svalid[k].p;
            }
        }
        uint64_t totals[BED_N_STR] = {0};
        if (gi.n) { KTimer tm(c, DHTS_K_BCF_CHECK); hipLaunchKernelGGL(bed_ints, dim3(rgrid), dim3(256), 0, c->stream, R, gi); }
        if (gs.n) {
            {
                KTimer tm(c, DHTS_K_BCF_MEASURE);
                hipLaunchKernelGGL(bed_str_measure, dim3(rgrid), dim3(256), 0, c->stream, R, gs);
            }
            const uint32_t *kin[BED_N_STR]; uint32_t *kout[BED_N_STR];
            for (int k = 0; k < gs.n; k++) { kin[k] = gs.len[k]; kout[k] = (uint32_t *)S.soff[k].p; }
            { KTimer tm(c, DHTS_K_SCAN); if (run_scan(c, gs.n, kin, kout, nullptr, nrows, totals)) return -1; }
            for (int k = 0; k < gs.n; k++) { ENSURE(c, S.sbytes[k], (size_t)totals[k] + 64); gs.bytes[k] = (uint8_t *)S.sbytes[k].p; }
            KTimer tm(c, DHTS_K_BCF_WRITE);
            hipLaunchKernelGGL(bed_str_gather, dim3(rgrid), dim3(256), 0, c->stream, R, gs);
        }
        HIPCHK(c, hipGetLastError());
        for (int i = 0; i < ncols; i++) {
            dhts_col &o = S.out[(size_t)i]; const int k = slot_of[i];
            if (bed_col_is_int(o.col)) { o.fixed = S.ival[k].p; o.valid = (const uint8_t *)S.ivalid[k].p; }
            else { o.off = (const uint32_t *)S.soff[k].p; o.bytes = (const uint8_t *)S.sbytes[k].p; o.nbytes = totals[k]; o.valid = (const uint8_t *)S.svalid[k].p; }
        }
    }
    out->n_rows = nrows;
    if (batch_end(c, B, carry_start, rec_err, finished, &out->status)) return -1;
    if (out->status < 0) S.status = out->status;
    return 0;
}

int dhts_bed_next_batch(dhts_ctx *c, int64_t max_blocks, dhts_bed_batch *out) {
    if (!c || !out) return -1;
    for (;;) {
        if (bed_next_batch_one(c, max_blocks, out)) return -1;
        // several index windows: the end of one window is the start of the next, not the end of the scan
        if (next_window(c, out->status) && out->n_rows == 0) continue;
        return 0;
    }
}

// read-back in the style of dhts_bcf_batch_fetch: out_cols[b->n_cols] = b->cols with HOST pointers into dst (every copy queued, one wait;
// cols_fetch, dhts_bam_accum.inc)
static int bed_col_kind(int col) { return bed_col_is_int(col) ? COL_INT64 : COL_STRING; }
uint64_t dhts_bed_batch_host_bytes(const dhts_bed_batch *b) { return b ? cols_host_bytes(b->n_rows, b->n_cols, b->cols, bed_col_kind) : 0; }
int dhts_bed_batch_fetch(dhts_ctx *c, const dhts_bed_batch *b, void *dst, uint64_t cap, dhts_col *out_cols) {
    return b ? cols_fetch(c, "read_bed", b->n_rows, b->n_cols, b->cols, bed_col_kind, dst, cap, out_cols) : -1;
}

// measurement hook (include/duckhts_amd_debug.h, tools/bench_bed.py): the lane-per-line walk the delimiter table is compared with, over the
// whole resident text of a BED context -- the line table (vcf_line_count / vcf_line_fill) and bed_intervals, which finds chrom / start / end
// of every line by walking it.  Device time of the two parts in milliseconds; returns the number of lines, < 0 on error.
int64_t dhts_debug_bed_walk(dhts_ctx *c, double *ms_line_table, double *ms_walk) {
    if (!c || !c->bed.open) return c ? fail(c, "dhts_bed_open not called") : -1;
    HIPCHK(c, hipSetDevice(c->device));
    if (dhts_bed_set_region(c, nullptr)) return -1;
    hipEvent_t e[3]; for (auto &x : e) HIPCHK(c, hipEventCreate(&x));
    double t_tab = 0, t_walk = 0; int64_t lines = 0;
    while (!c->stream_done && c->n_blocks > 0) {
        Batch B;
        if (batch_begin(c, 0, B)) return -1;
        const uint8_t *u = B.u; const uint64_t ulen = B.ulen;
        // (its own rule for the open last line: the end of the file alone, whatever the stream ended on -- it differs from batch_clean_end)
        LineTab T;
        HIPCHK(c, hipEventRecord(e[0], c->stream));
        if (line_table(c, c->lines, nullptr, u, 0, ulen, B.final_batch, ~0ull, -1, T)) return -1;
        HIPCHK(c, hipEventRecord(e[1], c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        { float ms = 0; HIPCHK(c, hipEventElapsedTime(&ms, e[0], e[1])); t_tab += ms; }
        const uint64_t carry_start = T.carry_start; const int64_t nlines = T.nlines; const int last_open = T.last_open;
        if (nlines > 0) {
            ENSURE(c, c->bed.tbx, (size_t)nlines * sizeof(TbxLine) + 64);
            HIPCHK(c, hipEventRecord(e[1], c->stream));
            hipLaunchKernelGGL(bed_intervals, dim3((unsigned)((nlines + 255) / 256)), dim3(256), 0, c->stream, u, (const uint32_t *)c->lines.line_off.p, nlines, ulen, (int32_t)last_open, (TbxLine *)c->bed.tbx.p);
            HIPCHK(c, hipEventRecord(e[2], c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            float ms = 0; HIPCHK(c, hipEventElapsedTime(&ms, e[1], e[2])); t_walk += ms;
            lines += nlines;
        }
        int32_t status = 0;
        if (batch_end(c, B, carry_start, false, false, &status)) return -1;
        if (status != 0) break;
    }
    for (auto &x : e) (void)hipEventDestroy(x);
    if (ms_line_table) *ms_line_table = t_tab;
    if (ms_walk) *ms_walk = t_walk;
    if (dhts_bed_set_region(c, nullptr)) return -1;
    return lines;
}
