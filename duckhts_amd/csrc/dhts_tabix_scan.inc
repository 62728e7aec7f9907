// dhts_tabix_scan.inc -- part of dhts_api.hip (included there, inside its extern "C" block; not a translation unit of its own):
// read_tabix / read_gtf / read_gff.  A batch of text gets read_bed's delimiter table (text_line_table), its lines are classified
// (tabix_text.hip), line_skip and the header line are taken off by scans of the flags, the rows are numbered and the projected columns are
// parsed / gathered, one lane per row.  Regions go through read_bed's windows (text_set_region / text_load_index).
static const char *tabix_who(const dhts_ctx *c) { return c->tbx.mode == DHTS_TABIX_GTF ? "read_gtf" : c->tbx.mode == DHTS_TABIX_GFF ? "read_gff" : "read_tabix"; }
#define TABIX_OPEN(c) do { if (!(c) || !(c)->tbx.open) return (c) ? fail(c, "dhts_tabix_open not called") : -1; } while (0)

int dhts_tabix_open(dhts_ctx *c, int mode) {
    if (!c) return -1;
    if (mode != DHTS_TABIX_GENERIC && mode != DHTS_TABIX_GTF && mode != DHTS_TABIX_GFF) return fail(c, "dhts_tabix_open: unknown mode %d", mode);
    c->tbx.mode = mode;
    if (text_open(c, tabix_who(c))) return -1;
    TabixState &Q = c->tbx;
    Q.meta_char = '#'; Q.line_skip = 0; Q.skip_header = false; Q.status = 0; Q.want_skip_cand = false;
    Q.types.clear(); Q.proj.clear();
    if (mode == DHTS_TABIX_GENERIC) { Q.n_cols = 1; Q.types.push_back(DHTS_T_VARCHAR); Q.proj.push_back(0); }
    else {
        // seqname, source, feature, start, end, score, strand, frame, attributes (:564-575)
        static const int32_t gxf[9] = {DHTS_T_VARCHAR, DHTS_T_VARCHAR, DHTS_T_VARCHAR, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_DOUBLE, DHTS_T_VARCHAR, DHTS_T_VARCHAR, DHTS_T_VARCHAR};
        Q.n_cols = 9; Q.types.assign(gxf, gxf + 9);
        for (int i = 0; i < 9; i++) Q.proj.push_back(i);
    }
    Q.open = true;
    return text_set_region(c, tabix_who(c), nullptr);
}

int dhts_tabix_set_conf(dhts_ctx *c, int meta_char, int line_skip) {
    TABIX_OPEN(c);
    if (c->tbx.mode != DHTS_TABIX_GENERIC) return fail(c, "%s: the meta character and line_skip are fixed ('#', 0)", tabix_who(c));
    if (meta_char < 0 || meta_char > 255 || line_skip < 0) return fail(c, "read_tabix: bad configuration (meta_char %d, line_skip %d)", meta_char, line_skip);
    c->tbx.meta_char = meta_char; c->tbx.line_skip = line_skip;
    return bed_rewind(c);
}

int dhts_tabix_index_conf(dhts_ctx *c, const void *bytes, uint64_t n, int32_t *meta_char, int32_t *line_skip) {
    if (!c || !bytes) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    const uint8_t *d = (const uint8_t *)bytes; std::vector<uint8_t> inflated;
    if (index_plain(c, d, n, inflated)) return -1;
    int32_t preset = 0; std::vector<std::string> names;
    const int rc = tabix_header(c, d, n, preset, names);
    if (rc < 0) return -1;
    if (rc == 1) return fail(c, "the index has no tabix header");
    const uint8_t *m = memcmp(d, "TBI\1", 4) == 0 ? d + 8 : d + 16;
    if (meta_char) *meta_char = (int32_t)hle32(m + 16);
    if (line_skip) *line_skip = (int32_t)hle32(m + 20);
    return 0;
}

int dhts_tabix_set_schema(dhts_ctx *c, int32_t n_cols, const int32_t *types, int skip_header_line) {
    TABIX_OPEN(c);
    if (c->tbx.mode != DHTS_TABIX_GENERIC) return fail(c, "%s: the schema is fixed", tabix_who(c));
    if (n_cols < 1 || n_cols > DHTS_TABIX_MAX_COLS || !types) return fail(c, "read_tabix: bad schema (%d columns)", (int)n_cols);
    TabixState &Q = c->tbx;
    for (int32_t i = 0; i < n_cols; i++) if (types[i] != DHTS_T_INTEGER && types[i] != DHTS_T_BIGINT && types[i] != DHTS_T_DOUBLE && types[i] != DHTS_T_VARCHAR) return fail(c, "read_tabix: bad schema (type %d of column %d)", (int)types[i], (int)i);
    Q.n_cols = n_cols; Q.types.assign(types, types + n_cols); Q.skip_header = skip_header_line != 0;
    Q.proj.clear(); for (int32_t i = 0; i < n_cols; i++) Q.proj.push_back(i);
    return bed_rewind(c);
}

int dhts_tabix_set_projection(dhts_ctx *c, const int32_t *col_ids, int32_t n) {
    TABIX_OPEN(c);
    TabixState &Q = c->tbx;
    if (n < 0 || (n > 0 && !col_ids)) return fail(c, "%s: bad projection", tabix_who(c));
    const int32_t lim = Q.mode == DHTS_TABIX_GENERIC ? Q.n_cols : DHTS_GXF_ATTRIBUTES_MAP + 1;
    std::vector<int32_t> p; std::vector<char> seen((size_t)lim, 0);
    for (int32_t i = 0; i < n; i++) {
        if (col_ids[i] < 0 || col_ids[i] >= lim || seen[(size_t)col_ids[i]]) return fail(c, "%s: bad projection (column %d)", tabix_who(c), (int)col_ids[i]);
        seen[(size_t)col_ids[i]] = 1; p.push_back(col_ids[i]);
    }
    Q.proj.swap(p);
    return 0;
}

int dhts_tabix_set_region(dhts_ctx *c, const char *region) { TABIX_OPEN(c); return text_set_region(c, tabix_who(c), region); }
int dhts_tabix_load_index(dhts_ctx *c, const void *bytes, uint64_t n) { TABIX_OPEN(c); return text_load_index(c, tabix_who(c), bytes, n); }
int dhts_tabix_region_segments(dhts_ctx *c, const char *region, const void *index_bytes, uint64_t n, uint64_t *beg, uint64_t *end, int64_t cap, int64_t *count) {
    return text_region_segments(c, "read_tabix", region, index_bytes, n, beg, end, cap, count);
}

// line `li` of the current batch as the reference's C string (CR dropped, cut at a NUL), and its tabs
static int tabix_fetch_line(dhts_ctx *c, const uint8_t *u, uint32_t li, std::string &text, uint32_t *ntab) {
    BedState &S = c->bed;
    uint32_t l0 = 0, l1 = 0;
    HIPCHK(c, hipMemcpy(&l0, (const uint32_t *)S.lines.line_off.p + li, 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&l1, (const uint32_t *)S.lend.p + li, 4, hipMemcpyDeviceToHost));
    if (ntab) HIPCHK(c, hipMemcpy(ntab, (const uint32_t *)S.ntab.p + li, 4, hipMemcpyDeviceToHost));
    text.assign((size_t)(l1 - l0), '\0');
    if (l1 > l0) HIPCHK(c, hipMemcpy(&text[0], u + l0, l1 - l0, hipMemcpyDeviceToHost));
    return 0;
}

// The rows of the next batch: batch_begin, the line table, the line classes, line_skip and the header line (sequential scans only, carried
// from batch to batch in skip_left / hdr_left), the region test, the row numbers.  The caller ends the batch (batch_end).
struct TabixRows { Batch B; LineTab T; int64_t nrows = 0; BedRows R; };
static int tabix_rows(dhts_ctx *c, int64_t max_blocks, bool need_lines, TabixRows &X) {
    BedState &S = c->bed; TabixState &Q = c->tbx;
    if (batch_begin(c, max_blocks, X.B)) return -1;
    if (text_line_table(c, X.B, X.T)) return -1;
    const uint8_t *u = X.B.u; const int64_t nlines = X.T.nlines;
    memset(&X.R, 0, sizeof(X.R)); X.nrows = 0;
    if (nlines <= 0) return 0;
    const size_t ln = (size_t)(nlines + 2) * 4 + 64;
    ENSURE(c, S.lend, ln); ENSURE(c, S.ntab, ln); ENSURE(c, S.is_row, ln); ENSURE(c, S.rank, ln); ENSURE(c, S.ctr, 64);
    const bool by_region = S.rg_active && !S.rg_all, seq = !S.rg_active;
    const bool skipping = seq && Q.skip_left > 0;
    if (skipping) ENSURE(c, Q.ne, ln);
    BedLines a; memset(&a, 0, sizeof(a));
    a.u = u; a.line_off = (const uint32_t *)S.lines.line_off.p; a.tab_off = (const uint32_t *)S.tabs.tab_off.p; a.tab0 = (const uint32_t *)S.tabs.tab0.p; a.has_nul = (const uint32_t *)S.tabs.has_nul.p;
    a.nlines = (uint32_t)nlines; a.text_end = (uint32_t)X.B.ulen; a.last_open = X.T.last_open; a.report_bad = 0;
    a.lend = (uint32_t *)S.lend.p; a.ntab = (uint32_t *)S.ntab.p; a.is_row = (uint32_t *)S.is_row.p; a.first_bad = (unsigned long long *)S.ctr.p;
    const unsigned lgrid = (unsigned)((nlines + 255) / 256);
    uint32_t *is_row = (uint32_t *)S.is_row.p, *rank = (uint32_t *)S.rank.p;
    {
        KTimer tm(c, DHTS_K_CORE);
        hipLaunchKernelGGL(tabix_classify, dim3(lgrid), dim3(256), 0, c->stream, a, (uint32_t)Q.meta_char, skipping ? (uint32_t *)Q.ne.p : (uint32_t *)nullptr);
        if (by_region) {
            // hts_itr_next's test on the interval tbx_parse1 gives the line under the index's configuration, as read_bed applies it
            ENSURE(c, S.tbx, (size_t)nlines * sizeof(TbxLine) + 64);
            HIPCHK(c, hipMemsetAsync(S.ctr.p, 0xff, 8, c->stream));
            hipLaunchKernelGGL(tabix_intervals, dim3(lgrid), dim3(256), 0, c->stream, u, (const uint32_t *)S.lines.line_off.p, nlines, X.B.ulen, (int32_t)X.T.last_open, S.conf, (TbxLine *)S.tbx.p);
            hipLaunchKernelGGL(bed_region_keep, dim3(lgrid), dim3(256), 0, c->stream, u, (const TbxLine *)S.tbx.p, (uint32_t)nlines, (const uint8_t *)S.rg_name_dev.p, (uint32_t)S.rg_name.size(),
                               (long long)S.rg_beg, (long long)S.rg_end, is_row, (unsigned long long *)S.ctr.p);
        }
    }
    if (skipping) {
        // the first skip_left lines that are not empty are no rows, meta lines among them (:898-901 stands in front of :902)
        KTimer tm(c, DHTS_K_SCAN);
        const uint32_t *kin[1] = {(const uint32_t *)Q.ne.p}; uint32_t *kout[1] = {rank}; uint64_t n_ne = 0;
        if (run_scan(c, 1, kin, kout, nullptr, nlines, &n_ne)) return -1;
        const uint32_t take = n_ne < (uint64_t)Q.skip_left ? (uint32_t)n_ne : (uint32_t)Q.skip_left;
        if (Q.want_skip_cand && take > 0) {                                    // the sniff: the last skipped line so far is the header candidate
            uint32_t li = 0;
            hipLaunchKernelGGL(tabix_pick, dim3(lgrid), dim3(256), 0, c->stream, (const uint32_t *)Q.ne.p, (const uint32_t *)rank, (uint32_t)nlines, take - 1u, (uint32_t *)S.ctr.p + 4);
            HIPCHK(c, hipMemcpyAsync(&li, (const uint32_t *)S.ctr.p + 4, 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (tabix_fetch_line(c, u, li, Q.cand, nullptr)) return -1;
            Q.have_cand = true;
        }
        hipLaunchKernelGGL(tabix_skip_apply, dim3(lgrid), dim3(256), 0, c->stream, is_row, (const uint32_t *)rank, (uint32_t)nlines, (uint32_t)Q.skip_left);
        Q.skip_left -= (int32_t)take;
    }
    if (seq && Q.skip_left == 0 && Q.hdr_left > 0) {
        // behind the skipped lines, the first line that is neither empty nor meta is the header line (:903-906)
        KTimer tm(c, DHTS_K_SCAN);
        const uint32_t *kin[1] = {(const uint32_t *)is_row}; uint32_t *kout[1] = {rank}; uint64_t n_data = 0;
        if (run_scan(c, 1, kin, kout, nullptr, nlines, &n_data)) return -1;
        hipLaunchKernelGGL(tabix_skip_apply, dim3(lgrid), dim3(256), 0, c->stream, is_row, (const uint32_t *)rank, (uint32_t)nlines, (uint32_t)Q.hdr_left);
        if (n_data > 0) Q.hdr_left = 0;
    }
    uint64_t nr = 0;
    {
        KTimer tm(c, DHTS_K_SCAN);
        const uint32_t *kin[1] = {(const uint32_t *)is_row}; uint32_t *kout[1] = {rank};
        if (run_scan(c, 1, kin, kout, nullptr, nlines, &nr)) return -1;
    }
    X.nrows = (int64_t)nr;
    if (nr > 0 && need_lines) {
        ENSURE(c, S.row_line, (size_t)nr * 4 + 64);
        hipLaunchKernelGGL(fq_compact, dim3(lgrid), dim3(256), 0, c->stream, (const uint32_t *)is_row, (const uint32_t *)rank, (uint32_t)nlines, (uint32_t *)S.row_line.p);
        BedRows &R = X.R;
        R.u = u; R.line_off = a.line_off; R.tab_off = a.tab_off; R.tab0 = a.tab0; R.lend = a.lend; R.ntab = a.ntab; R.row_line = (const uint32_t *)S.row_line.p; R.nrows = (uint32_t)nr;
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

// the peek of bind (:658-679): the header candidate and the first data line's field count, from the line tables of the first batches
int dhts_tabix_sniff(dhts_ctx *c, int header, int have_header_names, dhts_tabix_sniffed *out) {
    TABIX_OPEN(c);
    if (!out) return fail(c, "dhts_tabix_sniff: no result");
    memset(out, 0, sizeof(*out));
    TabixState &Q = c->tbx;
    if (c->bed.rg_active) return fail(c, "%s: the schema is sniffed on a sequential scan (clear the region first)", tabix_who(c));
    HIPCHK(c, hipSetDevice(c->device));
    const bool want_names = header && !have_header_names;
    const bool saved_hdr = Q.skip_header;
    Q.skip_header = false;                                                      // every line behind the skip prefix that is not meta counts here
    if (bed_rewind(c)) { Q.skip_header = saved_hdr; return -1; }
    Q.cand.clear(); Q.have_cand = false; Q.want_skip_cand = want_names && Q.line_skip > 0;
    bool from_skip = false, have_first = false; std::string first; int32_t n_fields = 0; int rc = 0;
    // the candidate is a skipped line when line_skip is set (header_from_skip: data lines only follow a skipped one); otherwise it is the first
    // data line, and the count comes from the second
    const bool first_is_cand = want_names && Q.line_skip == 0;
    const int64_t need = first_is_cand ? 2 : 1; int64_t seen = 0;
    while (rc == 0 && !c->stream_done && c->n_blocks > 0) {
        TabixRows X;
        if (tabix_rows(c, 64, true, X)) { rc = -1; break; }
        if (Q.have_cand) from_skip = true;
        for (int64_t r = 0; r < X.nrows && seen < need && rc == 0; r++, seen++) {
            uint32_t li = 0, nt = 0; std::string text;
            if (hipMemcpy(&li, (const uint32_t *)c->bed.row_line.p + r, 4, hipMemcpyDeviceToHost) != hipSuccess || tabix_fetch_line(c, X.B.u, li, text, &nt)) { rc = fail(c, "dhts_tabix_sniff: read-back failed"); break; }
            if (first_is_cand && !have_first) { first.swap(text); have_first = true; }
            else n_fields = (int32_t)nt + 1;
        }
        int32_t status = 0;
        if (batch_end(c, X.B, X.T.carry_start, false, X.T.finished || seen >= need, &status)) { rc = -1; break; }
        if (status != 0 || seen >= need) break;
    }
    Q.want_skip_cand = false; Q.skip_header = saved_hdr;
    if (rc == 0) {
        if (first_is_cand && have_first) { Q.cand.swap(first); Q.have_cand = true; }
        out->n_fields = n_fields; out->have_candidate = (want_names && Q.have_cand) ? 1 : 0; out->candidate_from_skip = from_skip ? 1 : 0;
        out->candidate = out->have_candidate ? Q.cand.c_str() : nullptr; out->candidate_len = out->have_candidate ? Q.cand.size() : 0;
    }
    if (bed_rewind(c)) return -1;
    return rc;
}

// ---- bind behind the peek: pure host ------------------------------------------------------------------------------------------------------
static int tabix_type_of_name(const char *s) {                                 // parse_type_name :218-230
    if (!s) return DHTS_T_VARCHAR;
    if (!strcasecmp(s, "INT") || !strcasecmp(s, "INTEGER")) return DHTS_T_INTEGER;
    if (!strcasecmp(s, "BIGINT") || !strcasecmp(s, "LONG")) return DHTS_T_BIGINT;
    if (!strcasecmp(s, "DOUBLE") || !strcasecmp(s, "FLOAT") || !strcasecmp(s, "REAL")) return DHTS_T_DOUBLE;
    return DHTS_T_VARCHAR;
}
int dhts_tabix_resolve_schema(const dhts_tabix_sniffed *sn, int header, const char *const *header_names, int32_t n_header_names,
                              const char *const *column_types, int32_t n_column_types, int auto_detect,
                              const char *const *cells, const uint32_t *cell_len, int32_t n_cell_rows, dhts_tabix_schema *out, char *err, uint64_t err_cap) {
    if (err && err_cap) err[0] = 0;
    if (!sn || !out) return -1;
    memset(out, 0, sizeof(*out));
    if (!header_names) n_header_names = 0;
    if (!column_types) n_column_types = 0;
    std::vector<std::string> names;
    int n_cols = sn->n_fields;
    if (n_header_names > 0) {                                                  // :684-686
        for (int32_t i = 0; i < n_header_names; i++) names.push_back(header_names[i] ? header_names[i] : "");
        n_cols = n_header_names; out->skip_header_line = header ? 1 : 0;
    } else if (header && sn->have_candidate) {                                 // :687-691, parse_header_names: the candidate's trimmed fields
        const std::string line(sn->candidate ? sn->candidate : "", sn->candidate ? (size_t)sn->candidate_len : 0);
        size_t b = 0;
        for (;;) {
            size_t e = line.find('\t', b); if (e == std::string::npos) e = line.size();
            size_t s0 = b, s1 = e;
            while (s0 < s1 && (line[s0] == ' ' || line[s0] == '\t')) s0++;
            while (s1 > s0 && (line[s1 - 1] == ' ' || line[s1 - 1] == '\t')) s1--;
            names.push_back(line.substr(s0, s1 - s0));
            if (e >= line.size()) break;
            b = e + 1;
        }
        n_cols = (int)names.size(); out->skip_header_line = sn->candidate_from_skip ? 0 : 1;
    }
    if (n_cols == 0) n_cols = 1;
    if (n_cols > DHTS_TABIX_MAX_COLS) n_cols = DHTS_TABIX_MAX_COLS;
    int bd_n_cols = n_column_types > 0 ? n_column_types : n_cols;              // :630, 696
    if (n_column_types > 0 && bd_n_cols != n_cols) {
        if (err && err_cap) snprintf(err, (size_t)err_cap, "column_types length does not match detected column count");
        return -1;
    }
    out->n_cols = bd_n_cols;
    for (int i = 0; i < bd_n_cols; i++) out->types[i] = n_column_types > 0 ? tabix_type_of_name(column_types[i]) : DHTS_T_VARCHAR;
    static thread_local std::string name_mem;                                   // a name is a C string: it ends at a NUL of the header line
    std::vector<size_t> at((size_t)bd_n_cols, 0);
    name_mem.clear();
    for (int i = 0; i < bd_n_cols; i++) {                                      // :758-771
        char fallback[32]; snprintf(fallback, sizeof(fallback), "column%d", i);
        at[(size_t)i] = name_mem.size();
        name_mem += ((size_t)i < names.size() && !names[(size_t)i].empty()) ? names[(size_t)i].c_str() : fallback;
        name_mem.push_back('\0');
    }
    for (int i = 0; i < bd_n_cols; i++) out->names[i] = name_mem.c_str() + at[(size_t)i];
    if (auto_detect && n_column_types == 0) {                                  // :709-755
        if (!cells || !cell_len) return 1;
        enum { ST_INT = 0, ST_DBL = 1, ST_STR = 2 };
        std::vector<int> st((size_t)bd_n_cols, ST_INT);
        if (n_cell_rows > 100) n_cell_rows = 100;
        for (int32_t r = 0; r < n_cell_rows; r++) for (int i = 0; i < bd_n_cols; i++) {
            const char *f = cells[(size_t)r * bd_n_cols + i]; const uint32_t fl = cell_len[(size_t)r * bd_n_cols + i];
            if (!f || fl == 0 || (fl == 1 && f[0] == '.')) continue;
            uint32_t k = (f[0] == '-' || f[0] == '+') ? 1u : 0u; bool is_int = k < fl;                  // is_integer_field :194-203
            for (; is_int && k < fl; k++) if (f[k] < '0' || f[k] > '9') is_int = false;
            if (is_int) continue;
            // is_float_field :205-216: strtod over a C string of the field's bytes, which ends at a NUL inside it
            const std::string t(f, fl); char *endp = nullptr; (void)strtod(t.c_str(), &endp);
            const bool is_flt = endp && *endp == 0;
            if (is_flt) { if (st[(size_t)i] != ST_STR) st[(size_t)i] = ST_DBL; } else st[(size_t)i] = ST_STR;
        }
        for (int i = 0; i < bd_n_cols; i++) out->types[i] = st[(size_t)i] == ST_INT ? DHTS_T_BIGINT : st[(size_t)i] == ST_DBL ? DHTS_T_DOUBLE : DHTS_T_VARCHAR;
    }
    return 0;
}

// ---- the scan -------------------------------------------------------------------------------------------------------------------------------
static int tabix_next_batch_one(dhts_ctx *c, int64_t max_blocks, dhts_tabix_batch *out) {
    memset(out, 0, sizeof(*out));
    BedState &S = c->bed; TabixState &Q = c->tbx;
    HIPCHK(c, hipSetDevice(c->device));
    const int ncols = (int)Q.proj.size();
    const bool gxf = Q.mode != DHTS_TABIX_GENERIC;
    Q.out.assign((size_t)ncols, dhts_col()); Q.out_types.assign((size_t)ncols, 0); Q.cols.assign((size_t)ncols, TabixCol());
    int nfix = 0, nstr = 0, ndbl = 0, map_at = -1;
    for (int i = 0; i < ncols; i++) {
        const int32_t col = Q.proj[(size_t)i];
        memset(&Q.out[(size_t)i], 0, sizeof(dhts_col)); Q.out[(size_t)i].col = col;
        TabixCol &t = Q.cols[(size_t)i]; memset(&t, 0, sizeof(t));
        if (gxf && col == DHTS_GXF_ATTRIBUTES_MAP) { t.kind = TABIX_K_MAP; map_at = i; continue; }
        const int32_t ty = Q.types[(size_t)col];
        Q.out_types[(size_t)i] = ty; t.field = col;
        if (ty == DHTS_T_VARCHAR) { t.kind = TABIX_K_STR; t.slot = nstr++; }
        else { t.kind = ty == DHTS_T_DOUBLE ? TABIX_K_DBL : TABIX_K_INT; t.slot = nfix++; if (ty == DHTS_T_DOUBLE) ndbl++; }
    }
    out->n_cols = ncols; out->cols = Q.out.data(); out->col_types = Q.out_types.data(); out->has_map = map_at >= 0 ? 1 : 0;
    if (c->stream_done || c->n_blocks <= 0) { out->status = Q.status ? Q.status : 1; return 0; }
    if (S.rg_pending) return fail(c, "%s: a region query needs the tabix index (dhts_tabix_load_index) before the scan", tabix_who(c));
    TabixRows X;
    if (tabix_rows(c, max_blocks, ncols > 0, X)) return -1;
    const uint8_t *u = X.B.u; const int64_t nrows = X.nrows; const BedRows &R = X.R;
    if (nrows > 0 && ncols > 0) {
        const unsigned rgrid = (unsigned)((nrows + 255) / 256);
        const size_t stride = (size_t)nrows + 1;
        ENSURE(c, Q.coldev, (size_t)ncols * sizeof(TabixCol) + 64); ENSURE(c, Q.valid, (size_t)ncols * (size_t)nrows + 64); ENSURE(c, Q.ctr, 64);
        if (nfix) ENSURE(c, Q.fixed, (size_t)nfix * (size_t)nrows * 8 + 64);
        if (nstr) { ENSURE(c, Q.len, (size_t)nstr * stride * 4 + 64); ENSURE(c, Q.off, (size_t)nstr * stride * 4 + 64); }
        if (ndbl) ENSURE(c, Q.patch, (size_t)ndbl * (size_t)nrows * sizeof(TabixPatch) + 64);      // one per row and DOUBLE column: it cannot overflow
        HIPCHK(c, hipMemcpyAsync(Q.coldev.p, Q.cols.data(), (size_t)ncols * sizeof(TabixCol), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(Q.ctr.p, 0, 16, c->stream));
        TabixCols g; memset(&g, 0, sizeof(g));
        g.col = (const TabixCol *)Q.coldev.p; g.n = ncols; g.gxf = gxf ? 1 : 0; g.nrows = (uint32_t)nrows;
        g.valid = (uint8_t *)Q.valid.p; g.fixed = (unsigned long long *)Q.fixed.p; g.len = (uint32_t *)Q.len.p; g.off = (const uint32_t *)Q.off.p;
        g.patch = (TabixPatch *)Q.patch.p; g.ctr = (uint32_t *)Q.ctr.p;
        if (nfix) {
            uint32_t ctr[2] = {0, 0};
            {
                KTimer tm(c, DHTS_K_BCF_CHECK);
                hipLaunchKernelGGL(tabix_fixed, dim3(rgrid), dim3(256), 0, c->stream, R, g);
            }
            if (ndbl) {
                HIPCHK(c, hipMemcpyAsync(ctr, Q.ctr.p, 8, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
            }
            const uint32_t npatch = ctr[0];
            out->n_double_fast = ctr[1]; out->n_double_patched = npatch;
            if ((uint64_t)npatch > (uint64_t)ndbl * (uint64_t)nrows) return fail(c, "internal: more DOUBLE patches than DOUBLE values");
            if (npatch) {
                // the tokens the one-operation fast path declined: strtod on the host, value and validity written back before the batch leaves
                std::vector<TabixPatch> pt(npatch);
                HIPCHK(c, hipMemcpy(pt.data(), Q.patch.p, (size_t)npatch * sizeof(TabixPatch), hipMemcpyDeviceToHost));
                std::vector<uint32_t> tk_off((size_t)npatch + 1, 0);
                for (uint32_t i = 0; i < npatch; i++) tk_off[i + 1] = tk_off[i] + pt[i].len;
                std::vector<char> tk((size_t)tk_off[npatch] + 1, 0);
                ENSURE(c, Q.tok_off, (size_t)npatch * 4 + 64); ENSURE(c, Q.tok_bytes, (size_t)tk_off[npatch] + 64);
                HIPCHK(c, hipMemcpy(Q.tok_off.p, tk_off.data(), (size_t)npatch * 4, hipMemcpyHostToDevice));
                hipLaunchKernelGGL(vcf_gather_tokens, dim3((npatch + 255) / 256), dim3(256), 0, c->stream, u, (const uint32_t *)Q.patch.p, 2, 3, (const uint32_t *)Q.tok_off.p, npatch, (uint8_t *)Q.tok_bytes.p);
                HIPCHK(c, hipMemcpyAsync(tk.data(), Q.tok_bytes.p, tk_off[npatch], hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                std::vector<uint64_t> val(npatch, 0); std::vector<uint8_t> ok(npatch, 0);
                for (uint32_t i = 0; i < npatch; i++) {
                    const std::string t(tk.data() + tk_off[i], pt[i].len);     // (shorter than 128 bytes and free of NULs: the line ends at its first NUL)
                    char *endp = nullptr; const double d = strtod(t.c_str(), &endp);
                    if (endp && (size_t)(endp - t.c_str()) == t.size()) { memcpy(&val[i], &d, 8); ok[i] = 1; }
                }
                ENSURE(c, Q.pval, (size_t)npatch * 8 + 64); ENSURE(c, Q.pok, (size_t)npatch + 64);
                HIPCHK(c, hipMemcpy(Q.pval.p, val.data(), (size_t)npatch * 8, hipMemcpyHostToDevice)); HIPCHK(c, hipMemcpy(Q.pok.p, ok.data(), npatch, hipMemcpyHostToDevice));
                hipLaunchKernelGGL(tabix_patch_apply, dim3((npatch + 255) / 256), dim3(256), 0, c->stream, (const TabixPatch *)Q.patch.p, (const unsigned long long *)Q.pval.p, (const uint8_t *)Q.pok.p, npatch, g);
            }
        }
        std::vector<uint64_t> totals((size_t)nstr + 1, 0);
        if (nstr) {
            {
                KTimer tm(c, DHTS_K_BCF_MEASURE);
                hipLaunchKernelGGL(tabix_str_measure, dim3(rgrid), dim3(256), 0, c->stream, R, g);
            }
            {
                KTimer tm(c, DHTS_K_SCAN);                                      // the scan kernels take eight arrays at a time
                for (int k0 = 0; k0 < nstr; k0 += 8) {
                    const int nk = nstr - k0 < 8 ? nstr - k0 : 8;
                    const uint32_t *kin[8]; uint32_t *kout[8];
                    for (int k = 0; k < nk; k++) { kin[k] = (const uint32_t *)Q.len.p + (size_t)(k0 + k) * stride; kout[k] = (uint32_t *)Q.off.p + (size_t)(k0 + k) * stride; }
                    if (run_scan(c, nk, kin, kout, nullptr, nrows, totals.data() + k0)) return -1;
                }
            }
            uint64_t arena = 0;
            for (int i = 0; i < ncols; i++) if (Q.cols[(size_t)i].kind == TABIX_K_STR) {
                const uint64_t t = totals[(size_t)Q.cols[(size_t)i].slot];
                if (t >= (1ull << 32)) return fail(c, "%s: a VARCHAR column of one batch holds more than 4 GiB: use a smaller max_blocks", tabix_who(c));
                Q.cols[(size_t)i].base = arena; arena += (t + 15) & ~15ull;
            }
            ENSURE(c, Q.bytes, (size_t)arena + 64);
            g.bytes = (uint8_t *)Q.bytes.p;
            HIPCHK(c, hipMemcpyAsync(Q.coldev.p, Q.cols.data(), (size_t)ncols * sizeof(TabixCol), hipMemcpyHostToDevice, c->stream));
            KTimer tm(c, DHTS_K_BCF_WRITE);
            hipLaunchKernelGGL(tabix_str_gather, dim3(rgrid), dim3(256), 0, c->stream, R, g);
        }
        if (map_at >= 0) {
            const size_t rn = stride * 4 + 64;
            ENSURE(c, Q.a_np, rn); ENSURE(c, Q.a_kb, rn); ENSURE(c, Q.a_vb, rn); ENSURE(c, Q.a_po, rn); ENSURE(c, Q.a_ko, rn); ENSURE(c, Q.a_vo, rn); ENSURE(c, Q.a_valid, (size_t)nrows + 64);
            TabixAttr m; memset(&m, 0, sizeof(m));
            m.gff = Q.mode == DHTS_TABIX_GFF ? 1 : 0;
            m.npair = (uint32_t *)Q.a_np.p; m.kbytes = (uint32_t *)Q.a_kb.p; m.vbytes = (uint32_t *)Q.a_vb.p;
            m.pair_off = (const uint32_t *)Q.a_po.p; m.kb_off = (const uint32_t *)Q.a_ko.p; m.vb_off = (const uint32_t *)Q.a_vo.p; m.valid = (uint8_t *)Q.a_valid.p;
            {
                KTimer tm(c, DHTS_K_STRINGS);
                hipLaunchKernelGGL(tabix_attr<false>, dim3(rgrid), dim3(256), 0, c->stream, R, m);
            }
            uint64_t tot[3] = {0, 0, 0};
            {
                KTimer tm(c, DHTS_K_SCAN);
                const uint32_t *kin[3] = {m.npair, m.kbytes, m.vbytes}; uint32_t *kout[3] = {(uint32_t *)Q.a_po.p, (uint32_t *)Q.a_ko.p, (uint32_t *)Q.a_vo.p};
                if (run_scan(c, 3, kin, kout, nullptr, nrows, tot)) return -1;
            }
            if (tot[0] >= (1ull << 32) - 1 || tot[1] >= (1ull << 32) || tot[2] >= (1ull << 32)) return fail(c, "%s: the attribute pairs of one batch exceed 4 GiB: use a smaller max_blocks", tabix_who(c));
            ENSURE(c, Q.a_keyoff, (size_t)(tot[0] + 1) * 4 + 64); ENSURE(c, Q.a_valoff, (size_t)(tot[0] + 1) * 4 + 64); ENSURE(c, Q.a_kbytes, (size_t)tot[1] + 64); ENSURE(c, Q.a_vbytes, (size_t)tot[2] + 64);
            m.key_off = (uint32_t *)Q.a_keyoff.p; m.val_off = (uint32_t *)Q.a_valoff.p; m.key_bytes = (uint8_t *)Q.a_kbytes.p; m.val_bytes = (uint8_t *)Q.a_vbytes.p;
            {
                KTimer tm(c, DHTS_K_STRINGS);
                hipLaunchKernelGGL(tabix_attr<true>, dim3(rgrid), dim3(256), 0, c->stream, R, m);
            }
            dhts_tabix_map &o = out->map;
            o.pair_off = m.pair_off; o.valid = m.valid; o.n_pairs = tot[0];
            o.key_off = m.key_off; o.key_bytes = m.key_bytes; o.key_nbytes = tot[1]; o.val_off = m.val_off; o.val_bytes = m.val_bytes; o.val_nbytes = tot[2];
        }
        HIPCHK(c, hipGetLastError());
        for (int i = 0; i < ncols; i++) {
            dhts_col &o = Q.out[(size_t)i]; const TabixCol &t = Q.cols[(size_t)i];
            if (t.kind == TABIX_K_MAP) continue;
            o.valid = (const uint8_t *)Q.valid.p + (size_t)i * (size_t)nrows;
            if (t.kind == TABIX_K_STR) { o.off = (const uint32_t *)Q.off.p + (size_t)t.slot * stride; o.bytes = (const uint8_t *)Q.bytes.p + t.base; o.nbytes = totals[(size_t)t.slot]; }
            else o.fixed = (const uint8_t *)Q.fixed.p + (size_t)t.slot * (size_t)nrows * 8;
        }
    }
    out->n_rows = nrows;
    if (batch_end(c, X.B, X.T.carry_start, false, X.T.finished, &out->status)) return -1;
    if (out->status < 0) Q.status = out->status;
    return 0;
}

int dhts_tabix_next_batch(dhts_ctx *c, int64_t max_blocks, dhts_tabix_batch *out) {
    if (!c || !out) return -1;
    TABIX_OPEN(c);
    for (;;) {
        if (tabix_next_batch_one(c, max_blocks, out)) return -1;
        // several index windows: the end of one window is the start of the next, not the end of the scan
        if (next_window(c, out->status) && out->n_rows == 0) continue;
        return 0;
    }
}

// read-back: as dhts_bed_batch_fetch, and the five arrays of the map behind the columns
static uint64_t pad8(uint64_t n) { return (n + 7) & ~7ull; }
uint64_t dhts_tabix_batch_host_bytes(const dhts_tabix_batch *b) {
    if (!b) return 0;
    uint64_t need = 0; const uint64_t n = (uint64_t)b->n_rows;
    for (int i = 0; i < b->n_cols; i++) {
        if (b->col_types[i] == 0) continue;
        need += pad8(n);
        if (b->col_types[i] != DHTS_T_VARCHAR) need += n * 8; else need += pad8((n + 1) * 4) + pad8(b->cols[i].nbytes);
    }
    if (b->has_map) need += pad8(n) + pad8((n + 1) * 4) + 2 * pad8((b->map.n_pairs + 1) * 4) + pad8(b->map.key_nbytes) + pad8(b->map.val_nbytes);
    return need;
}
int dhts_tabix_batch_fetch(dhts_ctx *c, const dhts_tabix_batch *b, void *dst, uint64_t cap, dhts_col *out_cols, dhts_tabix_map *out_map) {
    if (!c || !b || !out_cols || (!dst && cap)) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    if (cap < dhts_tabix_batch_host_bytes(b)) return fail(c, "read_tabix: fetch buffer too small");
    if (b->has_map && !out_map) return fail(c, "read_tabix: the batch has a map and the caller no room for it");
    uint8_t *p = (uint8_t *)dst; const uint64_t n = (uint64_t)b->n_rows;
    auto take = [&](const void *src, uint64_t nbytes) -> const uint8_t * {
        const uint8_t *at = p;
        if (nbytes && hipMemcpyAsync(p, src, nbytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return nullptr;
        p += pad8(nbytes);
        return at;
    };
    bool ok = true;
    for (int i = 0; i < b->n_cols; i++) {
        const dhts_col &s = b->cols[i]; dhts_col &o = out_cols[i];
        memset(&o, 0, sizeof(o)); o.col = s.col;
        if (n == 0 || b->col_types[i] == 0) continue;
        ok = ok && (o.valid = take(s.valid, n));
        if (b->col_types[i] != DHTS_T_VARCHAR) ok = ok && (o.fixed = take(s.fixed, n * 8));
        else { ok = ok && (o.off = (const uint32_t *)take(s.off, (n + 1) * 4)); ok = ok && (o.bytes = take(s.bytes, s.nbytes)); o.nbytes = s.nbytes; }
    }
    if (out_map) memset(out_map, 0, sizeof(*out_map));
    if (b->has_map && n > 0) {
        const dhts_tabix_map &m = b->map; dhts_tabix_map &o = *out_map;
        o.n_pairs = m.n_pairs; o.key_nbytes = m.key_nbytes; o.val_nbytes = m.val_nbytes;
        ok = ok && (o.valid = take(m.valid, n)); ok = ok && (o.pair_off = (const uint32_t *)take(m.pair_off, (n + 1) * 4));
        ok = ok && (o.key_off = (const uint32_t *)take(m.key_off, (m.n_pairs + 1) * 4)); ok = ok && (o.val_off = (const uint32_t *)take(m.val_off, (m.n_pairs + 1) * 4));
        ok = ok && (o.key_bytes = take(m.key_bytes, m.key_nbytes)); ok = ok && (o.val_bytes = take(m.val_bytes, m.val_nbytes));
    }
    if (!ok) return fail(c, "read_tabix: read-back failed");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
