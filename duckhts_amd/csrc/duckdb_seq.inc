// duckdb_seq.inc -- part of duckdb_ext.cpp (included there; not a translation unit of its own): the read_fastq and read_fasta table functions.
// ================================================================================================
// read_fastq -- mirrors register_read_fastq_function src/seq_reader.c:752-775, seq_read_bind 235-325, seq_read_init 334-402,
// seq_read_function 413-639.  The rows come out of the same read_bam batches (fastq_text.hip): NAME = QNAME, SEQUENCE = SEQ ('' for an
// empty read), QUALITY = QUAL (NULL where read_bam shows '*'), DESCRIPTION always NULL (the reference sets no CO tag under default
// options).  One thread (duckdb_init_set_max_threads(info, 1)); mate_path runs a second context and interleaves the rows.
// Registered by duckhts_init_c_api only when DHTS_SEQ_FUNCTIONS=1 (INTEGRATION.md).
// ================================================================================================
enum { FQ_COL_NAME = 0, FQ_COL_DESCRIPTION, FQ_COL_SEQUENCE, FQ_COL_QUALITY, FQ_COL_MATE, FQ_COL_PAIR_ID };
static const uint32_t kFqMask = (1u << DHTS_BAM_QNAME) | (1u << DHTS_BAM_SEQ) | (1u << DHTS_BAM_QUAL);
struct FqBind { std::string path, mate_path; bool paired = false, interleaved = false; dhts_ctx *ctx[2] = {nullptr, nullptr}; };
struct FqStream {
    dhts_ctx *ctx = nullptr; PinnedArena arena; dhts_bam_batch hb; int64_t pos = 0; bool done = false; std::string err;
    // the next record of the stream (its row in hb), or -1 at the end: EOF or the first record the reader refuses (sam_read1 < 0)
    int64_t next() {
        for (;;) {
            if (pos < hb.n_rows) return pos++;
            if (done) return -1;
            dhts_bam_batch b;
            if (dhts_bam_next_batch(ctx, 0, kFqMask, &b) != 0) { err = dhts_error(ctx); done = true; return -1; }
            if (b.status != 0) done = true;
            memset(&hb, 0, sizeof(hb)); pos = 0;
            if (b.n_rows == 0) continue;
            const uint64_t need = dhts_bam_batch_host_bytes(&b, kFqMask);
            const bool room = arena.reserve(need);
            if (!room || dhts_bam_batch_fetch(ctx, &b, kFqMask, arena.p, arena.cap, &hb) != 0) { err = room ? dhts_error(ctx) : "read_fastq: out of pinned host memory"; done = true; memset(&hb, 0, sizeof(hb)); return -1; }
        }
    }
    const char *name(int64_t r, uint32_t *n) const { *n = hb.qname.len[r]; return (const char *)hb.qname.bytes + hb.qname.off[r]; }
};
struct FqScan { FqStream st[2]; bool paired = false, interleaved = false, done = false; int pending_mate = 0, interleaved_mate = 1; int64_t mate_row = -1; Projection pj; std::vector<char> tmp; };
static const char *const kFqCols[6] = {"NAME", "DESCRIPTION", "SEQUENCE", "QUALITY", "MATE", "PAIR_ID"};                                             // seq_reader.c:311-320
static const int32_t kFqTypes[6] = {DUCKDB_TYPE_VARCHAR, DUCKDB_TYPE_VARCHAR, DUCKDB_TYPE_VARCHAR, DUCKDB_TYPE_VARCHAR, DUCKDB_TYPE_USMALLINT, DUCKDB_TYPE_VARCHAR};
// NAME / DESCRIPTION / SEQUENCE of record r of a stream's batch -> row `row` of the column's vector; false: the column is another one
static bool fill_seq_record(idx_t col, duckdb_vector vec, idx_t row, const FqStream &s, int64_t r, std::vector<char> &tmp) {
    auto assign_len = API(void, duckdb_vector_assign_string_element_len, duckdb_vector, idx_t, const char *, idx_t);
    switch (col) {
    case FQ_COL_NAME: { uint32_t n; const char *q = s.name(r, &n); assign_len(vec, row, q, strnlen(q, n)); return true; }
    case FQ_COL_DESCRIPTION: set_null(vec, row); return true;
    case FQ_COL_SEQUENCE: {
        const uint32_t l_seq = s.hb.seq.len[r];
        if (l_seq == 0) { assign_len(vec, row, "", 0); return true; }
        if (tmp.size() < (size_t)l_seq + 32) tmp.resize((size_t)l_seq + 32 + l_seq / 2);
        expand_seq(s.hb.seq.bytes + s.hb.seq.off[r], l_seq, tmp.data());
        assign_len(vec, row, tmp.data(), l_seq);
        return true;
    }
    default: return false;
    }
}
static void destroy_fq_bind(void *p) { FqBind *b = (FqBind *)p; if (!b) return; for (auto c : b->ctx) if (c) dhts_destroy(c); delete b; }
static void destroy_fq_scan(void *p) { delete (FqScan *)p; }

static void fastq_read_bind(duckdb_bind_info info) {
    auto set_error = API(void, duckdb_bind_set_error, duckdb_bind_info, const char *);
    std::string file_path;
    if (!take_path(info, file_path)) { set_error(info, "read_fastq requires a file path"); return; }   // seq_reader.c:240-246
    FqBind *b = new FqBind();
    b->path = file_path;
    char err[768];
    if (!file_exists(b->path)) { snprintf(err, sizeof(err), "Failed to open file: %s", b->path.c_str()); set_error(info, err); delete b; return; }   // seq_reader.c:250-256
    b->paired = named_string(info, "mate_path", b->mate_path);
    b->interleaved = named_flag(info, "interleaved");
    if (b->paired && b->interleaved) { set_error(info, "read_fastq: use mate_path or interleaved, not both"); delete b; return; }                     // seq_reader.c:287-291
    // the files are staged whole here; the scan reads them batch by batch (a file that is not FASTQ / FASTA text is refused: INTEGRATION.md)
    for (int k = 0; k < (b->paired ? 2 : 1); k++) {
        const std::string &path = k ? b->mate_path : b->path;
        if (k && !file_exists(path)) { set_error(info, "Failed to open mate FASTQ file"); destroy_fq_bind(b); return; }                              // seq_reader.c:369-370 (raised at init there)
        std::string no_device;
        b->ctx[k] = create_ctx("read_fastq", no_device);
        if (!b->ctx[k]) { set_error(info, no_device.c_str()); destroy_fq_bind(b); return; }
        if (dhts_open_path(b->ctx[k], path.c_str()) != 0 || dhts_bgzf_index(b->ctx[k]) <= 0 || dhts_bam_open(b->ctx[k]) != 0 || dhts_bam_is_text(b->ctx[k]) < 3) {
            snprintf(err, sizeof(err), "read_fastq: %s is not read as FASTQ/FASTA text by this build (a first record the FASTQ parser refuses counts as that)", path.c_str());
            set_error(info, err); destroy_fq_bind(b); return;
        }
    }
    add_columns(info, kFqCols, kFqTypes, b->paired || b->interleaved ? 6 : 4);
    API(void, duckdb_bind_set_bind_data, duckdb_bind_info, void *, duckdb_delete_callback_t)(info, b, destroy_fq_bind);
}
static void fastq_read_init(duckdb_init_info info) {
    FqBind *bind = (FqBind *)API(void *, duckdb_init_get_bind_data, duckdb_init_info)(info);
    FqScan *g = new FqScan();
    g->paired = bind->paired; g->interleaved = bind->interleaved;
    for (int k = 0; k < (bind->paired ? 2 : 1); k++) {
        g->st[k].ctx = bind->ctx[k]; memset(&g->st[k].hb, 0, sizeof(g->st[k].hb));
        dhts_bam_set_seq_packed(bind->ctx[k], 1); dhts_bam_set_qual_packed(bind->ctx[k], 0);
        if (dhts_bam_rewind(bind->ctx[k]) != 0) { API(void, duckdb_init_set_error, duckdb_init_info, const char *)(info, "Failed to open sequence file"); delete g; return; }
    }
    map_projection(info, 0, g->pj);
    API(void, duckdb_init_set_max_threads, duckdb_init_info, idx_t)(info, 1);
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, g, destroy_fq_scan);
}
static void fastq_read_function(duckdb_function_info info, duckdb_data_chunk output) {
    FqScan *g = (FqScan *)API(void *, duckdb_function_get_init_data, duckdb_function_info)(info);
    auto set_size = API(void, duckdb_data_chunk_set_size, duckdb_data_chunk, idx_t);
    if (!g || g->done) { set_size(output, 0); return; }
    const idx_t vector_size = API(idx_t, duckdb_vector_size, void)();
    auto get_vec = API(duckdb_vector, duckdb_data_chunk_get_vector, duckdb_data_chunk, idx_t);
    auto get_data = API(void *, duckdb_vector_get_data, duckdb_vector);
    auto assign_len = API(void, duckdb_vector_assign_string_element_len, duckdb_vector, idx_t, const char *, idx_t);
    auto fail_scan = [&](const char *msg) { API(void, duckdb_function_set_error, duckdb_function_info, const char *)(info, msg); g->done = true; set_size(output, 0); };
    idx_t row_count = 0;
    while (row_count < vector_size) {
        FqStream *s = &g->st[0]; int64_t r; int mate = 0;
        if (g->paired) {                                                                             // seq_reader.c:476-511
            if (g->pending_mate) { s = &g->st[1]; r = g->mate_row; mate = 2; g->pending_mate = 0; }
            else {
                const int64_t r1 = g->st[0].next(), r2 = g->st[1].next();
                if (r1 < 0 || r2 < 0) {
                    if (r1 < 0 && r2 < 0) { g->done = true; break; }
                    fail_scan("read_fastq: mate files have different record counts"); return;
                }
                uint32_t n1, n2; const char *q1 = g->st[0].name(r1, &n1), *q2 = g->st[1].name(r2, &n2);
                const size_t l1 = strnlen(q1, n1), l2 = strnlen(q2, n2);                             // (strcmp reads C strings)
                if (l1 != l2 || memcmp(q1, q2, l1) != 0) {
                    char msg[256]; snprintf(msg, sizeof(msg), "read_fastq: mate files out of sync (QNAME mismatch: '%.*s' vs '%.*s')", (int)l1, q1, (int)l2, q2);
                    fail_scan(msg); return;
                }
                r = r1; mate = 1; g->pending_mate = 1; g->mate_row = r2;
            }
        } else {                                                                                     // seq_reader.c:512-531
            r = s->next();
            if (r < 0) {
                if (g->interleaved && g->interleaved_mate == 2) { fail_scan("read_fastq: interleaved file has an unpaired record"); return; }
                g->done = true; break;
            }
            if (g->interleaved) { mate = g->interleaved_mate; g->interleaved_mate = mate == 1 ? 2 : 1; }
        }
        const dhts_bam_batch &b = s->hb;
        const uint32_t l_seq = b.seq.len[r];
        for (size_t ci = 0; ci < g->pj.column_ids.size(); ci++) {
            duckdb_vector vec = get_vec(output, ci);
            if (fill_seq_record(g->pj.column_ids[ci], vec, row_count, *s, r, g->tmp)) continue;
            switch (g->pj.column_ids[ci]) {
            case FQ_COL_QUALITY: {
                // "seq_len > 0 && qual[0] != 255": the batch shows an absent QUAL as the one character '*' (a one-base read of quality 9 reads the same: INTEGRATION.md)
                const uint32_t n = b.qual.len[r]; const char *q = (const char *)b.qual.bytes + b.qual.off[r];
                if (l_seq == 0 || (n == 1 && q[0] == '*' )) set_null(vec, row_count); else assign_len(vec, row_count, q, n);
                break;
            }
            case FQ_COL_MATE:
                if (g->paired || g->interleaved) ((uint16_t *)get_data(vec))[row_count] = (uint16_t)mate; else set_null(vec, row_count);
                break;
            case FQ_COL_PAIR_ID: {
                if (!(g->paired || g->interleaved)) { set_null(vec, row_count); break; }
                uint32_t n; const char *q = s->name(r, &n); size_t len = strnlen(q, n);
                if (len >= 2 && q[len - 2] == '/' && (q[len - 1] == '1' || q[len - 1] == '2')) len -= 2;     // strip_pair_suffix, seq_reader.c:171-182
                assign_len(vec, row_count, q, len);
                break;
            }
            default: break;
            }
        }
        row_count++;
    }
    for (auto &st : g->st) if (!st.err.empty()) { fail_scan(st.err.c_str()); return; }
    set_size(output, row_count);
}
extern "C" __attribute__((visibility("default"))) void register_read_fastq_function(duckdb_connection connection) {                    // seq_reader.c:752-775
    register_table_function(connection, "read_fastq", {{"mate_path", DUCKDB_TYPE_VARCHAR}, {"interleaved", DUCKDB_TYPE_BOOLEAN}}, fastq_read_bind, fastq_read_init, nullptr, fastq_read_function, true);
}

// ================================================================================================
// read_fasta -- mirrors register_read_fasta_function src/seq_reader.c:645-662, seq_read_bind 235-325, seq_read_init 334-402,
// seq_read_function 413-472 (regions) and 533-583 (records).  Without a region the rows come out of the read_bam batches of FASTA text
// like read_fastq's (NAME = QNAME, SEQUENCE = SEQ, '' when empty; DESCRIPTION is the CO tag in the reference, which fastq_parse1 makes only
// under the fastq_aux option the reference never sets, so it is NULL).  With a region: one row per region in the order given, from the
// device .fai fetch (dhts_fasta_load_index / dhts_fasta_open_regions / dhts_fasta_fetch); the index is <path>.fai or index_path and is
// never built here.  One thread.  Registered by duckhts_init_c_api only when DHTS_SEQ_FUNCTIONS=1.
// ================================================================================================
struct FaBind { std::string path, region, index_path; int n_regions = 0; dhts_ctx *ctx = nullptr; };
struct FaScan { FqStream st; bool regions = false, done = false; dhts_ctx *rctx = nullptr; PinnedArena arena; dhts_fasta_batch hb; int64_t pos = 0; std::string err; Projection pj; std::vector<char> tmp;
                ~FaScan() { if (rctx) dhts_destroy(rctx); } };
static void destroy_fa_bind(void *p) { FaBind *b = (FaBind *)p; if (!b) return; if (b->ctx) dhts_destroy(b->ctx); delete b; }
static void destroy_fa_scan(void *p) { delete (FaScan *)p; }
// parse_regions_duckdb (seq_reader.c:192-229): pieces between commas, blanks and tabs trimmed, empty ones dropped
static std::vector<std::string> fasta_split_regions(const std::string &all) {
    std::vector<std::string> out; size_t p = 0;
    while (p <= all.size()) {
        size_t e = all.find(',', p); if (e == std::string::npos) e = all.size();
        size_t a = p, b = e; while (a < b && (all[a] == ' ' || all[a] == '\t')) a++; while (b > a && (all[b - 1] == ' ' || all[b - 1] == '\t')) b--;
        if (b > a) out.push_back(all.substr(a, b - a));
        p = e + 1;
    }
    return out;
}
static void fasta_read_bind(duckdb_bind_info info) {
    auto set_error = API(void, duckdb_bind_set_error, duckdb_bind_info, const char *);
    std::string file_path;
    if (!take_path(info, file_path)) { set_error(info, "read_fasta requires a file path"); return; }   // seq_reader.c:240-246
    FaBind *b = new FaBind();
    b->path = file_path;
    char err[768];
    if (!file_exists(b->path)) { snprintf(err, sizeof(err), "Failed to open file: %s", b->path.c_str()); set_error(info, err); delete b; return; }   // seq_reader.c:250-256
    if (named_string(info, "region", b->region)) b->n_regions = (int)fasta_split_regions(b->region).size();
    (void)named_string(info, "index_path", b->index_path);
    if (b->n_regions == 0) {                                     // a whole-file scan: the file is staged here, the scan reads it batch by batch
        std::string no_device;
        b->ctx = create_ctx("read_fasta", no_device);
        if (!b->ctx) { set_error(info, no_device.c_str()); destroy_fa_bind(b); return; }
        if (dhts_open_path(b->ctx, b->path.c_str()) != 0 || dhts_bgzf_index(b->ctx) <= 0 || dhts_bam_open(b->ctx) != 0 || dhts_bam_is_text(b->ctx) < 3) {
            snprintf(err, sizeof(err), "read_fasta: %s is not read as FASTQ/FASTA text by this build (a first record the FASTQ parser refuses counts as that)", b->path.c_str());
            set_error(info, err); destroy_fa_bind(b); return;
        }
    }
    add_columns(info, kFqCols, kFqTypes, 3);                                                                                                         // seq_reader.c:311-313
    API(void, duckdb_bind_set_bind_data, duckdb_bind_info, void *, duckdb_delete_callback_t)(info, b, destroy_fa_bind);
}
static void fasta_read_init(duckdb_init_info info) {
    FaBind *bind = (FaBind *)API(void *, duckdb_init_get_bind_data, duckdb_init_info)(info);
    auto init_error = API(void, duckdb_init_set_error, duckdb_init_info, const char *);
    FaScan *g = new FaScan();
    memset(&g->hb, 0, sizeof(g->hb)); memset(&g->st.hb, 0, sizeof(g->st.hb));
    if (bind->n_regions > 0) {                                   // seq_reader.c:383-390: the index is loaded, never built
        g->regions = true;
        const std::string fai_path = bind->index_path.empty() ? bind->path + ".fai" : bind->index_path;
        std::string fai, no_device; const bool have = read_file(fai_path, fai);
        g->rctx = have ? create_ctx("read_fasta", no_device) : nullptr;
        if (have && !g->rctx) { init_error(info, no_device.c_str()); delete g; return; }
        if (!have || dhts_fasta_load_index(g->rctx, fai.data(), fai.size()) != 0 || dhts_fasta_open_regions(g->rctx, bind->path.c_str(), bind->region.c_str()) != 0) {
            init_error(info, "read_fasta: region query requires a FASTA index (.fai); run fasta_index(path) first"); delete g; return;
        }
        dhts_fasta_batch db;
        if (dhts_fasta_fetch(g->rctx, bind->region.c_str(), &db) != 0) {
            // fai_fetch64 fails region by region (seq_reader.c:432-441): name the first one that does
            std::string bad;
            for (auto &r : fasta_split_regions(bind->region)) { dhts_fasta_batch one; if (dhts_fasta_fetch(g->rctx, r.c_str(), &one) != 0) { bad = r; break; } }
            g->err = "read_fasta: invalid or missing region '" + bad + "'";
        } else {
            const uint64_t need = dhts_fasta_batch_host_bytes(&db);
            const bool room = g->arena.reserve(need) && g->arena.p;
            if (!room || dhts_fasta_batch_fetch(g->rctx, &db, g->arena.p, need, &g->hb) != 0) { init_error(info, room ? dhts_error(g->rctx) : "read_fasta: out of pinned host memory"); delete g; return; }
        }
    } else {
        g->st.ctx = bind->ctx;
        dhts_bam_set_seq_packed(bind->ctx, 1); dhts_bam_set_qual_packed(bind->ctx, 0);
        if (dhts_bam_rewind(bind->ctx) != 0) { init_error(info, "Failed to open sequence file"); delete g; return; }
    }
    map_projection(info, 0, g->pj);
    API(void, duckdb_init_set_max_threads, duckdb_init_info, idx_t)(info, 1);
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, g, destroy_fa_scan);
}
static void fasta_read_function(duckdb_function_info info, duckdb_data_chunk output) {
    FaScan *g = (FaScan *)API(void *, duckdb_function_get_init_data, duckdb_function_info)(info);
    auto set_size = API(void, duckdb_data_chunk_set_size, duckdb_data_chunk, idx_t);
    if (!g || g->done) { set_size(output, 0); return; }
    const idx_t vector_size = API(idx_t, duckdb_vector_size, void)();
    auto get_vec = API(duckdb_vector, duckdb_data_chunk_get_vector, duckdb_data_chunk, idx_t);
    auto assign_len = API(void, duckdb_vector_assign_string_element_len, duckdb_vector, idx_t, const char *, idx_t);
    auto fail_scan = [&](const char *msg) { API(void, duckdb_function_set_error, duckdb_function_info, const char *)(info, msg); g->done = true; set_size(output, 0); };
    if (!g->err.empty()) { fail_scan(g->err.c_str()); return; }
    idx_t row_count = 0;
    while (row_count < vector_size) {
        if (g->regions) {                                                                            // seq_reader.c:425-472
            if (g->pos >= g->hb.n_rows) { g->done = true; break; }
            const int64_t r = g->pos++;
            for (size_t ci = 0; ci < g->pj.column_ids.size(); ci++) {
                duckdb_vector vec = get_vec(output, ci);
                switch (g->pj.column_ids[ci]) {
                case FQ_COL_NAME: assign_len(vec, row_count, (const char *)g->hb.name_bytes + g->hb.name_off[r], g->hb.name_off[r + 1] - g->hb.name_off[r]); break;
                case FQ_COL_DESCRIPTION: set_null(vec, row_count); break;
                case FQ_COL_SEQUENCE: assign_len(vec, row_count, (const char *)g->hb.seq_bytes + g->hb.seq_off[r], g->hb.seq_off[r + 1] - g->hb.seq_off[r]); break;
                default: break;
                }
            }
            row_count++;
            continue;
        }
        const int64_t r = g->st.next();
        if (r < 0) { g->done = true; break; }
        for (size_t ci = 0; ci < g->pj.column_ids.size(); ci++) (void)fill_seq_record(g->pj.column_ids[ci], get_vec(output, ci), row_count, g->st, r, g->tmp);
        row_count++;
    }
    if (!g->st.err.empty()) { fail_scan(g->st.err.c_str()); return; }
    set_size(output, row_count);
}
extern "C" __attribute__((visibility("default"))) void register_read_fasta_function(duckdb_connection connection) {                    // seq_reader.c:645-662
    register_table_function(connection, "read_fasta", {{"region", DUCKDB_TYPE_VARCHAR}, {"index_path", DUCKDB_TYPE_VARCHAR}}, fasta_read_bind, fasta_read_init, nullptr, fasta_read_function, true);
}
