// duckdb_interval.inc -- part of duckdb_ext.cpp (included there; not a translation unit of its own): the read_bed and fasta_nuc table functions.
// ---- read_bed (src/interval_udf.c:217-426, 838-852): one thread, file order, vector_size rows per chunk -------------------------------------
// bind checks the path and, for a region, that a tabix index can be read (tbx_index_load3: index_path, else <path>.tbi, <path>.csi); init
// stages the file -- for a region only the index windows -- and resolves the region; the scan fills chunks from device batches read back
// by dhts_bed_batch_fetch.  A line with fewer than 3 fields replaces the chunk it would have been in by read_bed's error.
static const char *const kBedCols[DHTS_BED_COL_COUNT] = {"chrom", "start", "end", "name", "score", "strand", "thick_start", "thick_end", "item_rgb", "block_count", "block_sizes", "block_starts", "extra"};
static const int32_t kBedTypes[DHTS_BED_COL_COUNT] = {DHTS_T_VARCHAR, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_VARCHAR, DHTS_T_VARCHAR, DHTS_T_VARCHAR, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_VARCHAR, DHTS_T_BIGINT, DHTS_T_VARCHAR, DHTS_T_VARCHAR, DHTS_T_VARCHAR};   // interval_udf.c:217-235
struct BedBind { std::string path, region; bool has_region = false; std::string index; };
struct BedScanState { dhts_ctx *ctx = nullptr; PinnedArena arena; Projection pj; ColBatch cb; ~BedScanState() { if (ctx) dhts_destroy(ctx); } };
static void destroy_bed_bind(void *p) { delete (BedBind *)p; }
static void destroy_bed_scan(void *p) { delete (BedScanState *)p; }
static void bed_read_bind(duckdb_bind_info info) {
    auto set_error = API(void, duckdb_bind_set_error, duckdb_bind_info, const char *);
    std::string file_path, index_path;
    if (!take_path(info, file_path)) { set_error(info, "read_bed requires a file path"); return; }   // interval_udf.c:242-246
    BedBind *b = new BedBind();
    b->path = file_path;
    b->has_region = named_string(info, "region", b->region);
    (void)named_string(info, "index_path", index_path);
    char err[768];
    if (!file_exists(b->path)) { snprintf(err, sizeof(err), "read_bed: failed to open file: %s", b->path.c_str()); set_error(info, err); delete b; return; }   // :262-271
    if (b->has_region && !load_tabix_index(b->path, index_path, b->index)) { set_error(info, "read_bed: region queries require a tabix index"); delete b; return; }   // :274-283
    add_columns(info, kBedCols, kBedTypes, DHTS_BED_COL_COUNT);
    API(void, duckdb_bind_set_bind_data, duckdb_bind_info, void *, duckdb_delete_callback_t)(info, b, destroy_bed_bind);
}
static void bed_read_init(duckdb_init_info info) {
    BedBind *bind = (BedBind *)API(void *, duckdb_init_get_bind_data, duckdb_init_info)(info);
    auto init_error = API(void, duckdb_init_set_error, duckdb_init_info, const char *);
    BedScanState *g = new BedScanState();
    std::string no_device;
    g->ctx = create_ctx("read_bed", no_device);
    if (!g->ctx) { init_error(info, no_device.c_str()); delete g; return; }
    bool staged = false;
    if (bind->has_region && file_is_bgzf(bind->path)) {
        // a BGZF file is staged by the index: nothing but the windows of the region (BED text has no header)
        int rc;
        const int st = stage_region_windows(g->ctx, bind->path, dhts_bed_region_segments, bind->region, bind->index, 0, &rc);
        if (rc == 1) { init_error(info, "read_bed: failed to create region iterator"); delete g; return; }                             // :314-319
        if (rc < 0) { init_error(info, "read_bed: failed to load tabix index"); delete g; return; }                                   // :308-313
        if (st == WINDOWS_OPEN_FAILED) { init_error(info, "read_bed: failed to open file during init"); delete g; return; }
        staged = st == WINDOWS_STAGED;
    }
    if (!staged && dhts_open_path(g->ctx, bind->path.c_str()) != 0) { init_error(info, "read_bed: failed to open file during init"); delete g; return; }   // :300-305
    (void)dhts_bgzf_index(g->ctx);                               // (text that is not BGZF fails here and is taken as text by dhts_bed_open)
    if (dhts_bed_open(g->ctx) != 0) { init_error(info, "read_bed: failed to open file during init"); delete g; return; }
    map_projection(info, DHTS_BED_COL_COUNT, g->pj);
    for (size_t ci = 0; ci < g->pj.slot.size(); ci++) g->cb.kind.push_back(g->pj.slot[ci] < 0 ? COL_NULL : kind_of_type(kBedTypes[g->pj.column_ids[ci]]));
    if (dhts_bed_set_projection(g->ctx, g->pj.proj.data(), (int32_t)g->pj.proj.size()) != 0) { init_error(info, dhts_error(g->ctx)); delete g; return; }
    if (bind->has_region) {
        if (dhts_bed_set_region(g->ctx, bind->region.c_str()) != 0) { const std::string m = dhts_error(g->ctx); init_error(info, m.c_str()); delete g; return; }
        const int rc = dhts_bed_load_index(g->ctx, bind->index.data(), bind->index.size());
        if (rc == 1) { init_error(info, "read_bed: failed to create region iterator"); delete g; return; }
        if (rc < 0) { init_error(info, "read_bed: failed to load tabix index"); delete g; return; }
    }
    g->cb.init(g->pj);
    API(void, duckdb_init_set_max_threads, duckdb_init_info, idx_t)(info, 1);
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, g, destroy_bed_scan);
}
// the next device batch, read back; false at the end of the stream (cb.status says how it ended) or on a failure (err set)
static bool bed_next(BedScanState *g, std::string &err) {
    ColBatch &cb = g->cb;
    while (cb.status == 0) {
        dhts_bed_batch b;
        if (dhts_bed_next_batch(g->ctx, 0, &b) != 0) { err = dhts_error(g->ctx); return false; }
        cb.status = b.status;
        if (b.n_rows == 0) continue;
        if (!g->arena.reserve(dhts_bed_batch_host_bytes(&b))) { err = "read_bed: out of pinned host memory"; return false; }
        if (dhts_bed_batch_fetch(g->ctx, &b, g->arena.p, g->arena.cap, cb.host.data()) != 0) { err = dhts_error(g->ctx); return false; }
        cb.n = b.n_rows; cb.pos = 0;
        return true;
    }
    return false;
}
static void bed_read_function(duckdb_function_info info, duckdb_data_chunk output) {
    BedScanState *g = (BedScanState *)API(void *, duckdb_function_get_init_data, duckdb_function_info)(info);
    if (!g) { API(void, duckdb_data_chunk_set_size, duckdb_data_chunk, idx_t)(output, 0); return; }
    // the short line would have been a row of this chunk: the chunk is the error (interval_udf.c:358-365); any other end of the
    // stream ends the scan as a failed hts_getline does (:334-337)
    scan_chunks(info, output, g->pj, g->cb, nullptr, [&](std::string &err) { return bed_next(g, err); }, [&]() -> const char * {
        return g->cb.status < 0 && strstr(dhts_error(g->ctx), "fewer than 3 tab-delimited fields") ? "read_bed: BED line has fewer than 3 tab-delimited fields" : nullptr; });
}
extern "C" __attribute__((visibility("default"))) void register_read_bed_function(duckdb_connection connection) {                      // interval_udf.c:838-852
    register_table_function(connection, "read_bed", {{"region", DUCKDB_TYPE_VARCHAR}, {"index_path", DUCKDB_TYPE_VARCHAR}}, bed_read_bind, bed_read_init, nullptr, bed_read_function, true);
}

// ---- fasta_nuc (src/interval_udf.c:451-836, 854-876): one thread, BED file order or bin order, vector_size rows per chunk --------------------
// bind checks the arguments and reads the .fai (index_path, else <fasta>.fai; unlike fai_load3_format a missing one is never built: it is
// the bind error); init stages the FASTA -- with a region of an uncompressed file only what the region reads -- puts the index on the
// device, resolves the region and prepares the BED context (with a region and a tabix index: the index windows only); the scan fills
// chunks from device batches read back by dhts_nuc_batch_fetch.  The BED lines' columns never visit the host.
static const char *const kNucCols[DHTS_NUC_COL_COUNT] = {"chrom", "start", "end", "pct_at", "pct_gc", "num_a", "num_c", "num_g", "num_t", "num_n", "num_other", "seq_len", "seq"};
static const int32_t kNucTypes[DHTS_NUC_COL_COUNT] = {DHTS_T_VARCHAR, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_DOUBLE, DHTS_T_DOUBLE, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_VARCHAR};   // interval_udf.c:451-473
struct NucBind { std::string fasta, bed, region, bed_index_path, fai; bool has_bed = false, has_region = false, include_seq = false; int64_t bin_width = 0; };
struct NucScanState {
    dhts_ctx *ctx = nullptr, *bed = nullptr; PinnedArena arena; int64_t bin_width = 0; Projection pj; ColBatch cb;
    ~NucScanState() { if (bed) dhts_destroy(bed); if (ctx) dhts_destroy(ctx); }
};
static void destroy_nuc_bind(void *p) { delete (NucBind *)p; }
static void destroy_nuc_scan(void *p) { delete (NucScanState *)p; }
static void fasta_nuc_bind(duckdb_bind_info info) {
    auto set_error = API(void, duckdb_bind_set_error, duckdb_bind_info, const char *);
    NucBind *b = new NucBind();
    if (!take_path(info, b->fasta)) { set_error(info, "fasta_nuc requires a FASTA path"); delete b; return; }   // interval_udf.c:479-483
    b->has_bed = named_string(info, "bed_path", b->bed);
    const bool has_bin_width = named_int(info, "bin_width", &b->bin_width);
    if (b->has_bed == has_bin_width) { set_error(info, "fasta_nuc requires exactly one of bed_path or bin_width"); delete b; return; }        // :499-504
    if (has_bin_width && b->bin_width <= 0) { set_error(info, "fasta_nuc bin_width must be > 0"); delete b; return; }                          // :505-510
    std::string index_path;
    b->has_region = named_string(info, "region", b->region) && !b->region.empty();
    (void)named_string(info, "index_path", index_path); (void)named_string(info, "bed_index_path", b->bed_index_path);
    b->include_seq = named_flag(info, "include_seq");
    // fai_load3_format (:532) opens the FASTA and its index; it would BUILD a missing index, this project never does
    if (!file_exists(b->fasta) || !read_file(index_path.empty() ? b->fasta + ".fai" : index_path, b->fai)) { set_error(info, "fasta_nuc: failed to open FASTA index"); delete b; return; }
    add_columns(info, kNucCols, kNucTypes, b->include_seq ? DHTS_NUC_COL_COUNT : DHTS_NUC_SEQ);
    API(void, duckdb_bind_set_bind_data, duckdb_bind_info, void *, duckdb_delete_callback_t)(info, b, destroy_nuc_bind);
}
static void fasta_nuc_init(duckdb_init_info info) {
    NucBind *bind = (NucBind *)API(void *, duckdb_init_get_bind_data, duckdb_init_info)(info);
    auto init_error = API(void, duckdb_init_set_error, duckdb_init_info, const char *);
    NucScanState *g = new NucScanState();
    g->bin_width = bind->bin_width;
    std::string no_device;
    g->ctx = create_ctx("fasta_nuc", no_device);
    if (!g->ctx) { init_error(info, no_device.c_str()); delete g; return; }
    auto fail_ctx = [&]() { const std::string m = std::string("fasta_nuc: ") + dhts_error(g->ctx); init_error(info, m.c_str()); delete g; };
    if (dhts_fasta_load_index(g->ctx, bind->fai.data(), bind->fai.size()) != 0) { init_error(info, "fasta_nuc: failed to load FASTA index"); delete g; return; }   // :578-583
    if (bind->has_region && !file_is_bgzf(bind->fasta)) {
        // an uncompressed file: only what the region reads -- its own window for bins, its whole sequence for BED rows, which may reach past it
        if (dhts_nuc_open_region(g->ctx, bind->fasta.c_str(), bind->region.c_str(), bind->has_bed ? 1 : 0) != 0) { init_error(info, "fasta_nuc: failed to load FASTA index"); delete g; return; }
    } else {
        if (dhts_open_path(g->ctx, bind->fasta.c_str()) != 0) { init_error(info, "fasta_nuc: failed to load FASTA index"); delete g; return; }
        (void)dhts_bgzf_index(g->ctx);
    }
    if (dhts_nuc_open(g->ctx, bind->include_seq ? 1 : 0) != 0) { fail_ctx(); return; }
    if (bind->has_region) {
        const int rc = dhts_nuc_set_region(g->ctx, bind->region.c_str());
        if (rc != 0) { init_error(info, "fasta_nuc: invalid FASTA region"); delete g; return; }                                                // :584-588
    }
    if (bind->has_bed) {
        if (!file_exists(bind->bed)) { init_error(info, "fasta_nuc: failed to open BED file"); delete g; return; }                              // :591-596
        g->bed = create_ctx("fasta_nuc", no_device);
        if (!g->bed) { init_error(info, no_device.c_str()); delete g; return; }
        // tbx_index_load3 with HTS_IDX_SILENT_FAIL (:598): without an index there is no iterator, the whole BED is read and filtered
        std::string index; bool staged = false;
        const bool have = bind->has_region && file_is_bgzf(bind->bed) && load_tabix_index(bind->bed, bind->bed_index_path, index);
        if (have) {
            int rc;
            const int st = stage_region_windows(g->bed, bind->bed, dhts_bed_region_segments, bind->region, index, 0, &rc);
            if (rc != 0) { init_error(info, "fasta_nuc: failed to create BED region iterator"); delete g; return; }                          // :600-605
            if (st == WINDOWS_OPEN_FAILED) { init_error(info, "fasta_nuc: failed to open BED file"); delete g; return; }
            staged = st == WINDOWS_STAGED;
        }
        if (!staged && dhts_open_path(g->bed, bind->bed.c_str()) != 0) { init_error(info, "fasta_nuc: failed to open BED file"); delete g; return; }
        (void)dhts_bgzf_index(g->bed);
        if (dhts_bed_open(g->bed) != 0) { init_error(info, "fasta_nuc: failed to open BED file"); delete g; return; }
        if (have) {
            if (dhts_bed_set_region(g->bed, bind->region.c_str()) != 0 || dhts_bed_load_index(g->bed, index.data(), index.size()) != 0) { init_error(info, "fasta_nuc: failed to create BED region iterator"); delete g; return; }
        }
    }
    map_projection(info, bind->include_seq ? DHTS_NUC_COL_COUNT : DHTS_NUC_SEQ, g->pj);
    for (size_t ci = 0; ci < g->pj.slot.size(); ci++)                                        // BIGINT and DOUBLE: eight bytes either way, never NULL
        g->cb.kind.push_back(g->pj.slot[ci] < 0 ? COL_NULL : kNucTypes[g->pj.column_ids[ci]] == DHTS_T_VARCHAR ? COL_STRING : COL_FIXED8_NOT_NULL);
    if (dhts_nuc_set_projection(g->ctx, g->pj.proj.data(), (int32_t)g->pj.proj.size()) != 0) { fail_ctx(); return; }
    g->cb.init(g->pj);
    API(void, duckdb_init_set_max_threads, duckdb_init_info, idx_t)(info, 1);
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, g, destroy_nuc_scan);
}
// the next device batch, read back; false at the end (or on a failure: err set)
static bool nuc_next(NucScanState *g, std::string &err) {
    ColBatch &cb = g->cb;
    while (cb.status == 0) {
        dhts_nuc_batch b;
        const int rc = g->bed ? dhts_nuc_next_bed(g->ctx, g->bed, 0, &b) : dhts_nuc_next_bins(g->ctx, g->bin_width, 0, &b);
        if (rc != 0) { err = dhts_error(g->ctx); return false; }
        cb.status = b.status;
        if (b.n_rows == 0) continue;
        if (!g->arena.reserve(dhts_nuc_batch_host_bytes(&b))) { err = "fasta_nuc: out of pinned host memory"; return false; }
        if (dhts_nuc_batch_fetch(g->ctx, &b, g->arena.p, g->arena.cap, cb.host.data()) != 0) { err = dhts_error(g->ctx); return false; }
        cb.n = b.n_rows; cb.pos = 0;
        return true;
    }
    return false;
}
static void fasta_nuc_function(duckdb_function_info info, duckdb_data_chunk output) {
    NucScanState *g = (NucScanState *)API(void *, duckdb_function_get_init_data, duckdb_function_info)(info);
    if (!g) { API(void, duckdb_data_chunk_set_size, duckdb_data_chunk, idx_t)(output, 0); return; }
    scan_chunks(info, output, g->pj, g->cb, nullptr, [&](std::string &err) { return nuc_next(g, err); });
}
extern "C" __attribute__((visibility("default"))) void register_fasta_nuc_function(duckdb_connection connection) {                     // interval_udf.c:854-876
    register_table_function(connection, "fasta_nuc", {{"bed_path", DUCKDB_TYPE_VARCHAR}, {"bin_width", DUCKDB_TYPE_BIGINT}, {"region", DUCKDB_TYPE_VARCHAR}, {"index_path", DUCKDB_TYPE_VARCHAR},
                            {"bed_index_path", DUCKDB_TYPE_VARCHAR}, {"include_seq", DUCKDB_TYPE_BOOLEAN}}, fasta_nuc_bind, fasta_nuc_init, nullptr, fasta_nuc_function, true);
}
