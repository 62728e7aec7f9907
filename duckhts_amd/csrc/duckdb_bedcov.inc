// duckdb_bedcov.inc -- part of duckdb_ext.cpp (included there behind duckdb_interval.inc; not a translation unit of its own): the bam_bedcov table function.
// bam_bedcov(path, bed_path, min_mapq, include_flags, require_flags, exclude_flags, count_deletions, count_ref_skips, region, index_path): for
// every row of the BED file the summed per-base depth and the number of overlapping reads (the contract: include/duckhts_amd.h).  bind checks
// the parameters and opens the BAM as read_bam does (bam_bind_file, bam_region_prepare: the same errors) and looks for the BED as read_bed does;
// init stages the BAM -- for a region only the index windows -- and the BED on one device and runs the whole scan there: no read leaves
// it; the scan callback pages the BED's rows out with their two results, vector_size rows per chunk.
static const char *const kBedcovCols[DHTS_BEDCOV_COL_COUNT] = {"chrom", "start", "end", "name", "score", "strand", "bases_covered", "read_count"};
static const int32_t kBedcovTypes[DHTS_BEDCOV_COL_COUNT] = {DHTS_T_VARCHAR, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_VARCHAR, DHTS_T_VARCHAR, DHTS_T_VARCHAR, DHTS_T_BIGINT, DHTS_T_BIGINT};
struct BedcovBind {
    BamBind bam; dhts_bedcov_params P; std::string bed;
    std::vector<uint8_t> index_bytes; std::vector<uint64_t> seg_beg, seg_end; int64_t seg_count = -1;
    ~BedcovBind() { if (bam.ctx) dhts_destroy(bam.ctx); }
};
struct BedcovScanState {
    dhts_ctx *ctx = nullptr, *bed = nullptr; PinnedArena arena; Projection pj; ColBatch cb;
    ~BedcovScanState() { if (bed) dhts_destroy(bed); if (ctx) dhts_destroy(ctx); }
};
static void destroy_bedcov_bind(void *p) { delete (BedcovBind *)p; }
static void destroy_bedcov_scan(void *p) { delete (BedcovScanState *)p; }
static void bam_bedcov_bind(duckdb_bind_info info) {
    auto set_error = API(void, duckdb_bind_set_error, duckdb_bind_info, const char *);
    std::string file_path, region, idx;
    if (!take_path(info, file_path)) { set_error(info, "bam_bedcov requires a file path"); return; }
    BedcovBind *b = new BedcovBind();
    if (!named_string(info, "bed_path", b->bed) || b->bed.empty()) { set_error(info, "bam_bedcov requires bed_path"); delete b; return; }
    int64_t min_mapq = 0, include_flags = 0, require_flags = 0, exclude_flags = 0x704;
    bool count_deletions = true, count_ref_skips = true;
    (void)named_int(info, "min_mapq", &min_mapq);
    (void)named_int(info, "include_flags", &include_flags); (void)named_int(info, "require_flags", &require_flags); (void)named_int(info, "exclude_flags", &exclude_flags);
    (void)named_bool(info, "count_deletions", &count_deletions); (void)named_bool(info, "count_ref_skips", &count_ref_skips);
    (void)named_string(info, "region", region); (void)named_string(info, "index_path", idx);
    BamFilterMsg m;
    const char *bad = bam_filter_check(m, "bam_bedcov", 0, min_mapq, 0, include_flags, require_flags, exclude_flags, false, false);
    if (bad) { set_error(info, bad); delete b; return; }
    b->P.min_mapq = (int32_t)min_mapq; b->P.include_flags = (int32_t)include_flags; b->P.require_flags = (int32_t)require_flags; b->P.exclude_flags = (int32_t)exclude_flags;
    b->P.count_deletions = count_deletions ? 1 : 0; b->P.count_ref_skips = count_ref_skips ? 1 : 0;
    std::string err;
    if (!bam_bind_file(&b->bam, "bam_bedcov", file_path, region, idx, err) || !bam_region_prepare(&b->bam, b->index_bytes, b->seg_beg, b->seg_end, b->seg_count, err)) { set_error(info, err.c_str()); delete b; return; }
    if (!file_exists(b->bed)) { err = "read_bed: failed to open file: " + b->bed; set_error(info, err.c_str()); delete b; return; }      // (read_bed's bind error)
    add_columns(info, kBedcovCols, kBedcovTypes, DHTS_BEDCOV_COL_COUNT);
    API(void, duckdb_bind_set_bind_data, duckdb_bind_info, void *, duckdb_delete_callback_t)(info, b, destroy_bedcov_bind);
}
static void bam_bedcov_init(duckdb_init_info info) {
    BedcovBind *bind = (BedcovBind *)API(void *, duckdb_init_get_bind_data, duckdb_init_info)(info);
    auto init_error = API(void, duckdb_init_set_error, duckdb_init_info, const char *);
    BedcovScanState *g = new BedcovScanState();
    std::string msg;
    g->ctx = create_ctx("bam_bedcov", msg);
    if (!g->ctx) { init_error(info, msg.c_str()); delete g; return; }
    g->bed = create_ctx("bam_bedcov", msg);
    if (!g->bed) { init_error(info, msg.c_str()); delete g; return; }
    dhts_ctx *c = g->ctx;
    const std::string &path = bind->bam.path;
    int rc = bind->seg_count >= 0 ? dhts_open_path_segments(c, path.c_str(), bind->bam.header_bytes, bind->seg_beg.data(), bind->seg_end.data(), bind->seg_count) : dhts_open_path(c, path.c_str());
    if (rc == 0 && (dhts_bgzf_index(c) <= 0 || dhts_bam_open(c) != 0)) rc = -1;
    if (rc != 0) { msg = std::string("Failed to open SAM/BAM/CRAM file: ") + path; init_error(info, msg.c_str()); delete g; return; }   // (as read_bam's producer)
    // the BED side, opened as read_bed opens it
    if (dhts_open_path(g->bed, bind->bed.c_str()) != 0) { init_error(info, "read_bed: failed to open file during init"); delete g; return; }
    (void)dhts_bgzf_index(g->bed);                              // (text that is not BGZF fails here and is taken as text by dhts_bed_open)
    if (dhts_bed_open(g->bed) != 0) { init_error(info, "read_bed: failed to open file during init"); delete g; return; }
    if (!bind->bam.region.empty()) {
        rc = dhts_bam_set_regions(c, bind->bam.region.c_str());
        if (rc == 0 && !bind->index_bytes.empty()) rc = dhts_bam_load_index(c, bind->index_bytes.data(), bind->index_bytes.size());
    }
    if (rc == 0) rc = dhts_bam_bedcov_open(c, g->bed, &bind->P);
    if (rc == 0 && dhts_bam_bedcov_scan(c, env_batch_blocks(0)) < 0) {
        // a stream that ends on an error ends the scan silently, its rows counted (bam_reader.c:754-766); a call that failed is the error
        dhts_bedcov_stats st;
        if (dhts_bam_bedcov_stats(c, &st) != 0 || st.status == 0) rc = -1;
    }
    if (rc != 0) { msg = dhts_error(c); init_error(info, msg.c_str()); delete g; return; }
    map_projection(info, DHTS_BEDCOV_COL_COUNT, g->pj);
    for (size_t ci = 0; ci < g->pj.slot.size(); ci++) {                     // all eight columns are read back: a slot is the column's own id
        const idx_t id = g->pj.column_ids[ci];
        if (g->pj.slot[ci] >= 0) g->pj.slot[ci] = (int)id;
        g->cb.kind.push_back(g->pj.slot[ci] < 0 ? COL_NULL : id >= DHTS_BEDCOV_BASES_COVERED ? COL_FIXED8_NOT_NULL : kind_of_type(kBedcovTypes[id]));
    }
    g->cb.host.resize(DHTS_BEDCOV_COL_COUNT);
    API(void, duckdb_init_set_max_threads, duckdb_init_info, idx_t)(info, 1);
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, g, destroy_bedcov_scan);
}
// the next rows of the BED with their results, read back; false at the end (or on a failure: err set)
static bool bedcov_next(BedcovScanState *g, std::string &err) {
    ColBatch &cb = g->cb;
    while (cb.status == 0) {
        dhts_bedcov_batch b;
        if (dhts_bam_bedcov_next(g->ctx, g->bed, 0, &b) != 0) { err = dhts_error(g->ctx); return false; }
        cb.status = b.status;
        if (b.n_rows == 0) continue;
        if (!g->arena.reserve(dhts_bam_bedcov_batch_host_bytes(&b))) { err = "bam_bedcov: out of pinned host memory"; return false; }
        if (dhts_bam_bedcov_batch_fetch(g->ctx, &b, g->arena.p, g->arena.cap, cb.host.data()) != 0) { err = dhts_error(g->ctx); return false; }
        cb.n = b.n_rows; cb.pos = 0;
        return true;
    }
    return false;
}
static void bam_bedcov_function(duckdb_function_info info, duckdb_data_chunk output) {
    BedcovScanState *g = (BedcovScanState *)API(void *, duckdb_function_get_init_data, duckdb_function_info)(info);
    if (!g) { API(void, duckdb_data_chunk_set_size, duckdb_data_chunk, idx_t)(output, 0); return; }
    scan_chunks(info, output, g->pj, g->cb, nullptr, [&](std::string &err) { return bedcov_next(g, err); });
}
extern "C" __attribute__((visibility("default"))) void register_bam_bedcov_function(duckdb_connection connection) {
    register_table_function(connection, "bam_bedcov", {{"bed_path", DUCKDB_TYPE_VARCHAR}, {"min_mapq", DUCKDB_TYPE_BIGINT}, {"include_flags", DUCKDB_TYPE_BIGINT}, {"require_flags", DUCKDB_TYPE_BIGINT},
                            {"exclude_flags", DUCKDB_TYPE_BIGINT}, {"count_deletions", DUCKDB_TYPE_BOOLEAN}, {"count_ref_skips", DUCKDB_TYPE_BOOLEAN}, {"region", DUCKDB_TYPE_VARCHAR}, {"index_path", DUCKDB_TYPE_VARCHAR}},
                            bam_bedcov_bind, bam_bedcov_init, nullptr, bam_bedcov_function, true);
}
