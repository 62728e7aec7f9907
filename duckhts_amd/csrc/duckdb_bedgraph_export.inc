// duckdb_bedgraph_export.inc -- part of duckdb_ext.cpp (included there behind duckdb_depth_hist.inc; not a translation unit of its own): the
// bam_bedgraph_export table function.  bam_bedgraph_export(path, out_path, index, level, overwrite, and every named parameter of
// bam_bedgraph): the bedGraph of bam_bedgraph written as a bgzipped file with its tabix index, printed, compressed and indexed on the device (the
// contract: include/duckhts_amd.h), and one result row that says what was written.  bind refuses a missing out_path first, then checks what
// bam_bedgraph's bind checks, in its order and with this function's prefix; init stages the file, runs the scan and the export on one device;
// the scan callback hands out the row.
static const char *const kExportCols[6] = {"success", "output_path", "index_path", "n_rows", "bytes_text", "bytes_out"};
static const int32_t kExportTypes[6] = {DUCKDB_TYPE_BOOLEAN, DHTS_T_VARCHAR, DHTS_T_VARCHAR, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT};
struct ExportBind {
    BedgraphBind g; dhts_bedgraph_export_params X; std::string out_path;
};
struct ExportScanState { std::string index_path; dhts_bedgraph_export_stats st; bool emitted = false; };
static void destroy_export_bind(void *p) { delete (ExportBind *)p; }
static void destroy_export_scan(void *p) { delete (ExportScanState *)p; }
static void bam_bedgraph_export_bind(duckdb_bind_info info) {
    auto set_error = API(void, duckdb_bind_set_error, duckdb_bind_info, const char *);
    std::string file_path, region, idx, breaks, kind = "tbi";
    ExportBind *e = new ExportBind();
    BedgraphBind *b = &e->g;
    if (!named_string(info, "out_path", e->out_path) || e->out_path.empty()) { set_error(info, "bam_bedgraph_export requires out_path"); delete e; return; }
    if (!take_path(info, file_path)) { set_error(info, "bam_bedgraph_export requires a file path"); delete e; return; }
    int64_t min_read_len = 0, min_mapq = 0, min_baseq = 0, include_flags = 0, require_flags = 0, exclude_flags = 0x704, level = -1;
    bool zero_runs = false, include_deletions = false, overwrite = false;
    (void)named_int(info, "min_read_len", &min_read_len); (void)named_int(info, "min_mapq", &min_mapq); (void)named_int(info, "min_baseq", &min_baseq);
    (void)named_int(info, "include_flags", &include_flags); (void)named_int(info, "require_flags", &require_flags); (void)named_int(info, "exclude_flags", &exclude_flags);
    (void)named_bool(info, "zero_runs", &zero_runs); (void)named_bool(info, "include_deletions", &include_deletions);
    (void)named_string(info, "region", region); (void)named_string(info, "index_path", idx); (void)named_string(info, "bed_path", b->bed);
    (void)named_string(info, "index", kind); (void)named_int(info, "level", &level); (void)named_bool(info, "overwrite", &overwrite);
    const bool have_breaks = named_string(info, "breaks", breaks);
    memset(&b->P, 0, sizeof(b->P)); memset(&e->X, 0, sizeof(e->X));
    BamFilterMsg m;
    std::string msg;
    const char *bad = bam_filter_check(m, "bam_bedgraph_export", min_read_len, min_mapq, min_baseq, include_flags, require_flags, exclude_flags, true, true);
    if (!bad && have_breaks) bad = bedgraph_parse_breaks(breaks, b->P);
    if (!bad && !b->bed.empty() && !region.empty()) bad = "bam_bedgraph: a BED and regions cannot be combined (give the target rows one way)";
    if (!bad && kind != "tbi" && kind != "csi" && kind != "none") bad = "bam_bedgraph_export: index must be one of: tbi, csi, none";
    if (bad) {                                                 // (bam_bedgraph's own lines carry this function's name)
        msg = bad;
        if (msg.compare(0, 13, "bam_bedgraph:") == 0) msg = "bam_bedgraph_export:" + msg.substr(13);
        set_error(info, msg.c_str()); delete e; return;
    }
    b->P.min_read_len = min_read_len; b->P.min_mapq = (int32_t)min_mapq; b->P.min_baseq = (int32_t)min_baseq;
    b->P.include_flags = (int32_t)include_flags; b->P.require_flags = (int32_t)require_flags; b->P.exclude_flags = (int32_t)exclude_flags;
    b->P.include_deletions = include_deletions ? 1 : 0; b->P.zero_runs = zero_runs ? 1 : 0;
    e->X.level = level < -1 || level > 9 ? -1 : (int32_t)level; e->X.index = kind == "none" ? 0 : kind == "tbi" ? 1 : 2;
    e->X.min_shift = 0; e->X.overwrite = overwrite ? 1 : 0;      // (a CSI gets the default min_shift, 14)
    std::string err;
    if (!bam_bind_file(&b->bam, "bam_bedgraph_export", file_path, region, idx, err) || !bam_region_prepare(&b->bam, b->index_bytes, b->seg_beg, b->seg_end, b->seg_count, err)) { set_error(info, err.c_str()); delete e; return; }
    if (!b->bed.empty() && !file_exists(b->bed)) { err = "read_bed: failed to open file: " + b->bed; set_error(info, err.c_str()); delete e; return; }      // (read_bed's bind error)
    add_columns(info, kExportCols, kExportTypes, 6);
    API(void, duckdb_bind_set_bind_data, duckdb_bind_info, void *, duckdb_delete_callback_t)(info, e, destroy_export_bind);
}
static void bam_bedgraph_export_init(duckdb_init_info info) {
    ExportBind *e = (ExportBind *)API(void *, duckdb_init_get_bind_data, duckdb_init_info)(info);
    BedgraphBind *bind = &e->g;
    auto init_error = API(void, duckdb_init_set_error, duckdb_init_info, const char *);
    std::string msg;
    dhts_ctx *c = create_ctx("bam_bedgraph_export", msg), *bed = nullptr;
    if (!c) { init_error(info, msg.c_str()); return; }
    struct Close { dhts_ctx *&c, *&bed; ~Close() { if (bed) dhts_destroy(bed); if (c) dhts_destroy(c); } } close_both{c, bed};
    if (!bind->bed.empty()) { bed = create_ctx("bam_bedgraph_export", msg); if (!bed) { init_error(info, msg.c_str()); return; } }
    const std::string &path = bind->bam.path;
    int rc = bind->seg_count >= 0 ? dhts_open_path_segments(c, path.c_str(), bind->bam.header_bytes, bind->seg_beg.data(), bind->seg_end.data(), bind->seg_count) : dhts_open_path(c, path.c_str());
    if (rc == 0 && (dhts_bgzf_index(c) <= 0 || dhts_bam_open(c) != 0)) rc = -1;
    if (rc != 0) { msg = std::string("Failed to open SAM/BAM/CRAM file: ") + path; init_error(info, msg.c_str()); return; }   // (as read_bam's producer)
    if (bed) {                                                 // the BED side, opened as read_bed opens it
        if (dhts_open_path(bed, bind->bed.c_str()) != 0) { init_error(info, "read_bed: failed to open file during init"); return; }
        (void)dhts_bgzf_index(bed);
        if (dhts_bed_open(bed) != 0) { init_error(info, "read_bed: failed to open file during init"); return; }
    }
    if (!bind->bam.region.empty()) {
        rc = dhts_bam_set_regions(c, bind->bam.region.c_str());
        if (rc == 0 && !bind->index_bytes.empty()) rc = dhts_bam_load_index(c, bind->index_bytes.data(), bind->index_bytes.size());
    }
    if (rc == 0) rc = dhts_bam_bedgraph_open(c, &bind->P, bed);
    if (rc == 0 && dhts_bam_bedgraph_scan(c, env_batch_blocks(0)) < 0) {
        dhts_bedgraph_stats st;                                // (a stream that ends on an error has its rows counted and written; a call that failed is the error)
        if (dhts_bam_bedgraph_stats(c, &st) != 0 || st.status == 0) rc = -1;
    }
    ExportScanState *g = new ExportScanState();
    if (rc == 0) rc = dhts_bedgraph_export(c, e->out_path.c_str(), &e->X, &g->st);
    if (rc != 0) { msg = dhts_error(c); init_error(info, msg.c_str()); delete g; return; }
    if (e->X.index) g->index_path = e->out_path + (e->X.index == 1 ? ".tbi" : ".csi");
    API(void, duckdb_init_set_max_threads, duckdb_init_info, idx_t)(info, 1);
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, g, destroy_export_scan);
}
static void bam_bedgraph_export_function(duckdb_function_info info, duckdb_data_chunk output) {
    ExportScanState *g = (ExportScanState *)API(void *, duckdb_function_get_init_data, duckdb_function_info)(info);
    ExportBind *e = (ExportBind *)API(void *, duckdb_function_get_bind_data, duckdb_function_info)(info);
    auto set_size = API(void, duckdb_data_chunk_set_size, duckdb_data_chunk, idx_t);
    if (!g || !e || g->emitted) { set_size(output, 0); return; }
    auto vec = API(duckdb_vector, duckdb_data_chunk_get_vector, duckdb_data_chunk, idx_t);
    auto data = API(void *, duckdb_vector_get_data, duckdb_vector);
    auto str = API(void, duckdb_vector_assign_string_element_len, duckdb_vector, idx_t, const char *, idx_t);
    const int64_t nums[3] = {(int64_t)g->st.n_rows, (int64_t)g->st.bytes_text, (int64_t)g->st.bytes_out};
    for (idx_t ci = 0; ci < 6; ci++) {                               // (no projection pushdown: all six vectors are there)
        duckdb_vector v = vec(output, ci);
        if (ci == 0) ((bool *)data(v))[0] = true;
        else if (ci == 1) str(v, 0, e->out_path.data(), e->out_path.size());
        else if (ci == 2) { if (g->index_path.empty()) set_null(v, 0); else str(v, 0, g->index_path.data(), g->index_path.size()); }
        else ((int64_t *)data(v))[0] = nums[ci - 3];
    }
    g->emitted = true;
    set_size(output, 1);
}
extern "C" __attribute__((visibility("default"))) void register_bedgraph_export_function(duckdb_connection connection) {
    register_table_function(connection, "bam_bedgraph_export", {{"out_path", DUCKDB_TYPE_VARCHAR}, {"index", DUCKDB_TYPE_VARCHAR}, {"level", DUCKDB_TYPE_BIGINT},
                            {"overwrite", DUCKDB_TYPE_BOOLEAN}, {"zero_runs", DUCKDB_TYPE_BOOLEAN}, {"breaks", DUCKDB_TYPE_VARCHAR}, {"bed_path", DUCKDB_TYPE_VARCHAR},
                            {"region", DUCKDB_TYPE_VARCHAR}, {"index_path", DUCKDB_TYPE_VARCHAR}, {"min_read_len", DUCKDB_TYPE_BIGINT}, {"min_mapq", DUCKDB_TYPE_BIGINT}, {"min_baseq", DUCKDB_TYPE_BIGINT},
                            {"include_deletions", DUCKDB_TYPE_BOOLEAN}, {"include_flags", DUCKDB_TYPE_BIGINT}, {"require_flags", DUCKDB_TYPE_BIGINT}, {"exclude_flags", DUCKDB_TYPE_BIGINT}},
                            bam_bedgraph_export_bind, bam_bedgraph_export_init, nullptr, bam_bedgraph_export_function, false);
}
