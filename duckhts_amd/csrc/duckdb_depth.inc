// duckdb_depth.inc -- part of duckdb_ext.cpp (included there behind duckdb_coverage.inc; not a translation unit of its own): the bam_depth table function.
// bam_depth(path, all_positions, all_reference_positions, bed_path, region, index_path, min_read_len, min_mapq, min_baseq, include_deletions,
// suppress_overlaps, include_flags, require_flags, exclude_flags): chrom, pos, depth per position, what `samtools depth` prints (the contract:
// include/duckhts_amd.h).  bind checks the parameters in front of the file, opens the file as read_bam does (bam_bind_file, bam_region_prepare:
// the same errors) and looks for the BED as bam_bedcov does; init stages the file -- for a region only the index windows -- and runs the whole
// scan on one device: no read leaves it.  The scan callback takes the result page by page (DHTS_DEPTH_PAGE_ROWS rows, default the ABI's) and
// hands it out in chunks; only the projected columns are written on the device and fetched.
static const char *const kDepthCols[DHTS_DEPTH_COL_COUNT] = {"chrom", "pos", "depth"};
static const int32_t kDepthTypes[DHTS_DEPTH_COL_COUNT] = {DHTS_T_VARCHAR, DHTS_T_BIGINT, DHTS_T_BIGINT};
#define DEPTH_NO_OVERLAPS "bam_depth: suppress_overlaps is not supported (mates are not paired on the device)"
struct DepthBind {
    BamBind bam; dhts_depth_params P; std::string bed;
    std::vector<uint8_t> index_bytes; std::vector<uint64_t> seg_beg, seg_end; int64_t seg_count = -1;
    ~DepthBind() { if (bam.ctx) dhts_destroy(bam.ctx); }
};
struct DepthScanState {
    dhts_ctx *ctx = nullptr, *bed = nullptr; DepthBind *bind = nullptr; PinnedArena arena; Projection pj; ColBatch cb; uint32_t colmask = 0; int64_t page_rows = 0;
    std::vector<uint32_t> name_off; std::string name_bytes;                    // the contigs' names by id: what the chrom column's ids stand for
    ~DepthScanState() { if (bed) dhts_destroy(bed); if (ctx) dhts_destroy(ctx); }
};
static void destroy_depth_bind(void *p) { delete (DepthBind *)p; }
static void destroy_depth_scan(void *p) { delete (DepthScanState *)p; }
static void bam_depth_bind(duckdb_bind_info info) {
    auto set_error = API(void, duckdb_bind_set_error, duckdb_bind_info, const char *);
    std::string file_path, region, idx;
    if (!take_path(info, file_path)) { set_error(info, "bam_depth requires a file path"); return; }
    DepthBind *b = new DepthBind();
    int64_t min_read_len = 0, min_mapq = 0, min_baseq = 0, include_flags = 0, require_flags = 0, exclude_flags = 0x704;
    bool all_positions = false, all_reference_positions = false, include_deletions = false, suppress_overlaps = false;
    (void)named_int(info, "min_read_len", &min_read_len); (void)named_int(info, "min_mapq", &min_mapq); (void)named_int(info, "min_baseq", &min_baseq);
    (void)named_int(info, "include_flags", &include_flags); (void)named_int(info, "require_flags", &require_flags); (void)named_int(info, "exclude_flags", &exclude_flags);
    (void)named_bool(info, "all_positions", &all_positions); (void)named_bool(info, "all_reference_positions", &all_reference_positions);
    (void)named_bool(info, "include_deletions", &include_deletions); (void)named_bool(info, "suppress_overlaps", &suppress_overlaps);
    (void)named_string(info, "region", region); (void)named_string(info, "index_path", idx); (void)named_string(info, "bed_path", b->bed);
    BamFilterMsg m;
    const char *bad = bam_filter_check(m, "bam_depth", min_read_len, min_mapq, min_baseq, include_flags, require_flags, exclude_flags, true, true);
    if (!bad && suppress_overlaps) bad = DEPTH_NO_OVERLAPS;
    if (!bad && !b->bed.empty() && !region.empty()) bad = "bam_depth: a BED and regions cannot be combined (give the target rows one way)";
    if (bad) { set_error(info, bad); delete b; return; }
    memset(&b->P, 0, sizeof(b->P));
    b->P.min_read_len = min_read_len; b->P.min_mapq = (int32_t)min_mapq; b->P.min_baseq = (int32_t)min_baseq;
    b->P.include_flags = (int32_t)include_flags; b->P.require_flags = (int32_t)require_flags; b->P.exclude_flags = (int32_t)exclude_flags;
    b->P.include_deletions = include_deletions ? 1 : 0; b->P.all_positions = all_reference_positions ? 2 : all_positions ? 1 : 0;     // (-aa wins over -a)
    std::string err;
    if (!bam_bind_file(&b->bam, "bam_depth", file_path, region, idx, err) || !bam_region_prepare(&b->bam, b->index_bytes, b->seg_beg, b->seg_end, b->seg_count, err)) { set_error(info, err.c_str()); delete b; return; }
    if (!b->bed.empty() && !file_exists(b->bed)) { err = "read_bed: failed to open file: " + b->bed; set_error(info, err.c_str()); delete b; return; }      // (read_bed's bind error)
    add_columns(info, kDepthCols, kDepthTypes, DHTS_DEPTH_COL_COUNT);
    API(void, duckdb_bind_set_bind_data, duckdb_bind_info, void *, duckdb_delete_callback_t)(info, b, destroy_depth_bind);
}
static void bam_depth_init(duckdb_init_info info) {
    DepthBind *bind = (DepthBind *)API(void *, duckdb_init_get_bind_data, duckdb_init_info)(info);
    auto init_error = API(void, duckdb_init_set_error, duckdb_init_info, const char *);
    DepthScanState *g = new DepthScanState();
    g->bind = bind;
    std::string msg;
    g->ctx = create_ctx("bam_depth", msg);
    if (!g->ctx) { init_error(info, msg.c_str()); delete g; return; }
    if (!bind->bed.empty()) { g->bed = create_ctx("bam_depth", msg); if (!g->bed) { init_error(info, msg.c_str()); delete g; return; } }
    dhts_ctx *c = g->ctx;
    const std::string &path = bind->bam.path;
    int rc = bind->seg_count >= 0 ? dhts_open_path_segments(c, path.c_str(), bind->bam.header_bytes, bind->seg_beg.data(), bind->seg_end.data(), bind->seg_count) : dhts_open_path(c, path.c_str());
    if (rc == 0 && (dhts_bgzf_index(c) <= 0 || dhts_bam_open(c) != 0)) rc = -1;
    if (rc != 0) { msg = std::string("Failed to open SAM/BAM/CRAM file: ") + path; init_error(info, msg.c_str()); delete g; return; }   // (as read_bam's producer)
    if (g->bed) {                                              // the BED side, opened as read_bed opens it
        if (dhts_open_path(g->bed, bind->bed.c_str()) != 0) { init_error(info, "read_bed: failed to open file during init"); delete g; return; }
        (void)dhts_bgzf_index(g->bed);                          // (text that is not BGZF fails here and is taken as text by dhts_bed_open)
        if (dhts_bed_open(g->bed) != 0) { init_error(info, "read_bed: failed to open file during init"); delete g; return; }
    }
    if (!bind->bam.region.empty()) {
        rc = dhts_bam_set_regions(c, bind->bam.region.c_str());
        if (rc == 0 && !bind->index_bytes.empty()) rc = dhts_bam_load_index(c, bind->index_bytes.data(), bind->index_bytes.size());
    }
    // (the depth table is made here, not at bind: overlapping regions and a table over the cap are this call's errors)
    if (rc == 0) rc = dhts_bam_depth_open(c, &bind->P, g->bed);
    if (rc == 0 && dhts_bam_depth_scan(c, env_batch_blocks(0)) < 0) {
        // a stream that ends on an error ends the scan silently, its rows counted (bam_reader.c:754-766); a call that failed is the error
        dhts_depth_stats st;
        if (dhts_bam_depth_stats(c, &st) != 0 || st.status == 0) rc = -1;
    }
    if (rc != 0) { msg = dhts_error(c); init_error(info, msg.c_str()); delete g; return; }
    const int64_t env_rows = getenv("DHTS_DEPTH_PAGE_ROWS") ? atoll(getenv("DHTS_DEPTH_PAGE_ROWS")) : 0;
    g->page_rows = env_rows > 0 ? env_rows : 0;
    map_projection(info, DHTS_DEPTH_COL_COUNT, g->pj);
    for (size_t ci = 0; ci < g->pj.slot.size(); ci++) {                     // a slot is the column's own id; the projected ones make the mask
        const idx_t id = g->pj.column_ids[ci];
        if (g->pj.slot[ci] >= 0) { g->pj.slot[ci] = (int)id; g->colmask |= 1u << id; }
        g->cb.kind.push_back(g->pj.slot[ci] < 0 ? COL_NULL : id == DHTS_DEPTH_CHROM ? COL_DICT32 : id == DHTS_DEPTH_POS ? COL_FIXED8_NOT_NULL : COL_WIDEN32);
    }
    g->cb.host.resize(DHTS_DEPTH_COL_COUNT);
    const dhts_bam_header &h = bind->bam.hdr;
    g->name_off.assign((size_t)h.n_ref + 1, 0);
    for (int32_t t = 0; t < h.n_ref; t++) { g->name_bytes += h.ref_name[t]; g->name_off[(size_t)t + 1] = (uint32_t)g->name_bytes.size(); }
    API(void, duckdb_init_set_max_threads, duckdb_init_info, idx_t)(info, 1);
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, g, destroy_depth_scan);
}
// the next page of the result, read back; false at the end (or on a failure: err set)
static bool depth_next(DepthScanState *g, std::string &err) {
    ColBatch &cb = g->cb;
    while (cb.status == 0) {
        dhts_depth_batch b;
        if (dhts_bam_depth_next(g->ctx, g->page_rows, g->colmask, &b) != 0) { err = dhts_error(g->ctx); return false; }
        cb.status = b.status;
        if (b.n_rows == 0) continue;
        if (!g->arena.reserve(dhts_bam_depth_batch_host_bytes(&b) + 8)) { err = "bam_depth: out of pinned host memory"; return false; }
        if (dhts_bam_depth_batch_fetch(g->ctx, &b, g->arena.p, g->arena.cap, cb.host.data()) != 0) { err = dhts_error(g->ctx); return false; }
        dhts_col &hc = cb.host[DHTS_DEPTH_CHROM];
        hc.off = g->name_off.data(); hc.bytes = (const uint8_t *)g->name_bytes.data(); hc.nbytes = g->name_bytes.size();
        cb.n = b.n_rows; cb.pos = 0;
        return true;
    }
    return false;
}
static void bam_depth_function(duckdb_function_info info, duckdb_data_chunk output) {
    DepthScanState *g = (DepthScanState *)API(void *, duckdb_function_get_init_data, duckdb_function_info)(info);
    if (!g) { API(void, duckdb_data_chunk_set_size, duckdb_data_chunk, idx_t)(output, 0); return; }
    scan_chunks(info, output, g->pj, g->cb, nullptr, [&](std::string &err) { return depth_next(g, err); });
}
extern "C" __attribute__((visibility("default"))) void register_bam_depth_function(duckdb_connection connection) {
    register_table_function(connection, "bam_depth", {{"all_positions", DUCKDB_TYPE_BOOLEAN}, {"all_reference_positions", DUCKDB_TYPE_BOOLEAN}, {"bed_path", DUCKDB_TYPE_VARCHAR},
                            {"region", DUCKDB_TYPE_VARCHAR}, {"index_path", DUCKDB_TYPE_VARCHAR}, {"min_read_len", DUCKDB_TYPE_BIGINT}, {"min_mapq", DUCKDB_TYPE_BIGINT}, {"min_baseq", DUCKDB_TYPE_BIGINT},
                            {"include_deletions", DUCKDB_TYPE_BOOLEAN}, {"suppress_overlaps", DUCKDB_TYPE_BOOLEAN}, {"include_flags", DUCKDB_TYPE_BIGINT}, {"require_flags", DUCKDB_TYPE_BIGINT},
                            {"exclude_flags", DUCKDB_TYPE_BIGINT}},
                            bam_depth_bind, bam_depth_init, nullptr, bam_depth_function, true);
}
