// duckdb_depth_hist.inc -- part of duckdb_ext.cpp (included there behind duckdb_bedgraph.inc; not a translation unit of its own): the bam_depth_hist
// table function.  bam_depth_hist(path, depth_cap, per, bed_path, region, index_path, min_read_len, min_mapq, min_baseq, include_deletions,
// include_flags, require_flags, exclude_flags): chrom, start, end, depth, n_positions, n_at_least, length per group and non-empty depth bin (the
// contract: include/duckhts_amd.h) and fraction_at_least = n_at_least / length, which is computed here from the two integers.  bind checks the
// parameters in front of the file -- the filter, depth_cap, per, bed_path beside region -- opens the file as read_bam does (bam_bind_file,
// bam_region_prepare: the same errors) and looks for the BED as bam_depth does; init stages the file -- for a region only the index windows -- and
// runs the whole scan on one device: no read leaves it.  The scan callback takes the result page by page (DHTS_DEPTH_HIST_PAGE_ROWS rows, default
// the ABI's) and hands it out in chunks; only the projected columns are written on the device and fetched.
#define DEPTH_HIST_N_COLS (DHTS_DEPTH_HIST_COL_COUNT + 1)
#define DEPTH_HIST_FRACTION DHTS_DEPTH_HIST_COL_COUNT
static const char *const kDepthHistCols[DEPTH_HIST_N_COLS] = {"chrom", "start", "end", "depth", "n_positions", "n_at_least", "length", "fraction_at_least"};
static const int32_t kDepthHistTypes[DEPTH_HIST_N_COLS] = {DHTS_T_VARCHAR, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_DOUBLE};
struct DepthHistBind {
    BamBind bam; dhts_depth_hist_params P; std::string bed;
    std::vector<uint8_t> index_bytes; std::vector<uint64_t> seg_beg, seg_end; int64_t seg_count = -1;
    ~DepthHistBind() { if (bam.ctx) dhts_destroy(bam.ctx); }
};
struct DepthHistScanState {
    dhts_ctx *ctx = nullptr, *bed = nullptr; DepthHistBind *bind = nullptr; PinnedArena arena; Projection pj; ColBatch cb; uint32_t colmask = 0; int64_t page_rows = 0;
    bool fraction = false; std::vector<double> frac;                            // fraction_at_least is projected; its values of the page
    std::vector<uint32_t> name_off; std::string name_bytes;                    // the contigs' names by id: what the chrom column's ids stand for
    ~DepthHistScanState() { if (bed) dhts_destroy(bed); if (ctx) dhts_destroy(ctx); }
};
static void destroy_depth_hist_bind(void *p) { delete (DepthHistBind *)p; }
static void destroy_depth_hist_scan(void *p) { delete (DepthHistScanState *)p; }
static void bam_depth_hist_bind(duckdb_bind_info info) {
    auto set_error = API(void, duckdb_bind_set_error, duckdb_bind_info, const char *);
    std::string file_path, region, idx, per = "row";
    if (!take_path(info, file_path)) { set_error(info, "bam_depth_hist requires a file path"); return; }
    DepthHistBind *b = new DepthHistBind();
    int64_t min_read_len = 0, min_mapq = 0, min_baseq = 0, include_flags = 0, require_flags = 0, exclude_flags = 0x704, depth_cap = 1000;
    bool include_deletions = false;
    (void)named_int(info, "min_read_len", &min_read_len); (void)named_int(info, "min_mapq", &min_mapq); (void)named_int(info, "min_baseq", &min_baseq);
    (void)named_int(info, "include_flags", &include_flags); (void)named_int(info, "require_flags", &require_flags); (void)named_int(info, "exclude_flags", &exclude_flags);
    (void)named_int(info, "depth_cap", &depth_cap); (void)named_bool(info, "include_deletions", &include_deletions); (void)named_string(info, "per", per);
    (void)named_string(info, "region", region); (void)named_string(info, "index_path", idx); (void)named_string(info, "bed_path", b->bed);
    memset(&b->P, 0, sizeof(b->P));
    BamFilterMsg m;
    const char *bad = bam_filter_check(m, "bam_depth_hist", min_read_len, min_mapq, min_baseq, include_flags, require_flags, exclude_flags, true, true);
    if (!bad && (depth_cap < 1 || depth_cap > 1048575)) bad = "bam_depth_hist: depth_cap must be between 1 and 1048575";
    if (!bad && per != "row" && per != "contig") bad = "bam_depth_hist: per must be 'row' or 'contig'";
    if (!bad && !b->bed.empty() && !region.empty()) bad = "bam_depth_hist: a BED and regions cannot be combined (give the target rows one way)";
    if (bad) { set_error(info, bad); delete b; return; }
    b->P.min_read_len = min_read_len; b->P.min_mapq = (int32_t)min_mapq; b->P.min_baseq = (int32_t)min_baseq;
    b->P.include_flags = (int32_t)include_flags; b->P.require_flags = (int32_t)require_flags; b->P.exclude_flags = (int32_t)exclude_flags;
    b->P.include_deletions = include_deletions ? 1 : 0; b->P.depth_cap = (int32_t)depth_cap; b->P.per = per == "contig" ? 1 : 0;
    std::string err;
    if (!bam_bind_file(&b->bam, "bam_depth_hist", file_path, region, idx, err) || !bam_region_prepare(&b->bam, b->index_bytes, b->seg_beg, b->seg_end, b->seg_count, err)) { set_error(info, err.c_str()); delete b; return; }
    if (!b->bed.empty() && !file_exists(b->bed)) { err = "read_bed: failed to open file: " + b->bed; set_error(info, err.c_str()); delete b; return; }      // (read_bed's bind error)
    add_columns(info, kDepthHistCols, kDepthHistTypes, DEPTH_HIST_N_COLS);
    API(void, duckdb_bind_set_bind_data, duckdb_bind_info, void *, duckdb_delete_callback_t)(info, b, destroy_depth_hist_bind);
}
static void bam_depth_hist_init(duckdb_init_info info) {
    DepthHistBind *bind = (DepthHistBind *)API(void *, duckdb_init_get_bind_data, duckdb_init_info)(info);
    auto init_error = API(void, duckdb_init_set_error, duckdb_init_info, const char *);
    DepthHistScanState *g = new DepthHistScanState();
    g->bind = bind;
    std::string msg;
    g->ctx = create_ctx("bam_depth_hist", msg);
    if (!g->ctx) { init_error(info, msg.c_str()); delete g; return; }
    if (!bind->bed.empty()) { g->bed = create_ctx("bam_depth_hist", msg); if (!g->bed) { init_error(info, msg.c_str()); delete g; return; } }
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
    // (the two tables are made here, not at bind: overlapping regions and a table over its cap are this call's errors)
    if (rc == 0) rc = dhts_bam_hist_open(c, &bind->P, g->bed);
    if (rc == 0 && dhts_bam_hist_scan(c, env_batch_blocks(0)) < 0) {
        // a stream that ends on an error ends the scan silently, its rows counted (bam_reader.c:754-766); a call that failed is the error
        dhts_depth_hist_stats st;
        if (dhts_bam_hist_stats(c, &st) != 0 || st.status == 0) rc = -1;
    }
    if (rc != 0) { msg = dhts_error(c); init_error(info, msg.c_str()); delete g; return; }
    const int64_t env_rows = getenv("DHTS_DEPTH_HIST_PAGE_ROWS") ? atoll(getenv("DHTS_DEPTH_HIST_PAGE_ROWS")) : 0;
    g->page_rows = env_rows > 0 ? env_rows : 0;
    map_projection(info, DEPTH_HIST_N_COLS, g->pj);
    for (size_t ci = 0; ci < g->pj.slot.size(); ci++) {                     // a slot is the column's own id; the projected device columns make the mask
        const idx_t id = g->pj.column_ids[ci];
        if (g->pj.slot[ci] >= 0) {
            g->pj.slot[ci] = (int)id;
            if (id == DEPTH_HIST_FRACTION) { g->fraction = true; g->colmask |= (1u << DHTS_DEPTH_HIST_N_AT_LEAST) | (1u << DHTS_DEPTH_HIST_LENGTH); }      // the two integers it is made of
            else g->colmask |= 1u << id;
        }
        g->cb.kind.push_back(g->pj.slot[ci] < 0 ? COL_NULL : id == DHTS_DEPTH_HIST_CHROM ? COL_DICT32 : id == DHTS_DEPTH_HIST_DEPTH ? COL_WIDEN32 : COL_FIXED8_NOT_NULL);
    }
    g->cb.host.resize(DEPTH_HIST_N_COLS);
    const dhts_bam_header &h = bind->bam.hdr;
    g->name_off.assign((size_t)h.n_ref + 1, 0);
    for (int32_t t = 0; t < h.n_ref; t++) { g->name_bytes += h.ref_name[t]; g->name_off[(size_t)t + 1] = (uint32_t)g->name_bytes.size(); }
    API(void, duckdb_init_set_max_threads, duckdb_init_info, idx_t)(info, 1);
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, g, destroy_depth_hist_scan);
}
// the next page of the result, read back; false at the end (or on a failure: err set)
static bool depth_hist_next(DepthHistScanState *g, std::string &err) {
    ColBatch &cb = g->cb;
    while (cb.status == 0) {
        dhts_depth_hist_batch b;
        if (dhts_bam_hist_next(g->ctx, g->page_rows, g->colmask, &b) != 0) { err = dhts_error(g->ctx); return false; }
        cb.status = b.status;
        if (b.n_rows == 0) continue;
        if (!g->arena.reserve(dhts_bam_hist_batch_host_bytes(&b) + 8)) { err = "bam_depth_hist: out of pinned host memory"; return false; }
        if (dhts_bam_hist_batch_fetch(g->ctx, &b, g->arena.p, g->arena.cap, cb.host.data()) != 0) { err = dhts_error(g->ctx); return false; }
        dhts_col &hc = cb.host[DHTS_DEPTH_HIST_CHROM];
        hc.off = g->name_off.data(); hc.bytes = (const uint8_t *)g->name_bytes.data(); hc.nbytes = g->name_bytes.size();
        dhts_col &fc = cb.host[DEPTH_HIST_FRACTION];
        memset(&fc, 0, sizeof(fc)); fc.col = DEPTH_HIST_FRACTION;
        if (g->fraction) {                                                     // one IEEE division of the two integers per row (length > 0: an empty row has no group)
            const int64_t *al = (const int64_t *)cb.host[DHTS_DEPTH_HIST_N_AT_LEAST].fixed, *ln = (const int64_t *)cb.host[DHTS_DEPTH_HIST_LENGTH].fixed;
            g->frac.resize((size_t)b.n_rows);
            for (int64_t r = 0; r < b.n_rows; r++) g->frac[(size_t)r] = (double)al[r] / (double)ln[r];
            fc.fixed = g->frac.data();
        }
        cb.n = b.n_rows; cb.pos = 0;
        return true;
    }
    return false;
}
static void bam_depth_hist_function(duckdb_function_info info, duckdb_data_chunk output) {
    DepthHistScanState *g = (DepthHistScanState *)API(void *, duckdb_function_get_init_data, duckdb_function_info)(info);
    if (!g) { API(void, duckdb_data_chunk_set_size, duckdb_data_chunk, idx_t)(output, 0); return; }
    scan_chunks(info, output, g->pj, g->cb, nullptr, [&](std::string &err) { return depth_hist_next(g, err); });
}
extern "C" __attribute__((visibility("default"))) void register_bam_hist_function(duckdb_connection connection) {
    register_table_function(connection, "bam_depth_hist", {{"depth_cap", DUCKDB_TYPE_BIGINT}, {"per", DUCKDB_TYPE_VARCHAR}, {"bed_path", DUCKDB_TYPE_VARCHAR},
                            {"region", DUCKDB_TYPE_VARCHAR}, {"index_path", DUCKDB_TYPE_VARCHAR}, {"min_read_len", DUCKDB_TYPE_BIGINT}, {"min_mapq", DUCKDB_TYPE_BIGINT}, {"min_baseq", DUCKDB_TYPE_BIGINT},
                            {"include_deletions", DUCKDB_TYPE_BOOLEAN}, {"include_flags", DUCKDB_TYPE_BIGINT}, {"require_flags", DUCKDB_TYPE_BIGINT}, {"exclude_flags", DUCKDB_TYPE_BIGINT}},
                            bam_depth_hist_bind, bam_depth_hist_init, nullptr, bam_depth_hist_function, true);
}
