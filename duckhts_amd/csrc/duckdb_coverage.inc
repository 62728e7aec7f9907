// duckdb_coverage.inc -- part of duckdb_ext.cpp (included there behind duckdb_bedcov.inc; not a translation unit of its own): the bam_coverage table function.
// bam_coverage(path, region, index_path, min_read_len, min_mapq, min_baseq, include_flags, require_flags, exclude_flags, min_depth): per contig or
// region what `samtools coverage` prints (the contract: include/duckhts_amd.h).  bind checks the parameters and opens the file as read_bam
// does (bam_bind_file, bam_region_prepare: the same errors); init stages the file -- for a region only the index windows -- and runs the whole
// scan on one device: no read leaves it; the scan callback pages the rows out.  The three sums of the ABI batch are not shown.
enum { COVERAGE_SHOWN = DHTS_COVERAGE_MEANMAPQ + 1 };
static const char *const kCoverageCols[COVERAGE_SHOWN] = {"chrom", "start", "end", "numreads", "covbases", "coverage", "meandepth", "meanbaseq", "meanmapq"};
static const int32_t kCoverageTypes[COVERAGE_SHOWN] = {DHTS_T_VARCHAR, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_DOUBLE, DHTS_T_DOUBLE, DHTS_T_DOUBLE, DHTS_T_DOUBLE};
struct CoverageBind {
    BamBind bam; dhts_coverage_params P;
    std::vector<uint8_t> index_bytes; std::vector<uint64_t> seg_beg, seg_end; int64_t seg_count = -1;
    ~CoverageBind() { if (bam.ctx) dhts_destroy(bam.ctx); }
};
struct CoverageScanState {
    dhts_ctx *ctx = nullptr; CoverageBind *bind = nullptr; PinnedArena arena; Projection pj; ColBatch cb; bool want_chrom = false;
    std::vector<uint32_t> chrom_off; std::string chrom_bytes;                  // the chrom column of the batch at hand: the contigs' names by id
    ~CoverageScanState() { if (ctx) dhts_destroy(ctx); }
};
static void destroy_coverage_bind(void *p) { delete (CoverageBind *)p; }
static void destroy_coverage_scan(void *p) { delete (CoverageScanState *)p; }
static void bam_coverage_bind(duckdb_bind_info info) {
    auto set_error = API(void, duckdb_bind_set_error, duckdb_bind_info, const char *);
    std::string file_path, region, idx;
    if (!take_path(info, file_path)) { set_error(info, "bam_coverage requires a file path"); return; }
    CoverageBind *b = new CoverageBind();
    int64_t min_read_len = 0, min_mapq = 0, min_baseq = 0, include_flags = 0, require_flags = 0, exclude_flags = 0x704, min_depth = 1;
    (void)named_int(info, "min_read_len", &min_read_len); (void)named_int(info, "min_mapq", &min_mapq); (void)named_int(info, "min_baseq", &min_baseq);
    (void)named_int(info, "include_flags", &include_flags); (void)named_int(info, "require_flags", &require_flags); (void)named_int(info, "exclude_flags", &exclude_flags);
    (void)named_int(info, "min_depth", &min_depth);
    (void)named_string(info, "region", region); (void)named_string(info, "index_path", idx);
    BamFilterMsg m;
    const char *bad = bam_filter_check(m, "bam_coverage", min_read_len, min_mapq, min_baseq, include_flags, require_flags, exclude_flags, true, true);
    if (!bad && min_depth < 1) bad = "bam_coverage: min_depth must be >= 1";
    if (bad) { set_error(info, bad); delete b; return; }
    memset(&b->P, 0, sizeof(b->P));
    b->P.min_read_len = min_read_len; b->P.min_depth = min_depth; b->P.min_mapq = (int32_t)min_mapq; b->P.min_baseq = (int32_t)min_baseq;
    b->P.include_flags = (int32_t)include_flags; b->P.require_flags = (int32_t)require_flags; b->P.exclude_flags = (int32_t)exclude_flags;
    std::string err;
    if (!bam_bind_file(&b->bam, "bam_coverage", file_path, region, idx, err) || !bam_region_prepare(&b->bam, b->index_bytes, b->seg_beg, b->seg_end, b->seg_count, err)) { set_error(info, err.c_str()); delete b; return; }
    add_columns(info, kCoverageCols, kCoverageTypes, COVERAGE_SHOWN);
    API(void, duckdb_bind_set_bind_data, duckdb_bind_info, void *, duckdb_delete_callback_t)(info, b, destroy_coverage_bind);
}
static void bam_coverage_init(duckdb_init_info info) {
    CoverageBind *bind = (CoverageBind *)API(void *, duckdb_init_get_bind_data, duckdb_init_info)(info);
    auto init_error = API(void, duckdb_init_set_error, duckdb_init_info, const char *);
    CoverageScanState *g = new CoverageScanState();
    g->bind = bind;
    std::string msg;
    g->ctx = create_ctx("bam_coverage", msg);
    if (!g->ctx) { init_error(info, msg.c_str()); delete g; return; }
    dhts_ctx *c = g->ctx;
    const std::string &path = bind->bam.path;
    int rc = bind->seg_count >= 0 ? dhts_open_path_segments(c, path.c_str(), bind->bam.header_bytes, bind->seg_beg.data(), bind->seg_end.data(), bind->seg_count) : dhts_open_path(c, path.c_str());
    if (rc == 0 && (dhts_bgzf_index(c) <= 0 || dhts_bam_open(c) != 0)) rc = -1;
    if (rc != 0) { msg = std::string("Failed to open SAM/BAM/CRAM file: ") + path; init_error(info, msg.c_str()); delete g; return; }   // (as read_bam's producer)
    if (!bind->bam.region.empty()) {
        rc = dhts_bam_set_regions(c, bind->bam.region.c_str());
        if (rc == 0 && !bind->index_bytes.empty()) rc = dhts_bam_load_index(c, bind->index_bytes.data(), bind->index_bytes.size());
    }
    // (the depth table is made here, not at bind: overlapping regions and a table over the cap are this call's errors)
    if (rc == 0) rc = dhts_bam_coverage_open(c, &bind->P);
    if (rc == 0 && dhts_bam_coverage_scan(c, env_batch_blocks(0)) < 0) {
        // a stream that ends on an error ends the scan silently, its rows counted (bam_reader.c:754-766); a call that failed is the error
        dhts_coverage_stats st;
        if (dhts_bam_coverage_stats(c, &st) != 0 || st.status == 0) rc = -1;
    }
    if (rc != 0) { msg = dhts_error(c); init_error(info, msg.c_str()); delete g; return; }
    map_projection(info, COVERAGE_SHOWN, g->pj);
    for (size_t ci = 0; ci < g->pj.slot.size(); ci++) {                     // every column is read back: a slot is the column's own id
        const idx_t id = g->pj.column_ids[ci];
        if (g->pj.slot[ci] >= 0) { g->pj.slot[ci] = (int)id; if (id == DHTS_COVERAGE_CHROM) g->want_chrom = true; }
        g->cb.kind.push_back(g->pj.slot[ci] < 0 ? COL_NULL : id == DHTS_COVERAGE_CHROM ? COL_STRING : COL_FIXED8_NOT_NULL);
    }
    g->cb.host.resize(DHTS_COVERAGE_COL_COUNT);
    API(void, duckdb_init_set_max_threads, duckdb_init_info, idx_t)(info, 1);
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, g, destroy_coverage_scan);
}
// the next rows of the result, read back; false at the end (or on a failure: err set)
static bool coverage_next(CoverageScanState *g, std::string &err) {
    ColBatch &cb = g->cb;
    while (cb.status == 0) {
        dhts_coverage_batch b;
        if (dhts_bam_coverage_next(g->ctx, 0, &b) != 0) { err = dhts_error(g->ctx); return false; }
        cb.status = b.status;
        if (b.n_rows == 0) continue;
        if (!g->arena.reserve(dhts_bam_coverage_batch_host_bytes(&b))) { err = "bam_coverage: out of pinned host memory"; return false; }
        if (dhts_bam_coverage_batch_fetch(g->ctx, &b, g->arena.p, g->arena.cap, cb.host.data()) != 0) { err = dhts_error(g->ctx); return false; }
        if (g->want_chrom) {
            const dhts_bam_header &h = g->bind->bam.hdr;
            dhts_col &hc = cb.host[DHTS_COVERAGE_CHROM]; const int64_t *tid = (const int64_t *)hc.fixed;
            g->chrom_off.assign((size_t)b.n_rows + 1, 0); g->chrom_bytes.clear();
            for (int64_t r = 0; r < b.n_rows; r++) { if (tid[r] >= 0 && tid[r] < h.n_ref) g->chrom_bytes += h.ref_name[tid[r]]; g->chrom_off[(size_t)r + 1] = (uint32_t)g->chrom_bytes.size(); }
            hc.off = g->chrom_off.data(); hc.bytes = (const uint8_t *)g->chrom_bytes.data(); hc.nbytes = g->chrom_bytes.size();
        }
        cb.n = b.n_rows; cb.pos = 0;
        return true;
    }
    return false;
}
static void bam_coverage_function(duckdb_function_info info, duckdb_data_chunk output) {
    CoverageScanState *g = (CoverageScanState *)API(void *, duckdb_function_get_init_data, duckdb_function_info)(info);
    if (!g) { API(void, duckdb_data_chunk_set_size, duckdb_data_chunk, idx_t)(output, 0); return; }
    scan_chunks(info, output, g->pj, g->cb, nullptr, [&](std::string &err) { return coverage_next(g, err); });
}
extern "C" __attribute__((visibility("default"))) void register_bam_coverage_function(duckdb_connection connection) {
    register_table_function(connection, "bam_coverage", {{"region", DUCKDB_TYPE_VARCHAR}, {"index_path", DUCKDB_TYPE_VARCHAR}, {"min_read_len", DUCKDB_TYPE_BIGINT}, {"min_mapq", DUCKDB_TYPE_BIGINT},
                            {"min_baseq", DUCKDB_TYPE_BIGINT}, {"include_flags", DUCKDB_TYPE_BIGINT}, {"require_flags", DUCKDB_TYPE_BIGINT}, {"exclude_flags", DUCKDB_TYPE_BIGINT}, {"min_depth", DUCKDB_TYPE_BIGINT}},
                            bam_coverage_bind, bam_coverage_init, nullptr, bam_coverage_function, true);
}
