// duckdb_interval_algebra.inc -- part of duckdb_ext.cpp (included there behind duckdb_interval.inc; not a translation unit of its own): the table
// functions interval_merge(path, max_gap) and interval_overlap(path, right_path, mode) (the contract: include/duckhts_amd.h, "interval algebra").
// bind checks the parameters and that the files exist (read_bed's bind error); init opens the files as read_bed does, loads, sorts and indexes
// them on one device and opens the result; the scan callback takes it page by page (DHTS_INTERVAL_PAGE_ROWS rows, default the ABI's) and hands it
// out in chunks.  chrom is resolved from the name id on the host; only the projected columns are written on the device and fetched.
static const char *const kIvlMergeCols[DHTS_IVL_MERGE_COL_COUNT] = {"chrom", "start", "end", "n_merged"};
static const int32_t kIvlMergeTypes[DHTS_IVL_MERGE_COL_COUNT] = {DHTS_T_VARCHAR, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT};
static const char *const kIvlOverlapCols[DHTS_IVL_OV_COL_COUNT] = {"chrom", "start", "end", "left_row", "right_start", "right_end", "right_row", "overlap"};
static const int32_t kIvlOverlapTypes[DHTS_IVL_OV_COL_COUNT] = {DHTS_T_VARCHAR, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT};
struct IvlBind { bool overlap = false; std::string path, right; int64_t max_gap = 0; int32_t mode = DHTS_IVL_ANY; };
struct IvlScanState {
    dhts_ctx *ctx = nullptr, *right = nullptr; IvlBind *bind = nullptr; PinnedArena arena; Projection pj; ColBatch cb; uint32_t colmask = 0; int64_t page_rows = 0;
    std::vector<uint32_t> name_off; std::string name_bytes;                    // the chrom names by name id: what the chrom column's ids stand for
    ~IvlScanState() { if (right) dhts_destroy(right); if (ctx) dhts_destroy(ctx); }
};
static void destroy_ivl_bind(void *p) { delete (IvlBind *)p; }
static void destroy_ivl_scan(void *p) { delete (IvlScanState *)p; }

static void interval_merge_bind(duckdb_bind_info info) {
    auto set_error = API(void, duckdb_bind_set_error, duckdb_bind_info, const char *);
    IvlBind *b = new IvlBind();
    if (!take_path(info, b->path)) { set_error(info, "interval_merge requires a file path"); delete b; return; }
    (void)named_int(info, "max_gap", &b->max_gap);
    if (b->max_gap < 0 || b->max_gap > DHTS_IVL_MAX_GAP) { set_error(info, "interval_merge: max_gap must be between 0 and 1099511627776"); delete b; return; }
    if (!file_exists(b->path)) { const std::string err = "read_bed: failed to open file: " + b->path; set_error(info, err.c_str()); delete b; return; }
    add_columns(info, kIvlMergeCols, kIvlMergeTypes, DHTS_IVL_MERGE_COL_COUNT);
    API(void, duckdb_bind_set_bind_data, duckdb_bind_info, void *, duckdb_delete_callback_t)(info, b, destroy_ivl_bind);
}
static void interval_overlap_bind(duckdb_bind_info info) {
    auto set_error = API(void, duckdb_bind_set_error, duckdb_bind_info, const char *);
    IvlBind *b = new IvlBind();
    b->overlap = true;
    if (!take_path(info, b->path)) { set_error(info, "interval_overlap requires a file path"); delete b; return; }
    if (!named_string(info, "right_path", b->right) || b->right.empty()) { set_error(info, "interval_overlap requires right_path"); delete b; return; }
    std::string mode = "any";
    (void)named_string(info, "mode", mode);
    if (mode == "any") b->mode = DHTS_IVL_ANY; else if (mode == "contain") b->mode = DHTS_IVL_CONTAIN; else if (mode == "within") b->mode = DHTS_IVL_WITHIN;
    else { set_error(info, "interval_overlap: mode must be 'any', 'contain' or 'within'"); delete b; return; }
    for (const std::string *p : {&b->path, &b->right})
        if (!file_exists(*p)) { const std::string err = "read_bed: failed to open file: " + *p; set_error(info, err.c_str()); delete b; return; }
    add_columns(info, kIvlOverlapCols, kIvlOverlapTypes, DHTS_IVL_OV_COL_COUNT);
    API(void, duckdb_bind_set_bind_data, duckdb_bind_info, void *, duckdb_delete_callback_t)(info, b, destroy_ivl_bind);
}
// a context with `path` open as read_bed opens it, loaded, sorted and indexed; nullptr with msg set
static dhts_ctx *ivl_open_file(const char *fn, const std::string &path, std::string &msg) {
    dhts_ctx *c = create_ctx(fn, msg);
    if (!c) return nullptr;
    if (dhts_open_path(c, path.c_str()) != 0) { msg = "read_bed: failed to open file during init"; dhts_destroy(c); return nullptr; }
    (void)dhts_bgzf_index(c);                                  // (text that is not BGZF fails here and is taken as text by dhts_bed_open)
    if (dhts_bed_open(c) != 0) { msg = "read_bed: failed to open file during init"; dhts_destroy(c); return nullptr; }
    if (dhts_ivl_load(c, env_batch_blocks(0)) != 0) { msg = dhts_error(c); dhts_destroy(c); return nullptr; }
    return c;
}
static void interval_init(duckdb_init_info info) {
    IvlBind *bind = (IvlBind *)API(void *, duckdb_init_get_bind_data, duckdb_init_info)(info);
    auto init_error = API(void, duckdb_init_set_error, duckdb_init_info, const char *);
    IvlScanState *g = new IvlScanState();
    g->bind = bind;
    const char *fn = bind->overlap ? "interval_overlap" : "interval_merge";
    std::string msg;
    g->ctx = ivl_open_file(fn, bind->path, msg);
    if (g->ctx && bind->overlap) g->right = ivl_open_file(fn, bind->right, msg);
    if (!g->ctx || (bind->overlap && !g->right)) { init_error(info, msg.c_str()); delete g; return; }
    if ((bind->overlap ? dhts_ivl_overlap_open(g->ctx, g->right, bind->mode) : dhts_ivl_merge_open(g->ctx, bind->max_gap)) != 0) { msg = dhts_error(g->ctx); init_error(info, msg.c_str()); delete g; return; }
    const int64_t env_rows = getenv("DHTS_INTERVAL_PAGE_ROWS") ? atoll(getenv("DHTS_INTERVAL_PAGE_ROWS")) : 0;
    g->page_rows = env_rows > 0 ? env_rows : 0;
    const idx_t ncols = bind->overlap ? (idx_t)DHTS_IVL_OV_COL_COUNT : (idx_t)DHTS_IVL_MERGE_COL_COUNT;
    map_projection(info, ncols, g->pj);
    for (size_t ci = 0; ci < g->pj.slot.size(); ci++) {                     // a slot is the column's own id; the projected ones make the mask
        const idx_t id = g->pj.column_ids[ci];
        if (g->pj.slot[ci] >= 0) { g->pj.slot[ci] = (int)id; g->colmask |= 1u << id; }
        g->cb.kind.push_back(g->pj.slot[ci] < 0 ? COL_NULL : id == 0 ? COL_DICT32 : COL_FIXED8_NOT_NULL);
    }
    g->cb.host.resize(ncols);
    g->name_off.push_back(0);
    for (int32_t id = 0;; id++) {
        uint64_t len = 0; const char *nm = dhts_ivl_chrom_name(g->ctx, id, &len);
        if (!nm) break;
        g->name_bytes.append(nm, (size_t)len); g->name_off.push_back((uint32_t)g->name_bytes.size());
    }
    API(void, duckdb_init_set_max_threads, duckdb_init_info, idx_t)(info, 1);
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, g, destroy_ivl_scan);
}
// the next page of the result, read back; false at the end (or on a failure: err set)
static bool interval_next(IvlScanState *g, std::string &err) {
    ColBatch &cb = g->cb;
    while (cb.status == 0) {
        dhts_ivl_batch b;
        if ((g->bind->overlap ? dhts_ivl_overlap_next(g->ctx, g->page_rows, g->colmask, &b) : dhts_ivl_merge_next(g->ctx, g->page_rows, g->colmask, &b)) != 0) { err = dhts_error(g->ctx); return false; }
        cb.status = b.status;
        if (b.n_rows == 0) continue;
        if (!g->arena.reserve(dhts_ivl_batch_host_bytes(&b) + 8)) { err = std::string(g->bind->overlap ? "interval_overlap" : "interval_merge") + ": out of pinned host memory"; return false; }
        if (dhts_ivl_batch_fetch(g->ctx, &b, g->arena.p, g->arena.cap, cb.host.data()) != 0) { err = dhts_error(g->ctx); return false; }
        dhts_col &hc = cb.host[0];
        hc.off = g->name_off.data(); hc.bytes = (const uint8_t *)g->name_bytes.data(); hc.nbytes = g->name_bytes.size();
        cb.n = b.n_rows; cb.pos = 0;
        return true;
    }
    return false;
}
static void interval_function(duckdb_function_info info, duckdb_data_chunk output) {
    IvlScanState *g = (IvlScanState *)API(void *, duckdb_function_get_init_data, duckdb_function_info)(info);
    if (!g) { API(void, duckdb_data_chunk_set_size, duckdb_data_chunk, idx_t)(output, 0); return; }
    scan_chunks(info, output, g->pj, g->cb, nullptr, [&](std::string &err) { return interval_next(g, err); });
}
extern "C" __attribute__((visibility("default"))) void register_interval_merge_function(duckdb_connection connection) {
    register_table_function(connection, "interval_merge", {{"max_gap", DUCKDB_TYPE_BIGINT}}, interval_merge_bind, interval_init, nullptr, interval_function, true);
}
extern "C" __attribute__((visibility("default"))) void register_interval_overlap_function(duckdb_connection connection) {
    register_table_function(connection, "interval_overlap", {{"right_path", DUCKDB_TYPE_VARCHAR}, {"mode", DUCKDB_TYPE_VARCHAR}}, interval_overlap_bind, interval_init, nullptr, interval_function, true);
}
