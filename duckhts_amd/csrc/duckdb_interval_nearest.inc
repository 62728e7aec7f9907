// duckdb_interval_nearest.inc -- part of duckdb_ext.cpp (included there behind duckdb_interval_algebra.inc; not a translation unit of its own): the
// table function interval_nearest(path, right_path, k, max_distance, ties) (the contract: include/duckhts_amd.h, "interval nearest").  bind checks
// the parameters, then that the files exist (read_bed's bind error); init opens and loads both files with ivl_open_file, opens the result and maps
// the projection; the scan takes it page by page (DHTS_INTERVAL_PAGE_ROWS) into the scan state of interval_overlap and hands it out with scan_chunks.
static const char *const kIvlNearestCols[DHTS_IVL_NEAR_COL_COUNT] = {"chrom", "start", "end", "left_row", "right_start", "right_end", "right_row", "overlap", "distance"};
static const int32_t kIvlNearestTypes[DHTS_IVL_NEAR_COL_COUNT] = {DHTS_T_VARCHAR, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_BIGINT};
struct IvlNearBind { std::string path, right; int64_t k = 1, max_distance = -1; int32_t ties = DHTS_IVL_TIES_ALL; };
struct IvlNearScanState : IvlScanState { IvlNearBind *nbind = nullptr; };
static void destroy_ivl_near_bind(void *p) { delete (IvlNearBind *)p; }
static void destroy_ivl_near_scan(void *p) { delete (IvlNearScanState *)p; }

static void interval_nearest_bind(duckdb_bind_info info) {
    auto set_error = API(void, duckdb_bind_set_error, duckdb_bind_info, const char *);
    IvlNearBind *b = new IvlNearBind();
    if (!take_path(info, b->path)) { set_error(info, "interval_nearest requires a file path"); delete b; return; }
    if (!named_string(info, "right_path", b->right) || b->right.empty()) { set_error(info, "interval_nearest requires right_path"); delete b; return; }
    (void)named_int(info, "k", &b->k);
    if (b->k < 1 || b->k > DHTS_IVL_MAX_K) { set_error(info, "interval_nearest: k must be between 1 and 1048576"); delete b; return; }
    int64_t md = 0;
    if (named_int(info, "max_distance", &md)) {                                // (NULL or unset: none)
        if (md < 0) { set_error(info, "interval_nearest: max_distance must not be negative"); delete b; return; }
        b->max_distance = md;
    }
    std::string ties = "all";
    (void)named_string(info, "ties", ties);
    if (ties == "all") b->ties = DHTS_IVL_TIES_ALL; else if (ties == "first") b->ties = DHTS_IVL_TIES_FIRST;
    else { set_error(info, "interval_nearest: ties must be 'all' or 'first'"); delete b; return; }
    for (const std::string *p : {&b->path, &b->right})
        if (!file_exists(*p)) { const std::string err = "read_bed: failed to open file: " + *p; set_error(info, err.c_str()); delete b; return; }
    add_columns(info, kIvlNearestCols, kIvlNearestTypes, DHTS_IVL_NEAR_COL_COUNT);
    API(void, duckdb_bind_set_bind_data, duckdb_bind_info, void *, duckdb_delete_callback_t)(info, b, destroy_ivl_near_bind);
}
static void interval_nearest_init(duckdb_init_info info) {
    IvlNearBind *bind = (IvlNearBind *)API(void *, duckdb_init_get_bind_data, duckdb_init_info)(info);
    auto init_error = API(void, duckdb_init_set_error, duckdb_init_info, const char *);
    IvlNearScanState *g = new IvlNearScanState();
    g->nbind = bind;
    std::string msg;
    g->ctx = ivl_open_file("interval_nearest", bind->path, msg);
    if (g->ctx) g->right = ivl_open_file("interval_nearest", bind->right, msg);
    if (!g->ctx || !g->right) { init_error(info, msg.c_str()); delete g; return; }
    if (dhts_ivl_nearest_open(g->ctx, g->right, bind->k, bind->max_distance, bind->ties) != 0) { msg = dhts_error(g->ctx); init_error(info, msg.c_str()); delete g; return; }
    const int64_t env_rows = getenv("DHTS_INTERVAL_PAGE_ROWS") ? atoll(getenv("DHTS_INTERVAL_PAGE_ROWS")) : 0;
    g->page_rows = env_rows > 0 ? env_rows : 0;
    map_projection(info, (idx_t)DHTS_IVL_NEAR_COL_COUNT, g->pj);
    for (size_t ci = 0; ci < g->pj.slot.size(); ci++) {                     // a slot is the column's own id; the projected ones make the mask
        const idx_t id = g->pj.column_ids[ci];
        if (g->pj.slot[ci] >= 0) { g->pj.slot[ci] = (int)id; g->colmask |= 1u << id; }
        g->cb.kind.push_back(g->pj.slot[ci] < 0 ? COL_NULL : id == 0 ? COL_DICT32 : COL_FIXED8_NOT_NULL);
    }
    g->cb.host.resize(DHTS_IVL_NEAR_COL_COUNT);
    g->name_off.push_back(0);
    for (int32_t id = 0;; id++) {
        uint64_t len = 0; const char *nm = dhts_ivl_chrom_name(g->ctx, id, &len);
        if (!nm) break;
        g->name_bytes.append(nm, (size_t)len); g->name_off.push_back((uint32_t)g->name_bytes.size());
    }
    API(void, duckdb_init_set_max_threads, duckdb_init_info, idx_t)(info, 1);
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, g, destroy_ivl_near_scan);
}
// the next page of the result, read back; false at the end (or on a failure: err set)
static bool interval_nearest_next(IvlNearScanState *g, std::string &err) {
    ColBatch &cb = g->cb;
    while (cb.status == 0) {
        dhts_ivl_batch b;
        if (dhts_ivl_nearest_next(g->ctx, g->page_rows, g->colmask, &b) != 0) { err = dhts_error(g->ctx); return false; }
        cb.status = b.status;
        if (b.n_rows == 0) continue;
        if (!g->arena.reserve(dhts_ivl_batch_host_bytes(&b) + 8)) { err = "interval_nearest: out of pinned host memory"; return false; }
        if (dhts_ivl_batch_fetch(g->ctx, &b, g->arena.p, g->arena.cap, cb.host.data()) != 0) { err = dhts_error(g->ctx); return false; }
        dhts_col &hc = cb.host[0];
        hc.off = g->name_off.data(); hc.bytes = (const uint8_t *)g->name_bytes.data(); hc.nbytes = g->name_bytes.size();
        cb.n = b.n_rows; cb.pos = 0;
        return true;
    }
    return false;
}
static void interval_nearest_function(duckdb_function_info info, duckdb_data_chunk output) {
    IvlNearScanState *g = (IvlNearScanState *)API(void *, duckdb_function_get_init_data, duckdb_function_info)(info);
    if (!g) { API(void, duckdb_data_chunk_set_size, duckdb_data_chunk, idx_t)(output, 0); return; }
    scan_chunks(info, output, g->pj, g->cb, nullptr, [&](std::string &err) { return interval_nearest_next(g, err); });
}
extern "C" __attribute__((visibility("default"))) void register_interval_nearest_function(duckdb_connection connection) {
    register_table_function(connection, "interval_nearest", {{"right_path", DUCKDB_TYPE_VARCHAR}, {"k", DUCKDB_TYPE_BIGINT}, {"max_distance", DUCKDB_TYPE_BIGINT}, {"ties", DUCKDB_TYPE_VARCHAR}},
                            interval_nearest_bind, interval_nearest_init, nullptr, interval_nearest_function, true);
}
