// duckdb_tabix.inc -- part of duckdb_ext.cpp (included there; not a translation unit of its own): the read_tabix, read_gtf and read_gff table functions.
// ---- read_tabix / read_gtf / read_gff (src/tabix_reader.c): one thread, file order, vector_size rows per chunk ------------------------------
// Generic bind is the reference's peek at the file (:636-771) on the device: dhts_tabix_sniff + dhts_tabix_resolve_schema, with the meta
// character and line_skip of the index when there is one; GTF / GFF have their fixed schema.  Init stages the file -- for a single region
// only its index windows -- and the scan chains the regions of region := 'a,b' (tabix_advance_region_iterator :346-360).
static const char *const kTabixFn[3] = {"read_tabix", "read_gtf", "read_gff"};
static const char *const kGxfCols[9] = {"seqname", "source", "feature", "start", "end", "score", "strand", "frame", "attributes"};
static const int32_t kGxfTypes[9] = {DHTS_T_VARCHAR, DHTS_T_VARCHAR, DHTS_T_VARCHAR, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_DOUBLE, DHTS_T_VARCHAR, DHTS_T_VARCHAR, DHTS_T_VARCHAR};
struct TabixBind {
    int mode = DHTS_TABIX_GENERIC; std::string path, index_path, index; bool has_index = false, attr_map = false;
    std::vector<std::string> regions;
    int32_t meta = '#', skip = 0, n_cols = 9; std::vector<int32_t> types; bool skip_header = false;
};
struct TabixScanState {
    dhts_ctx *ctx = nullptr; PinnedArena arena; Projection pj; ColBatch cb; dhts_tabix_map hmap;
    size_t next_region = 0;
    ~TabixScanState() { if (ctx) dhts_destroy(ctx); }
};
static void destroy_tabix_bind(void *p) { delete (TabixBind *)p; }
static void destroy_tabix_scan(void *p) { delete (TabixScanState *)p; }
// parse_regions :301-344
static std::vector<std::string> tabix_split_regions(const std::string &s) {
    std::vector<std::string> out; size_t b = 0;
    while (b <= s.size()) {
        size_t e = s.find(',', b); if (e == std::string::npos) e = s.size();
        size_t s0 = b, s1 = e;
        while (s0 < s1 && (s[s0] == ' ' || s[s0] == '\t')) s0++;
        while (s1 > s0 && (s[s1 - 1] == ' ' || s[s1 - 1] == '\t')) s1--;
        if (s1 > s0) out.push_back(s.substr(s0, s1 - s0));
        b = e + 1;
    }
    return out;
}
// a LIST(VARCHAR) named parameter.  The two getters are touched only when the parameter is present and not NULL.
static bool get_named_list(duckdb_bind_info info, const char *name, std::vector<std::string> &out) {
    duckdb_value v = named_value(info, name);
    if (!v) return false;
    const idx_t n = API(idx_t, duckdb_get_list_size, duckdb_value)(v);
    for (idx_t i = 0; i < n; i++) {
        duckdb_value e = API(duckdb_value, duckdb_get_list_child, duckdb_value, idx_t)(v, i);
        char *t = API(char *, duckdb_get_varchar, duckdb_value)(e);
        out.push_back(t ? t : ""); if (t) API(void, duckdb_free, void *)(t);
        API(void, duckdb_destroy_value, duckdb_value *)(&e);
    }
    API(void, duckdb_destroy_value, duckdb_value *)(&v);
    return n > 0;
}
// the first 100 data rows under the provisional all-VARCHAR schema, for auto_detect (:713-743)
static bool tabix_first_rows(dhts_ctx *c, int32_t n_cols, std::vector<std::string> &text, std::vector<char> &have, int32_t &n_rows) {
    n_rows = 0;
    std::vector<dhts_col> host((size_t)n_cols); std::vector<uint8_t> arena;
    for (int32_t st = 0; st == 0 && n_rows < 100;) {
        dhts_tabix_batch b;
        if (dhts_tabix_next_batch(c, 64, &b) != 0) return false;
        st = b.status;
        if (b.n_rows == 0) continue;
        arena.resize(dhts_tabix_batch_host_bytes(&b) + 8);
        if (dhts_tabix_batch_fetch(c, &b, arena.data(), arena.size(), host.data(), nullptr) != 0) return false;
        for (int64_t r = 0; r < b.n_rows && n_rows < 100; r++, n_rows++) for (int32_t k = 0; k < n_cols; k++) {
            const dhts_col &h = host[(size_t)k];
            have.push_back(h.valid[r] ? 1 : 0);
            text.push_back(h.valid[r] ? std::string((const char *)h.bytes + h.off[r], h.off[r + 1] - h.off[r]) : std::string());
        }
    }
    return dhts_tabix_set_region(c, nullptr) == 0;                             // rewinds
}
static void tabix_bind(duckdb_bind_info info, int mode) {
    auto set_error = API(void, duckdb_bind_set_error, duckdb_bind_info, const char *);
    std::string file_path, region;
    if (!take_path(info, file_path)) { const std::string m = std::string(kTabixFn[mode]) + " requires a file path"; set_error(info, m.c_str()); return; }   // :520-527
    TabixBind *b = new TabixBind();
    b->mode = mode; b->path = file_path;
    if (named_string(info, "region", region)) b->regions = tabix_split_regions(region);
    (void)named_string(info, "index_path", b->index_path);
    // tbx_index_load2: index_path, else <path>.tbi, else <path>.csi; a file without a readable index is scanned without one
    b->has_index = load_tabix_index(b->path, b->index_path, b->index);
    if (mode != DHTS_TABIX_GENERIC) {                                          // :555-587
        b->attr_map = named_flag(info, "attributes_map");
        b->n_cols = 9; b->types.assign(kGxfTypes, kGxfTypes + 9);
        add_columns(info, kGxfCols, kGxfTypes, 9);
        if (b->attr_map) add_map_column(info, "attributes_map");
    } else {
        const bool header = named_flag(info, "header"), auto_detect = named_flag(info, "auto_detect");
        std::vector<std::string> hn, ct;
        const bool have_hn = get_named_list(info, "header_names", hn), have_ct = get_named_list(info, "column_types", ct);
        if (!file_exists(b->path)) { set_error(info, "Cannot open file"); delete b; return; }               // :636-641
        std::string no_device;
        dhts_ctx *c = create_ctx("read_tabix", no_device);
        if (!c) { set_error(info, no_device.c_str()); delete b; return; }
        auto bail = [&](const char *msg) { const std::string m = msg; set_error(info, m.c_str()); dhts_destroy(c); delete b; };
        if (dhts_open_path(c, b->path.c_str()) != 0) { bail("Cannot open file"); return; }
        (void)dhts_bgzf_index(c);
        if (dhts_tabix_open(c, DHTS_TABIX_GENERIC) != 0) { bail("Cannot open file"); return; }
        if (b->has_index) {                                                    // :649-656
            int32_t m = 0, sk = 0;
            if (dhts_tabix_index_conf(c, b->index.data(), b->index.size(), &m, &sk) == 0) { b->meta = m ? m : '#'; b->skip = sk; } else b->has_index = false;
        }
        if (dhts_tabix_set_conf(c, b->meta, b->skip) != 0) { bail(dhts_error(c)); return; }
        dhts_tabix_sniffed sn;
        if (dhts_tabix_sniff(c, header, have_hn, &sn) != 0) { bail(dhts_error(c)); return; }
        std::vector<const char *> hn_p, ct_p;
        for (auto &x : hn) hn_p.push_back(x.c_str());
        for (auto &x : ct) ct_p.push_back(x.c_str());
        dhts_tabix_schema *sch = new dhts_tabix_schema();
        char emsg[256];
        int rc = dhts_tabix_resolve_schema(&sn, header, have_hn ? hn_p.data() : nullptr, (int32_t)hn_p.size(), have_ct ? ct_p.data() : nullptr, (int32_t)ct_p.size(), auto_detect,
                                           nullptr, nullptr, 0, sch, emsg, sizeof(emsg));
        if (rc == 1) {
            std::vector<std::string> text; std::vector<char> have; int32_t n_rows = 0;
            if (dhts_tabix_set_schema(c, sch->n_cols, sch->types, sch->skip_header_line) != 0 || !tabix_first_rows(c, sch->n_cols, text, have, n_rows)) { delete sch; bail(dhts_error(c)); return; }
            std::vector<const char *> cells(text.size() + 1, nullptr); std::vector<uint32_t> lens(text.size() + 1, 0);
            for (size_t i = 0; i < text.size(); i++) if (have[i]) { cells[i] = text[i].data(); lens[i] = (uint32_t)text[i].size(); }
            rc = dhts_tabix_resolve_schema(&sn, header, have_hn ? hn_p.data() : nullptr, (int32_t)hn_p.size(), nullptr, 0, auto_detect, cells.data(), lens.data(), n_rows, sch, emsg, sizeof(emsg));
        }
        if (rc < 0) { delete sch; bail(emsg); return; }                        // "column_types length does not match detected column count" :698-702
        b->n_cols = sch->n_cols; b->types.assign(sch->types, sch->types + sch->n_cols); b->skip_header = sch->skip_header_line != 0;
        add_columns(info, sch->names, sch->types, (idx_t)sch->n_cols);
        delete sch;
        dhts_destroy(c);
    }
    API(void, duckdb_bind_set_bind_data, duckdb_bind_info, void *, duckdb_delete_callback_t)(info, b, destroy_tabix_bind);
}
static void tabix_read_bind(duckdb_bind_info info) { tabix_bind(info, DHTS_TABIX_GENERIC); }
static void gtf_read_bind(duckdb_bind_info info) { tabix_bind(info, DHTS_TABIX_GTF); }
static void gff_read_bind(duckdb_bind_info info) { tabix_bind(info, DHTS_TABIX_GFF); }
// the next region the index resolves becomes the scan (tabix_advance_region_iterator): 1 positioned, 0 none left, -1 error (err set)
static int tabix_advance(const TabixBind *bind, TabixScanState *g, std::string &err) {
    while (g->next_region < bind->regions.size()) {
        const std::string &r = bind->regions[g->next_region++];
        if (dhts_tabix_set_region(g->ctx, r.c_str()) != 0) { err = dhts_error(g->ctx); return -1; }
        const int rc = dhts_tabix_load_index(g->ctx, bind->index.data(), bind->index.size());
        if (rc < 0) { err = dhts_error(g->ctx); return -1; }
        if (rc == 0) { g->cb.status = 0; return 1; }
    }
    return 0;
}
static void tabix_read_init(duckdb_init_info info) {
    TabixBind *bind = (TabixBind *)API(void *, duckdb_init_get_bind_data, duckdb_init_info)(info);
    auto init_error = API(void, duckdb_init_set_error, duckdb_init_info, const char *);
    char msg[768];
    if (!file_exists(bind->path)) { snprintf(msg, sizeof(msg), "Cannot open file: %s", bind->path.c_str()); init_error(info, msg); return; }                                  // :794-801
    if (!bind->regions.empty() && !bind->has_index) { snprintf(msg, sizeof(msg), "Region query requested but no tabix index found for: %s", bind->path.c_str()); init_error(info, msg); return; }   // :806-816
    TabixScanState *g = new TabixScanState();
    memset(&g->hmap, 0, sizeof(g->hmap));
    std::string no_device;
    g->ctx = create_ctx(kTabixFn[bind->mode], no_device);
    if (!g->ctx) { init_error(info, no_device.c_str()); delete g; return; }
    auto bail = [&](const char *m) { const std::string t = m; init_error(info, t.c_str()); delete g; };
    snprintf(msg, sizeof(msg), "Cannot open file: %s", bind->path.c_str());
    bool staged = false;
    if (bind->regions.size() == 1 && file_is_bgzf(bind->path)) {
        // one region of a BGZF file: nothing but its index windows is staged
        int rc;
        const int st = stage_region_windows(g->ctx, bind->path, dhts_tabix_region_segments, bind->regions[0], bind->index, 1, &rc);
        if (rc < 0) { bail(dhts_error(g->ctx)); return; }
        if (st == WINDOWS_OPEN_FAILED) { bail(msg); return; }
        staged = st == WINDOWS_STAGED;
    }
    if (!staged && dhts_open_path(g->ctx, bind->path.c_str()) != 0) { bail(msg); return; }
    (void)dhts_bgzf_index(g->ctx);                               // (text that is not BGZF fails here and is taken as text by dhts_tabix_open)
    if (dhts_tabix_open(g->ctx, bind->mode) != 0) { bail(msg); return; }
    if (bind->mode == DHTS_TABIX_GENERIC) {
        if (dhts_tabix_set_conf(g->ctx, bind->meta, bind->skip) != 0 || dhts_tabix_set_schema(g->ctx, bind->n_cols, bind->types.data(), bind->skip_header ? 1 : 0) != 0) { bail(dhts_error(g->ctx)); return; }
    }
    map_projection(info, bind->mode == DHTS_TABIX_GENERIC ? (idx_t)bind->n_cols : (idx_t)(bind->attr_map ? 10 : 9), g->pj);
    for (size_t ci = 0; ci < g->pj.slot.size(); ci++) {
        const idx_t id = g->pj.column_ids[ci];                                 // (the id behind the schema's columns is attributes_map)
        g->cb.kind.push_back(g->pj.slot[ci] < 0 ? COL_NULL : id < (idx_t)bind->n_cols ? kind_of_type(bind->types[id]) : COL_MAP);
    }
    if (dhts_tabix_set_projection(g->ctx, g->pj.proj.data(), (int32_t)g->pj.proj.size()) != 0) { bail(dhts_error(g->ctx)); return; }
    if (!bind->regions.empty()) {
        std::string err;
        const int rc = tabix_advance(bind, g, err);
        if (rc < 0) { bail(err.c_str()); return; }
        if (rc == 0) g->cb.done = true;                             // no region matches a sequence of the index: an empty result (:821-824)
    }
    g->cb.init(g->pj);
    API(void, duckdb_init_set_max_threads, duckdb_init_info, idx_t)(info, 1);
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, g, destroy_tabix_scan);
}
// the next device batch, read back; false at the end of the scan or on a failure (err set)
static bool tabix_next(const TabixBind *bind, TabixScanState *g, std::string &err) {
    ColBatch &cb = g->cb;
    for (;;) {
        while (cb.status == 0) {
            dhts_tabix_batch b;
            if (dhts_tabix_next_batch(g->ctx, 0, &b) != 0) { err = dhts_error(g->ctx); return false; }
            cb.status = b.status;
            if (b.n_rows == 0) continue;
            if (!g->arena.reserve(dhts_tabix_batch_host_bytes(&b))) { err = "read_tabix: out of pinned host memory"; return false; }
            if (dhts_tabix_batch_fetch(g->ctx, &b, g->arena.p, g->arena.cap, cb.host.data(), &g->hmap) != 0) { err = dhts_error(g->ctx); return false; }
            cb.n = b.n_rows; cb.pos = 0;
            return true;
        }
        if (bind->regions.empty() || cb.status < 0) return false;
        const int rc = tabix_advance(bind, g, err);                            // the iterator is exhausted: the next region (:888-894)
        if (rc <= 0) return false;
    }
}
static void tabix_read_function(duckdb_function_info info, duckdb_data_chunk output) {
    TabixScanState *g = (TabixScanState *)API(void *, duckdb_function_get_init_data, duckdb_function_info)(info);
    const TabixBind *bind = (const TabixBind *)API(void *, duckdb_function_get_bind_data, duckdb_function_info)(info);
    if (!g) { API(void, duckdb_data_chunk_set_size, duckdb_data_chunk, idx_t)(output, 0); return; }
    scan_chunks(info, output, g->pj, g->cb, &g->hmap, [&](std::string &err) { return tabix_next(bind, g, err); });
}
static void register_tabix_tf(duckdb_connection connection, const char *name, duckdb_table_function_bind_t bind) {          // create_tabix_tf :1038-1079
    register_table_function(connection, name, {{"region", DUCKDB_TYPE_VARCHAR}, {"index_path", DUCKDB_TYPE_VARCHAR}, {"attributes_map", DUCKDB_TYPE_BOOLEAN}, {"header", DUCKDB_TYPE_BOOLEAN},
                            {"header_names", PARAM_LIST_VARCHAR}, {"auto_detect", DUCKDB_TYPE_BOOLEAN}, {"column_types", PARAM_LIST_VARCHAR}}, bind, tabix_read_init, nullptr, tabix_read_function, true);
}
extern "C" __attribute__((visibility("default"))) void register_read_tabix_function(duckdb_connection connection) { register_tabix_tf(connection, "read_tabix", tabix_read_bind); }   // :1081-1085
extern "C" __attribute__((visibility("default"))) void register_read_gtf_function(duckdb_connection connection) { register_tabix_tf(connection, "read_gtf", gtf_read_bind); }
extern "C" __attribute__((visibility("default"))) void register_read_gff_function(duckdb_connection connection) { register_tabix_tf(connection, "read_gff", gff_read_bind); }
