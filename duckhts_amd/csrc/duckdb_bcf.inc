// duckdb_bcf.inc -- part of duckdb_ext.cpp (included there; not a translation unit of its own): the read_bcf table function.
// =====================================================================================================================
// read_bcf -- mirrors register_read_bcf_function src/bcf_reader.c:2055-2080, bcf_read_bind 452-880 (schema 540-760),
// global/local init 886-1150 (projection ids, region error), bcf_read_function 1155-2049 (<= vector_size rows per call).
// Sequential mode; tidy_format and region supported; BCF, and VCF text (plain or bgzipped) through the device text encoder.
// =====================================================================================================================
struct BcfBind {
    std::string path, region;
    std::vector<std::string> regions;    // comma split, empty tokens dropped (parse_regions_duckdb, bcf_reader.c:423-446)
    std::string index_file; std::vector<uint8_t> index_bytes;
    uint64_t header_bytes = 0; std::vector<uint64_t> seg_beg, seg_end; int64_t seg_count = -1;     // region query: header blocks + index windows are all that is staged
    dhts_ctx *ctx = nullptr;             // bind-time context: holds only the head of the file (header, dictionaries, schema)
    dhts_bcf_info inf;                   // schema of the bind context (column names / types live there)
    int has_index = 0, tidy = 0, device = 0;
};
// ---- scan pipeline, as for read_bam: a producer thread drives the device and reads every batch back into a pinned arena (four queued
// copies, dhts_bcf_batch_fetch); the scan callbacks fill DataChunks from those arenas while the device works on the next batch.
// DHTS_THREADS = 1 (default): one worker, rows in file order, full 2048-row chunks (the reference's only mode for read_bcf without
// an index); DHTS_THREADS = k: k workers claim 2048-row slices, row order across workers unspecified.
struct BcfHostBatch : PipeSlot {
    std::vector<dhts_bcf_col> cols;                 // HOST pointers, projection order (deduplicated)
    std::vector<std::vector<uint32_t>> conv;        // per column: DHTS_ENC_FLOAT_TEXT children converted to float bits
    int ncols_fetched = 0;
};
typedef Pipeline<BcfHostBatch> BcfPipe;
struct BcfScan {
    BcfBind *bind = nullptr;
    std::vector<idx_t> column_ids;       // schema ids per output vector
    std::vector<int> slot;               // output vector -> index into the batch's columns (or -1 for unknown ids)
    std::vector<int32_t> proj;           // projected (deduplicated) schema columns
    dhts_bcf_info inf;                   // the name tables of the scan's own context -- a text scan adds the names records use without a header definition.
    BcfPipe pipe;                        // That context (the source's ctx: the producer stages the file into it) lives until the chunks are filled: teardown destroys it
    ~BcfScan() { pipe.teardown(); }      // (joins the producer, which reads the fields above)
};
struct BcfLocal { BcfPipe::Cursor at; };
static void destroy_bcf_bind(void *p) { BcfBind *b = (BcfBind *)p; if (!b) return; if (b->ctx) dhts_destroy(b->ctx); delete b; }
static void destroy_bcf_local(void *p) { delete (BcfLocal *)p; }
static void destroy_bcf_global(void *p) { delete (BcfScan *)p; }

static void bcf_read_bind(duckdb_bind_info info) {
    auto set_error = API(void, duckdb_bind_set_error, duckdb_bind_info, const char *);
    std::string file_path, idx;
    if (!take_path(info, file_path)) { set_error(info, "read_bcf requires a file path"); return; }                           // bcf_reader.c:461
    BcfBind *b = new BcfBind();
    b->path = file_path;
    (void)named_string(info, "region", b->region); (void)named_string(info, "index_path", idx);
    const int tidy = named_flag(info, "tidy_format");
    for (size_t p0 = 0; p0 <= b->region.size() && !b->region.empty();) {
        size_t q = b->region.find(',', p0); if (q == std::string::npos) q = b->region.size();
        if (q > p0) b->regions.push_back(b->region.substr(p0, q - p0));
        p0 = q + 1;
    }
    char err[768];
    if (!file_exists(b->path)) {
        snprintf(err, sizeof(err), "Failed to open BCF/VCF file: %s", b->path.c_str());       // bcf_reader.c:494
        set_error(info, err); delete b; return;
    }
    const int dev = env_device();
    static const bool trace_bcf_bind = getenv("DHTS_TRACE") != nullptr;
    const double tb0 = now_s();
    std::string no_device;
    b->ctx = create_ctx("read_bcf", no_device, dev); b->tidy = tidy; b->device = dev;
    const double tb1 = now_s();
    if (!b->ctx) { set_error(info, no_device.c_str()); destroy_bcf_bind(b); return; }
    // like the reference, bind reads the header only (bcf_open + bcf_hdr_read, bcf_reader.c:480-505): the head of the file is staged, four
    // times more whenever the header turns out to be longer; every scan stages the file in its own context (bcf_read_global_init)
    bool hdr_ok = false;
    for (uint64_t head = 1u << 20;; head *= 4) {
        if (dhts_open_path_range(b->ctx, b->path.c_str(), 0, head) != 0) {
            snprintf(err, sizeof(err), "Failed to open BCF/VCF file: %s", b->path.c_str());
            set_error(info, err); destroy_bcf_bind(b); return;
        }
        const bool whole = dhts_resident_bytes(b->ctx) < head;
        if (dhts_bgzf_index(b->ctx) > 0 && dhts_bcf_open(b->ctx, tidy) == 0 && dhts_bcf_info_get(b->ctx, &b->inf) == 0) { hdr_ok = true; break; }
        if (whole || head >= (1ull << 34)) break;
        const char *m0 = dhts_error(b->ctx);
        if (m0 && strncmp(m0, "read_bcf:", 9) == 0) break;                   // a refusal, not a header that is merely longer than the head
    }
    if (!hdr_ok) {
        const char *m = dhts_error(b->ctx);
        set_error(info, (m && strncmp(m, "read_bcf:", 9) == 0) ? m : "Failed to read BCF/VCF header");       // bcf_reader.c:505 (or what this build does not read yet)
        destroy_bcf_bind(b); return;
    }
    const double tb2 = now_s();
    for (const std::string &f : {idx, b->path + ".csi", b->path + ".tbi"}) if (!f.empty() && file_exists(f)) { b->index_file = f; break; }
    b->has_index = !b->index_file.empty();
    if (b->has_index && !b->regions.empty()) (void)read_file(b->index_file, b->index_bytes);
    {
        // only the header blocks and the index windows of the regions are staged (the reference seeks to the chunks): byte ranges from this
        // context, which holds the header.  DHTS_SPARSE=0 stages the whole file.
        if (!b->index_bytes.empty() && !b->regions.empty() && env_sparse()) {
            b->header_bytes = dhts_bcf_header_bytes(b->ctx);
            b->seg_beg.resize(4096); b->seg_end.resize(4096);
            if (b->header_bytes == 0 || dhts_bcf_region_segments(b->ctx, b->region.c_str(), b->index_bytes.data(), b->index_bytes.size(), b->seg_beg.data(), b->seg_end.data(), 4096, &b->seg_count) != 0) b->seg_count = -1;
        }
    }
    if (trace_bcf_bind) fprintf(stderr, "[dhts] read_bcf bind: context %.4f s, head of the file + block table + header %.4f s, index file + windows %.4f s (%lld byte ranges)\n", tb1 - tb0, tb2 - tb1, now_s() - tb2, (long long)b->seg_count);
    auto mk = API(duckdb_logical_type, duckdb_create_logical_type, int);
    auto mklist = API(duckdb_logical_type, duckdb_create_list_type, duckdb_logical_type);
    auto add = API(void, duckdb_bind_add_result_column, duckdb_bind_info, const char *, duckdb_logical_type);
    auto rm = API(void, duckdb_destroy_logical_type, duckdb_logical_type *);
    for (int i = 0; i < b->inf.n_cols; i++) {                                               // create_bcf_field_type bcf_reader.c:388-418
        const dhts_bcf_colinfo &ci = b->inf.cols[i];
        duckdb_logical_type el = mk(ci.type);
        if (ci.is_list) { duckdb_logical_type lt = mklist(el); add(info, ci.name, lt); rm(&lt); }
        else add(info, ci.name, el);
        rm(&el);
    }
    API(void, duckdb_bind_set_bind_data, duckdb_bind_info, void *, duckdb_delete_callback_t)(info, b, destroy_bcf_bind);
}

// chained single-region iterators (bcf_reader.c:1327-1345): the next region that yields an iterator; false when none is left
static bool bcf_next_region(BcfBind *bind, dhts_ctx *c, size_t *next_region) {
    while (*next_region < bind->regions.size()) {
        const std::string &rg = bind->regions[(*next_region)++];
        if (dhts_bcf_set_region(c, rg.c_str()) == 0) {                          // unknown contig / malformed: skipped (bcf_reader.c:944-953)
            // BCF: the index only narrows the window, a failure keeps the full scan.  VCF text: the region names a sequence of the tabix
            // index (tbx_itr_querys), 1 = the index does not know it; a failure surfaces with the first batch
            if (!bind->index_bytes.empty() && dhts_bcf_load_index(c, bind->index_bytes.data(), bind->index_bytes.size()) == 1) continue;
            return true;
        }
    }
    return false;
}

// the bytes of a batch have landed: Float fields of a transcript arrive as text -- (float)strtod, NaN unless the whole token converts
// (vep_parse_float, src/vep_parser.c:222-235)
static void bcf_convert_text_floats(const BcfBind *bind, BcfHostBatch *hb) {
    hb->conv.assign((size_t)hb->ncols_fetched, std::vector<uint32_t>());
    for (int i = 0; i < hb->ncols_fetched; i++) {
        const dhts_bcf_col &h = hb->cols[i];
        if (bind->inf.cols[h.col].encoding != DHTS_ENC_FLOAT_TEXT) continue;
        std::vector<uint32_t> &cv = hb->conv[i]; cv.assign(h.child_n + 1, 0);
        std::string tok;
        for (uint64_t k = 0; k < h.child_n; k++) {
            if (h.child_valid && !h.child_valid[k]) continue;
            tok.assign((const char *)h.bytes + h.child_off[k], h.child_off[k + 1] - h.child_off[k]);
            char *end = nullptr; const double v = strtod(tok.c_str(), &end);
            const float f = (end == tok.c_str() || *end) ? NAN : (float)v;
            memcpy(&cv[k], &f, 4);
        }
    }
}

static void bcf_producer_main(BcfScan *g) {
    BcfBind *bind = g->bind; BcfPipe &pipe = g->pipe; BcfPipe::Source &src = *pipe.src[0];
    auto finish = [&](const std::string &err) { pipe.finish(src, err); };
    static const bool trace = getenv("DHTS_TRACE") != nullptr;       // stage timings on stderr
    const double t_start = now_s();
    (void)dhts_bind_thread_near_device(bind->device);          // (as read_bam's producers: thread, staging readers and pinned arenas on the GPU's NUMA node)
    dhts_ctx *c = dhts_create(bind->device);
    src.ctx = c;
    if (!c) { finish(no_device_message("read_bcf")); return; }
    dhts_set_super_blocks(c, 196608);
    const double t_ctx = now_s() - t_start;
    // a plain whole-file scan starts decoding while the file is still being staged (as read_bam does): the block table is built over the
    // resident prefix and extended as more bytes arrive.  DHTS_STREAM=0, region queries and uncompressed text stage first.
    const bool streaming = bind->regions.empty() && env_stream() && bind->seg_count < 0 && dhts_bcf_is_text(bind->ctx) != 2;
    int staged_all = 1;
    int orc = bind->seg_count >= 0 ? dhts_open_path_segments(c, bind->path.c_str(), bind->header_bytes, bind->seg_beg.data(), bind->seg_end.data(), bind->seg_count)
              : streaming ? dhts_open_path_async(c, bind->path.c_str()) : dhts_open_path(c, bind->path.c_str());
    if (orc == 0 && !streaming && (dhts_bgzf_index(c) <= 0 || dhts_bcf_open(c, bind->tidy) != 0)) orc = -1;
    if (orc == 0 && streaming) orc = stream_open(c, 32u << 20, &staged_all, [&](dhts_ctx *x) { return dhts_bcf_open(x, bind->tidy); });
    if (orc != 0 || dhts_bcf_info_get(c, &g->inf) != 0) {
        finish(std::string("Failed to open BCF/VCF file: ") + bind->path); return;
    }
    const double t_open = now_s() - t_start;
    if (dhts_bcf_set_projection(c, g->proj.data(), (int32_t)g->proj.size()) != 0 || dhts_bcf_set_region(c, nullptr) != 0) { finish("Failed to open BCF/VCF file"); return; }
    size_t next_region = 0;
    if (!bind->regions.empty() && !bcf_next_region(bind, c, &next_region)) { finish(""); return; }     // no region produced an iterator: zero rows (bcf_reader.c:955-959)
    const double t_region = now_s() - t_start;
    if (trace) fprintf(stderr, "[dhts] read_bcf producer dev %d: context %.4f s, staged + block table + header at %.4f s (%s, %llu bytes resident), first region set at %.4f s\n", bind->device, t_ctx, t_open,
                       bind->seg_count >= 0 ? "header + index windows" : streaming ? "streaming" : "whole file", (unsigned long long)dhts_resident_bytes(c), t_region);
    const int64_t max_blocks = env_batch_blocks(4096);
    dhts_bcf_batch b;
    // the previous batch has this batch's scan to cross PCIe; then it is finished (text floats) and handed to the fill threads
    auto rb = make_readback(pipe, src, !env_overlap_readback(),
                            [&](BcfHostBatch *hb) { return dhts_bcf_batch_fetch(c, &b, hb->arena, hb->cap, hb->cols.data()) == 0; },
                            [&](BcfHostBatch *hb, int sl) { return dhts_bcf_batch_fetch_begin(c, &b, hb->arena, hb->cap, hb->cols.data(), sl) == 0; },
                            [&](int sl) { return dhts_bcf_batch_fetch_wait(c, sl) == 0; }, [&](BcfHostBatch *hb) { bcf_convert_text_floats(bind, hb); });
    for (;;) {
        if (streaming && stream_extend(c, max_blocks, &staged_all) < 0) { finish(dhts_error(c)); return; }
        if (dhts_bcf_next_batch(c, max_blocks, &b) != 0) { finish(dhts_error(c)); return; }
        if (b.n_rows > 0) {
            BcfHostBatch *hb = pipe.take_slot(src);
            if (!hb) break;
            if (!pipe.reserve(hb, dhts_bcf_batch_host_bytes(c))) { finish("read_bcf: out of pinned host memory"); return; }
            hb->cols.assign((size_t)b.n_cols, dhts_bcf_col());
            if (!rb.begin(hb)) { finish(dhts_error(c)); return; }
            hb->n = b.n_rows; hb->status = b.status; hb->next = 0; hb->readers = 0; hb->retired = false; hb->ncols_fetched = b.n_cols;
            if (!rb.turn(hb)) { finish(dhts_error(c)); return; }
        }
        if (b.status != 0) {                                     // EOF, or the silent stop at the first bad record (bcf_reader.c:1319-1349)
            if (!bind->regions.empty() && bcf_next_region(bind, c, &next_region)) continue;
            break;
        }
        if (pipe.cancelled()) break;
    }
    if (!rb.flush()) { finish(dhts_error(c)); return; }
    finish("");
}
static void bcf_read_global_init(duckdb_init_info info) {
    BcfBind *bind = (BcfBind *)API(void *, duckdb_init_get_bind_data, duckdb_init_info)(info);
    if (!bind->regions.empty() && !bind->has_index) {
        char err[900];
        snprintf(err, sizeof(err), "Region query requires an index file (.tbi or .csi). Region: %s", bind->region.c_str());   // bcf_reader.c:922-923
        API(void, duckdb_init_set_error, duckdb_init_info, const char *)(info, err);
        return;
    }
    BcfScan *g = new BcfScan();
    g->bind = bind;
    Projection pj; map_projection(info, (idx_t)bind->inf.n_cols, pj);
    g->column_ids.swap(pj.column_ids); g->slot.swap(pj.slot); g->proj.swap(pj.proj);
    const int thr = env_fill_threads();
    g->pipe.init(1, 3, thr, dhts_host_alloc, dhts_host_free, [](void *c) { dhts_destroy((dhts_ctx *)c); });
    g->pipe.start(0, [g] { bcf_producer_main(g); });
    API(void, duckdb_init_set_max_threads, duckdb_init_info, idx_t)(info, (idx_t)thr);
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, g, destroy_bcf_global);
}

static void bcf_read_local_init(duckdb_init_info info) {
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, new BcfLocal(), destroy_bcf_local);
}

static size_t bcf_fixed_width(const dhts_bcf_colinfo &ci) {
    if (ci.is_list) return 0;
    if (ci.encoding != DHTS_ENC_PLAIN) return 4;
    switch (ci.type) { case DHTS_T_BOOLEAN: return 1; case DHTS_T_INTEGER: case DHTS_T_FLOAT: return 4; case DHTS_T_BIGINT: case DHTS_T_DOUBLE: return 8; default: return 0; }
}

// rows [s, s + take) of a host batch -> rows [row_count, row_count + take) of the output chunk
static void bcf_fill(const BcfBind *bind, const BcfScan *g, const BcfHostBatch *hb, int64_t s, idx_t take, duckdb_data_chunk output, idx_t row_count) {
    auto get_vec = API(duckdb_vector, duckdb_data_chunk_get_vector, duckdb_data_chunk, idx_t);
    auto get_data = API(void *, duckdb_vector_get_data, duckdb_vector);
    auto assign_len = API(void, duckdb_vector_assign_string_element_len, duckdb_vector, idx_t, const char *, idx_t);
    for (size_t ci = 0; ci < g->column_ids.size(); ci++) {
        if (g->slot[ci] < 0) continue;                          // ids outside the schema write nothing
        const dhts_bcf_col &h = hb->cols[g->slot[ci]];
        const dhts_bcf_colinfo &inf = bind->inf.cols[h.col];
        duckdb_vector vec = get_vec(output, ci);
        const char *const *names = inf.encoding == DHTS_ENC_CONTIG ? g->inf.contig_name : inf.encoding == DHTS_ENC_DICT ? g->inf.dict_name :
                                   inf.encoding == DHTS_ENC_SAMPLE ? g->inf.sample_name : nullptr;      // (the SCAN's tables: a text scan may have added names)
        auto name_of = [&](int32_t id) -> const char * { if (id < 0) return "PASS"; const char *nm = names[id]; return nm ? nm : "."; };
        if (!inf.is_list) {
            const size_t w = bcf_fixed_width(inf);
            if (names) {
                for (idx_t r = 0; r < take; r++) { const char *nm = name_of(((const int32_t *)h.fixed)[s + r]); assign_len(vec, row_count + r, nm, strlen(nm)); }
            } else if (w) {
                memcpy((uint8_t *)get_data(vec) + row_count * w, (const uint8_t *)h.fixed + (size_t)s * w, take * w);
                for (idx_t r = 0; r < take; r++) if (!h.valid[s + r]) set_null(vec, row_count + r);
            } else {
                for (idx_t r = 0; r < take; r++) {
                    if (h.valid[s + r]) assign_len(vec, row_count + r, (const char *)h.bytes + h.off[s + r], h.off[s + r + 1] - h.off[s + r]);
                    else set_null(vec, row_count + r);
                }
            }
            continue;
        }
        // LIST: entries {offset = current child size, length}; children appended in row order (bcf_reader.c:1403-1424, 1436-1461, 1584-1610)
        const ListFrame f = list_entries(vec, h.off, h.valid, s, take, row_count);
        const idx_t base = f.base; const uint32_t c0 = f.c0, c1 = f.c1; duckdb_vector child = f.child;
        if (c1 > c0) {
            const std::vector<uint32_t> &cv32 = hb->conv[g->slot[ci]];
            if (names) for (uint32_t k = c0; k < c1; k++) { const char *nm = name_of((int32_t)h.child_fixed[k]); assign_len(child, base + (k - c0), nm, strlen(nm)); }
            else if (inf.type == DHTS_T_VARCHAR) {
                for (uint32_t k = c0; k < c1; k++)
                    if (!h.child_valid || h.child_valid[k]) assign_len(child, base + (k - c0), (const char *)h.bytes + h.child_off[k], h.child_off[k + 1] - h.child_off[k]);
            } else memcpy((uint32_t *)get_data(child) + base, (inf.encoding == DHTS_ENC_FLOAT_TEXT ? cv32.data() : h.child_fixed) + c0, (size_t)(c1 - c0) * 4);
            if (h.child_valid) {                                // NULL elements: a field the transcript does not have (bcf_reader.c:1485-1530)
                API(void, duckdb_vector_ensure_validity_writable, duckdb_vector)(child);
                uint64_t *cv = API(uint64_t *, duckdb_vector_get_validity, duckdb_vector)(child);
                for (uint32_t k = c0; k < c1; k++) {
                    const idx_t at = base + (k - c0);
                    if (h.child_valid[k]) cv[at / 64] |= (uint64_t)1 << (at % 64); else cv[at / 64] &= ~((uint64_t)1 << (at % 64));
                }
            }
        }
    }
}

static void bcf_read_function(duckdb_function_info info, duckdb_data_chunk output) {
    BcfBind *bind = (BcfBind *)API(void *, duckdb_function_get_bind_data, duckdb_function_info)(info);
    BcfScan *g = (BcfScan *)API(void *, duckdb_function_get_init_data, duckdb_function_info)(info);
    BcfLocal *l = (BcfLocal *)API(void *, duckdb_function_get_local_init_data, duckdb_function_info)(info);
    auto set_size = API(void, duckdb_data_chunk_set_size, duckdb_data_chunk, idx_t);
    if (!l || !g) { set_size(output, 0); return; }                                            // bcf_reader.c:1166-1169
    std::string err;
    const int64_t n = g->pipe.fill_chunk(l->at, API(idx_t, duckdb_vector_size, void)(), err, [&](const BcfHostBatch &hb, int64_t s, idx_t take, idx_t row_count) { bcf_fill(bind, g, &hb, s, take, output, row_count); });
    if (n < 0) API(void, duckdb_function_set_error, duckdb_function_info, const char *)(info, err.c_str());
    set_size(output, n < 0 ? 0 : (idx_t)n);
}

extern "C" __attribute__((visibility("default"))) void register_read_bcf_function(duckdb_connection connection) {                       // bcf_reader.c:2055-2080
    register_table_function(connection, "read_bcf", {{"region", DUCKDB_TYPE_VARCHAR}, {"index_path", DUCKDB_TYPE_VARCHAR}, {"tidy_format", DUCKDB_TYPE_BOOLEAN}},
                            bcf_read_bind, bcf_read_global_init, bcf_read_local_init, bcf_read_function, true);
}
