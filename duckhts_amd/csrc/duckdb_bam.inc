// duckdb_bam.inc -- part of duckdb_ext.cpp (included there; not a translation unit of its own): the read_bam table function.
//
// Mirrors, callback for callback, the reference's read_bam table function:
//   register_read_bam_function   src/bam_reader.c:1044-1068
//   bam_read_bind                src/bam_reader.c:410-557   (parameters, schema, error strings)
//   bam_read_global_init         src/bam_reader.c:563-588
//   bam_read_local_init          src/bam_reader.c:594-682   (projection ids)
//   bam_read_function            src/bam_reader.c:722-1038  (<= vector_size rows per call, size 0 = done)
// The htslib calls underneath are replaced by include/duckhts_amd.h (HIP kernels); DuckDB is reached only
// through the function-pointer table returned by access->get_api(info, "v1.2.0").
//
// Scan mode: the reference's sequential mode (i) (SURVEY.md 8(a) A0): all records in file order including
// unplaced reads, full 2048-row chunks except the last.  region, standard_tags and auxiliary_tags are served by
// the GPU path; CRAM / SAM text input fails at bind with the reference's header error.
struct BamBind {
    std::string path, region, index_file;
    dhts_ctx *ctx = nullptr;          // bind-time context: holds only the head of the file (header + dictionaries)
    dhts_bam_header hdr;
    uint64_t header_bytes = 0;        // compressed bytes [0, header_bytes) cover the header blocks
    int has_index = 0;
    int standard_tags = 0, auxiliary_tags = 0;
    idx_t aux_col_idx = (idx_t)-1;
    std::vector<duckdb_string_t> ref_inl; std::vector<char> ref_is_inl;      // RNAME / RNEXT values of <= 12 bytes, ready to store
    duckdb_string_t star_inl;
};

// ---- scan pipeline: GPU producer thread(s) -> pinned host batches -> scan callbacks ------------------------------------------------
// The reference's callback reads one record at a time from its htsFile (src/bam_reader.c:747-1035).  Here a producer thread per GPU
// owns a scan context and turns the file into batches: stage (reader threads -> pinned -> HBM), inflate + unpack on the device, then
// ONE queued read-back of the projected columns into a pinned arena (dhts_bam_batch_fetch).  The scan callbacks only copy from
// those arenas into DataChunk vectors, so the device works on batch k+1 while the engine's threads fill chunks from batch k.
//   DHTS_THREADS = 1 (default): the reference's sequential mode (i) -- one worker, rows in file order, full 2048-row chunks.
//   DHTS_THREADS = k > 1: k workers claim 2048-row slices of the ready batches, the row ORDER across workers is unspecified,
//                  exactly like the reference's own parallel mode (contig-parallel, src/bam_reader.c:577-585, 689-716).
//   DHTS_DEVICES = 0,1,...: one producer per listed GPU, each staging and scanning its own BGZF block range of the file.
struct HostTag { std::vector<uint8_t> valid, bytes; std::vector<int64_t> fixed; std::vector<uint32_t> off; std::vector<int64_t> child; };
struct HostBatch : PipeSlot {
    dhts_bam_batch b;                 // HOST pointers for the core columns
    std::vector<HostTag> tags;
    std::vector<uint8_t> aux_valid; std::vector<uint32_t> aux_off, aux_koff, aux_voff; std::string aux_keys, aux_vals;    // the auxiliary map, laid out as a dhts_tabix_map
    std::vector<uint32_t> qual_lut;   // QUAL as 2- / 4-bit codes (dhts_bam_batch.qual_bits): code byte -> its 4 / 2 characters, built when the batch's bytes have landed
};
typedef Pipeline<HostBatch> BamPipe;
// one producer's share of the file; where its rows begin and end, as BGZF virtual offsets: adjacent ranks must meet exactly (SURVEY 8(e) hand-off)
struct Shard { int device = 0, rank = 0, world = 1; bool has_rows = false; uint64_t first_v = 0, end_v = 0; };
struct BamScan {
    BamBind *bind = nullptr;
    std::vector<idx_t> column_ids; uint32_t colmask = 0;
    std::vector<int32_t> tag_ids; std::vector<int> tag_slot; bool want_aux = false;
    std::vector<Shard> shard;                                            // one per source of `pipe`
    std::vector<uint8_t> index_bytes;
    std::vector<uint64_t> seg_beg, seg_end; int64_t seg_count = -1;      // region query: the file byte ranges to stage (-1: the whole file)
    BamPipe pipe;
    ~BamScan() { pipe.teardown(); }                                      // (joins the producers, which read the fields above)
};
struct BamLocal {
    std::vector<char> seq_tmp;         // packed SEQ expands here before it is assigned
    std::vector<char> qual_tmp;        // packed QUAL: a row that starts inside a code byte is expanded here first
    BamPipe::Cursor at;
};

static void destroy_bind(void *p) { BamBind *b = (BamBind *)p; if (!b) return; if (b->ctx) dhts_destroy(b->ctx); delete b; }
static void destroy_local(void *p) { delete (BamLocal *)p; }
static void destroy_global(void *p) { delete (BamScan *)p; }

// a string of <= 12 bytes is stored inside duckdb_string_t itself (duckdb.h:377-391: length, then the bytes, zero padded): no heap, no call
static inline bool inl_string(duckdb_string_t *d, const char *s, size_t len) {
    if (len > 12) return false;
    memset(d, 0, sizeof(*d)); d->value.inlined.length = (uint32_t)len; memcpy(d->value.inlined.inlined, s, len);
    return true;
}
// 4-bit base codes -> text, high nibble first ("=ACMGRSVTWYHKDBN", htslib hts.c:260, sam.h:325): 16 bases per step through pshufb
// (the table is the shuffle's own 16-byte lookup), a 512-byte pair table for the tail.  out must have room for n + 16 bytes.
#include <immintrin.h>
static const char kSeqNt16[] = "=ACMGRSVTWYHKDBN";
static uint16_t g_seq_pair[256];
static const bool g_seq_pair_init = [] { for (int b = 0; b < 256; b++) { const uint8_t p[2] = {(uint8_t)kSeqNt16[b >> 4], (uint8_t)kSeqNt16[b & 15]}; uint16_t v; memcpy(&v, p, 2); g_seq_pair[b] = v; } return true; }();
__attribute__((target("ssse3"))) static inline void expand_seq(const uint8_t *src, uint32_t n, char *out) {
    const __m128i tab = _mm_loadu_si128((const __m128i *)kSeqNt16), lo_mask = _mm_set1_epi8(0x0f);
    uint32_t i = 0;
    for (; i + 16 <= n; i += 16) {
        const __m128i v = _mm_loadl_epi64((const __m128i *)(src + i / 2));             // 8 bytes = 16 bases
        const __m128i hi = _mm_and_si128(_mm_srli_epi16(v, 4), lo_mask), lo = _mm_and_si128(v, lo_mask);
        _mm_storeu_si128((__m128i *)(out + i), _mm_shuffle_epi8(tab, _mm_unpacklo_epi8(hi, lo)));
    }
    for (; i < n; i += 2) { const uint16_t v = g_seq_pair[src[i / 2]]; memcpy(out + i, &v, 2); }    // (may write one byte past an odd n: room is there)
    (void)g_seq_pair_init;
}

// What bind does with the file, for read_bam and for bam_bin_counts: the head of the file on a bind-time context, the header, the index
// lookup, the region string.  false: `error` is the bind error (the caller destroys b).
static bool bam_bind_file(BamBind *b, const char *fn_name, const std::string &file_path, const std::string &region, const std::string &idx, std::string &error) {
    b->path = file_path;
    // parse_regions (bam_reader.c:319-345) splits with strtok: a string without a non-empty token ('' or ',,') is no region at all
    const bool has_region = region.find_first_not_of(',') != std::string::npos;

    char err[768];
    if (!file_exists(b->path)) {
        snprintf(err, sizeof(err), "Failed to open SAM/BAM/CRAM file: %s", b->path.c_str());   // bam_reader.c:446
        error = err; return false;
    }
    static const bool trace_bind = getenv("DHTS_TRACE") != nullptr;
    const double tb0 = now_s();
    std::string no_device;
    b->ctx = create_ctx(fn_name, no_device);
    const double tb1 = now_s();
    if (!b->ctx) { error = no_device; return false; }
    // like the reference, bind reads the header only (sam_open + sam_hdr_read, bam_reader.c:441-461): the head of the file is staged,
    // four times more whenever the header turns out to be longer.  The scan stages the file itself (bam_read_global_init).
    bool hdr_ok = false;
    for (uint64_t head = 1u << 20;; head *= 4) {
        if (dhts_open_path_range(b->ctx, b->path.c_str(), 0, head) != 0) {
            snprintf(err, sizeof(err), "Failed to open SAM/BAM/CRAM file: %s", b->path.c_str());
            error = err; return false;
        }
        const bool whole = dhts_resident_bytes(b->ctx) < head;
        if (dhts_bgzf_index(b->ctx) > 0 && dhts_bam_open(b->ctx) == 0 && dhts_bam_header_get(b->ctx, &b->hdr) == 0) { hdr_ok = true; break; }
        if (whole || head >= (1ull << 34)) break;
    }
    if (!hdr_ok) {
        error = "Failed to read SAM/BAM/CRAM header";                             // bam_reader.c:461 (also what SAM/CRAM input gets here)
        return false;
    }
    b->header_bytes = dhts_bam_header_bytes(b->ctx);
    if (trace_bind) fprintf(stderr, "[dhts] bind: context %.4f s, head of the file + block table + header %.4f s\n", tb1 - tb0, now_s() - tb1);
    for (int32_t i = 0; i < b->hdr.n_ref; i++) { duckdb_string_t t; b->ref_is_inl.push_back(inl_string(&t, b->hdr.ref_name[i], strlen(b->hdr.ref_name[i])) ? 1 : 0); b->ref_inl.push_back(t); }
    inl_string(&b->star_inl, "*", 1);
    // index lookup order of sam_index_load3 (hts.c:4720-4790): explicit path, <file>.csi, <file>.bai, <file minus .bam>.bai/.csi
    {
        std::string stem = b->path.size() > 4 && b->path.compare(b->path.size() - 4, 4, ".bam") == 0 ? b->path.substr(0, b->path.size() - 4) : std::string();
        std::vector<std::string> cand;
        if (!idx.empty()) cand.push_back(idx);
        else { cand.push_back(b->path + ".csi"); cand.push_back(b->path + ".bai"); if (!stem.empty()) { cand.push_back(stem + ".csi"); cand.push_back(stem + ".bai"); } }
        for (auto &f : cand) if (file_exists(f)) { b->index_file = f; break; }
    }
    b->has_index = !b->index_file.empty();                                       // bam_reader.c:499-503
    if (has_region) b->region = region;
    return true;
}

static void bam_read_bind(duckdb_bind_info info) {
    auto set_error = API(void, duckdb_bind_set_error, duckdb_bind_info, const char *);
    std::string file_path, region, idx;
    if (!take_path(info, file_path)) { set_error(info, "read_bam requires a file path"); return; }                          // bam_reader.c:416
    (void)named_string(info, "region", region); (void)named_string(info, "index_path", idx);          // (reference is accepted and not read: CRAM is refused)
    const int standard_tags = named_flag(info, "standard_tags"), auxiliary_tags = named_flag(info, "auxiliary_tags");
    BamBind *b = new BamBind();
    std::string bind_error;
    if (!bam_bind_file(b, "read_bam", file_path, region, idx, bind_error)) { set_error(info, bind_error.c_str()); destroy_bind(b); return; }
    b->standard_tags = standard_tags; b->auxiliary_tags = auxiliary_tags;

    static const char *const core_names[DHTS_BAM_CORE_COUNT] = {"QNAME", "FLAG", "RNAME", "POS", "MAPQ", "CIGAR", "RNEXT", "PNEXT", "TLEN", "SEQ", "QUAL", "READ_GROUP_ID", "SAMPLE_ID"};   // bam_reader.c:514-526
    static const int32_t V = DUCKDB_TYPE_VARCHAR, I = DUCKDB_TYPE_BIGINT, core_types[DHTS_BAM_CORE_COUNT] = {V, DUCKDB_TYPE_USMALLINT, V, I, DUCKDB_TYPE_INTEGER, V, V, I, I, V, V, V, V};
    add_columns(info, core_names, core_types, DHTS_BAM_CORE_COUNT);
    if (b->standard_tags) {                                                                     // bam_reader.c:527-537 + bam_std_tag_type 88-104
        auto mk = API(duckdb_logical_type, duckdb_create_logical_type, int);
        auto rm = API(void, duckdb_destroy_logical_type, duckdb_logical_type *);
        duckdb_logical_type t_varchar = mk(V), t_big = mk(I), t_list = API(duckdb_logical_type, duckdb_create_list_type, duckdb_logical_type)(t_big);
        for (int i = 0; i < dhts_bam_std_tag_count(); i++) {
            char nm[3], ty, sub; dhts_bam_std_tag_info(i, nm, &ty, &sub);
            API(void, duckdb_bind_add_result_column, duckdb_bind_info, const char *, duckdb_logical_type)(info, nm, ty == 'i' ? t_big : ty == 'B' ? t_list : t_varchar);
        }
        rm(&t_list); rm(&t_big); rm(&t_varchar);
    }
    if (b->auxiliary_tags) {                                                                    // bam_reader.c:539-548
        b->aux_col_idx = DHTS_BAM_CORE_COUNT + (b->standard_tags ? (idx_t)dhts_bam_std_tag_count() : 0);
        add_map_column(info, "AUXILIARY_TAGS");
    }
    API(void, duckdb_bind_set_bind_data, duckdb_bind_info, void *, duckdb_delete_callback_t)(info, b, destroy_bind);
}

// copies the standard-tag columns and the auxiliary map of a device batch to pageable host memory (optional columns, off by default)
static int fetch_optional(dhts_ctx *c, BamScan *g, const dhts_bam_batch &b, HostBatch *hb) {
    const int64_t n = b.n_rows;
    if (g->want_aux && b.aux_map) {
        // typed entries -> value text, bam_aux_to_string (bam_reader.c:140-183); assigned through the NUL-terminated API
        const dhts_aux_map &am = *b.aux_map; const size_t ne = (size_t)am.n_ent;
        std::vector<uint16_t> key(ne + 1); std::vector<uint8_t> kind(ne + 1), sub(ne + 1), pay(am.payload_bytes + 8); std::vector<uint32_t> po(ne + 2);
        hb->aux_valid.resize(n); hb->aux_off.resize(n + 1);
        if (dhts_memcpy_d2h(c, hb->aux_valid.data(), am.valid, n) || dhts_memcpy_d2h(c, hb->aux_off.data(), am.off, (n + 1) * 4)) return -1;
        if (ne && (dhts_memcpy_d2h(c, key.data(), am.key, ne * 2) || dhts_memcpy_d2h(c, kind.data(), am.kind, ne) || dhts_memcpy_d2h(c, sub.data(), am.sub, ne))) return -1;
        if (dhts_memcpy_d2h(c, po.data(), am.pay_off, (ne + 1) * 4)) return -1;
        if (am.payload_bytes && dhts_memcpy_d2h(c, pay.data(), am.payload, am.payload_bytes)) return -1;
        hb->aux_keys.clear(); hb->aux_vals.clear(); hb->aux_koff.assign(1, 0); hb->aux_voff.assign(1, 0);
        char tmp[64];
        for (size_t i = 0; i < ne; i++) {
            char kb[3] = {(char)(key[i] & 0xff), (char)(key[i] >> 8), 0};
            hb->aux_keys += kb; hb->aux_koff.push_back((uint32_t)hb->aux_keys.size());
            const uint8_t *p = pay.data() + po[i]; const size_t pl = po[i + 1] - po[i];
            std::string v;
            int64_t iv; double dv;
            switch (kind[i]) {
            case 0: memcpy(&iv, p, 8); snprintf(tmp, sizeof tmp, "%lld", (long long)iv); v = tmp; break;
            case 1: memcpy(&dv, p, 8); snprintf(tmp, sizeof tmp, "%g", dv); v = tmp; break;
            case 2: case 3: v.assign((const char *)p, pl); break;
            case 4: v.push_back((char)sub[i]); for (size_t q = 0; q < pl / 8; q++) { memcpy(&iv, p + 8 * q, 8); snprintf(tmp, sizeof tmp, ",%lld", (long long)iv); v += tmp; } break;
            case 5: v.push_back((char)sub[i]); for (size_t q = 0; q < pl / 8; q++) { memcpy(&dv, p + 8 * q, 8); snprintf(tmp, sizeof tmp, ",%g", dv); v += tmp; } break;
            default: break;
            }
            hb->aux_vals += v.c_str(); hb->aux_voff.push_back((uint32_t)hb->aux_vals.size());     // C-string semantics: cut at the first NUL
        }
    }
    hb->tags.resize(b.n_tag_cols);
    for (int i = 0; i < b.n_tag_cols; i++) {
        const dhts_col &d = b.tag_cols[i]; HostTag &h = hb->tags[i];
        h.valid.resize(n); if (dhts_memcpy_d2h(c, h.valid.data(), d.valid, n)) return -1;
        if (d.fixed) { h.fixed.resize(n); if (dhts_memcpy_d2h(c, h.fixed.data(), d.fixed, n * 8)) return -1; }
        if (d.off) { h.off.resize(n + 1); if (dhts_memcpy_d2h(c, h.off.data(), d.off, (n + 1) * 4)) return -1; }
        if (d.bytes || d.nbytes == 0) { h.bytes.resize(d.nbytes + 1); if (d.nbytes && dhts_memcpy_d2h(c, h.bytes.data(), d.bytes, d.nbytes)) return -1; }
        if (d.child_fixed) { h.child.resize(d.child_n + 1); if (d.child_n && dhts_memcpy_d2h(c, h.child.data(), d.child_fixed, d.child_n * 8)) return -1; }
    }
    return 0;
}

// producer thread: one GPU, one scan context, one block range of the file
// QUAL as codes of the batch's own alphabet (dhts_bam_batch.qual_bits = 2 / 4): qual.bytes = 16-byte symbol table + code stream, character k
// of the heap at bit k * bits.  The table of a batch: code byte -> its 4 (2-bit) or 2 (4-bit) characters.
static void build_qual_lut(HostBatch *hb) {
    hb->qual_lut.clear();
    const dhts_bam_batch &b = hb->b;
    if (!b.qual_bits || !b.qual.bytes) return;
    const uint8_t *sym = b.qual.bytes;
    hb->qual_lut.resize(256);
    for (uint32_t v = 0; v < 256; v++) {
        if (b.qual_bits == 2) hb->qual_lut[v] = (uint32_t)sym[v & 3] | ((uint32_t)sym[(v >> 2) & 3] << 8) | ((uint32_t)sym[(v >> 4) & 3] << 16) | ((uint32_t)sym[v >> 6] << 24);
        else hb->qual_lut[v] = (uint32_t)sym[v & 15] | ((uint32_t)sym[v >> 4] << 8);
    }
}
// characters [off, off + n) of the heap -> out[0, n) (out has room for n + 8)
static inline void expand_qual(const uint8_t *stream, int bits, const uint32_t *lut, uint32_t off, uint32_t n, char *out, std::vector<char> &tmp) {
    const uint32_t per = bits == 2 ? 4u : 2u, first = off / per, skip = off % per, nb = (skip + n + per - 1) / per;
    char *w = out;
    if (skip) { if (tmp.size() < (size_t)nb * per + 8) tmp.resize((size_t)nb * per + 8 + n / 2); w = tmp.data(); }
    if (bits == 2) for (uint32_t k = 0; k < nb; k++) { const uint32_t v = lut[stream[first + k]]; memcpy(w + 4 * k, &v, 4); }
    else for (uint32_t k = 0; k < nb; k++) { const uint16_t v = (uint16_t)lut[stream[first + k]]; memcpy(w + 2 * k, &v, 2); }
    if (skip) memcpy(out, w + skip, n);
}
static void producer_main(BamScan *g, size_t k) {
    BamBind *bind = g->bind; BamPipe &pipe = g->pipe; BamPipe::Source &src = *pipe.src[k]; Shard *p = &g->shard[k];
    static const bool trace = getenv("DHTS_TRACE") != nullptr;       // stage timings of every producer on stderr
    const double t_start = now_s(); double t_open = 0, t_gpu = 0, t_fetch = 0, t_slot = 0, t_ext[2] = {0, 0}; int64_t n_batches = 0, n_rows = 0, n_index = 0;
    // the producer, the staging readers it starts and the pinned arenas it allocates live on the NUMA node of its GPU
    const int numa_rc = dhts_bind_thread_near_device(p->device);
    if (trace) fprintf(stderr, "[dhts] producer %d: device %d on NUMA node %d (%s)\n", p->rank, p->device, dhts_device_numa_node(p->device), numa_rc == 0 ? "bound" : numa_rc == 1 ? "not bound" : "bind failed");
    dhts_ctx *c = dhts_create(p->device);
    // the context dies before the producer reports done: its HBM goes back to the pool for the next query
    auto fail_with = [&](std::string msg) { if (c) dhts_destroy(c); pipe.finish(src, msg); };
    auto fail = [&] { fail_with(dhts_error(c)); };
    if (!c) { fail_with(no_device_message("read_bam")); return; }
    dhts_set_super_blocks(c, 196608);                    // a scratch the device pool keeps from query to query (29 GB instead of 67 GB for a 10 GB file)
    dhts_bam_set_qual_packed(c, env_is_zero("DHTS_QUAL_PACKED") ? 0 : 1);     // QUAL crosses PCIe as 2- / 4-bit codes when the batch holds at most 4 / 16 different characters
    dhts_bam_set_seq_packed(c, env_is_zero("DHTS_SEQ_PACKED") ? 0 : 1);       // SEQ crosses PCIe as 4-bit codes, the fill threads expand it
    const double t_created = now_s() - t_start; double t_staged = 0;
    int rc;
    // a plain whole-file scan on one device starts decoding while the file is still being staged: the block table is built over the
    // resident prefix and extended as more bytes arrive (DHTS_STREAM=0 stages the whole file first)
    const bool streaming = p->world == 1 && bind->region.empty() && env_stream() && (dhts_bam_is_text(bind->ctx) == 0 || dhts_bam_is_text(bind->ctx) % 2 != 0);   // (uncompressed text -- 2, 4, 6 -- is staged first)
    int staged_all = 1;
    if (g->seg_count >= 0) rc = dhts_open_path_segments(c, bind->path.c_str(), bind->header_bytes, g->seg_beg.data(), g->seg_end.data(), g->seg_count);
    else if (p->world > 1) rc = dhts_open_path_shard(c, bind->path.c_str(), p->rank, p->world, bind->header_bytes);
    else if (streaming) rc = dhts_open_path_async(c, bind->path.c_str());
    else rc = dhts_open_path(c, bind->path.c_str());
    t_staged = now_s() - t_start;
    const bool from_cache = rc == 0 && dhts_resident_from_cache(c) != 0;
    double t_idx = 0, t_hdr = 0;
    if (rc == 0 && !streaming) {
        const double q0 = now_s();
        if (dhts_bgzf_index(c) <= 0) rc = -1;
        const double q1 = now_s(); t_idx = q1 - q0;
        if (rc == 0 && dhts_bam_open(c) != 0) rc = -1;
        t_hdr = now_s() - q1;
    }
    if (rc == 0 && streaming) rc = stream_open(c, bind->header_bytes + (32u << 20), &staged_all, dhts_bam_open);     // start with what the bind saw
    if (rc != 0) { fail_with(std::string("Failed to open SAM/BAM/CRAM file: ") + bind->path); return; }
    t_open = now_s() - t_start;
    dhts_bam_set_tag_columns(c, g->tag_ids.data(), (int32_t)g->tag_ids.size());
    dhts_bam_set_aux_map(c, g->want_aux ? 1 : 0, bind->standard_tags);
    if (!bind->region.empty()) {
        rc = dhts_bam_set_regions(c, bind->region.c_str());
        if (rc == 0 && !g->index_bytes.empty()) rc = dhts_bam_load_index(c, g->index_bytes.data(), g->index_bytes.size());
    } else rc = dhts_bam_set_regions(c, nullptr);
    if (rc == 0 && p->world > 1) rc = dhts_bam_set_file_shard(c, p->rank, p->world);
    else if (rc == 0 && bind->region.empty()) rc = dhts_bam_rewind(c);
    if (rc != 0) { fail(); return; }
    const int64_t max_blocks = env_batch_blocks(4096);           // ~270 MB of inflated stream per batch: the engine gets its first chunk early and the stages overlap
    int64_t n_qual[3] = {0, 0, 0};                               // batches whose QUAL crossed PCIe as 2-bit codes / 4-bit codes / characters
    dhts_bam_batch b;
    // the read-back of a batch runs on a copy stream while the next batch is scanned: the batch is handed to the fill threads one turn
    // later, when its bytes have had a whole scan's time to cross PCIe (DHTS_OVERLAP_READBACK=0: copy, wait, hand over)
    auto rb = make_readback(pipe, src, !env_overlap_readback(),
                            [&](HostBatch *hb) { return dhts_bam_batch_fetch(c, &b, g->colmask, hb->arena, hb->cap, &hb->b) == 0; },
                            [&](HostBatch *hb, int sl) { return dhts_bam_batch_fetch_begin(c, &b, g->colmask, hb->arena, hb->cap, &hb->b, sl) == 0; },
                            [&](int sl) { return dhts_bam_batch_fetch_wait(c, sl) == 0; }, build_qual_lut);
    for (;;) {
        if (streaming) { const int e = stream_extend(c, max_blocks, &staged_all, t_ext); if (e < 0) { fail(); return; } n_index += e; }
        const double tb0 = now_s();
        if (dhts_bam_next_batch(c, max_blocks, g->colmask, &b) != 0) { fail(); return; }
        const double tb1 = now_s(); t_gpu += tb1 - tb0; n_batches++; n_rows += b.n_rows;
        if (b.n_rows > 0) {
            HostBatch *hb = pipe.take_slot(src);
            if (!hb) break;
            const double tb2 = now_s(); t_slot += tb2 - tb1;
            if (!pipe.reserve(hb, dhts_bam_batch_host_bytes(&b, g->colmask))) { fail_with("read_bam: out of pinned host memory"); return; }
            if (!rb.begin(hb) || fetch_optional(c, g, b, hb) != 0) { fail(); return; }
            hb->n = b.n_rows; hb->status = b.status; hb->next = 0; hb->readers = 0; hb->retired = false;
            if (g->colmask & (1u << DHTS_BAM_QUAL)) n_qual[hb->b.qual_bits == 2 ? 0 : hb->b.qual_bits == 4 ? 1 : 2]++;
            if (!p->has_rows) { p->has_rows = true; p->first_v = dhts_voffset(c, b.first_rec_uoff); }
            p->end_v = dhts_voffset(c, b.end_uoff);
            if (!rb.turn(hb)) { fail(); return; }
            t_fetch += now_s() - tb2;
        }
        if (b.status != 0) { src.clean_end = b.status == 1; break; }       // end of the stream, or the silent stop at the first bad block / record (bam_reader.c:754-766)
        if (pipe.cancelled()) break;
    }
    if (!rb.flush()) { fail(); return; }
    dhts_destroy(c);
    if (trace) { uint64_t mc = 0, mb = 0; double ms = 0; dhts_debug_malloc_stats(&mc, &mb, &ms); fprintf(stderr, "[dhts] hipMalloc calls the pool could not serve so far in this process: %llu, %.2f GB, %.3f s\n", (unsigned long long)mc, 1e-9 * (double)mb, ms); }
    if (trace && (n_qual[0] + n_qual[1] + n_qual[2])) fprintf(stderr, "[dhts] producer %d QUAL over PCIe: %lld batches as 2-bit codes, %lld as 4-bit codes, %lld as characters (the batch's own alphabet: <= 4 / <= 16 / more distinct characters)\n",
                       p->rank, (long long)n_qual[0], (long long)n_qual[1], (long long)n_qual[2]);
    if (trace) fprintf(stderr, "[dhts] producer %d/%d dev %d: context %.4f s, staged at %.4f s%s, block table %.4f s, header %.4f s, open+index+header %.4f s, %lld batches %lld rows: device %.3f s, waiting for a free host slot %.3f s, read-back %.3f s, waiting for staged bytes %.3f s, %lld table extensions %.3f s, total %.3f s\n",
                       p->rank, p->world, p->device, t_created, t_staged, from_cache ? " (file still resident in HBM)" : "", t_idx, t_hdr, t_open, (long long)n_batches, (long long)n_rows, t_gpu, t_slot, t_fetch, t_ext[0], (long long)n_index, t_ext[1], now_s() - t_start);
    pipe.finish(src);
}

// What init does with the region of a query, for read_bam and for bam_bin_counts: the index is required, the regions are validated on the
// bind context, the index bytes are read and turned into the file byte ranges to stage (seg_count -1: the whole file).  false: `error`.
static bool bam_region_prepare(BamBind *bind, std::vector<uint8_t> &index_bytes, std::vector<uint64_t> &seg_beg, std::vector<uint64_t> &seg_end, int64_t &seg_count, std::string &error) {
    if (bind->region.empty()) return true;
    {
        // bam_reader.c:639-668: a region needs an index; sam_itr_regarray failing reports "No reads found"
        if (!bind->has_index) { error = "Region query requires an index (.bai/.csi/.crai)"; return false; }
        int rc = dhts_bam_set_regions(bind->ctx, bind->region.c_str());          // (validated on the bind context: it holds the header)
        if (rc != 0) {
            char err[640]; snprintf(err, sizeof(err), "No reads found for region(s): %s", bind->region.c_str());
            error = rc == 1 ? err : dhts_error(bind->ctx); return false;
        }
        // the index (BAI or CSI) narrows the scan window; the device predicate decides the rows
        std::vector<uint8_t> ib;
        if (read_file(bind->index_file, ib) && ib.size() >= 4 && (memcmp(ib.data(), "BAI\1", 4) == 0 || memcmp(ib.data(), "CSI\1", 4) == 0 || (ib[0] == 0x1f && ib[1] == 0x8b))) index_bytes.swap(ib);
        // only the index windows are staged (the reference seeks to them): byte ranges from the bind context, which holds the header
        if (!index_bytes.empty() && env_sparse()) {
            seg_beg.resize(4096); seg_end.resize(4096);
            if (dhts_bam_region_segments(bind->ctx, index_bytes.data(), index_bytes.size(), seg_beg.data(), seg_end.data(), 4096, &seg_count) != 0) seg_count = -1;   // fall back to the whole file
        }
    }
    return true;
}

// several GPUs on one file, every rank done: every rank's last record must end exactly where the next rank's first record begins
static void bam_handoff_check(const BamScan *g, std::string &error) {
    const Shard *prev = nullptr; bool prev_clean = false;
    if (g->pipe.n_workers > 1) for (auto s : g->pipe.src) if (!s->clean_end && error.empty())
        error = "read_bam: the stream ended on an error inside one GPU's block range; rerun with DHTS_THREADS=1 for the reference's rows-before-the-error result";
    for (size_t k = 0; k < g->shard.size(); k++) {
        const Shard *p = &g->shard[k]; const bool clean = g->pipe.src[k]->clean_end;
        if (prev && p->has_rows && prev_clean && prev->end_v != p->first_v && error.empty()) {
            char m[256]; snprintf(m, sizeof(m), "read_bam: GPU shard hand-off mismatch between ranks %d and %d (%llx vs %llx)", prev->rank, p->rank, (unsigned long long)prev->end_v, (unsigned long long)p->first_v);
            error = m;
        }
        if (p->has_rows) { prev = p; prev_clean = clean; }
        if (!clean) break;                        // the stream ended on an error inside this rank: later ranks' rows are not reachable sequentially
    }
}

static void bam_read_global_init(duckdb_init_info info) {
    BamBind *bind = (BamBind *)API(void *, duckdb_init_get_bind_data, duckdb_init_info)(info);
    auto init_error = API(void, duckdb_init_set_error, duckdb_init_info, const char *);
    BamScan *g = new BamScan();
    g->bind = bind;
    Projection pj; map_projection(info, 0, pj); g->column_ids.swap(pj.column_ids);            // bam_reader.c:676-679
    for (const idx_t id : g->column_ids) {
        if (id < DHTS_BAM_CORE_COUNT) g->colmask |= 1u << id;
        int sl = -1;
        if (bind->standard_tags && id >= DHTS_BAM_CORE_COUNT && id < (idx_t)(DHTS_BAM_CORE_COUNT + dhts_bam_std_tag_count())) {
            const int32_t tid_ = (int32_t)(id - DHTS_BAM_CORE_COUNT);
            for (size_t k = 0; k < g->tag_ids.size(); k++) if (g->tag_ids[k] == tid_) sl = (int)k;
            if (sl < 0) { sl = (int)g->tag_ids.size(); g->tag_ids.push_back(tid_); }
        }
        g->tag_slot.push_back(sl);
        if (bind->auxiliary_tags && id == bind->aux_col_idx) g->want_aux = true;
    }
    { std::string rg_error; if (!bam_region_prepare(bind, g->index_bytes, g->seg_beg, g->seg_end, g->seg_count, rg_error)) { init_error(info, rg_error.c_str()); delete g; return; } }
    // sequential mode unless the user asks for parallel fill (bam_reader.c:577-585: the reference goes parallel only with an index)
    const int thr = env_fill_threads();
    std::vector<int> devs = device_list();
    if (!bind->region.empty()) devs.resize(1);          // an index window is one short scan: a single device serves it
    if (dhts_bam_is_text(bind->ctx) != 0) devs.resize(1);   // SAM / FASTQ / FASTA text is one sequential scan (the C ABI refuses shards of it)
    g->pipe.init(devs.size(), 3, thr, dhts_host_alloc, dhts_host_free, nullptr);       // (a producer destroys its own context: the sources own none)
    for (size_t k = 0; k < devs.size(); k++) { Shard sh; sh.device = devs[k]; sh.rank = (int)k; sh.world = (int)devs.size(); g->shard.push_back(sh); }
    if (devs.size() > 1) g->pipe.on_all_done = [g](std::string &error) { bam_handoff_check(g, error); };
    for (size_t k = 0; k < devs.size(); k++) g->pipe.start(k, [g, k] { producer_main(g, k); });
    API(void, duckdb_init_set_max_threads, duckdb_init_info, idx_t)(info, (idx_t)thr);
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, g, destroy_global);
}

static void bam_read_local_init(duckdb_init_info info) {
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, new BamLocal(), destroy_local);
}

// rows [s, s + take) of a host batch -> rows [row_count, row_count + take) of the output chunk
static void bam_fill(const BamBind *bind, const BamScan *g, BamLocal *l, const HostBatch *hb, int64_t s, idx_t take, duckdb_data_chunk output, idx_t row_count) {
    auto get_vec = API(duckdb_vector, duckdb_data_chunk_get_vector, duckdb_data_chunk, idx_t);
    auto get_data = API(void *, duckdb_vector_get_data, duckdb_vector);
    auto assign_len = API(void, duckdb_vector_assign_string_element_len, duckdb_vector, idx_t, const char *, idx_t);
    const dhts_bam_batch &b = hb->b;
    for (size_t ci = 0; ci < g->column_ids.size(); ci++) {
        duckdb_vector vec = get_vec(output, ci);
        // strings of <= 12 bytes are written in place (no call, no heap); longer ones are copied into the vector's heap by the engine
        auto put_str = [&](const dhts_strcol &h) {
            duckdb_string_t *d = (duckdb_string_t *)get_data(vec) + row_count;
            for (idx_t r = 0; r < take; r++) { const char *p = (const char *)h.bytes + h.off[s + r]; const uint32_t n = h.len[s + r]; if (!inl_string(d + r, p, n)) assign_len(vec, row_count + r, p, n); } };
        auto put_name = [&](const int32_t *ids) {
            duckdb_string_t *d = (duckdb_string_t *)get_data(vec) + row_count;
            for (idx_t r = 0; r < take; r++) {
                const int32_t t = ids[s + r];
                if (t < 0) d[r] = bind->star_inl; else if (bind->ref_is_inl[t]) d[r] = bind->ref_inl[t];
                else { const char *nm = bind->hdr.ref_name[t]; assign_len(vec, row_count + r, nm, strlen(nm)); }
            } };
        switch (g->column_ids[ci]) {
        case DHTS_BAM_QNAME: put_str(b.qname); break;
        case DHTS_BAM_FLAG: memcpy((uint16_t *)get_data(vec) + row_count, b.flag + s, take * 2); break;
        case DHTS_BAM_RNAME: put_name(b.tid); break;
        case DHTS_BAM_POS: memcpy((int64_t *)get_data(vec) + row_count, b.pos + s, take * 8); break;
        case DHTS_BAM_MAPQ: memcpy((int32_t *)get_data(vec) + row_count, b.mapq + s, take * 4); break;
        case DHTS_BAM_CIGAR: put_str(b.cigar); break;
        case DHTS_BAM_RNEXT: put_name(b.mtid); break;
        case DHTS_BAM_PNEXT: memcpy((int64_t *)get_data(vec) + row_count, b.pnext + s, take * 8); break;
        case DHTS_BAM_TLEN: memcpy((int64_t *)get_data(vec) + row_count, b.tlen + s, take * 8); break;
        case DHTS_BAM_SEQ:
            if (!b.seq_packed) { put_str(b.seq); break; }
            {   // the batch carries the file's 4-bit codes: expand here (seq_to_string, bam_reader.c:560-575; "*" for an empty SEQ)
                duckdb_string_t *d = (duckdb_string_t *)get_data(vec) + row_count;
                for (idx_t r = 0; r < take; r++) {
                    const uint32_t n = b.seq.len[s + r];
                    if (n == 0) { inl_string(d + r, "*", 1); continue; }
                    if (l->seq_tmp.size() < (size_t)n + 32) l->seq_tmp.resize((size_t)n + 32 + n / 2);
                    expand_seq(b.seq.bytes + b.seq.off[s + r], n, l->seq_tmp.data());
                    if (!inl_string(d + r, l->seq_tmp.data(), n)) assign_len(vec, row_count + r, l->seq_tmp.data(), n);
                }
            }
            break;
        case DHTS_BAM_QUAL:
            if (!b.qual_bits) { put_str(b.qual); break; }
            {   // the batch carries codes of its own alphabet: expand here (qual_to_string's characters, bam_reader.c:577-600, were made on the device)
                duckdb_string_t *d = (duckdb_string_t *)get_data(vec) + row_count;
                const uint8_t *stream = b.qual.bytes + 16; const uint32_t *lut = hb->qual_lut.data();
                for (idx_t r = 0; r < take; r++) {
                    const uint32_t n = b.qual.len[s + r];
                    if (l->seq_tmp.size() < (size_t)n + 40) l->seq_tmp.resize((size_t)n + 40 + n / 2);
                    expand_qual(stream, b.qual_bits, lut, b.qual.off[s + r], n, l->seq_tmp.data(), l->qual_tmp);
                    if (!inl_string(d + r, l->seq_tmp.data(), n)) assign_len(vec, row_count + r, l->seq_tmp.data(), n);
                }
            }
            break;
        case DHTS_BAM_READ_GROUP_ID: {
            duckdb_string_t *d = (duckdb_string_t *)get_data(vec) + row_count;
            for (idx_t r = 0; r < take; r++) {
                int64_t q = s + (int64_t)r;
                if ((b.rg_valid[q >> 6] >> (q & 63)) & 1) { const char *p = (const char *)b.rg.bytes + b.rg.off[q]; const uint32_t n = b.rg.len[q]; if (!inl_string(d + r, p, n)) assign_len(vec, row_count + r, p, n); }
                else set_null(vec, row_count + r);
            }
            break;
        }
        case DHTS_BAM_SAMPLE_ID:
            for (idx_t r = 0; r < take; r++) {
                int64_t q = s + (int64_t)r; int32_t k = b.rg_idx[q];
                const char *sm = (((b.rg_valid[q >> 6] >> (q & 63)) & 1) && k >= 0) ? bind->hdr.rg_sm[k] : nullptr;
                if (sm) assign_len(vec, row_count + r, sm, strlen(sm)); else set_null(vec, row_count + r);
            }
            break;
        default: {
            if (g->want_aux && g->column_ids[ci] == bind->aux_col_idx) {               // bam_reader.c:967-1027
                // no tags: NULL, entry {size, 0}; the pairs go in as the attributes map of the text readers does
                const dhts_tabix_map m = {hb->aux_off.data(), hb->aux_valid.data(), hb->aux_koff.size() - 1, hb->aux_koff.data(), (const uint8_t *)hb->aux_keys.data(), hb->aux_keys.size(),
                                          hb->aux_voff.data(), (const uint8_t *)hb->aux_vals.data(), hb->aux_vals.size()};
                fill_col(vec, COL_MAP, dhts_col(), &m, s, take, row_count);
                break;
            }
            const int sl = g->tag_slot[ci];
            if (sl < 0) break;                                 // unknown ids (e.g. a row-id pseudo column) write nothing, like the reference's default arm
            const HostTag &h = hb->tags[sl];
            char nm[3], ty, sub; dhts_bam_std_tag_info(g->tag_ids[sl], nm, &ty, &sub);
            if (ty == 'i') {                                    // bam_reader.c:946-950
                memcpy((int64_t *)get_data(vec) + row_count, h.fixed.data() + s, take * 8);
                for (idx_t r = 0; r < take; r++) if (!h.valid[s + r]) set_null(vec, row_count + r);
            } else if (ty == 'B') {                             // bam_assign_list_int / _double bam_reader.c:106-138
                const ListFrame f = list_entries(vec, h.off.data(), h.valid.data(), s, take, row_count, true);     // absent tag: set_null only, the entry is left untouched (bam_reader.c:927-930)
                if (f.c1 > f.c0) memcpy((int64_t *)get_data(f.child) + f.base, h.child.data() + f.c0, (size_t)(f.c1 - f.c0) * 8);
            } else {
                for (idx_t r = 0; r < take; r++) {
                    if (h.valid[s + r]) assign_len(vec, row_count + r, (const char *)h.bytes.data() + h.off[s + r], h.off[s + r + 1] - h.off[s + r]);
                    else set_null(vec, row_count + r);
                }
            }
            break;
        }
        }
    }
}

static void bam_read_function(duckdb_function_info info, duckdb_data_chunk output) {
    BamBind *bind = (BamBind *)API(void *, duckdb_function_get_bind_data, duckdb_function_info)(info);
    BamScan *g = (BamScan *)API(void *, duckdb_function_get_init_data, duckdb_function_info)(info);
    BamLocal *l = (BamLocal *)API(void *, duckdb_function_get_local_init_data, duckdb_function_info)(info);
    auto set_size = API(void, duckdb_data_chunk_set_size, duckdb_data_chunk, idx_t);
    if (!l || !g) { set_size(output, 0); return; }                                            // bam_reader.c:730-733
    std::string err;
    const int64_t n = g->pipe.fill_chunk(l->at, API(idx_t, duckdb_vector_size, void)(), err, [&](const HostBatch &hb, int64_t s, idx_t take, idx_t row_count) { bam_fill(bind, g, l, &hb, s, take, output, row_count); });
    if (n < 0) API(void, duckdb_function_set_error, duckdb_function_info, const char *)(info, err.c_str());
    set_size(output, n < 0 ? 0 : (idx_t)n);
}

extern "C" __attribute__((visibility("default"))) void register_read_bam_function(duckdb_connection connection) {                      // bam_reader.c:1044-1068
    register_table_function(connection, "read_bam", {{"region", DUCKDB_TYPE_VARCHAR}, {"index_path", DUCKDB_TYPE_VARCHAR}, {"reference", DUCKDB_TYPE_VARCHAR}, {"standard_tags", DUCKDB_TYPE_BOOLEAN}, {"auxiliary_tags", DUCKDB_TYPE_BOOLEAN}},
                            bam_read_bind, bam_read_global_init, bam_read_local_init, bam_read_function, true);
}
