// duckdb_ext.cpp -- DuckDB C-API extension surface (outer drop-in boundary) over the MI355X scan path.
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
// Scan mode: the reference's sequential mode (i): all records in file order including
// unplaced reads, full 2048-row chunks except the last.  region, standard_tags and auxiliary_tags are served by
// the GPU path; CRAM / SAM text input fails at bind with the reference's header error.
//
// Linkage (src/duckhts.c:13-16,54-55): register_read_bam_function / register_read_bcf_function have external
// linkage and read the DuckDB API through the global `duckdb_ext_api`, exactly like the reference's readers
// (DUCKDB_EXTENSION_EXTERN, duckdb_extension.h:1161), so a reference-built src/duckhts.c links against them
// unchanged.  This file also carries a weak definition of that global and a weak duckhts_init_c_api, which
// are what a stand-alone libduckhts_amd.so uses; strong definitions from src/duckhts.c win at link time.
#include "../../include/duckhts_amd.h"
#include "../../include/duckhts_extension.h"

#include <stdio.h>
#include <time.h>
#include <stdlib.h>
#include <string.h>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <cmath>
#include <string>
#include <thread>
#include <vector>

// duckdb_ext_api_v1 viewed as an array of function pointers (slot numbers: include/duckdb_abi_slots.h).  Weak: the definition
// DUCKDB_EXTENSION_GLOBAL emits in a reference-built src/duckhts.c (duckdb_extension.h:1151) replaces it.
extern "C" __attribute__((visibility("default"), weak)) const void *duckdb_ext_api[DUCKDB_ABI_V120_NSLOTS] = {nullptr};

#define API(ret, name, ...) ((ret(*)(__VA_ARGS__))duckdb_ext_api[SLOT_##name])

// what DUCKDB_EXTENSION_API_INIT does (`duckdb_ext_api = *res`, duckdb_extension.h:1153-1158), for hosts that hold the table
extern "C" __attribute__((visibility("default"))) void dhts_set_duckdb_api(const void *api_table) {
    if (api_table) memcpy((void *)duckdb_ext_api, api_table, sizeof(void *) * DUCKDB_ABI_V120_NSLOTS);
}

extern "C" void dhts_debug_malloc_stats(uint64_t *calls, uint64_t *bytes, double *seconds);
static double now_s() { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec; }

static inline void set_null(duckdb_vector vec, idx_t row) {           // src/bam_reader.c:38-42
    API(void, duckdb_vector_ensure_validity_writable, duckdb_vector)(vec);
    uint64_t *v = API(uint64_t *, duckdb_vector_get_validity, duckdb_vector)(vec);
    v[row / 64] &= ~((uint64_t)1 << (row % 64));
}

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
struct HostBatch {
    void *arena = nullptr; uint64_t cap = 0;
    dhts_bam_batch b;                 // HOST pointers for the core columns
    int64_t n = 0; int status = 0;
    std::vector<HostTag> tags;
    std::vector<uint8_t> aux_valid; std::vector<uint32_t> aux_off; std::vector<std::string> aux_key, aux_val;
    std::vector<uint32_t> qual_lut;   // QUAL as 2- / 4-bit codes (dhts_bam_batch.qual_bits): code byte -> its 4 / 2 characters, built when the batch's bytes have landed
    // parallel mode
    int64_t next = 0; int readers = 0; bool retired = false;
};
struct Producer {
    int device = 0, rank = 0, world = 1;
    std::thread th;
    std::deque<HostBatch *> ready; std::vector<HostBatch *> free_slots; std::vector<HostBatch *> all;
    bool done = false;
    // where this rank's rows begin and end in the file, as BGZF virtual offsets: adjacent ranks must meet exactly (SURVEY 8(e) hand-off)
    bool has_rows = false, clean_end = false; uint64_t first_v = 0, end_v = 0;
};
struct BamScan {
    BamBind *bind = nullptr;
    std::vector<idx_t> column_ids; uint32_t colmask = 0;
    std::vector<int32_t> tag_ids; std::vector<int> tag_slot; bool want_aux = false;
    int n_workers = 1;
    std::mutex mu; std::condition_variable cv_ready, cv_free;
    std::vector<Producer *> prod; size_t cur_prod = 0;
    std::string error; bool cancel = false, handoff_checked = false;
    std::vector<uint8_t> index_bytes;
    std::vector<uint64_t> seg_beg, seg_end; int64_t seg_count = -1;      // region query: the file byte ranges to stage (-1: the whole file)
    ~BamScan() {
        { std::lock_guard<std::mutex> lk(mu); cancel = true; }
        cv_free.notify_all(); cv_ready.notify_all();
        for (auto p : prod) { if (p->th.joinable()) p->th.join(); for (auto hb : p->all) { dhts_host_free(hb->arena); delete hb; } delete p; }
    }
};
struct BamLocal {
    std::vector<char> seq_tmp;         // packed SEQ expands here before it is assigned
    std::vector<char> qual_tmp;        // packed QUAL: a row that starts inside a code byte is expanded here first
    bool done = false;
    HostBatch *cur = nullptr; Producer *cur_owner = nullptr; int64_t pos = 0, end = 0;     // rows [pos, end) of `cur` are this worker's
};

static void destroy_bind(void *p) { BamBind *b = (BamBind *)p; if (!b) return; if (b->ctx) dhts_destroy(b->ctx); delete b; }
static void destroy_local(void *p) { delete (BamLocal *)p; }
static void destroy_global(void *p) { delete (BamScan *)p; }

static char *get_named_varchar(duckdb_bind_info info, const char *name) {
    duckdb_value v = API(duckdb_value, duckdb_bind_get_named_parameter, duckdb_bind_info, const char *)(info, name);
    char *s = nullptr;
    if (v && !API(bool, duckdb_is_null_value, duckdb_value)(v)) s = API(char *, duckdb_get_varchar, duckdb_value)(v);
    if (v) API(void, duckdb_destroy_value, duckdb_value *)(&v);
    return s;
}
static int get_named_bool(duckdb_bind_info info, const char *name) {
    duckdb_value v = API(duckdb_value, duckdb_bind_get_named_parameter, duckdb_bind_info, const char *)(info, name);
    int r = 0;
    if (v && !API(bool, duckdb_is_null_value, duckdb_value)(v)) r = API(bool, duckdb_get_bool, duckdb_value)(v) ? 1 : 0;
    if (v) API(void, duckdb_destroy_value, duckdb_value *)(&v);
    return r;
}
static bool file_exists(const std::string &p) { FILE *f = fopen(p.c_str(), "rb"); if (!f) return false; fclose(f); return true; }
static std::vector<int> device_list() {
    std::vector<int> d;
    if (const char *e = getenv("DHTS_DEVICES")) { for (const char *q = e; *q;) { char *end; long v = strtol(q, &end, 10); if (end == q) break; d.push_back((int)v); q = *end ? end + 1 : end; } }
    if (d.empty()) d.push_back(getenv("DHTS_DEVICE") ? atoi(getenv("DHTS_DEVICE")) : 0);
    return d;
}
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

static void bam_read_bind(duckdb_bind_info info) {
    auto set_error = API(void, duckdb_bind_set_error, duckdb_bind_info, const char *);
    auto dfree = API(void, duckdb_free, void *);
    duckdb_value pv = API(duckdb_value, duckdb_bind_get_parameter, duckdb_bind_info, idx_t)(info, 0);
    char *file_path = API(char *, duckdb_get_varchar, duckdb_value)(pv);
    API(void, duckdb_destroy_value, duckdb_value *)(&pv);
    if (!file_path || strlen(file_path) == 0) {
        set_error(info, "read_bam requires a file path");                         // bam_reader.c:416
        if (file_path) dfree(file_path);
        return;
    }
    char *region = get_named_varchar(info, "region");
    char *index_path = get_named_varchar(info, "index_path");
    char *reference = get_named_varchar(info, "reference");
    int standard_tags = get_named_bool(info, "standard_tags"), auxiliary_tags = get_named_bool(info, "auxiliary_tags");
    BamBind *b = new BamBind();
    b->path = file_path;
    std::string idx = index_path ? index_path : "";
    // parse_regions (bam_reader.c:319-345) splits with strtok: a string without a non-empty token ('' or ',,') is no region at all
    bool has_region = false;
    for (const char *q = region; q && *q; q++) if (*q != ',') { has_region = true; break; }
    std::string region_copy = has_region ? region : "";
    dfree(file_path); if (region) dfree(region); if (index_path) dfree(index_path); if (reference) dfree(reference);

    char err[768];
    if (!file_exists(b->path)) {
        snprintf(err, sizeof(err), "Failed to open SAM/BAM/CRAM file: %s", b->path.c_str());   // bam_reader.c:446
        set_error(info, err); delete b; return;
    }
    static const bool trace_bind = getenv("DHTS_TRACE") != nullptr;
    const double tb0 = now_s();
    b->ctx = dhts_create(device_list()[0]);
    const double tb1 = now_s();
    if (!b->ctx) { set_error(info, "read_bam: no MI355X (gfx950) device available; this build has no CPU fallback"); destroy_bind(b); return; }
    // like the reference, bind reads the header only (sam_open + sam_hdr_read, bam_reader.c:441-461): the head of the file is staged,
    // four times more whenever the header turns out to be longer.  The scan stages the file itself (bam_read_global_init).
    bool hdr_ok = false;
    for (uint64_t head = 1u << 20;; head *= 4) {
        if (dhts_open_path_range(b->ctx, b->path.c_str(), 0, head) != 0) {
            snprintf(err, sizeof(err), "Failed to open SAM/BAM/CRAM file: %s", b->path.c_str());
            set_error(info, err); destroy_bind(b); return;
        }
        const bool whole = dhts_resident_bytes(b->ctx) < head;
        if (dhts_bgzf_index(b->ctx) > 0 && dhts_bam_open(b->ctx) == 0 && dhts_bam_header_get(b->ctx, &b->hdr) == 0) { hdr_ok = true; break; }
        if (whole || head >= (1ull << 34)) break;
    }
    if (!hdr_ok) {
        set_error(info, "Failed to read SAM/BAM/CRAM header");                    // bam_reader.c:461 (also what SAM/CRAM input gets here)
        destroy_bind(b); return;
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
    if (has_region) b->region = region_copy;
    b->standard_tags = standard_tags; b->auxiliary_tags = auxiliary_tags;

    auto mk = API(duckdb_logical_type, duckdb_create_logical_type, int);
    auto add = API(void, duckdb_bind_add_result_column, duckdb_bind_info, const char *, duckdb_logical_type);
    auto rm = API(void, duckdb_destroy_logical_type, duckdb_logical_type *);
    duckdb_logical_type t_varchar = mk(DUCKDB_TYPE_VARCHAR), t_int = mk(DUCKDB_TYPE_INTEGER), t_big = mk(DUCKDB_TYPE_BIGINT), t_us = mk(DUCKDB_TYPE_USMALLINT);
    add(info, "QNAME", t_varchar); add(info, "FLAG", t_us); add(info, "RNAME", t_varchar); add(info, "POS", t_big); add(info, "MAPQ", t_int);   // bam_reader.c:514-526
    add(info, "CIGAR", t_varchar); add(info, "RNEXT", t_varchar); add(info, "PNEXT", t_big); add(info, "TLEN", t_big); add(info, "SEQ", t_varchar);
    add(info, "QUAL", t_varchar); add(info, "READ_GROUP_ID", t_varchar); add(info, "SAMPLE_ID", t_varchar);
    if (b->standard_tags) {                                                                     // bam_reader.c:527-537 + bam_std_tag_type 88-104
        auto mklist = API(duckdb_logical_type, duckdb_create_list_type, duckdb_logical_type);
        duckdb_logical_type t_list = mklist(t_big);
        for (int i = 0; i < dhts_bam_std_tag_count(); i++) {
            char nm[3], ty, sub; dhts_bam_std_tag_info(i, nm, &ty, &sub);
            add(info, nm, ty == 'i' ? t_big : ty == 'B' ? t_list : t_varchar);
        }
        rm(&t_list);
    }
    if (b->auxiliary_tags) {                                                                    // bam_reader.c:539-548
        duckdb_logical_type t_map = API(duckdb_logical_type, duckdb_create_map_type, duckdb_logical_type, duckdb_logical_type)(t_varchar, t_varchar);
        b->aux_col_idx = DHTS_BAM_CORE_COUNT + (b->standard_tags ? (idx_t)dhts_bam_std_tag_count() : 0);
        add(info, "AUXILIARY_TAGS", t_map);
        rm(&t_map);
    }
    rm(&t_varchar); rm(&t_int); rm(&t_big); rm(&t_us);
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
        hb->aux_key.assign(ne, std::string()); hb->aux_val.assign(ne, std::string());
        char tmp[64];
        for (size_t i = 0; i < ne; i++) {
            char kb[3] = {(char)(key[i] & 0xff), (char)(key[i] >> 8), 0};
            hb->aux_key[i] = kb;
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
            hb->aux_val[i] = v.c_str();                              // C-string semantics: cut at the first NUL
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
static void producer_main(BamScan *g, Producer *p) {
    BamBind *bind = g->bind;
    static const bool trace = getenv("DHTS_TRACE") != nullptr;       // stage timings of every producer on stderr
    const double t_start = now_s(); double t_open = 0, t_gpu = 0, t_fetch = 0, t_slot = 0, t_wait = 0, t_index = 0; int64_t n_batches = 0, n_rows = 0, n_index = 0;
    auto fail_with = [&](const std::string &msg) {
        std::lock_guard<std::mutex> lk(g->mu);
        if (g->error.empty()) g->error = msg;
        p->done = true; g->cv_ready.notify_all();
    };
    // the producer, the staging readers it starts and the pinned arenas it allocates live on the NUMA node of its GPU
    const int numa_rc = dhts_bind_thread_near_device(p->device);
    if (trace) fprintf(stderr, "[dhts] producer %d: device %d on NUMA node %d (%s)\n", p->rank, p->device, dhts_device_numa_node(p->device), numa_rc == 0 ? "bound" : numa_rc == 1 ? "not bound" : "bind failed");
    dhts_ctx *c = dhts_create(p->device);
    if (!c) { fail_with("read_bam: no MI355X (gfx950) device available; this build has no CPU fallback"); return; }
    dhts_set_super_blocks(c, 196608);                    // a scratch the device pool keeps from query to query (29 GB instead of 67 GB for a 10 GB file)
    { static const bool env_qraw = getenv("DHTS_QUAL_PACKED") && atoi(getenv("DHTS_QUAL_PACKED")) == 0; dhts_bam_set_qual_packed(c, env_qraw ? 0 : 1); }         // QUAL crosses PCIe as 2- / 4-bit codes when the batch holds at most 4 / 16 different characters
    { static const bool env_unpacked = getenv("DHTS_SEQ_PACKED") && atoi(getenv("DHTS_SEQ_PACKED")) == 0; dhts_bam_set_seq_packed(c, env_unpacked ? 0 : 1); }   // SEQ crosses PCIe as 4-bit codes, the fill threads expand it
    const double t_created = now_s() - t_start; double t_staged = 0;
    int rc;
    // a plain whole-file scan on one device starts decoding while the file is still being staged: the block table is built over the
    // resident prefix and extended as more bytes arrive (DHTS_STREAM=0 stages the whole file first)
    static const bool env_nostream = getenv("DHTS_STREAM") && atoi(getenv("DHTS_STREAM")) == 0;
    const bool streaming = p->world == 1 && bind->region.empty() && !env_nostream && (dhts_bam_is_text(bind->ctx) == 0 || dhts_bam_is_text(bind->ctx) % 2 != 0);   // (uncompressed text -- 2, 4, 6 -- is staged first)
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
    if (rc == 0 && streaming) {
        // the header needs the first blocks only: start with what the bind saw, four times more whenever that is not enough
        uint64_t want = bind->header_bytes + (32u << 20);
        for (;;) {
            const int64_t f = dhts_stage_wait(c, want, &staged_all);
            if (f < 0) { rc = -1; break; }
            if (dhts_bgzf_index_staged(c) > 0 && dhts_bam_open(c) == 0) break;
            if (staged_all) { rc = -1; break; }
            want *= 4;
        }
    }
    if (rc != 0) { std::string m = std::string("Failed to open SAM/BAM/CRAM file: ") + bind->path; dhts_destroy(c); fail_with(m); return; }
    t_open = now_s() - t_start;
    dhts_bam_set_tag_columns(c, g->tag_ids.data(), (int32_t)g->tag_ids.size());
    dhts_bam_set_aux_map(c, g->want_aux ? 1 : 0, bind->standard_tags);
    if (!bind->region.empty()) {
        rc = dhts_bam_set_regions(c, bind->region.c_str());
        if (rc == 0 && !g->index_bytes.empty()) rc = dhts_bam_load_index(c, g->index_bytes.data(), g->index_bytes.size());
    } else rc = dhts_bam_set_regions(c, nullptr);
    if (rc == 0 && p->world > 1) rc = dhts_bam_set_file_shard(c, p->rank, p->world);
    else if (rc == 0 && bind->region.empty()) rc = dhts_bam_rewind(c);
    if (rc != 0) { std::string m = dhts_error(c); dhts_destroy(c); fail_with(m); return; }
    static const int64_t env_mb = getenv("DHTS_BATCH_BLOCKS") ? atoll(getenv("DHTS_BATCH_BLOCKS")) : 0;
    const int64_t max_blocks = env_mb > 0 ? env_mb : 4096;       // ~270 MB of inflated stream per batch: the engine gets its first chunk early and the stages overlap
    HostBatch *pending = nullptr; int pending_slot = 0, slot_no = 0;
    int64_t n_qual[3] = {0, 0, 0};                               // batches whose QUAL crossed PCIe as 2-bit codes / 4-bit codes / characters
    auto publish = [&](HostBatch *hb, int sl) -> bool {
        if (dhts_bam_batch_fetch_wait(c, sl) != 0) return false;
        build_qual_lut(hb);
        { std::lock_guard<std::mutex> lk(g->mu); p->ready.push_back(hb); }
        g->cv_ready.notify_all();
        return true;
    };
    for (;;) {
        dhts_bam_batch b;
        if (streaming && !staged_all && dhts_blocks_ahead(c) < max_blocks) {
            // not enough known blocks for a full batch: wait for (at least) another 128 MiB of the file, then extend the block table
            const double tw0 = now_s();
            int64_t f = dhts_stage_wait(c, 0, &staged_all);
            if (f >= 0 && !staged_all) f = dhts_stage_wait(c, (uint64_t)f + (128u << 20), &staged_all);
            const double tw1 = now_s(); t_wait += tw1 - tw0;
            if (f < 0 || dhts_bgzf_index_staged(c) < 0) { std::string m = dhts_error(c); dhts_destroy(c); fail_with(m); return; }
            t_index += now_s() - tw1; n_index++;
        }
        const double tb0 = now_s();
        if (dhts_bam_next_batch(c, max_blocks, g->colmask, &b) != 0) { std::string m = dhts_error(c); dhts_destroy(c); fail_with(m); return; }
        const double tb1 = now_s(); t_gpu += tb1 - tb0; n_batches++; n_rows += b.n_rows;
        if (b.n_rows > 0) {
            HostBatch *hb = nullptr;
            {
                std::unique_lock<std::mutex> lk(g->mu);
                g->cv_free.wait(lk, [&] { return g->cancel || !p->free_slots.empty(); });
                if (g->cancel) break;
                hb = p->free_slots.back(); p->free_slots.pop_back();
            }
            const double tb2 = now_s(); t_slot += tb2 - tb1;
            const uint64_t need = dhts_bam_batch_host_bytes(&b, g->colmask);
            if (need > hb->cap) { dhts_host_free(hb->arena); hb->arena = dhts_host_alloc(need); hb->cap = hb->arena ? need : 0; }
            // the read-back of this batch runs on a copy stream while the next batch is scanned: the batch is handed to the fill threads one
            // turn later, when its bytes have had a whole scan's time to cross PCIe (DHTS_OVERLAP_READBACK=0: copy, wait, hand over)
            static const bool env_serial = getenv("DHTS_OVERLAP_READBACK") && atoi(getenv("DHTS_OVERLAP_READBACK")) == 0;
            const int frc = env_serial ? dhts_bam_batch_fetch(c, &b, g->colmask, hb->arena, hb->cap, &hb->b) : dhts_bam_batch_fetch_begin(c, &b, g->colmask, hb->arena, hb->cap, &hb->b, slot_no);
            if ((need && !hb->arena) || frc != 0 || fetch_optional(c, g, b, hb) != 0) {
                std::string m = hb->arena || !need ? dhts_error(c) : "read_bam: out of pinned host memory"; dhts_destroy(c); fail_with(m); return;
            }
            hb->n = b.n_rows; hb->status = b.status; hb->next = 0; hb->readers = 0; hb->retired = false;
            if (g->colmask & (1u << DHTS_BAM_QUAL)) n_qual[hb->b.qual_bits == 2 ? 0 : hb->b.qual_bits == 4 ? 1 : 2]++;
            if (!p->has_rows) { p->has_rows = true; p->first_v = dhts_voffset(c, b.first_rec_uoff); }
            p->end_v = dhts_voffset(c, b.end_uoff);
            if (pending && !publish(pending, pending_slot)) { std::string m = dhts_error(c); dhts_destroy(c); fail_with(m); return; }
            pending = nullptr;
            if (env_serial) { build_qual_lut(hb); std::lock_guard<std::mutex> lk(g->mu); p->ready.push_back(hb); }
            else { pending = hb; pending_slot = slot_no; slot_no ^= 1; }
            if (env_serial) g->cv_ready.notify_all();
            t_fetch += now_s() - tb2;
        }
        if (b.status != 0) { p->clean_end = b.status == 1; break; }       // end of the stream, or the silent stop at the first bad block / record (bam_reader.c:754-766)
        { std::lock_guard<std::mutex> lk(g->mu); if (g->cancel) break; }
    }
    if (pending && !publish(pending, pending_slot)) { std::string m = dhts_error(c); dhts_destroy(c); fail_with(m); return; }
    dhts_destroy(c);
    if (trace) { uint64_t mc = 0, mb = 0; double ms = 0; dhts_debug_malloc_stats(&mc, &mb, &ms); fprintf(stderr, "[dhts] hipMalloc calls the pool could not serve so far in this process: %llu, %.2f GB, %.3f s\n", (unsigned long long)mc, 1e-9 * (double)mb, ms); }
    if (trace && (n_qual[0] + n_qual[1] + n_qual[2])) fprintf(stderr, "[dhts] producer %d QUAL over PCIe: %lld batches as 2-bit codes, %lld as 4-bit codes, %lld as characters (the batch's own alphabet: <= 4 / <= 16 / more distinct characters)\n",
                       p->rank, (long long)n_qual[0], (long long)n_qual[1], (long long)n_qual[2]);
    if (trace) fprintf(stderr, "[dhts] producer %d/%d dev %d: context %.4f s, staged at %.4f s%s, block table %.4f s, header %.4f s, open+index+header %.4f s, %lld batches %lld rows: device %.3f s, waiting for a free host slot %.3f s, read-back %.3f s, waiting for staged bytes %.3f s, %lld table extensions %.3f s, total %.3f s\n",
                       p->rank, p->world, p->device, t_created, t_staged, from_cache ? " (file still resident in HBM)" : "", t_idx, t_hdr, t_open, (long long)n_batches, (long long)n_rows, t_gpu, t_slot, t_fetch, t_wait, (long long)n_index, t_index, now_s() - t_start);
    { std::lock_guard<std::mutex> lk(g->mu); p->done = true; }
    g->cv_ready.notify_all();
}

static void bam_read_global_init(duckdb_init_info info) {
    BamBind *bind = (BamBind *)API(void *, duckdb_init_get_bind_data, duckdb_init_info)(info);
    auto init_error = API(void, duckdb_init_set_error, duckdb_init_info, const char *);
    BamScan *g = new BamScan();
    g->bind = bind;
    idx_t n = API(idx_t, duckdb_init_get_column_count, duckdb_init_info)(info);               // bam_reader.c:676-679
    for (idx_t i = 0; i < n; i++) {
        idx_t id = API(idx_t, duckdb_init_get_column_index, duckdb_init_info, idx_t)(info, i);
        g->column_ids.push_back(id);
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
    if (!bind->region.empty()) {
        // bam_reader.c:639-668: a region needs an index; sam_itr_regarray failing reports "No reads found"
        if (!bind->has_index) { init_error(info, "Region query requires an index (.bai/.csi/.crai)"); delete g; return; }
        int rc = dhts_bam_set_regions(bind->ctx, bind->region.c_str());          // (validated on the bind context: it holds the header)
        if (rc != 0) {
            char err[640]; snprintf(err, sizeof(err), "No reads found for region(s): %s", bind->region.c_str());
            init_error(info, rc == 1 ? err : dhts_error(bind->ctx)); delete g; return;
        }
        // the index (BAI or CSI) narrows the scan window; the device predicate decides the rows
        FILE *f = fopen(bind->index_file.c_str(), "rb");
        if (f) {
            std::vector<uint8_t> ib; uint8_t tmp[65536]; size_t k;
            while ((k = fread(tmp, 1, sizeof(tmp), f)) > 0) ib.insert(ib.end(), tmp, tmp + k);
            fclose(f);
            const bool known = ib.size() >= 4 && (memcmp(ib.data(), "BAI\1", 4) == 0 || memcmp(ib.data(), "CSI\1", 4) == 0 || (ib[0] == 0x1f && ib[1] == 0x8b));
            if (known) g->index_bytes.swap(ib);
        }
        // only the index windows are staged (the reference seeks to them): byte ranges from the bind context, which holds the header
        static const bool env_nosparse = getenv("DHTS_SPARSE") && atoi(getenv("DHTS_SPARSE")) == 0;
        if (!g->index_bytes.empty() && !env_nosparse) {
            g->seg_beg.resize(4096); g->seg_end.resize(4096);
            if (dhts_bam_region_segments(bind->ctx, g->index_bytes.data(), g->index_bytes.size(), g->seg_beg.data(), g->seg_end.data(), 4096, &g->seg_count) != 0) g->seg_count = -1;   // fall back to the whole file
        }
    }
    // sequential mode unless the user asks for parallel fill (bam_reader.c:577-585: the reference goes parallel only with an index)
    int thr = getenv("DHTS_THREADS") ? atoi(getenv("DHTS_THREADS")) : 1; if (thr < 1) thr = 1; if (thr > 64) thr = 64;
    g->n_workers = thr;
    std::vector<int> devs = device_list();
    if (!bind->region.empty()) devs.resize(1);          // an index window is one short scan: a single device serves it
    if (dhts_bam_is_text(bind->ctx) != 0) devs.resize(1);   // SAM / FASTQ / FASTA text is one sequential scan (the C ABI refuses shards of it)
    for (size_t k = 0; k < devs.size(); k++) {
        Producer *p = new Producer(); p->device = devs[k]; p->rank = (int)k; p->world = (int)devs.size();
        for (int q = 0; q < 3; q++) { HostBatch *hb = new HostBatch(); p->free_slots.push_back(hb); p->all.push_back(hb); }
        g->prod.push_back(p);
    }
    for (auto p : g->prod) p->th = std::thread(producer_main, g, p);
    API(void, duckdb_init_set_max_threads, duckdb_init_info, idx_t)(info, (idx_t)thr);
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, g, destroy_global);
}

static void bam_read_local_init(duckdb_init_info info) {
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, new BamLocal(), destroy_local);
}

// hands the calling worker its next run of rows: the rest of the current batch (sequential mode) or a 2048-row slice of a ready batch.
// Returns false at the end of the scan (or on a producer error: g->error).
static bool next_rows(BamScan *g, BamLocal *l, idx_t want) {
    std::unique_lock<std::mutex> lk(g->mu);
    // give back what the worker holds
    if (l->cur) {
        HostBatch *hb = l->cur; Producer *own = l->cur_owner;
        hb->readers--;
        const bool finished = g->n_workers == 1 ? true : (hb->retired && hb->readers == 0);
        if (finished) { own->free_slots.push_back(hb); g->cv_free.notify_all(); }
        l->cur = nullptr;
    }
    for (;;) {
        if (!g->error.empty()) return false;
        // ordered mode drains the producers one after the other (file order); parallel mode takes whatever is ready
        for (size_t k = 0; k < g->prod.size(); k++) {
            Producer *p = g->prod[g->n_workers == 1 ? g->cur_prod : (g->cur_prod + k) % g->prod.size()];
            while (!p->ready.empty()) {
                HostBatch *hb = p->ready.front();
                if (g->n_workers == 1) {
                    p->ready.pop_front(); hb->readers = 1;
                    l->cur = hb; l->cur_owner = p; l->pos = 0; l->end = hb->n;
                    return true;
                }
                if (hb->next >= hb->n) {            // every row is claimed: the last reader returns the slot
                    p->ready.pop_front(); hb->retired = true;
                    if (hb->readers == 0) { p->free_slots.push_back(hb); g->cv_free.notify_all(); }
                    continue;
                }
                l->cur = hb; l->cur_owner = p; l->pos = hb->next; l->end = hb->next + (int64_t)want < hb->n ? hb->next + (int64_t)want : hb->n;
                hb->next = l->end; hb->readers++;
                return true;
            }
            if (g->n_workers == 1) {
                if (p->done && p->ready.empty()) {
                    if (!p->clean_end) return false;      // the stream ended on an error inside this rank: the scan ends here, silently (bam_reader.c:754-766)
                    if (g->cur_prod + 1 < g->prod.size()) { g->cur_prod++; k = (size_t)-1; continue; }
                }
                break;
            }
        }
        bool all_done = true;
        for (auto p : g->prod) if (!p->done || !p->ready.empty()) all_done = false;
        if (all_done) {
            // several GPUs on one file: every rank's last record must end exactly where the next rank's first record begins
            if (g->prod.size() > 1 && !g->handoff_checked) {
                g->handoff_checked = true;
                const Producer *prev = nullptr;
                if (g->n_workers > 1) for (auto p : g->prod) if (!p->clean_end && g->error.empty())
                    g->error = "read_bam: the stream ended on an error inside one GPU's block range; rerun with DHTS_THREADS=1 for the reference's rows-before-the-error result";
                for (auto p : g->prod) {
                    if (prev && p->has_rows && prev->clean_end && prev->end_v != p->first_v && g->error.empty()) {
                        char m[256]; snprintf(m, sizeof(m), "read_bam: GPU shard hand-off mismatch between ranks %d and %d (%llx vs %llx)", prev->rank, p->rank, (unsigned long long)prev->end_v, (unsigned long long)p->first_v);
                        g->error = m;
                    }
                    if (p->has_rows) prev = p;
                    if (!p->clean_end) break;                 // the stream ended on an error inside this rank: later ranks' rows are not reachable sequentially
                }
                if (!g->error.empty()) return false;
            }
            return false;
        }
        g->cv_ready.wait(lk);
    }
}

static void bam_read_function(duckdb_function_info info, duckdb_data_chunk output) {
    BamBind *bind = (BamBind *)API(void *, duckdb_function_get_bind_data, duckdb_function_info)(info);
    BamScan *g = (BamScan *)API(void *, duckdb_function_get_init_data, duckdb_function_info)(info);
    BamLocal *l = (BamLocal *)API(void *, duckdb_function_get_local_init_data, duckdb_function_info)(info);
    auto set_size = API(void, duckdb_data_chunk_set_size, duckdb_data_chunk, idx_t);
    if (!l || !g || l->done) { set_size(output, 0); return; }                                // bam_reader.c:730-733
    const idx_t vector_size = API(idx_t, duckdb_vector_size, void)();
    auto get_vec = API(duckdb_vector, duckdb_data_chunk_get_vector, duckdb_data_chunk, idx_t);
    auto get_data = API(void *, duckdb_vector_get_data, duckdb_vector);
    auto assign_len = API(void, duckdb_vector_assign_string_element_len, duckdb_vector, idx_t, const char *, idx_t);
    idx_t row_count = 0;
    while (row_count < vector_size) {
        if (!l->cur || l->pos >= l->end) {
            if (g->n_workers > 1 && row_count > 0) break;           // parallel mode: one slice per chunk
            if (!next_rows(g, l, vector_size)) {
                l->done = true;
                if (!g->error.empty()) { API(void, duckdb_function_set_error, duckdb_function_info, const char *)(info, g->error.c_str()); set_size(output, 0); return; }
                break;
            }
        }
        const HostBatch *hb = l->cur; const dhts_bam_batch &b = hb->b;
        idx_t take = (idx_t)(l->end - l->pos); if (take > vector_size - row_count) take = vector_size - row_count;
        const int64_t s = l->pos;
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
                    auto list_size = API(idx_t, duckdb_list_vector_get_size, duckdb_vector);
                    duckdb_list_entry *le = (duckdb_list_entry *)get_data(vec);
                    idx_t base = list_size(vec);
                    const uint32_t c0 = hb->aux_off[s], c1 = hb->aux_off[s + take];
                    if (c1 > c0) { API(duckdb_state, duckdb_list_vector_reserve, duckdb_vector, idx_t)(vec, base + (c1 - c0)); API(duckdb_state, duckdb_list_vector_set_size, duckdb_vector, idx_t)(vec, base + (c1 - c0)); }
                    duckdb_vector child = API(duckdb_vector, duckdb_list_vector_get_child, duckdb_vector)(vec);
                    duckdb_vector kvec = API(duckdb_vector, duckdb_struct_vector_get_child, duckdb_vector, idx_t)(child, 0);
                    duckdb_vector vvec = API(duckdb_vector, duckdb_struct_vector_get_child, duckdb_vector, idx_t)(child, 1);
                    for (idx_t r = 0; r < take; r++) {
                        le[row_count + r].offset = base + (hb->aux_off[s + r] - c0); le[row_count + r].length = hb->aux_off[s + r + 1] - hb->aux_off[s + r];
                        if (!hb->aux_valid[s + r]) set_null(vec, row_count + r);            // no tags: NULL, entry {size, 0}
                    }
                    for (uint32_t k = c0; k < c1; k++) {
                        assign_len(kvec, base + (k - c0), hb->aux_key[k].data(), hb->aux_key[k].size());
                        assign_len(vvec, base + (k - c0), hb->aux_val[k].data(), hb->aux_val[k].size());
                    }
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
                    auto list_size = API(idx_t, duckdb_list_vector_get_size, duckdb_vector);
                    duckdb_list_entry *le = (duckdb_list_entry *)get_data(vec);
                    idx_t base = list_size(vec);
                    const uint32_t c0 = h.off[s], c1 = h.off[s + take];
                    if (c1 > c0) { API(duckdb_state, duckdb_list_vector_reserve, duckdb_vector, idx_t)(vec, base + (c1 - c0)); API(duckdb_state, duckdb_list_vector_set_size, duckdb_vector, idx_t)(vec, base + (c1 - c0)); }
                    duckdb_vector child = API(duckdb_vector, duckdb_list_vector_get_child, duckdb_vector)(vec);
                    for (idx_t r = 0; r < take; r++) {
                        if (h.valid[s + r]) { le[row_count + r].offset = base + (h.off[s + r] - c0); le[row_count + r].length = h.off[s + r + 1] - h.off[s + r]; }
                        else set_null(vec, row_count + r);          // absent tag: set_null only, the entry is left untouched (bam_reader.c:927-930)
                    }
                    if (c1 > c0) memcpy((int64_t *)get_data(child) + base, h.child.data() + c0, (size_t)(c1 - c0) * 8);
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
        row_count += take; l->pos += (int64_t)take;
    }
    set_size(output, row_count);
}

extern "C" __attribute__((visibility("default"))) void register_read_bam_function(duckdb_connection connection) {                      // bam_reader.c:1044-1068
    duckdb_table_function tf = API(duckdb_table_function, duckdb_create_table_function, void)();
    API(void, duckdb_table_function_set_name, duckdb_table_function, const char *)(tf, "read_bam");
    auto mk = API(duckdb_logical_type, duckdb_create_logical_type, int);
    auto rm = API(void, duckdb_destroy_logical_type, duckdb_logical_type *);
    auto named = API(void, duckdb_table_function_add_named_parameter, duckdb_table_function, const char *, duckdb_logical_type);
    duckdb_logical_type t_varchar = mk(DUCKDB_TYPE_VARCHAR);
    API(void, duckdb_table_function_add_parameter, duckdb_table_function, duckdb_logical_type)(tf, t_varchar);
    named(tf, "region", t_varchar); named(tf, "index_path", t_varchar); named(tf, "reference", t_varchar);
    rm(&t_varchar);
    duckdb_logical_type t_bool = mk(DUCKDB_TYPE_BOOLEAN);
    named(tf, "standard_tags", t_bool); named(tf, "auxiliary_tags", t_bool);
    rm(&t_bool);
    API(void, duckdb_table_function_set_bind, duckdb_table_function, duckdb_table_function_bind_t)(tf, bam_read_bind);
    API(void, duckdb_table_function_set_init, duckdb_table_function, duckdb_table_function_init_t)(tf, bam_read_global_init);
    API(void, duckdb_table_function_set_local_init, duckdb_table_function, duckdb_table_function_init_t)(tf, bam_read_local_init);
    API(void, duckdb_table_function_set_function, duckdb_table_function, duckdb_table_function_t)(tf, bam_read_function);
    API(void, duckdb_table_function_supports_projection_pushdown, duckdb_table_function, bool)(tf, true);
    API(duckdb_state, duckdb_register_table_function, duckdb_connection, duckdb_table_function)(connection, tf);
    API(void, duckdb_destroy_table_function, duckdb_table_function *)(&tf);
}


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
struct BcfHostBatch {
    void *arena = nullptr; uint64_t cap = 0;
    std::vector<dhts_bcf_col> cols;                 // HOST pointers, projection order (deduplicated)
    std::vector<std::vector<uint32_t>> conv;        // per column: DHTS_ENC_FLOAT_TEXT children converted to float bits
    int64_t n = 0; int status = 0; int ncols_fetched = 0;
    int64_t next = 0; int readers = 0; bool retired = false;
};
struct BcfScan {
    BcfBind *bind = nullptr;
    std::vector<idx_t> column_ids;       // schema ids per output vector
    std::vector<int> slot;               // output vector -> index into the batch's columns (or -1 for unknown ids)
    std::vector<int32_t> proj;           // projected (deduplicated) schema columns
    int n_workers = 1;
    std::mutex mu; std::condition_variable cv_ready, cv_free;
    std::deque<BcfHostBatch *> ready; std::vector<BcfHostBatch *> free_slots, all;
    std::thread th; bool done = false, cancel = false; std::string error;
    dhts_ctx *ctx = nullptr;             // the scan's own context (the producer stages the file into it); lives until the chunks are filled:
    dhts_bcf_info inf;                   // its name tables -- a text scan adds the names records use without a header definition
    ~BcfScan() {
        { std::lock_guard<std::mutex> lk(mu); cancel = true; }
        cv_free.notify_all(); cv_ready.notify_all();
        if (th.joinable()) th.join();
        if (ctx) dhts_destroy(ctx);                 // first: it waits for the copy stream, whose D2H may still be writing into an arena (error paths leave one in flight)
        for (auto hb : all) { dhts_host_free(hb->arena); delete hb; }
    }
};
struct BcfLocal {
    bool done = false;
    BcfHostBatch *cur = nullptr; int64_t pos = 0, end = 0;      // rows [pos, end) of `cur` are this worker's
};
static void destroy_bcf_bind(void *p) { BcfBind *b = (BcfBind *)p; if (!b) return; if (b->ctx) dhts_destroy(b->ctx); delete b; }
static void destroy_bcf_local(void *p) { delete (BcfLocal *)p; }
static void destroy_bcf_global(void *p) { delete (BcfScan *)p; }

static void bcf_read_bind(duckdb_bind_info info) {
    auto set_error = API(void, duckdb_bind_set_error, duckdb_bind_info, const char *);
    auto dfree = API(void, duckdb_free, void *);
    duckdb_value pv = API(duckdb_value, duckdb_bind_get_parameter, duckdb_bind_info, idx_t)(info, 0);
    char *file_path = API(char *, duckdb_get_varchar, duckdb_value)(pv);
    API(void, duckdb_destroy_value, duckdb_value *)(&pv);
    if (!file_path || strlen(file_path) == 0) {
        set_error(info, "read_bcf requires a file path");                          // bcf_reader.c:461
        if (file_path) dfree(file_path);
        return;
    }
    char *region = get_named_varchar(info, "region");
    char *index_path = get_named_varchar(info, "index_path");
    const int tidy = get_named_bool(info, "tidy_format");
    BcfBind *b = new BcfBind();
    b->path = file_path; if (region) b->region = region;
    for (size_t p0 = 0; p0 <= b->region.size() && !b->region.empty();) {
        size_t q = b->region.find(',', p0); if (q == std::string::npos) q = b->region.size();
        if (q > p0) b->regions.push_back(b->region.substr(p0, q - p0));
        p0 = q + 1;
    }
    std::string idx = index_path ? index_path : "";
    dfree(file_path); if (region) dfree(region); if (index_path) dfree(index_path);
    char err[768];
    if (!file_exists(b->path)) {
        snprintf(err, sizeof(err), "Failed to open BCF/VCF file: %s", b->path.c_str());       // bcf_reader.c:494
        set_error(info, err); delete b; return;
    }
    int dev = getenv("DHTS_DEVICE") ? atoi(getenv("DHTS_DEVICE")) : 0;
    static const bool trace_bcf_bind = getenv("DHTS_TRACE") != nullptr;
    const double tb0 = now_s();
    b->ctx = dhts_create(dev); b->tidy = tidy; b->device = dev;
    const double tb1 = now_s();
    if (!b->ctx) { set_error(info, "read_bcf: no MI355X (gfx950) device available; this build has no CPU fallback"); destroy_bcf_bind(b); return; }
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
    if (b->has_index && !b->regions.empty()) {
        FILE *f = fopen(b->index_file.c_str(), "rb");
        if (f) { uint8_t tmp[65536]; size_t k; while ((k = fread(tmp, 1, sizeof(tmp), f)) > 0) b->index_bytes.insert(b->index_bytes.end(), tmp, tmp + k); fclose(f); }
    }
    {
        // only the header blocks and the index windows of the regions are staged (the reference seeks to the chunks): byte ranges from this
        // context, which holds the header.  DHTS_SPARSE=0 stages the whole file.
        static const bool env_nosparse = getenv("DHTS_SPARSE") && atoi(getenv("DHTS_SPARSE")) == 0;
        if (!b->index_bytes.empty() && !b->regions.empty() && !env_nosparse) {
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

static void bcf_producer_main(BcfScan *g) {
    BcfBind *bind = g->bind;
    auto finish = [&](const std::string &err) {
        std::lock_guard<std::mutex> lk(g->mu);
        if (!err.empty() && g->error.empty()) g->error = err;
        g->done = true; g->cv_ready.notify_all();
    };
    static const bool trace = getenv("DHTS_TRACE") != nullptr;       // stage timings on stderr
    const double t_start = now_s();
    (void)dhts_bind_thread_near_device(bind->device);          // (as read_bam's producers: thread, staging readers and pinned arenas on the GPU's NUMA node)
    dhts_ctx *c = g->ctx = dhts_create(bind->device);
    if (!c) { finish("read_bcf: no MI355X (gfx950) device available; this build has no CPU fallback"); return; }
    dhts_set_super_blocks(c, 196608);
    const double t_ctx = now_s() - t_start;
    // a plain whole-file scan starts decoding while the file is still being staged (as read_bam does): the block table is built over the
    // resident prefix and extended as more bytes arrive.  DHTS_STREAM=0, region queries and uncompressed text stage first.
    static const bool env_nostream = getenv("DHTS_STREAM") && atoi(getenv("DHTS_STREAM")) == 0;
    const bool streaming = bind->regions.empty() && !env_nostream && bind->seg_count < 0 && dhts_bcf_is_text(bind->ctx) != 2;
    int staged_all = 1;
    int orc = bind->seg_count >= 0 ? dhts_open_path_segments(c, bind->path.c_str(), bind->header_bytes, bind->seg_beg.data(), bind->seg_end.data(), bind->seg_count)
              : streaming ? dhts_open_path_async(c, bind->path.c_str()) : dhts_open_path(c, bind->path.c_str());
    if (orc == 0 && !streaming && (dhts_bgzf_index(c) <= 0 || dhts_bcf_open(c, bind->tidy) != 0)) orc = -1;
    if (orc == 0 && streaming) {
        // the header needs the first blocks only: 32 MiB to start with, four times more whenever that is not enough
        uint64_t want = 32u << 20;
        for (;;) {
            const int64_t f = dhts_stage_wait(c, want, &staged_all);
            if (f < 0) { orc = -1; break; }
            if (dhts_bgzf_index_staged(c) > 0 && dhts_bcf_open(c, bind->tidy) == 0) break;
            if (staged_all) { orc = -1; break; }
            want *= 4;
        }
    }
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
    static const int64_t env_mb = getenv("DHTS_BATCH_BLOCKS") ? atoll(getenv("DHTS_BATCH_BLOCKS")) : 0;
    const int64_t max_blocks = env_mb > 0 ? env_mb : 4096;
    BcfHostBatch *pending = nullptr; int pending_slot = 0, slot_no = 0;
    auto publish = [&](BcfHostBatch *hb, int sl) -> bool {          // sl < 0: the bytes are already there
        if (sl >= 0 && dhts_bcf_batch_fetch_wait(c, sl) != 0) return false;
        hb->conv.assign((size_t)hb->ncols_fetched, std::vector<uint32_t>());
        for (int i = 0; i < hb->ncols_fetched; i++) {
            const dhts_bcf_col &h = hb->cols[i];
            if (bind->inf.cols[h.col].encoding != DHTS_ENC_FLOAT_TEXT) continue;
            // Float fields of a transcript arrive as text: (float)strtod, NaN unless the whole token converts (vep_parse_float, src/vep_parser.c:222-235)
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
        { std::lock_guard<std::mutex> lk(g->mu); g->ready.push_back(hb); }
        g->cv_ready.notify_all();
        return true;
    };
    for (;;) {
        dhts_bcf_batch b;
        if (streaming && !staged_all && dhts_blocks_ahead(c) < max_blocks) {
            // not enough known blocks for a full batch: wait for (at least) another 128 MiB of the file, then extend the block table
            int64_t f = dhts_stage_wait(c, 0, &staged_all);
            if (f >= 0 && !staged_all) f = dhts_stage_wait(c, (uint64_t)f + (128u << 20), &staged_all);
            if (f < 0 || dhts_bgzf_index_staged(c) < 0) { finish(dhts_error(c)); return; }
        }
        if (dhts_bcf_next_batch(c, max_blocks, &b) != 0) { finish(dhts_error(c)); return; }
        if (b.n_rows > 0) {
            BcfHostBatch *hb = nullptr;
            {
                std::unique_lock<std::mutex> lk(g->mu);
                g->cv_free.wait(lk, [&] { return g->cancel || !g->free_slots.empty(); });
                if (g->cancel) break;
                hb = g->free_slots.back(); g->free_slots.pop_back();
            }
            const uint64_t need = dhts_bcf_batch_host_bytes(c);
            if (need > hb->cap) { dhts_host_free(hb->arena); hb->arena = dhts_host_alloc(need); hb->cap = hb->arena ? need : 0; }
            hb->cols.assign((size_t)b.n_cols, dhts_bcf_col());
            static const bool env_serial = getenv("DHTS_OVERLAP_READBACK") && atoi(getenv("DHTS_OVERLAP_READBACK")) == 0;
            const int frc = env_serial ? dhts_bcf_batch_fetch(c, &b, hb->arena, hb->cap, hb->cols.data()) : dhts_bcf_batch_fetch_begin(c, &b, hb->arena, hb->cap, hb->cols.data(), slot_no);
            if ((need && !hb->arena) || frc != 0) { finish(hb->arena || !need ? dhts_error(c) : "read_bcf: out of pinned host memory"); return; }
            hb->n = b.n_rows; hb->status = b.status; hb->next = 0; hb->readers = 0; hb->retired = false; hb->ncols_fetched = b.n_cols;
            // the previous batch has had this batch's scan to cross PCIe: finish it (text floats) and hand it to the fill threads
            if (pending && !publish(pending, pending_slot)) { finish(dhts_error(c)); return; }
            pending = nullptr;
            if (env_serial) { if (!publish(hb, -1)) { finish(dhts_error(c)); return; } }
            else { pending = hb; pending_slot = slot_no; slot_no ^= 1; }
        }
        if (b.status != 0) {                                     // EOF, or the silent stop at the first bad record (bcf_reader.c:1319-1349)
            if (!bind->regions.empty() && bcf_next_region(bind, c, &next_region)) continue;
            break;
        }
        { std::lock_guard<std::mutex> lk(g->mu); if (g->cancel) break; }
    }
    if (pending && !publish(pending, pending_slot)) { finish(dhts_error(c)); return; }
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
    idx_t n = API(idx_t, duckdb_init_get_column_count, duckdb_init_info)(info);
    for (idx_t i = 0; i < n; i++) {
        idx_t id = API(idx_t, duckdb_init_get_column_index, duckdb_init_info, idx_t)(info, i);
        g->column_ids.push_back(id);
        int sl = -1;
        if (id < (idx_t)bind->inf.n_cols) {
            for (size_t k = 0; k < g->proj.size(); k++) if (g->proj[k] == (int32_t)id) sl = (int)k;
            if (sl < 0) { sl = (int)g->proj.size(); g->proj.push_back((int32_t)id); }
        }
        g->slot.push_back(sl);
    }
    int thr = getenv("DHTS_THREADS") ? atoi(getenv("DHTS_THREADS")) : 1; if (thr < 1) thr = 1; if (thr > 64) thr = 64;
    g->n_workers = thr;
    for (int q = 0; q < 3; q++) { BcfHostBatch *hb = new BcfHostBatch(); g->free_slots.push_back(hb); g->all.push_back(hb); }
    g->th = std::thread(bcf_producer_main, g);
    API(void, duckdb_init_set_max_threads, duckdb_init_info, idx_t)(info, (idx_t)thr);
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, g, destroy_bcf_global);
}

static void bcf_read_local_init(duckdb_init_info info) {
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, new BcfLocal(), destroy_bcf_local);
}

// rows of the next ready batch for this worker (ordered mode: the whole batch; parallel mode: a slice); false = the scan is over
static bool bcf_next_rows(BcfScan *g, BcfLocal *l, idx_t want) {
    std::unique_lock<std::mutex> lk(g->mu);
    if (l->cur) {
        BcfHostBatch *hb = l->cur;
        hb->readers--;
        if (g->n_workers == 1 || (hb->retired && hb->readers == 0)) { g->free_slots.push_back(hb); g->cv_free.notify_all(); }
        l->cur = nullptr;
    }
    for (;;) {
        if (!g->error.empty()) return false;
        while (!g->ready.empty()) {
            BcfHostBatch *hb = g->ready.front();
            if (g->n_workers == 1) { g->ready.pop_front(); hb->readers = 1; l->cur = hb; l->pos = 0; l->end = hb->n; return true; }
            if (hb->next >= hb->n) {
                g->ready.pop_front(); hb->retired = true;
                if (hb->readers == 0) { g->free_slots.push_back(hb); g->cv_free.notify_all(); }
                continue;
            }
            l->cur = hb; l->pos = hb->next; l->end = hb->next + (int64_t)want < hb->n ? hb->next + (int64_t)want : hb->n;
            hb->next = l->end; hb->readers++;
            return true;
        }
        if (g->done) return false;
        g->cv_ready.wait(lk);
    }
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
    auto list_size = API(idx_t, duckdb_list_vector_get_size, duckdb_vector);
    auto list_reserve = API(duckdb_state, duckdb_list_vector_reserve, duckdb_vector, idx_t);
    auto list_set_size = API(duckdb_state, duckdb_list_vector_set_size, duckdb_vector, idx_t);
    auto list_child = API(duckdb_vector, duckdb_list_vector_get_child, duckdb_vector);
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
        duckdb_list_entry *le = (duckdb_list_entry *)get_data(vec);
        idx_t base = list_size(vec);
        const uint32_t c0 = h.off[s], c1 = h.off[s + take];
        if (c1 > c0) { list_reserve(vec, base + (c1 - c0)); list_set_size(vec, base + (c1 - c0)); }
        duckdb_vector child = list_child(vec);
        for (idx_t r = 0; r < take; r++) {
            le[row_count + r].offset = base + (h.off[s + r] - c0); le[row_count + r].length = h.off[s + r + 1] - h.off[s + r];
            if (!h.valid[s + r]) set_null(vec, row_count + r);
        }
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
    if (!l || !g || l->done) { set_size(output, 0); return; }                                 // bcf_reader.c:1166-1169
    const idx_t vector_size = API(idx_t, duckdb_vector_size, void)();
    idx_t row_count = 0;
    while (row_count < vector_size) {
        if (!l->cur || l->pos >= l->end) {
            if (g->n_workers > 1 && row_count > 0) break;       // parallel mode: one slice per chunk
            if (!bcf_next_rows(g, l, vector_size)) {
                l->done = true;
                std::string err; { std::lock_guard<std::mutex> lk(g->mu); err = g->error; }
                if (!err.empty()) { API(void, duckdb_function_set_error, duckdb_function_info, const char *)(info, err.c_str()); set_size(output, 0); return; }
                break;
            }
        }
        idx_t take = (idx_t)(l->end - l->pos); if (take > vector_size - row_count) take = vector_size - row_count;
        bcf_fill(bind, g, l->cur, l->pos, take, output, row_count);
        row_count += take; l->pos += (int64_t)take;
    }
    if (l->done && l->cur) { std::lock_guard<std::mutex> lk(g->mu); l->cur->readers--; if (g->n_workers == 1 || (l->cur->retired && l->cur->readers == 0)) { g->free_slots.push_back(l->cur); g->cv_free.notify_all(); } l->cur = nullptr; }
    set_size(output, row_count);
}

extern "C" __attribute__((visibility("default"))) void register_read_bcf_function(duckdb_connection connection) {                       // bcf_reader.c:2055-2080
    duckdb_table_function tf = API(duckdb_table_function, duckdb_create_table_function, void)();
    API(void, duckdb_table_function_set_name, duckdb_table_function, const char *)(tf, "read_bcf");
    auto mk = API(duckdb_logical_type, duckdb_create_logical_type, int);
    auto rm = API(void, duckdb_destroy_logical_type, duckdb_logical_type *);
    auto named = API(void, duckdb_table_function_add_named_parameter, duckdb_table_function, const char *, duckdb_logical_type);
    duckdb_logical_type t_varchar = mk(DUCKDB_TYPE_VARCHAR);
    API(void, duckdb_table_function_add_parameter, duckdb_table_function, duckdb_logical_type)(tf, t_varchar);
    named(tf, "region", t_varchar); named(tf, "index_path", t_varchar);
    rm(&t_varchar);
    duckdb_logical_type t_bool = mk(DUCKDB_TYPE_BOOLEAN);
    named(tf, "tidy_format", t_bool);
    rm(&t_bool);
    API(void, duckdb_table_function_set_bind, duckdb_table_function, duckdb_table_function_bind_t)(tf, bcf_read_bind);
    API(void, duckdb_table_function_set_init, duckdb_table_function, duckdb_table_function_init_t)(tf, bcf_read_global_init);
    API(void, duckdb_table_function_set_local_init, duckdb_table_function, duckdb_table_function_init_t)(tf, bcf_read_local_init);
    API(void, duckdb_table_function_set_function, duckdb_table_function, duckdb_table_function_t)(tf, bcf_read_function);
    API(void, duckdb_table_function_supports_projection_pushdown, duckdb_table_function, bool)(tf, true);
    API(duckdb_state, duckdb_register_table_function, duckdb_connection, duckdb_table_function)(connection, tf);
    API(void, duckdb_destroy_table_function, duckdb_table_function *)(&tf);
}

// ================================================================================================
// read_fastq -- mirrors register_read_fastq_function src/seq_reader.c:752-775, seq_read_bind 235-325, seq_read_init 334-402,
// seq_read_function 413-639.  The rows come out of the same read_bam batches (fastq_text.hip): NAME = QNAME, SEQUENCE = SEQ ('' for an
// empty read), QUALITY = QUAL (NULL where read_bam shows '*'), DESCRIPTION always NULL (the reference sets no CO tag under default
// options).  One thread (duckdb_init_set_max_threads(info, 1)); mate_path runs a second context and interleaves the rows.
// Registered by duckhts_init_c_api only when DHTS_SEQ_FUNCTIONS=1.
// ================================================================================================
enum { FQ_COL_NAME = 0, FQ_COL_DESCRIPTION, FQ_COL_SEQUENCE, FQ_COL_QUALITY, FQ_COL_MATE, FQ_COL_PAIR_ID };
static const uint32_t kFqMask = (1u << DHTS_BAM_QNAME) | (1u << DHTS_BAM_SEQ) | (1u << DHTS_BAM_QUAL);
struct FqBind { std::string path, mate_path; bool paired = false, interleaved = false; dhts_ctx *ctx[2] = {nullptr, nullptr}; };
struct FqStream {
    dhts_ctx *ctx = nullptr; void *arena = nullptr; uint64_t cap = 0; dhts_bam_batch hb; int64_t pos = 0; bool done = false; std::string err;
    // the next record of the stream (its row in hb), or -1 at the end: EOF or the first record the reader refuses (sam_read1 < 0)
    int64_t next() {
        for (;;) {
            if (pos < hb.n_rows) return pos++;
            if (done) return -1;
            dhts_bam_batch b;
            if (dhts_bam_next_batch(ctx, 0, kFqMask, &b) != 0) { err = dhts_error(ctx); done = true; return -1; }
            if (b.status != 0) done = true;
            memset(&hb, 0, sizeof(hb)); pos = 0;
            if (b.n_rows == 0) continue;
            const uint64_t need = dhts_bam_batch_host_bytes(&b, kFqMask);
            if (need > cap) { if (arena) dhts_host_free(arena); arena = dhts_host_alloc(need + need / 4); cap = arena ? need + need / 4 : 0; }
            if (!arena || dhts_bam_batch_fetch(ctx, &b, kFqMask, arena, cap, &hb) != 0) { err = arena ? dhts_error(ctx) : "read_fastq: out of pinned host memory"; done = true; memset(&hb, 0, sizeof(hb)); return -1; }
        }
    }
    const char *name(int64_t r, uint32_t *n) const { *n = hb.qname.len[r]; return (const char *)hb.qname.bytes + hb.qname.off[r]; }
};
struct FqScan { FqStream st[2]; bool paired = false, interleaved = false, done = false; int pending_mate = 0, interleaved_mate = 1; int64_t mate_row = -1; std::vector<idx_t> column_ids; std::vector<char> tmp;
                ~FqScan() { for (auto &s : st) if (s.arena) dhts_host_free(s.arena); } };
static void destroy_fq_bind(void *p) { FqBind *b = (FqBind *)p; if (!b) return; for (auto c : b->ctx) if (c) dhts_destroy(c); delete b; }
static void destroy_fq_scan(void *p) { delete (FqScan *)p; }

static void fastq_read_bind(duckdb_bind_info info) {
    auto set_error = API(void, duckdb_bind_set_error, duckdb_bind_info, const char *);
    auto dfree = API(void, duckdb_free, void *);
    duckdb_value pv = API(duckdb_value, duckdb_bind_get_parameter, duckdb_bind_info, idx_t)(info, 0);
    char *file_path = API(char *, duckdb_get_varchar, duckdb_value)(pv);
    API(void, duckdb_destroy_value, duckdb_value *)(&pv);
    if (!file_path || strlen(file_path) == 0) { set_error(info, "read_fastq requires a file path"); if (file_path) dfree(file_path); return; }   // seq_reader.c:240-246
    FqBind *b = new FqBind();
    b->path = file_path; dfree(file_path);
    char err[768];
    if (!file_exists(b->path)) { snprintf(err, sizeof(err), "Failed to open file: %s", b->path.c_str()); set_error(info, err); delete b; return; }   // seq_reader.c:250-256
    if (char *m = get_named_varchar(info, "mate_path")) { b->mate_path = m; b->paired = true; dfree(m); }
    b->interleaved = get_named_bool(info, "interleaved") != 0;
    if (b->paired && b->interleaved) { set_error(info, "read_fastq: use mate_path or interleaved, not both"); delete b; return; }                     // seq_reader.c:287-291
    // the files are staged whole here; the scan reads them batch by batch (a file that is not FASTQ / FASTA text is refused: INTEGRATION.md)
    for (int k = 0; k < (b->paired ? 2 : 1); k++) {
        const std::string &path = k ? b->mate_path : b->path;
        if (k && !file_exists(path)) { set_error(info, "Failed to open mate FASTQ file"); destroy_fq_bind(b); return; }                              // seq_reader.c:369-370 (raised at init there)
        b->ctx[k] = dhts_create(device_list()[0]);
        if (!b->ctx[k]) { set_error(info, "read_fastq: no MI355X (gfx950) device available; this build has no CPU fallback"); destroy_fq_bind(b); return; }
        if (dhts_open_path(b->ctx[k], path.c_str()) != 0 || dhts_bgzf_index(b->ctx[k]) <= 0 || dhts_bam_open(b->ctx[k]) != 0 || dhts_bam_is_text(b->ctx[k]) < 3) {
            snprintf(err, sizeof(err), "read_fastq: %s is not read as FASTQ/FASTA text by this build (a first record the FASTQ parser refuses counts as that)", path.c_str());
            set_error(info, err); destroy_fq_bind(b); return;
        }
    }
    auto mk = API(duckdb_logical_type, duckdb_create_logical_type, int);
    auto add = API(void, duckdb_bind_add_result_column, duckdb_bind_info, const char *, duckdb_logical_type);
    auto rm = API(void, duckdb_destroy_logical_type, duckdb_logical_type *);
    duckdb_logical_type t_varchar = mk(DUCKDB_TYPE_VARCHAR), t_us = mk(DUCKDB_TYPE_USMALLINT);
    add(info, "NAME", t_varchar); add(info, "DESCRIPTION", t_varchar); add(info, "SEQUENCE", t_varchar); add(info, "QUALITY", t_varchar);            // seq_reader.c:311-320
    if (b->paired || b->interleaved) { add(info, "MATE", t_us); add(info, "PAIR_ID", t_varchar); }
    rm(&t_varchar); rm(&t_us);
    API(void, duckdb_bind_set_bind_data, duckdb_bind_info, void *, duckdb_delete_callback_t)(info, b, destroy_fq_bind);
}
static void fastq_read_init(duckdb_init_info info) {
    FqBind *bind = (FqBind *)API(void *, duckdb_init_get_bind_data, duckdb_init_info)(info);
    FqScan *g = new FqScan();
    g->paired = bind->paired; g->interleaved = bind->interleaved;
    for (int k = 0; k < (bind->paired ? 2 : 1); k++) {
        g->st[k].ctx = bind->ctx[k]; memset(&g->st[k].hb, 0, sizeof(g->st[k].hb));
        dhts_bam_set_seq_packed(bind->ctx[k], 1); dhts_bam_set_qual_packed(bind->ctx[k], 0);
        if (dhts_bam_rewind(bind->ctx[k]) != 0) { API(void, duckdb_init_set_error, duckdb_init_info, const char *)(info, "Failed to open sequence file"); delete g; return; }
    }
    const idx_t n = API(idx_t, duckdb_init_get_column_count, duckdb_init_info)(info);
    for (idx_t i = 0; i < n; i++) g->column_ids.push_back(API(idx_t, duckdb_init_get_column_index, duckdb_init_info, idx_t)(info, i));
    API(void, duckdb_init_set_max_threads, duckdb_init_info, idx_t)(info, 1);
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, g, destroy_fq_scan);
}
static void fastq_read_function(duckdb_function_info info, duckdb_data_chunk output) {
    FqScan *g = (FqScan *)API(void *, duckdb_function_get_init_data, duckdb_function_info)(info);
    auto set_size = API(void, duckdb_data_chunk_set_size, duckdb_data_chunk, idx_t);
    if (!g || g->done) { set_size(output, 0); return; }
    const idx_t vector_size = API(idx_t, duckdb_vector_size, void)();
    auto get_vec = API(duckdb_vector, duckdb_data_chunk_get_vector, duckdb_data_chunk, idx_t);
    auto get_data = API(void *, duckdb_vector_get_data, duckdb_vector);
    auto assign_len = API(void, duckdb_vector_assign_string_element_len, duckdb_vector, idx_t, const char *, idx_t);
    auto fail_scan = [&](const char *msg) { API(void, duckdb_function_set_error, duckdb_function_info, const char *)(info, msg); g->done = true; set_size(output, 0); };
    idx_t row_count = 0;
    while (row_count < vector_size) {
        FqStream *s = &g->st[0]; int64_t r; int mate = 0;
        if (g->paired) {                                                                             // seq_reader.c:476-511
            if (g->pending_mate) { s = &g->st[1]; r = g->mate_row; mate = 2; g->pending_mate = 0; }
            else {
                const int64_t r1 = g->st[0].next(), r2 = g->st[1].next();
                if (r1 < 0 || r2 < 0) {
                    if (r1 < 0 && r2 < 0) { g->done = true; break; }
                    fail_scan("read_fastq: mate files have different record counts"); return;
                }
                uint32_t n1, n2; const char *q1 = g->st[0].name(r1, &n1), *q2 = g->st[1].name(r2, &n2);
                const size_t l1 = strnlen(q1, n1), l2 = strnlen(q2, n2);                             // (strcmp reads C strings)
                if (l1 != l2 || memcmp(q1, q2, l1) != 0) {
                    char msg[256]; snprintf(msg, sizeof(msg), "read_fastq: mate files out of sync (QNAME mismatch: '%.*s' vs '%.*s')", (int)l1, q1, (int)l2, q2);
                    fail_scan(msg); return;
                }
                r = r1; mate = 1; g->pending_mate = 1; g->mate_row = r2;
            }
        } else {                                                                                     // seq_reader.c:512-531
            r = s->next();
            if (r < 0) {
                if (g->interleaved && g->interleaved_mate == 2) { fail_scan("read_fastq: interleaved file has an unpaired record"); return; }
                g->done = true; break;
            }
            if (g->interleaved) { mate = g->interleaved_mate; g->interleaved_mate = mate == 1 ? 2 : 1; }
        }
        const dhts_bam_batch &b = s->hb;
        const uint32_t l_seq = b.seq.len[r];
        for (size_t ci = 0; ci < g->column_ids.size(); ci++) {
            duckdb_vector vec = get_vec(output, ci);
            switch (g->column_ids[ci]) {
            case FQ_COL_NAME: { uint32_t n; const char *q = s->name(r, &n); assign_len(vec, row_count, q, strnlen(q, n)); break; }
            case FQ_COL_DESCRIPTION: set_null(vec, row_count); break;
            case FQ_COL_SEQUENCE:
                if (l_seq == 0) { assign_len(vec, row_count, "", 0); break; }
                if (g->tmp.size() < (size_t)l_seq + 32) g->tmp.resize((size_t)l_seq + 32 + l_seq / 2);
                expand_seq(b.seq.bytes + b.seq.off[r], l_seq, g->tmp.data());
                assign_len(vec, row_count, g->tmp.data(), l_seq);
                break;
            case FQ_COL_QUALITY: {
                // "seq_len > 0 && qual[0] != 255": the batch shows an absent QUAL as the one character '*' (a one-base read of quality 9 reads the same: INTEGRATION.md)
                const uint32_t n = b.qual.len[r]; const char *q = (const char *)b.qual.bytes + b.qual.off[r];
                if (l_seq == 0 || (n == 1 && q[0] == '*' )) set_null(vec, row_count); else assign_len(vec, row_count, q, n);
                break;
            }
            case FQ_COL_MATE:
                if (g->paired || g->interleaved) ((uint16_t *)get_data(vec))[row_count] = (uint16_t)mate; else set_null(vec, row_count);
                break;
            case FQ_COL_PAIR_ID: {
                if (!(g->paired || g->interleaved)) { set_null(vec, row_count); break; }
                uint32_t n; const char *q = s->name(r, &n); size_t len = strnlen(q, n);
                if (len >= 2 && q[len - 2] == '/' && (q[len - 1] == '1' || q[len - 1] == '2')) len -= 2;     // strip_pair_suffix, seq_reader.c:171-182
                assign_len(vec, row_count, q, len);
                break;
            }
            default: break;
            }
        }
        row_count++;
    }
    for (auto &st : g->st) if (!st.err.empty()) { fail_scan(st.err.c_str()); return; }
    set_size(output, row_count);
}
extern "C" __attribute__((visibility("default"))) void register_read_fastq_function(duckdb_connection connection) {                    // seq_reader.c:752-775
    duckdb_table_function tf = API(duckdb_table_function, duckdb_create_table_function, void)();
    API(void, duckdb_table_function_set_name, duckdb_table_function, const char *)(tf, "read_fastq");
    auto mk = API(duckdb_logical_type, duckdb_create_logical_type, int);
    auto rm = API(void, duckdb_destroy_logical_type, duckdb_logical_type *);
    auto named = API(void, duckdb_table_function_add_named_parameter, duckdb_table_function, const char *, duckdb_logical_type);
    duckdb_logical_type t_varchar = mk(DUCKDB_TYPE_VARCHAR);
    API(void, duckdb_table_function_add_parameter, duckdb_table_function, duckdb_logical_type)(tf, t_varchar);
    named(tf, "mate_path", t_varchar);
    rm(&t_varchar);
    duckdb_logical_type t_bool = mk(DUCKDB_TYPE_BOOLEAN);
    named(tf, "interleaved", t_bool);
    rm(&t_bool);
    API(void, duckdb_table_function_set_bind, duckdb_table_function, duckdb_table_function_bind_t)(tf, fastq_read_bind);
    API(void, duckdb_table_function_set_init, duckdb_table_function, duckdb_table_function_init_t)(tf, fastq_read_init);
    API(void, duckdb_table_function_set_function, duckdb_table_function, duckdb_table_function_t)(tf, fastq_read_function);
    API(void, duckdb_table_function_supports_projection_pushdown, duckdb_table_function, bool)(tf, true);
    API(duckdb_state, duckdb_register_table_function, duckdb_connection, duckdb_table_function)(connection, tf);
    API(void, duckdb_destroy_table_function, duckdb_table_function *)(&tf);
}

// ================================================================================================
// read_fasta -- mirrors register_read_fasta_function src/seq_reader.c:645-662, seq_read_bind 235-325, seq_read_init 334-402,
// seq_read_function 413-472 (regions) and 533-583 (records).  Without a region the rows come out of the read_bam batches of FASTA text
// like read_fastq's (NAME = QNAME, SEQUENCE = SEQ, '' when empty; DESCRIPTION is the CO tag in the reference, which fastq_parse1 makes only
// under the fastq_aux option the reference never sets, so it is NULL).  With a region: one row per region in the order given, from the
// device .fai fetch (dhts_fasta_load_index / dhts_fasta_open_regions / dhts_fasta_fetch); the index is <path>.fai or index_path and is
// never built here.  One thread.  Registered by duckhts_init_c_api only when DHTS_SEQ_FUNCTIONS=1.
// ================================================================================================
struct FaBind { std::string path, region, index_path; int n_regions = 0; dhts_ctx *ctx = nullptr; };
struct FaScan { FqStream st; bool regions = false, done = false; dhts_ctx *rctx = nullptr; void *arena = nullptr; dhts_fasta_batch hb; int64_t pos = 0; std::string err; std::vector<idx_t> column_ids; std::vector<char> tmp;
                ~FaScan() { if (st.arena) dhts_host_free(st.arena); if (arena) dhts_host_free(arena); if (rctx) dhts_destroy(rctx); } };
static void destroy_fa_bind(void *p) { FaBind *b = (FaBind *)p; if (!b) return; if (b->ctx) dhts_destroy(b->ctx); delete b; }
static void destroy_fa_scan(void *p) { delete (FaScan *)p; }
// parse_regions_duckdb (seq_reader.c:192-229): pieces between commas, blanks and tabs trimmed, empty ones dropped
static std::vector<std::string> fasta_split_regions(const std::string &all) {
    std::vector<std::string> out; size_t p = 0;
    while (p <= all.size()) {
        size_t e = all.find(',', p); if (e == std::string::npos) e = all.size();
        size_t a = p, b = e; while (a < b && (all[a] == ' ' || all[a] == '\t')) a++; while (b > a && (all[b - 1] == ' ' || all[b - 1] == '\t')) b--;
        if (b > a) out.push_back(all.substr(a, b - a));
        p = e + 1;
    }
    return out;
}
static void fasta_read_bind(duckdb_bind_info info) {
    auto set_error = API(void, duckdb_bind_set_error, duckdb_bind_info, const char *);
    auto dfree = API(void, duckdb_free, void *);
    duckdb_value pv = API(duckdb_value, duckdb_bind_get_parameter, duckdb_bind_info, idx_t)(info, 0);
    char *file_path = API(char *, duckdb_get_varchar, duckdb_value)(pv);
    API(void, duckdb_destroy_value, duckdb_value *)(&pv);
    if (!file_path || strlen(file_path) == 0) { set_error(info, "read_fasta requires a file path"); if (file_path) dfree(file_path); return; }   // seq_reader.c:240-246
    FaBind *b = new FaBind();
    b->path = file_path; dfree(file_path);
    char err[768];
    if (!file_exists(b->path)) { snprintf(err, sizeof(err), "Failed to open file: %s", b->path.c_str()); set_error(info, err); delete b; return; }   // seq_reader.c:250-256
    if (char *r = get_named_varchar(info, "region")) { b->region = r; dfree(r); b->n_regions = (int)fasta_split_regions(b->region).size(); }
    if (char *x = get_named_varchar(info, "index_path")) { b->index_path = x; dfree(x); }
    if (b->n_regions == 0) {                                     // a whole-file scan: the file is staged here, the scan reads it batch by batch
        b->ctx = dhts_create(device_list()[0]);
        if (!b->ctx) { set_error(info, "read_fasta: no MI355X (gfx950) device available; this build has no CPU fallback"); destroy_fa_bind(b); return; }
        if (dhts_open_path(b->ctx, b->path.c_str()) != 0 || dhts_bgzf_index(b->ctx) <= 0 || dhts_bam_open(b->ctx) != 0 || dhts_bam_is_text(b->ctx) < 3) {
            snprintf(err, sizeof(err), "read_fasta: %s is not read as FASTQ/FASTA text by this build (a first record the FASTQ parser refuses counts as that)", b->path.c_str());
            set_error(info, err); destroy_fa_bind(b); return;
        }
    }
    auto mk = API(duckdb_logical_type, duckdb_create_logical_type, int);
    auto add = API(void, duckdb_bind_add_result_column, duckdb_bind_info, const char *, duckdb_logical_type);
    auto rm = API(void, duckdb_destroy_logical_type, duckdb_logical_type *);
    duckdb_logical_type t_varchar = mk(DUCKDB_TYPE_VARCHAR);
    add(info, "NAME", t_varchar); add(info, "DESCRIPTION", t_varchar); add(info, "SEQUENCE", t_varchar);                                             // seq_reader.c:311-313
    rm(&t_varchar);
    API(void, duckdb_bind_set_bind_data, duckdb_bind_info, void *, duckdb_delete_callback_t)(info, b, destroy_fa_bind);
}
static void fasta_read_init(duckdb_init_info info) {
    FaBind *bind = (FaBind *)API(void *, duckdb_init_get_bind_data, duckdb_init_info)(info);
    auto init_error = API(void, duckdb_init_set_error, duckdb_init_info, const char *);
    FaScan *g = new FaScan();
    memset(&g->hb, 0, sizeof(g->hb)); memset(&g->st.hb, 0, sizeof(g->st.hb));
    if (bind->n_regions > 0) {                                   // seq_reader.c:383-390: the index is loaded, never built
        g->regions = true;
        const std::string fai_path = bind->index_path.empty() ? bind->path + ".fai" : bind->index_path;
        std::string fai; bool have = false;
        if (FILE *f = fopen(fai_path.c_str(), "rb")) { char buf[65536]; size_t n; while ((n = fread(buf, 1, sizeof(buf), f)) > 0) fai.append(buf, n); fclose(f); have = true; }
        g->rctx = have ? dhts_create(device_list()[0]) : nullptr;
        if (have && !g->rctx) { init_error(info, "read_fasta: no MI355X (gfx950) device available; this build has no CPU fallback"); delete g; return; }
        if (!have || dhts_fasta_load_index(g->rctx, fai.data(), fai.size()) != 0 || dhts_fasta_open_regions(g->rctx, bind->path.c_str(), bind->region.c_str()) != 0) {
            init_error(info, "read_fasta: region query requires a FASTA index (.fai); run fasta_index(path) first"); delete g; return;
        }
        dhts_fasta_batch db;
        if (dhts_fasta_fetch(g->rctx, bind->region.c_str(), &db) != 0) {
            // fai_fetch64 fails region by region (seq_reader.c:432-441): name the first one that does
            std::string bad;
            for (auto &r : fasta_split_regions(bind->region)) { dhts_fasta_batch one; if (dhts_fasta_fetch(g->rctx, r.c_str(), &one) != 0) { bad = r; break; } }
            g->err = "read_fasta: invalid or missing region '" + bad + "'";
        } else {
            const uint64_t need = dhts_fasta_batch_host_bytes(&db);
            g->arena = dhts_host_alloc(need);
            if (!g->arena || dhts_fasta_batch_fetch(g->rctx, &db, g->arena, need, &g->hb) != 0) { init_error(info, g->arena ? dhts_error(g->rctx) : "read_fasta: out of pinned host memory"); delete g; return; }
        }
    } else {
        g->st.ctx = bind->ctx;
        dhts_bam_set_seq_packed(bind->ctx, 1); dhts_bam_set_qual_packed(bind->ctx, 0);
        if (dhts_bam_rewind(bind->ctx) != 0) { init_error(info, "Failed to open sequence file"); delete g; return; }
    }
    const idx_t n = API(idx_t, duckdb_init_get_column_count, duckdb_init_info)(info);
    for (idx_t i = 0; i < n; i++) g->column_ids.push_back(API(idx_t, duckdb_init_get_column_index, duckdb_init_info, idx_t)(info, i));
    API(void, duckdb_init_set_max_threads, duckdb_init_info, idx_t)(info, 1);
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, g, destroy_fa_scan);
}
static void fasta_read_function(duckdb_function_info info, duckdb_data_chunk output) {
    FaScan *g = (FaScan *)API(void *, duckdb_function_get_init_data, duckdb_function_info)(info);
    auto set_size = API(void, duckdb_data_chunk_set_size, duckdb_data_chunk, idx_t);
    if (!g || g->done) { set_size(output, 0); return; }
    const idx_t vector_size = API(idx_t, duckdb_vector_size, void)();
    auto get_vec = API(duckdb_vector, duckdb_data_chunk_get_vector, duckdb_data_chunk, idx_t);
    auto assign_len = API(void, duckdb_vector_assign_string_element_len, duckdb_vector, idx_t, const char *, idx_t);
    auto fail_scan = [&](const char *msg) { API(void, duckdb_function_set_error, duckdb_function_info, const char *)(info, msg); g->done = true; set_size(output, 0); };
    if (!g->err.empty()) { fail_scan(g->err.c_str()); return; }
    idx_t row_count = 0;
    while (row_count < vector_size) {
        if (g->regions) {                                                                            // seq_reader.c:425-472
            if (g->pos >= g->hb.n_rows) { g->done = true; break; }
            const int64_t r = g->pos++;
            for (size_t ci = 0; ci < g->column_ids.size(); ci++) {
                duckdb_vector vec = get_vec(output, ci);
                switch (g->column_ids[ci]) {
                case FQ_COL_NAME: assign_len(vec, row_count, (const char *)g->hb.name_bytes + g->hb.name_off[r], g->hb.name_off[r + 1] - g->hb.name_off[r]); break;
                case FQ_COL_DESCRIPTION: set_null(vec, row_count); break;
                case FQ_COL_SEQUENCE: assign_len(vec, row_count, (const char *)g->hb.seq_bytes + g->hb.seq_off[r], g->hb.seq_off[r + 1] - g->hb.seq_off[r]); break;
                default: break;
                }
            }
            row_count++;
            continue;
        }
        const int64_t r = g->st.next();
        if (r < 0) { g->done = true; break; }
        const dhts_bam_batch &b = g->st.hb;
        const uint32_t l_seq = b.seq.len[r];
        for (size_t ci = 0; ci < g->column_ids.size(); ci++) {
            duckdb_vector vec = get_vec(output, ci);
            switch (g->column_ids[ci]) {
            case FQ_COL_NAME: { uint32_t n; const char *q = g->st.name(r, &n); assign_len(vec, row_count, q, strnlen(q, n)); break; }
            case FQ_COL_DESCRIPTION: set_null(vec, row_count); break;
            case FQ_COL_SEQUENCE:
                if (l_seq == 0) { assign_len(vec, row_count, "", 0); break; }
                if (g->tmp.size() < (size_t)l_seq + 32) g->tmp.resize((size_t)l_seq + 32 + l_seq / 2);
                expand_seq(b.seq.bytes + b.seq.off[r], l_seq, g->tmp.data());
                assign_len(vec, row_count, g->tmp.data(), l_seq);
                break;
            default: break;
            }
        }
        row_count++;
    }
    if (!g->st.err.empty()) { fail_scan(g->st.err.c_str()); return; }
    set_size(output, row_count);
}
extern "C" __attribute__((visibility("default"))) void register_read_fasta_function(duckdb_connection connection) {                    // seq_reader.c:645-662
    duckdb_table_function tf = API(duckdb_table_function, duckdb_create_table_function, void)();
    API(void, duckdb_table_function_set_name, duckdb_table_function, const char *)(tf, "read_fasta");
    auto mk = API(duckdb_logical_type, duckdb_create_logical_type, int);
    auto rm = API(void, duckdb_destroy_logical_type, duckdb_logical_type *);
    auto named = API(void, duckdb_table_function_add_named_parameter, duckdb_table_function, const char *, duckdb_logical_type);
    duckdb_logical_type t_varchar = mk(DUCKDB_TYPE_VARCHAR);
    API(void, duckdb_table_function_add_parameter, duckdb_table_function, duckdb_logical_type)(tf, t_varchar);
    named(tf, "region", t_varchar);
    named(tf, "index_path", t_varchar);
    rm(&t_varchar);
    API(void, duckdb_table_function_set_bind, duckdb_table_function, duckdb_table_function_bind_t)(tf, fasta_read_bind);
    API(void, duckdb_table_function_set_init, duckdb_table_function, duckdb_table_function_init_t)(tf, fasta_read_init);
    API(void, duckdb_table_function_set_function, duckdb_table_function, duckdb_table_function_t)(tf, fasta_read_function);
    API(void, duckdb_table_function_supports_projection_pushdown, duckdb_table_function, bool)(tf, true);
    API(duckdb_state, duckdb_register_table_function, duckdb_connection, duckdb_table_function)(connection, tf);
    API(void, duckdb_destroy_table_function, duckdb_table_function *)(&tf);
}

// ---- read_bed (src/interval_udf.c:217-426, 838-852): one thread, file order, vector_size rows per chunk -------------------------------------
// bind checks the path and, for a region, that a tabix index can be read (tbx_index_load3: index_path, else <path>.tbi, <path>.csi); init
// stages the file -- for a region only the index windows -- and resolves the region; the scan fills chunks from device batches read back
// by dhts_bed_batch_fetch.  A line with fewer than 3 fields replaces the chunk it would have been in by read_bed's error.
static const char *const kBedCols[DHTS_BED_COL_COUNT] = {"chrom", "start", "end", "name", "score", "strand", "thick_start", "thick_end", "item_rgb", "block_count", "block_sizes", "block_starts", "extra"};
static inline bool bed_is_bigint(idx_t c) { return c == DHTS_BED_START || c == DHTS_BED_END || c == DHTS_BED_THICK_START || c == DHTS_BED_THICK_END || c == DHTS_BED_BLOCK_COUNT; }
struct BedBind { std::string path, region; bool has_region = false; std::string index; };
struct BedScanState {
    dhts_ctx *ctx = nullptr; void *arena = nullptr; uint64_t arena_cap = 0;
    std::vector<idx_t> column_ids; std::vector<int> slot;       // output column -> position in the projection (-1: none)
    std::vector<dhts_col> host; int64_t n = 0, pos = 0; int32_t status = 0; bool done = false;
    ~BedScanState() { if (arena) dhts_host_free(arena); if (ctx) dhts_destroy(ctx); }
};
static void destroy_bed_bind(void *p) { delete (BedBind *)p; }
static void destroy_bed_scan(void *p) { delete (BedScanState *)p; }
static bool read_file(const std::string &path, std::string &out) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    char buf[65536]; size_t n; out.clear();
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) out.append(buf, n);
    fclose(f);
    return true;
}
static void bed_read_bind(duckdb_bind_info info) {
    auto set_error = API(void, duckdb_bind_set_error, duckdb_bind_info, const char *);
    auto dfree = API(void, duckdb_free, void *);
    duckdb_value pv = API(duckdb_value, duckdb_bind_get_parameter, duckdb_bind_info, idx_t)(info, 0);
    char *file_path = API(char *, duckdb_get_varchar, duckdb_value)(pv);
    API(void, duckdb_destroy_value, duckdb_value *)(&pv);
    if (!file_path || file_path[0] == '\0') { set_error(info, "read_bed requires a file path"); if (file_path) dfree(file_path); return; }   // interval_udf.c:242-246
    BedBind *b = new BedBind();
    b->path = file_path; dfree(file_path);
    std::string index_path;
    if (char *r = get_named_varchar(info, "region")) { b->region = r; b->has_region = true; dfree(r); }
    if (char *x = get_named_varchar(info, "index_path")) { index_path = x; dfree(x); }
    char err[768];
    if (!file_exists(b->path)) { snprintf(err, sizeof(err), "read_bed: failed to open file: %s", b->path.c_str()); set_error(info, err); delete b; return; }   // :262-271
    if (b->has_region) {                                          // :274-283
        bool have = index_path.empty() ? (read_file(b->path + ".tbi", b->index) || read_file(b->path + ".csi", b->index)) : read_file(index_path, b->index);
        if (have && b->index.size() < 4) have = false;
        if (!have) { set_error(info, "read_bed: region queries require a tabix index"); delete b; return; }
    }
    auto mk = API(duckdb_logical_type, duckdb_create_logical_type, int);
    auto add = API(void, duckdb_bind_add_result_column, duckdb_bind_info, const char *, duckdb_logical_type);
    auto rm = API(void, duckdb_destroy_logical_type, duckdb_logical_type *);
    duckdb_logical_type t_varchar = mk(DUCKDB_TYPE_VARCHAR), t_bigint = mk(DUCKDB_TYPE_BIGINT);
    for (idx_t c = 0; c < DHTS_BED_COL_COUNT; c++) add(info, kBedCols[c], bed_is_bigint(c) ? t_bigint : t_varchar);                            // :217-235
    rm(&t_varchar); rm(&t_bigint);
    API(void, duckdb_bind_set_bind_data, duckdb_bind_info, void *, duckdb_delete_callback_t)(info, b, destroy_bed_bind);
}
static void bed_read_init(duckdb_init_info info) {
    BedBind *bind = (BedBind *)API(void *, duckdb_init_get_bind_data, duckdb_init_info)(info);
    auto init_error = API(void, duckdb_init_set_error, duckdb_init_info, const char *);
    BedScanState *g = new BedScanState();
    g->ctx = dhts_create(device_list()[0]);
    if (!g->ctx) { init_error(info, "read_bed: no MI355X (gfx950) device available; this build has no CPU fallback"); delete g; return; }
    bool staged = false;
    if (bind->has_region) {
        // a BGZF file is staged by the index: nothing but the windows of the region (BED text has no header)
        uint8_t h[18] = {0}; size_t got = 0;
        if (FILE *f = fopen(bind->path.c_str(), "rb")) { got = fread(h, 1, 18, f); fclose(f); }
        const bool bgzf = got == 18 && h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && (h[3] & 4) && h[12] == 'B' && h[13] == 'C';
        if (bgzf) {
            uint64_t beg[4096], end[4096]; int64_t cnt = -1;
            const int rc = dhts_bed_region_segments(g->ctx, bind->region.c_str(), bind->index.data(), bind->index.size(), beg, end, 4096, &cnt);
            if (rc == 1) { init_error(info, "read_bed: failed to create region iterator"); delete g; return; }                             // :314-319
            if (rc < 0) { init_error(info, "read_bed: failed to load tabix index"); delete g; return; }                                   // :308-313
            if (cnt >= 0) {
                if (dhts_open_path_segments(g->ctx, bind->path.c_str(), 0, beg, end, cnt) != 0) { init_error(info, "read_bed: failed to open file during init"); delete g; return; }
                staged = true;
            }
        }
    }
    if (!staged && dhts_open_path(g->ctx, bind->path.c_str()) != 0) { init_error(info, "read_bed: failed to open file during init"); delete g; return; }   // :300-305
    (void)dhts_bgzf_index(g->ctx);                               // (text that is not BGZF fails here and is taken as text by dhts_bed_open)
    if (dhts_bed_open(g->ctx) != 0) { init_error(info, "read_bed: failed to open file during init"); delete g; return; }
    const idx_t n = API(idx_t, duckdb_init_get_column_count, duckdb_init_info)(info);
    std::vector<int32_t> proj;
    for (idx_t i = 0; i < n; i++) {
        const idx_t id = API(idx_t, duckdb_init_get_column_index, duckdb_init_info, idx_t)(info, i);
        g->column_ids.push_back(id);
        int at = -1;
        if (id < DHTS_BED_COL_COUNT) {
            for (size_t k = 0; k < proj.size(); k++) if (proj[k] == (int32_t)id) at = (int)k;
            if (at < 0) { at = (int)proj.size(); proj.push_back((int32_t)id); }
        }
        g->slot.push_back(at);
    }
    if (dhts_bed_set_projection(g->ctx, proj.data(), (int32_t)proj.size()) != 0) { init_error(info, dhts_error(g->ctx)); delete g; return; }
    if (bind->has_region) {
        if (dhts_bed_set_region(g->ctx, bind->region.c_str()) != 0) { const std::string m = dhts_error(g->ctx); init_error(info, m.c_str()); delete g; return; }
        const int rc = dhts_bed_load_index(g->ctx, bind->index.data(), bind->index.size());
        if (rc == 1) { init_error(info, "read_bed: failed to create region iterator"); delete g; return; }
        if (rc < 0) { init_error(info, "read_bed: failed to load tabix index"); delete g; return; }
    }
    g->host.resize(proj.size() ? proj.size() : 1);
    API(void, duckdb_init_set_max_threads, duckdb_init_info, idx_t)(info, 1);
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, g, destroy_bed_scan);
}
// the next device batch, read back; false at the end of the stream (g->status says how it ended) or on a failure (err set)
static bool bed_next(BedScanState *g, std::string &err) {
    while (g->status == 0) {
        dhts_bed_batch b;
        if (dhts_bed_next_batch(g->ctx, 0, &b) != 0) { err = dhts_error(g->ctx); return false; }
        g->status = b.status;
        if (b.n_rows == 0) continue;
        const uint64_t need = dhts_bed_batch_host_bytes(&b);
        if (need > g->arena_cap) { if (g->arena) dhts_host_free(g->arena); g->arena_cap = need + need / 4 + 4096; g->arena = dhts_host_alloc(g->arena_cap); if (!g->arena) { g->arena_cap = 0; err = "read_bed: out of pinned host memory"; return false; } }
        if (dhts_bed_batch_fetch(g->ctx, &b, g->arena, g->arena_cap, g->host.data()) != 0) { err = dhts_error(g->ctx); return false; }
        g->n = b.n_rows; g->pos = 0;
        return true;
    }
    return false;
}
static void bed_read_function(duckdb_function_info info, duckdb_data_chunk output) {
    BedScanState *g = (BedScanState *)API(void *, duckdb_function_get_init_data, duckdb_function_info)(info);
    auto set_size = API(void, duckdb_data_chunk_set_size, duckdb_data_chunk, idx_t);
    if (!g || g->done) { set_size(output, 0); return; }
    const idx_t vector_size = API(idx_t, duckdb_vector_size, void)();
    auto get_vec = API(duckdb_vector, duckdb_data_chunk_get_vector, duckdb_data_chunk, idx_t);
    auto assign_len = API(void, duckdb_vector_assign_string_element_len, duckdb_vector, idx_t, const char *, idx_t);
    auto get_data = API(void *, duckdb_vector_get_data, duckdb_vector);
    auto fail_scan = [&](const char *msg) { API(void, duckdb_function_set_error, duckdb_function_info, const char *)(info, msg); g->done = true; set_size(output, 0); };
    idx_t row_count = 0;
    while (row_count < vector_size) {
        if (g->pos >= g->n) {
            std::string err;
            if (!bed_next(g, err)) {
                if (!err.empty()) { fail_scan(err.c_str()); return; }
                g->done = true;
                // the short line would have been a row of this chunk: the chunk is the error (interval_udf.c:358-365); any other end of the
                // stream ends the scan as a failed hts_getline does (:334-337)
                if (g->status < 0 && strstr(dhts_error(g->ctx), "fewer than 3 tab-delimited fields")) { fail_scan("read_bed: BED line has fewer than 3 tab-delimited fields"); return; }
                break;
            }
        }
        const idx_t take = (idx_t)(g->n - g->pos) < vector_size - row_count ? (idx_t)(g->n - g->pos) : vector_size - row_count;
        for (size_t ci = 0; ci < g->column_ids.size(); ci++) {
            duckdb_vector vec = get_vec(output, ci);
            if (g->slot[ci] < 0) { for (idx_t r = 0; r < take; r++) set_null(vec, row_count + r); continue; }
            const dhts_col &hc = g->host[(size_t)g->slot[ci]];
            if (bed_is_bigint(g->column_ids[ci])) {
                int64_t *data = (int64_t *)get_data(vec); const int64_t *src = (const int64_t *)hc.fixed;
                for (idx_t r = 0; r < take; r++) { if (hc.valid[g->pos + r]) data[row_count + r] = src[g->pos + r]; else set_null(vec, row_count + r); }
            } else {
                for (idx_t r = 0; r < take; r++) {
                    const int64_t k = g->pos + (int64_t)r;
                    if (hc.valid[k]) assign_len(vec, row_count + r, (const char *)hc.bytes + hc.off[k], hc.off[k + 1] - hc.off[k]); else set_null(vec, row_count + r);
                }
            }
        }
        g->pos += (int64_t)take; row_count += take;
    }
    set_size(output, row_count);
}
extern "C" __attribute__((visibility("default"))) void register_read_bed_function(duckdb_connection connection) {                      // interval_udf.c:838-852
    duckdb_table_function tf = API(duckdb_table_function, duckdb_create_table_function, void)();
    API(void, duckdb_table_function_set_name, duckdb_table_function, const char *)(tf, "read_bed");
    auto mk = API(duckdb_logical_type, duckdb_create_logical_type, int);
    auto rm = API(void, duckdb_destroy_logical_type, duckdb_logical_type *);
    auto named = API(void, duckdb_table_function_add_named_parameter, duckdb_table_function, const char *, duckdb_logical_type);
    duckdb_logical_type t_varchar = mk(DUCKDB_TYPE_VARCHAR);
    API(void, duckdb_table_function_add_parameter, duckdb_table_function, duckdb_logical_type)(tf, t_varchar);
    named(tf, "region", t_varchar);
    named(tf, "index_path", t_varchar);
    rm(&t_varchar);
    API(void, duckdb_table_function_set_bind, duckdb_table_function, duckdb_table_function_bind_t)(tf, bed_read_bind);
    API(void, duckdb_table_function_set_init, duckdb_table_function, duckdb_table_function_init_t)(tf, bed_read_init);
    API(void, duckdb_table_function_set_function, duckdb_table_function, duckdb_table_function_t)(tf, bed_read_function);
    API(void, duckdb_table_function_supports_projection_pushdown, duckdb_table_function, bool)(tf, true);
    API(duckdb_state, duckdb_register_table_function, duckdb_connection, duckdb_table_function)(connection, tf);
    API(void, duckdb_destroy_table_function, duckdb_table_function *)(&tf);
}

// ---- fasta_nuc (src/interval_udf.c:451-836, 854-876): one thread, BED file order or bin order, vector_size rows per chunk --------------------
// bind checks the arguments and reads the .fai (index_path, else <fasta>.fai; unlike fai_load3_format a missing one is never built: it is
// the bind error); init stages the FASTA -- with a region of an uncompressed file only what the region reads -- puts the index on the
// device, resolves the region and prepares the BED context (with a region and a tabix index: the index windows only); the scan fills
// chunks from device batches read back by dhts_nuc_batch_fetch.  The BED lines' columns never visit the host.
static const char *const kNucCols[DHTS_NUC_COL_COUNT] = {"chrom", "start", "end", "pct_at", "pct_gc", "num_a", "num_c", "num_g", "num_t", "num_n", "num_other", "seq_len", "seq"};
static inline bool nuc_is_varchar(idx_t c) { return c == DHTS_NUC_CHROM || c == DHTS_NUC_SEQ; }
struct NucBind { std::string fasta, bed, region, bed_index_path, fai; bool has_bed = false, has_region = false, include_seq = false; int64_t bin_width = 0; };
struct NucScanState {
    dhts_ctx *ctx = nullptr, *bed = nullptr; void *arena = nullptr; uint64_t arena_cap = 0; int64_t bin_width = 0;
    std::vector<idx_t> column_ids; std::vector<int> slot;
    std::vector<dhts_col> host; int64_t n = 0, pos = 0; int32_t status = 0; bool done = false;
    ~NucScanState() { if (arena) dhts_host_free(arena); if (bed) dhts_destroy(bed); if (ctx) dhts_destroy(ctx); }
};
static void destroy_nuc_bind(void *p) { delete (NucBind *)p; }
static void destroy_nuc_scan(void *p) { delete (NucScanState *)p; }
static bool file_is_bgzf(const std::string &path) {
    uint8_t h[18] = {0}; size_t got = 0;
    if (FILE *f = fopen(path.c_str(), "rb")) { got = fread(h, 1, 18, f); fclose(f); }
    return got == 18 && h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && (h[3] & 4) && h[12] == 'B' && h[13] == 'C';
}
static void fasta_nuc_bind(duckdb_bind_info info) {
    auto set_error = API(void, duckdb_bind_set_error, duckdb_bind_info, const char *);
    auto dfree = API(void, duckdb_free, void *);
    duckdb_value pv = API(duckdb_value, duckdb_bind_get_parameter, duckdb_bind_info, idx_t)(info, 0);
    char *fasta_path = API(char *, duckdb_get_varchar, duckdb_value)(pv);
    API(void, duckdb_destroy_value, duckdb_value *)(&pv);
    if (!fasta_path || fasta_path[0] == '\0') { set_error(info, "fasta_nuc requires a FASTA path"); if (fasta_path) dfree(fasta_path); return; }   // interval_udf.c:479-483
    NucBind *b = new NucBind();
    b->fasta = fasta_path; dfree(fasta_path);
    if (char *x = get_named_varchar(info, "bed_path")) { b->bed = x; b->has_bed = true; dfree(x); }
    bool has_bin_width = false;
    {
        duckdb_value v = API(duckdb_value, duckdb_bind_get_named_parameter, duckdb_bind_info, const char *)(info, "bin_width");
        if (v && !API(bool, duckdb_is_null_value, duckdb_value)(v)) { b->bin_width = API(int64_t, duckdb_get_int64, duckdb_value)(v); has_bin_width = true; }
        if (v) API(void, duckdb_destroy_value, duckdb_value *)(&v);
    }
    if (b->has_bed == has_bin_width) { set_error(info, "fasta_nuc requires exactly one of bed_path or bin_width"); delete b; return; }        // :499-504
    if (has_bin_width && b->bin_width <= 0) { set_error(info, "fasta_nuc bin_width must be > 0"); delete b; return; }                          // :505-510
    std::string index_path;
    if (char *x = get_named_varchar(info, "region")) { b->region = x; b->has_region = x[0] != '\0'; dfree(x); }
    if (char *x = get_named_varchar(info, "index_path")) { index_path = x; dfree(x); }
    if (char *x = get_named_varchar(info, "bed_index_path")) { b->bed_index_path = x; dfree(x); }
    b->include_seq = get_named_bool(info, "include_seq") != 0;
    // fai_load3_format (:532) opens the FASTA and its index; it would BUILD a missing index, this project never does
    if (!file_exists(b->fasta) || !read_file(index_path.empty() ? b->fasta + ".fai" : index_path, b->fai)) { set_error(info, "fasta_nuc: failed to open FASTA index"); delete b; return; }
    auto mk = API(duckdb_logical_type, duckdb_create_logical_type, int);
    auto add = API(void, duckdb_bind_add_result_column, duckdb_bind_info, const char *, duckdb_logical_type);
    auto rm = API(void, duckdb_destroy_logical_type, duckdb_logical_type *);
    duckdb_logical_type t_varchar = mk(DUCKDB_TYPE_VARCHAR), t_bigint = mk(DUCKDB_TYPE_BIGINT), t_double = mk(DUCKDB_TYPE_DOUBLE);
    for (idx_t c = 0; c < (idx_t)(b->include_seq ? DHTS_NUC_COL_COUNT : DHTS_NUC_SEQ); c++)                                                  // :451-473
        add(info, kNucCols[c], nuc_is_varchar(c) ? t_varchar : (c == DHTS_NUC_PCT_AT || c == DHTS_NUC_PCT_GC) ? t_double : t_bigint);
    rm(&t_varchar); rm(&t_bigint); rm(&t_double);
    API(void, duckdb_bind_set_bind_data, duckdb_bind_info, void *, duckdb_delete_callback_t)(info, b, destroy_nuc_bind);
}
static void fasta_nuc_init(duckdb_init_info info) {
    NucBind *bind = (NucBind *)API(void *, duckdb_init_get_bind_data, duckdb_init_info)(info);
    auto init_error = API(void, duckdb_init_set_error, duckdb_init_info, const char *);
    NucScanState *g = new NucScanState();
    g->bin_width = bind->bin_width;
    g->ctx = dhts_create(device_list()[0]);
    if (!g->ctx) { init_error(info, "fasta_nuc: no MI355X (gfx950) device available; this build has no CPU fallback"); delete g; return; }
    auto fail_ctx = [&]() { const std::string m = std::string("fasta_nuc: ") + dhts_error(g->ctx); init_error(info, m.c_str()); delete g; };
    if (dhts_fasta_load_index(g->ctx, bind->fai.data(), bind->fai.size()) != 0) { init_error(info, "fasta_nuc: failed to load FASTA index"); delete g; return; }   // :578-583
    if (bind->has_region && !file_is_bgzf(bind->fasta)) {
        // an uncompressed file: only what the region reads -- its own window for bins, its whole sequence for BED rows, which may reach past it
        if (dhts_nuc_open_region(g->ctx, bind->fasta.c_str(), bind->region.c_str(), bind->has_bed ? 1 : 0) != 0) { init_error(info, "fasta_nuc: failed to load FASTA index"); delete g; return; }
    } else {
        if (dhts_open_path(g->ctx, bind->fasta.c_str()) != 0) { init_error(info, "fasta_nuc: failed to load FASTA index"); delete g; return; }
        (void)dhts_bgzf_index(g->ctx);
    }
    if (dhts_nuc_open(g->ctx, bind->include_seq ? 1 : 0) != 0) { fail_ctx(); return; }
    if (bind->has_region) {
        const int rc = dhts_nuc_set_region(g->ctx, bind->region.c_str());
        if (rc != 0) { init_error(info, "fasta_nuc: invalid FASTA region"); delete g; return; }                                                // :584-588
    }
    if (bind->has_bed) {
        if (!file_exists(bind->bed)) { init_error(info, "fasta_nuc: failed to open BED file"); delete g; return; }                              // :591-596
        g->bed = dhts_create(device_list()[0]);
        if (!g->bed) { init_error(info, "fasta_nuc: no MI355X (gfx950) device available; this build has no CPU fallback"); delete g; return; }
        // tbx_index_load3 with HTS_IDX_SILENT_FAIL (:598): without an index there is no iterator, the whole BED is read and filtered
        std::string index; bool have = false, staged = false;
        if (bind->has_region && file_is_bgzf(bind->bed)) {
            have = bind->bed_index_path.empty() ? (read_file(bind->bed + ".tbi", index) || read_file(bind->bed + ".csi", index)) : read_file(bind->bed_index_path, index);
            if (have && index.size() < 4) have = false;
        }
        if (have) {
            uint64_t beg[4096], end[4096]; int64_t cnt = -1;
            const int rc = dhts_bed_region_segments(g->bed, bind->region.c_str(), index.data(), index.size(), beg, end, 4096, &cnt);
            if (rc != 0) { init_error(info, "fasta_nuc: failed to create BED region iterator"); delete g; return; }                          // :600-605
            if (cnt >= 0) {
                if (dhts_open_path_segments(g->bed, bind->bed.c_str(), 0, beg, end, cnt) != 0) { init_error(info, "fasta_nuc: failed to open BED file"); delete g; return; }
                staged = true;
            }
        }
        if (!staged && dhts_open_path(g->bed, bind->bed.c_str()) != 0) { init_error(info, "fasta_nuc: failed to open BED file"); delete g; return; }
        (void)dhts_bgzf_index(g->bed);
        if (dhts_bed_open(g->bed) != 0) { init_error(info, "fasta_nuc: failed to open BED file"); delete g; return; }
        if (have) {
            if (dhts_bed_set_region(g->bed, bind->region.c_str()) != 0 || dhts_bed_load_index(g->bed, index.data(), index.size()) != 0) { init_error(info, "fasta_nuc: failed to create BED region iterator"); delete g; return; }
        }
    }
    const idx_t n = API(idx_t, duckdb_init_get_column_count, duckdb_init_info)(info);
    std::vector<int32_t> proj;
    const idx_t ncols = bind->include_seq ? DHTS_NUC_COL_COUNT : DHTS_NUC_SEQ;
    for (idx_t i = 0; i < n; i++) {
        const idx_t id = API(idx_t, duckdb_init_get_column_index, duckdb_init_info, idx_t)(info, i);
        g->column_ids.push_back(id);
        int at = -1;
        if (id < ncols) {
            for (size_t k = 0; k < proj.size(); k++) if (proj[k] == (int32_t)id) at = (int)k;
            if (at < 0) { at = (int)proj.size(); proj.push_back((int32_t)id); }
        }
        g->slot.push_back(at);
    }
    if (dhts_nuc_set_projection(g->ctx, proj.data(), (int32_t)proj.size()) != 0) { fail_ctx(); return; }
    g->host.resize(proj.size() ? proj.size() : 1);
    API(void, duckdb_init_set_max_threads, duckdb_init_info, idx_t)(info, 1);
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, g, destroy_nuc_scan);
}
// the next device batch, read back; false at the end (or on a failure: err set)
static bool nuc_next(NucScanState *g, std::string &err) {
    while (g->status == 0) {
        dhts_nuc_batch b;
        const int rc = g->bed ? dhts_nuc_next_bed(g->ctx, g->bed, 0, &b) : dhts_nuc_next_bins(g->ctx, g->bin_width, 0, &b);
        if (rc != 0) { err = dhts_error(g->ctx); return false; }
        g->status = b.status;
        if (b.n_rows == 0) continue;
        const uint64_t need = dhts_nuc_batch_host_bytes(&b);
        if (need > g->arena_cap) { if (g->arena) dhts_host_free(g->arena); g->arena_cap = need + need / 4 + 4096; g->arena = dhts_host_alloc(g->arena_cap); if (!g->arena) { g->arena_cap = 0; err = "fasta_nuc: out of pinned host memory"; return false; } }
        if (dhts_nuc_batch_fetch(g->ctx, &b, g->arena, g->arena_cap, g->host.data()) != 0) { err = dhts_error(g->ctx); return false; }
        g->n = b.n_rows; g->pos = 0;
        return true;
    }
    return false;
}
static void fasta_nuc_function(duckdb_function_info info, duckdb_data_chunk output) {
    NucScanState *g = (NucScanState *)API(void *, duckdb_function_get_init_data, duckdb_function_info)(info);
    auto set_size = API(void, duckdb_data_chunk_set_size, duckdb_data_chunk, idx_t);
    if (!g || g->done) { set_size(output, 0); return; }
    const idx_t vector_size = API(idx_t, duckdb_vector_size, void)();
    auto get_vec = API(duckdb_vector, duckdb_data_chunk_get_vector, duckdb_data_chunk, idx_t);
    auto assign_len = API(void, duckdb_vector_assign_string_element_len, duckdb_vector, idx_t, const char *, idx_t);
    auto get_data = API(void *, duckdb_vector_get_data, duckdb_vector);
    idx_t row_count = 0;
    while (row_count < vector_size) {
        if (g->pos >= g->n) {
            std::string err;
            if (!nuc_next(g, err)) {
                g->done = true;
                if (!err.empty()) { API(void, duckdb_function_set_error, duckdb_function_info, const char *)(info, err.c_str()); set_size(output, 0); return; }
                break;
            }
        }
        const idx_t take = (idx_t)(g->n - g->pos) < vector_size - row_count ? (idx_t)(g->n - g->pos) : vector_size - row_count;
        for (size_t ci = 0; ci < g->column_ids.size(); ci++) {
            duckdb_vector vec = get_vec(output, ci);
            if (g->slot[ci] < 0) { for (idx_t r = 0; r < take; r++) set_null(vec, row_count + r); continue; }
            const dhts_col &hc = g->host[(size_t)g->slot[ci]];
            if (!nuc_is_varchar(g->column_ids[ci])) {                                  // BIGINT and DOUBLE: eight bytes either way, never NULL
                uint64_t *data = (uint64_t *)get_data(vec); const uint64_t *src = (const uint64_t *)hc.fixed;
                for (idx_t r = 0; r < take; r++) data[row_count + r] = src[g->pos + r];
            } else {
                for (idx_t r = 0; r < take; r++) {
                    const int64_t k = g->pos + (int64_t)r;
                    if (hc.valid[k]) assign_len(vec, row_count + r, (const char *)hc.bytes + hc.off[k], hc.off[k + 1] - hc.off[k]); else set_null(vec, row_count + r);
                }
            }
        }
        g->pos += (int64_t)take; row_count += take;
    }
    set_size(output, row_count);
}
extern "C" __attribute__((visibility("default"))) void register_fasta_nuc_function(duckdb_connection connection) {                     // interval_udf.c:854-876
    duckdb_table_function tf = API(duckdb_table_function, duckdb_create_table_function, void)();
    API(void, duckdb_table_function_set_name, duckdb_table_function, const char *)(tf, "fasta_nuc");
    auto mk = API(duckdb_logical_type, duckdb_create_logical_type, int);
    auto rm = API(void, duckdb_destroy_logical_type, duckdb_logical_type *);
    auto named = API(void, duckdb_table_function_add_named_parameter, duckdb_table_function, const char *, duckdb_logical_type);
    duckdb_logical_type t_varchar = mk(DUCKDB_TYPE_VARCHAR), t_bigint = mk(DUCKDB_TYPE_BIGINT), t_bool = mk(DUCKDB_TYPE_BOOLEAN);
    API(void, duckdb_table_function_add_parameter, duckdb_table_function, duckdb_logical_type)(tf, t_varchar);
    named(tf, "bed_path", t_varchar);
    named(tf, "bin_width", t_bigint);
    named(tf, "region", t_varchar);
    named(tf, "index_path", t_varchar);
    named(tf, "bed_index_path", t_varchar);
    named(tf, "include_seq", t_bool);
    rm(&t_varchar); rm(&t_bigint); rm(&t_bool);
    API(void, duckdb_table_function_set_bind, duckdb_table_function, duckdb_table_function_bind_t)(tf, fasta_nuc_bind);
    API(void, duckdb_table_function_set_init, duckdb_table_function, duckdb_table_function_init_t)(tf, fasta_nuc_init);
    API(void, duckdb_table_function_set_function, duckdb_table_function, duckdb_table_function_t)(tf, fasta_nuc_function);
    API(void, duckdb_table_function_supports_projection_pushdown, duckdb_table_function, bool)(tf, true);
    API(duckdb_state, duckdb_register_table_function, duckdb_connection, duckdb_table_function)(connection, tf);
    API(void, duckdb_destroy_table_function, duckdb_table_function *)(&tf);
}

// ---- read_tabix / read_gtf / read_gff (src/tabix_reader.c): one thread, file order, vector_size rows per chunk ------------------------------
// Generic bind is the reference's peek at the file (:636-771) on the device: dhts_tabix_sniff + dhts_tabix_resolve_schema, with the meta
// character and line_skip of the index when there is one; GTF / GFF have their fixed schema.  Init stages the file -- for a single region
// only its index windows -- and the scan chains the regions of region := 'a,b' (tabix_advance_region_iterator :346-360).
static const char *const kTabixFn[3] = {"read_tabix", "read_gtf", "read_gff"};
static const char *const kGxfCols[9] = {"seqname", "source", "feature", "start", "end", "score", "strand", "frame", "attributes"};
struct TabixBind {
    int mode = DHTS_TABIX_GENERIC; std::string path, index_path, index; bool has_index = false, attr_map = false;
    std::vector<std::string> regions;
    int32_t meta = '#', skip = 0, n_cols = 9; std::vector<int32_t> types; bool skip_header = false;
};
struct TabixScanState {
    dhts_ctx *ctx = nullptr; void *arena = nullptr; uint64_t arena_cap = 0;
    std::vector<idx_t> column_ids; std::vector<int> slot; std::vector<int32_t> slot_type;     // output column -> position in the projection (-1: none)
    std::vector<dhts_col> host; dhts_tabix_map hmap; int64_t n = 0, pos = 0; int32_t status = 0; bool done = false;
    size_t next_region = 0;
    ~TabixScanState() { if (arena) dhts_host_free(arena); if (ctx) dhts_destroy(ctx); }
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
    duckdb_value v = API(duckdb_value, duckdb_bind_get_named_parameter, duckdb_bind_info, const char *)(info, name);
    if (!v) return false;
    bool have = false;
    if (!API(bool, duckdb_is_null_value, duckdb_value)(v)) {
        const idx_t n = API(idx_t, duckdb_get_list_size, duckdb_value)(v);
        for (idx_t i = 0; i < n; i++) {
            duckdb_value e = API(duckdb_value, duckdb_get_list_child, duckdb_value, idx_t)(v, i);
            char *t = API(char *, duckdb_get_varchar, duckdb_value)(e);
            out.push_back(t ? t : ""); if (t) API(void, duckdb_free, void *)(t);
            API(void, duckdb_destroy_value, duckdb_value *)(&e);
        }
        have = n > 0;
    }
    API(void, duckdb_destroy_value, duckdb_value *)(&v);
    return have;
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
    auto dfree = API(void, duckdb_free, void *);
    duckdb_value pv = API(duckdb_value, duckdb_bind_get_parameter, duckdb_bind_info, idx_t)(info, 0);
    char *file_path = API(char *, duckdb_get_varchar, duckdb_value)(pv);
    API(void, duckdb_destroy_value, duckdb_value *)(&pv);
    char err[768];
    if (!file_path || file_path[0] == '\0') { snprintf(err, sizeof(err), "%s requires a file path", kTabixFn[mode]); set_error(info, err); if (file_path) dfree(file_path); return; }   // :520-527
    TabixBind *b = new TabixBind();
    b->mode = mode; b->path = file_path; dfree(file_path);
    if (char *r = get_named_varchar(info, "region")) { b->regions = tabix_split_regions(r); dfree(r); }
    if (char *x = get_named_varchar(info, "index_path")) { b->index_path = x; dfree(x); }
    // tbx_index_load2: index_path, else <path>.tbi, else <path>.csi; a file without a readable index is scanned without one
    b->has_index = b->index_path.empty() ? (read_file(b->path + ".tbi", b->index) || read_file(b->path + ".csi", b->index)) : read_file(b->index_path, b->index);
    if (b->has_index && b->index.size() < 4) b->has_index = false;
    auto mk = API(duckdb_logical_type, duckdb_create_logical_type, int);
    auto add = API(void, duckdb_bind_add_result_column, duckdb_bind_info, const char *, duckdb_logical_type);
    auto rm = API(void, duckdb_destroy_logical_type, duckdb_logical_type *);
    duckdb_logical_type t_varchar = mk(DUCKDB_TYPE_VARCHAR), t_bigint = mk(DUCKDB_TYPE_BIGINT), t_double = mk(DUCKDB_TYPE_DOUBLE), t_integer = mk(DUCKDB_TYPE_INTEGER);
    auto type_of = [&](int32_t t) { return t == DHTS_T_BIGINT ? t_bigint : t == DHTS_T_DOUBLE ? t_double : t == DHTS_T_INTEGER ? t_integer : t_varchar; };
    auto done_types = [&]() { rm(&t_varchar); rm(&t_bigint); rm(&t_double); rm(&t_integer); };
    if (mode != DHTS_TABIX_GENERIC) {                                          // :555-587
        static const int32_t gxf[9] = {DHTS_T_VARCHAR, DHTS_T_VARCHAR, DHTS_T_VARCHAR, DHTS_T_BIGINT, DHTS_T_BIGINT, DHTS_T_DOUBLE, DHTS_T_VARCHAR, DHTS_T_VARCHAR, DHTS_T_VARCHAR};
        b->attr_map = get_named_bool(info, "attributes_map") != 0;
        b->n_cols = 9; b->types.assign(gxf, gxf + 9);
        for (int i = 0; i < 9; i++) add(info, kGxfCols[i], type_of(gxf[i]));
        if (b->attr_map) {
            duckdb_logical_type t_map = API(duckdb_logical_type, duckdb_create_map_type, duckdb_logical_type, duckdb_logical_type)(t_varchar, t_varchar);
            add(info, "attributes_map", t_map); rm(&t_map);
        }
    } else {
        const bool header = get_named_bool(info, "header") != 0, auto_detect = get_named_bool(info, "auto_detect") != 0;
        std::vector<std::string> hn, ct;
        const bool have_hn = get_named_list(info, "header_names", hn), have_ct = get_named_list(info, "column_types", ct);
        if (!file_exists(b->path)) { set_error(info, "Cannot open file"); done_types(); delete b; return; }               // :636-641
        dhts_ctx *c = dhts_create(device_list()[0]);
        if (!c) { set_error(info, "read_tabix: no MI355X (gfx950) device available; this build has no CPU fallback"); done_types(); delete b; return; }
        auto bail = [&](const char *msg) { const std::string m = msg; set_error(info, m.c_str()); dhts_destroy(c); done_types(); delete b; };
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
        for (int32_t i = 0; i < sch->n_cols; i++) add(info, sch->names[i], type_of(sch->types[i]));
        delete sch;
        dhts_destroy(c);
    }
    done_types();
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
        if (rc == 0) { g->status = 0; return 1; }
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
    g->ctx = dhts_create(device_list()[0]);
    if (!g->ctx) { snprintf(msg, sizeof(msg), "%s: no MI355X (gfx950) device available; this build has no CPU fallback", kTabixFn[bind->mode]); init_error(info, msg); delete g; return; }
    auto bail = [&](const char *m) { const std::string t = m; init_error(info, t.c_str()); delete g; };
    snprintf(msg, sizeof(msg), "Cannot open file: %s", bind->path.c_str());
    bool staged = false;
    if (bind->regions.size() == 1) {
        // one region of a BGZF file: nothing but its index windows is staged
        uint8_t h[18] = {0}; size_t got = 0;
        if (FILE *f = fopen(bind->path.c_str(), "rb")) { got = fread(h, 1, 18, f); fclose(f); }
        const bool bgzf = got == 18 && h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && (h[3] & 4) && h[12] == 'B' && h[13] == 'C';
        if (bgzf) {
            uint64_t beg[4096], end[4096]; int64_t cnt = -1;
            const int rc = dhts_tabix_region_segments(g->ctx, bind->regions[0].c_str(), bind->index.data(), bind->index.size(), beg, end, 4096, &cnt);
            if (rc < 0) { bail(dhts_error(g->ctx)); return; }
            if (rc == 0 && cnt > 0) {
                if (dhts_open_path_segments(g->ctx, bind->path.c_str(), 0, beg, end, cnt) != 0) { bail(msg); return; }
                staged = true;
            }
        }
    }
    if (!staged && dhts_open_path(g->ctx, bind->path.c_str()) != 0) { bail(msg); return; }
    (void)dhts_bgzf_index(g->ctx);                               // (text that is not BGZF fails here and is taken as text by dhts_tabix_open)
    if (dhts_tabix_open(g->ctx, bind->mode) != 0) { bail(msg); return; }
    if (bind->mode == DHTS_TABIX_GENERIC) {
        if (dhts_tabix_set_conf(g->ctx, bind->meta, bind->skip) != 0 || dhts_tabix_set_schema(g->ctx, bind->n_cols, bind->types.data(), bind->skip_header ? 1 : 0) != 0) { bail(dhts_error(g->ctx)); return; }
    }
    const idx_t n = API(idx_t, duckdb_init_get_column_count, duckdb_init_info)(info);
    const idx_t lim = bind->mode == DHTS_TABIX_GENERIC ? (idx_t)bind->n_cols : (idx_t)(bind->attr_map ? 10 : 9);
    std::vector<int32_t> proj, proj_type;
    for (idx_t i = 0; i < n; i++) {
        const idx_t id = API(idx_t, duckdb_init_get_column_index, duckdb_init_info, idx_t)(info, i);
        g->column_ids.push_back(id);
        int at = -1;
        if (id < lim) {
            for (size_t k = 0; k < proj.size(); k++) if (proj[k] == (int32_t)id) at = (int)k;
            if (at < 0) { at = (int)proj.size(); proj.push_back((int32_t)id); proj_type.push_back(id < (idx_t)bind->n_cols ? bind->types[id] : 0); }
        }
        g->slot.push_back(at); g->slot_type.push_back(at >= 0 ? proj_type[(size_t)at] : 0);
    }
    if (dhts_tabix_set_projection(g->ctx, proj.data(), (int32_t)proj.size()) != 0) { bail(dhts_error(g->ctx)); return; }
    if (!bind->regions.empty()) {
        std::string err;
        const int rc = tabix_advance(bind, g, err);
        if (rc < 0) { bail(err.c_str()); return; }
        if (rc == 0) g->done = true;                             // no region matches a sequence of the index: an empty result (:821-824)
    }
    g->host.resize(proj.size() ? proj.size() : 1);
    API(void, duckdb_init_set_max_threads, duckdb_init_info, idx_t)(info, 1);
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, g, destroy_tabix_scan);
}
// the next device batch, read back; false at the end of the scan or on a failure (err set)
static bool tabix_next(const TabixBind *bind, TabixScanState *g, std::string &err) {
    for (;;) {
        while (g->status == 0) {
            dhts_tabix_batch b;
            if (dhts_tabix_next_batch(g->ctx, 0, &b) != 0) { err = dhts_error(g->ctx); return false; }
            g->status = b.status;
            if (b.n_rows == 0) continue;
            const uint64_t need = dhts_tabix_batch_host_bytes(&b);
            if (need > g->arena_cap) { if (g->arena) dhts_host_free(g->arena); g->arena_cap = need + need / 4 + 4096; g->arena = dhts_host_alloc(g->arena_cap); if (!g->arena) { g->arena_cap = 0; err = "read_tabix: out of pinned host memory"; return false; } }
            if (dhts_tabix_batch_fetch(g->ctx, &b, g->arena, g->arena_cap, g->host.data(), &g->hmap) != 0) { err = dhts_error(g->ctx); return false; }
            g->n = b.n_rows; g->pos = 0;
            return true;
        }
        if (bind->regions.empty() || g->status < 0) return false;
        const int rc = tabix_advance(bind, g, err);                            // the iterator is exhausted: the next region (:888-894)
        if (rc <= 0) return false;
    }
}
static void tabix_read_function(duckdb_function_info info, duckdb_data_chunk output) {
    TabixScanState *g = (TabixScanState *)API(void *, duckdb_function_get_init_data, duckdb_function_info)(info);
    const TabixBind *bind = (const TabixBind *)API(void *, duckdb_function_get_bind_data, duckdb_function_info)(info);
    auto set_size = API(void, duckdb_data_chunk_set_size, duckdb_data_chunk, idx_t);
    if (!g || g->done) { set_size(output, 0); return; }
    const idx_t vector_size = API(idx_t, duckdb_vector_size, void)();
    auto get_vec = API(duckdb_vector, duckdb_data_chunk_get_vector, duckdb_data_chunk, idx_t);
    auto assign_len = API(void, duckdb_vector_assign_string_element_len, duckdb_vector, idx_t, const char *, idx_t);
    auto get_data = API(void *, duckdb_vector_get_data, duckdb_vector);
    idx_t row_count = 0;
    while (row_count < vector_size) {
        if (g->pos >= g->n) {
            std::string err;
            if (!tabix_next(bind, g, err)) {
                g->done = true;
                if (!err.empty()) { API(void, duckdb_function_set_error, duckdb_function_info, const char *)(info, err.c_str()); set_size(output, 0); return; }
                break;
            }
        }
        const idx_t take = (idx_t)(g->n - g->pos) < vector_size - row_count ? (idx_t)(g->n - g->pos) : vector_size - row_count;
        for (size_t ci = 0; ci < g->column_ids.size(); ci++) {
            duckdb_vector vec = get_vec(output, ci);
            if (g->slot[ci] < 0) { for (idx_t r = 0; r < take; r++) set_null(vec, row_count + r); continue; }
            const dhts_col &hc = g->host[(size_t)g->slot[ci]];
            const int32_t ty = g->slot_type[ci];
            const int64_t s = g->pos;
            if (ty == 0) {                                                     // attributes_map, filled like the auxiliary-tag map of read_bam
                const dhts_tabix_map &m = g->hmap;
                duckdb_list_entry *le = (duckdb_list_entry *)get_data(vec);
                const idx_t base = API(idx_t, duckdb_list_vector_get_size, duckdb_vector)(vec);
                const uint32_t c0 = m.pair_off[s], c1 = m.pair_off[s + (int64_t)take];
                if (c1 > c0) { API(duckdb_state, duckdb_list_vector_reserve, duckdb_vector, idx_t)(vec, base + (c1 - c0)); API(duckdb_state, duckdb_list_vector_set_size, duckdb_vector, idx_t)(vec, base + (c1 - c0)); }
                duckdb_vector child = API(duckdb_vector, duckdb_list_vector_get_child, duckdb_vector)(vec);
                duckdb_vector kvec = API(duckdb_vector, duckdb_struct_vector_get_child, duckdb_vector, idx_t)(child, 0);
                duckdb_vector vvec = API(duckdb_vector, duckdb_struct_vector_get_child, duckdb_vector, idx_t)(child, 1);
                for (idx_t r = 0; r < take; r++) {
                    le[row_count + r].offset = base + (m.pair_off[s + r] - c0); le[row_count + r].length = m.pair_off[s + r + 1] - m.pair_off[s + r];
                    if (!m.valid[s + r]) set_null(vec, row_count + r);
                }
                for (uint32_t k = c0; k < c1; k++) {
                    assign_len(kvec, base + (k - c0), (const char *)m.key_bytes + m.key_off[k], m.key_off[k + 1] - m.key_off[k]);
                    assign_len(vvec, base + (k - c0), (const char *)m.val_bytes + m.val_off[k], m.val_off[k + 1] - m.val_off[k]);
                }
            } else if (ty == DHTS_T_VARCHAR) {
                for (idx_t r = 0; r < take; r++) {
                    const int64_t k = s + (int64_t)r;
                    if (hc.valid[k]) assign_len(vec, row_count + r, (const char *)hc.bytes + hc.off[k], hc.off[k + 1] - hc.off[k]); else set_null(vec, row_count + r);
                }
            } else if (ty == DHTS_T_INTEGER) {
                // the reference declares INTEGER and stores 8-byte values into the 4-byte vector (:1004-1008); here a value that fits is stored, another is NULL
                int32_t *data = (int32_t *)get_data(vec); const int64_t *src = (const int64_t *)hc.fixed;
                for (idx_t r = 0; r < take; r++) { const int64_t v = src[s + r]; if (hc.valid[s + r] && v >= INT32_MIN && v <= INT32_MAX) data[row_count + r] = (int32_t)v; else set_null(vec, row_count + r); }
            } else {                                                           // BIGINT and DOUBLE: 8 bytes as they are
                int64_t *data = (int64_t *)get_data(vec); const int64_t *src = (const int64_t *)hc.fixed;
                for (idx_t r = 0; r < take; r++) { if (hc.valid[s + r]) data[row_count + r] = src[s + r]; else set_null(vec, row_count + r); }
            }
        }
        g->pos += (int64_t)take; row_count += take;
    }
    set_size(output, row_count);
}
static void register_tabix_tf(duckdb_connection connection, const char *name, duckdb_table_function_bind_t bind) {          // create_tabix_tf :1038-1079
    duckdb_table_function tf = API(duckdb_table_function, duckdb_create_table_function, void)();
    API(void, duckdb_table_function_set_name, duckdb_table_function, const char *)(tf, name);
    auto mk = API(duckdb_logical_type, duckdb_create_logical_type, int);
    auto rm = API(void, duckdb_destroy_logical_type, duckdb_logical_type *);
    auto named = API(void, duckdb_table_function_add_named_parameter, duckdb_table_function, const char *, duckdb_logical_type);
    duckdb_logical_type t_varchar = mk(DUCKDB_TYPE_VARCHAR), t_bool = mk(DUCKDB_TYPE_BOOLEAN);
    duckdb_logical_type t_list = API(duckdb_logical_type, duckdb_create_list_type, duckdb_logical_type)(t_varchar);
    API(void, duckdb_table_function_add_parameter, duckdb_table_function, duckdb_logical_type)(tf, t_varchar);
    named(tf, "region", t_varchar);
    named(tf, "index_path", t_varchar);
    named(tf, "attributes_map", t_bool);
    named(tf, "header", t_bool);
    named(tf, "header_names", t_list);
    named(tf, "auto_detect", t_bool);
    named(tf, "column_types", t_list);
    rm(&t_list); rm(&t_bool); rm(&t_varchar);
    API(void, duckdb_table_function_set_bind, duckdb_table_function, duckdb_table_function_bind_t)(tf, bind);
    API(void, duckdb_table_function_set_init, duckdb_table_function, duckdb_table_function_init_t)(tf, tabix_read_init);
    API(void, duckdb_table_function_set_function, duckdb_table_function, duckdb_table_function_t)(tf, tabix_read_function);
    API(void, duckdb_table_function_supports_projection_pushdown, duckdb_table_function, bool)(tf, true);
    API(duckdb_state, duckdb_register_table_function, duckdb_connection, duckdb_table_function)(connection, tf);
    API(void, duckdb_destroy_table_function, duckdb_table_function *)(&tf);
}
extern "C" __attribute__((visibility("default"))) void register_read_tabix_function(duckdb_connection connection) { register_tabix_tf(connection, "read_tabix", tabix_read_bind); }   // :1081-1085
extern "C" __attribute__((visibility("default"))) void register_read_gtf_function(duckdb_connection connection) { register_tabix_tf(connection, "read_gtf", gtf_read_bind); }
extern "C" __attribute__((visibility("default"))) void register_read_gff_function(duckdb_connection connection) { register_tabix_tf(connection, "read_gff", gff_read_bind); }

#include "duckdb_udf.inc"

extern "C" __attribute__((visibility("default"), weak)) bool duckhts_init_c_api(duckdb_extension_info info, struct duckdb_extension_access *access) {
    // duckdb_extension.h:1151-1158,1182-1194: fetch the API table, connect, register, disconnect
    const void *api = access->get_api(info, DUCKHTS_API_VERSION);
    if (!api) return false;
    dhts_set_duckdb_api(api);
    duckdb_database *db = access->get_database(info);
    duckdb_connection conn = nullptr;
    if (API(duckdb_state, duckdb_connect, duckdb_database, duckdb_connection *)(*db, &conn) == DuckDBError) {
        access->set_error(info, "Failed to open connection to database");
        return false;
    }
    register_read_bcf_function(conn);                     // registration order of src/duckhts.c:54-71
    register_read_bam_function(conn);
    register_bgzip_function(conn); register_bgunzip_function(conn);           // (the readers between them in src/duckhts.c are not on this path)
    register_bam_index_function(conn); register_bcf_index_function(conn); register_tabix_index_function(conn);
    // read_fastq (src/duckhts.c registers it between the readers) is opt-in until the registered set is widened: DHTS_SEQ_FUNCTIONS=1
    // read_fasta and fasta_index are opt-in with it, in the reference's order (src/duckhts.c:56-58): read_fasta, read_fastq, fasta_index
    if (const char *e = getenv("DHTS_SEQ_FUNCTIONS")) if (atoi(e) == 1) { register_read_fasta_function(conn); register_read_fastq_function(conn); register_fasta_index_function(conn); }
    // read_bed follows fasta_index (src/duckhts.c:59), opt-in as well: DHTS_INTERVAL_FUNCTIONS=1
    if (const char *e = getenv("DHTS_INTERVAL_FUNCTIONS")) if (atoi(e) == 1) register_read_bed_function(conn);
    // fasta_nuc follows read_bed (src/duckhts.c:59-60), behind a variable of its own: DHTS_NUC_FUNCTIONS=1
    if (const char *e = getenv("DHTS_NUC_FUNCTIONS")) if (atoi(e) == 1) register_fasta_nuc_function(conn);
    // the k-mer family follows tabix_index and precedes read_tabix (src/duckhts.c:66), behind a variable of its own: DHTS_KMER_FUNCTIONS=1
    if (const char *e = getenv("DHTS_KMER_FUNCTIONS")) if (atoi(e) == 1) register_kmer_udf_functions(conn);
    // read_tabix, read_gtf, read_gff close the list (src/duckhts.c:67-69), opt-in: DHTS_TABIX_FUNCTIONS=1
    if (const char *e = getenv("DHTS_TABIX_FUNCTIONS")) if (atoi(e) == 1) { register_read_tabix_function(conn); register_read_gtf_function(conn); register_read_gff_function(conn); }
    API(void, duckdb_disconnect, duckdb_connection *)(&conn);
    return true;
}
