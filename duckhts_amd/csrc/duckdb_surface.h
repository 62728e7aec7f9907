// duckdb_surface.h -- what the DuckDB table functions share (duckdb_ext.cpp with its duckdb_*.inc parts, duckdb_tools.cpp): one
// definition per idiom of the C-API surface.  Registration, parameter access, result columns, the environment switches, the bind-time
// context, the file helpers of the region readers, the streaming open, the pinned read-back arena, the projection map, the LIST / MAP entry
// frame and the chunk loop over a batch of dhts_col columns.  (The batch pipeline of read_bam and read_bcf is duckdb_pipeline.h.)
// static / inline only: every translation unit that includes it gets its own copy, nothing here is exported.
#ifndef DUCKHTS_DUCKDB_SURFACE_H
#define DUCKHTS_DUCKDB_SURFACE_H
#include "../../include/duckhts_amd.h"
#include "../../include/duckhts_extension.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <string>
#include <vector>

// duckdb_ext_api_v1 viewed as an array of function pointers (slot numbers: include/duckdb_abi_slots.h)
#define API(ret, name, ...) ((ret(*)(__VA_ARGS__))duckdb_ext_api[SLOT_##name])

static inline void set_null(duckdb_vector vec, idx_t row) {           // src/bam_reader.c:38-42
    API(void, duckdb_vector_ensure_validity_writable, duckdb_vector)(vec);
    uint64_t *v = API(uint64_t *, duckdb_vector_get_validity, duckdb_vector)(vec);
    v[row / 64] &= ~((uint64_t)1 << (row % 64));
}

// ---- registration: create, name, VARCHAR path, parameters, callbacks, pushdown, register, destroy ----------------------------------
// (register_read_bam_function src/bam_reader.c:1044-1068 and its like in every reader of the reference)
enum { PARAM_LIST_VARCHAR = -1 };                                      // Param.type: a DUCKDB_TYPE_* id, or LIST(VARCHAR)
struct Param { const char *name; int type; };                          // name == nullptr: one more positional parameter behind the path
static inline void register_table_function(duckdb_connection connection, const char *name, const std::vector<Param> &params, duckdb_table_function_bind_t bind,
                                           duckdb_table_function_init_t init, duckdb_table_function_init_t local_init, duckdb_table_function_t function, bool pushdown) {
    duckdb_table_function tf = API(duckdb_table_function, duckdb_create_table_function, void)();
    API(void, duckdb_table_function_set_name, duckdb_table_function, const char *)(tf, name);
    auto mk = API(duckdb_logical_type, duckdb_create_logical_type, int);
    auto rm = API(void, duckdb_destroy_logical_type, duckdb_logical_type *);
    duckdb_logical_type tv = mk(DUCKDB_TYPE_VARCHAR);
    API(void, duckdb_table_function_add_parameter, duckdb_table_function, duckdb_logical_type)(tf, tv);
    for (const Param &p : params) {
        duckdb_logical_type t = p.type == PARAM_LIST_VARCHAR ? API(duckdb_logical_type, duckdb_create_list_type, duckdb_logical_type)(tv) : mk(p.type);
        if (p.name) API(void, duckdb_table_function_add_named_parameter, duckdb_table_function, const char *, duckdb_logical_type)(tf, p.name, t);
        else API(void, duckdb_table_function_add_parameter, duckdb_table_function, duckdb_logical_type)(tf, t);
        rm(&t);
    }
    rm(&tv);
    API(void, duckdb_table_function_set_bind, duckdb_table_function, duckdb_table_function_bind_t)(tf, bind);
    API(void, duckdb_table_function_set_init, duckdb_table_function, duckdb_table_function_init_t)(tf, init);
    if (local_init) API(void, duckdb_table_function_set_local_init, duckdb_table_function, duckdb_table_function_init_t)(tf, local_init);
    API(void, duckdb_table_function_set_function, duckdb_table_function, duckdb_table_function_t)(tf, function);
    if (pushdown) API(void, duckdb_table_function_supports_projection_pushdown, duckdb_table_function, bool)(tf, true);
    API(duckdb_state, duckdb_register_table_function, duckdb_connection, duckdb_table_function)(connection, tf);
    API(void, duckdb_destroy_table_function, duckdb_table_function *)(&tf);
}

// ---- bind parameters: DuckDB's value and buffer are released here, the caller owns a std::string ------------------------------------
// the first positional parameter; false when it is missing or empty (every reader's "... requires a file path")
static inline bool take_path(duckdb_bind_info info, std::string &out) {
    duckdb_value v = API(duckdb_value, duckdb_bind_get_parameter, duckdb_bind_info, idx_t)(info, 0);
    char *s = API(char *, duckdb_get_varchar, duckdb_value)(v);
    API(void, duckdb_destroy_value, duckdb_value *)(&v);
    out = s ? s : "";
    if (s) API(void, duckdb_free, void *)(s);
    return !out.empty();
}
// a named parameter's value, or nullptr when it is unset or NULL; the caller destroys it
static inline duckdb_value named_value(duckdb_bind_info info, const char *name) {
    duckdb_value v = API(duckdb_value, duckdb_bind_get_named_parameter, duckdb_bind_info, const char *)(info, name);
    if (v && API(bool, duckdb_is_null_value, duckdb_value)(v)) API(void, duckdb_destroy_value, duckdb_value *)(&v);
    return v;
}
// each: true when the parameter is set (and not NULL); *out is left alone otherwise
static inline bool named_string(duckdb_bind_info info, const char *name, std::string &out) {
    duckdb_value v = named_value(info, name);
    if (!v) return false;
    char *s = API(char *, duckdb_get_varchar, duckdb_value)(v);
    API(void, duckdb_destroy_value, duckdb_value *)(&v);
    if (!s) return false;
    out = s; API(void, duckdb_free, void *)(s);
    return true;
}
static inline bool named_int(duckdb_bind_info info, const char *name, int64_t *out) {
    duckdb_value v = named_value(info, name);
    if (!v) return false;
    *out = API(int64_t, duckdb_get_int64, duckdb_value)(v);
    API(void, duckdb_destroy_value, duckdb_value *)(&v);
    return true;
}
static inline bool named_bool(duckdb_bind_info info, const char *name, bool *out) {
    duckdb_value v = named_value(info, name);
    if (!v) return false;
    *out = API(bool, duckdb_get_bool, duckdb_value)(v);
    API(void, duckdb_destroy_value, duckdb_value *)(&v);
    return true;
}
static inline bool named_flag(duckdb_bind_info info, const char *name) { bool b = false; (void)named_bool(info, name, &b); return b; }   // unset = false

// result columns of a fixed schema: n names with their DUCKDB_TYPE_* / DHTS_T_* ids (the two numberings agree)
static inline void add_columns(duckdb_bind_info info, const char *const *names, const int32_t *types, idx_t n) {
    for (idx_t i = 0; i < n; i++) {
        duckdb_logical_type t = API(duckdb_logical_type, duckdb_create_logical_type, int)(types[i]);
        API(void, duckdb_bind_add_result_column, duckdb_bind_info, const char *, duckdb_logical_type)(info, names[i], t);
        API(void, duckdb_destroy_logical_type, duckdb_logical_type *)(&t);
    }
}
static inline void add_map_column(duckdb_bind_info info, const char *name) {                  // MAP(VARCHAR, VARCHAR), src/bam_reader.c:539-548
    duckdb_logical_type tv = API(duckdb_logical_type, duckdb_create_logical_type, int)(DUCKDB_TYPE_VARCHAR);
    duckdb_logical_type tm = API(duckdb_logical_type, duckdb_create_map_type, duckdb_logical_type, duckdb_logical_type)(tv, tv);
    API(void, duckdb_bind_add_result_column, duckdb_bind_info, const char *, duckdb_logical_type)(info, name, tm);
    API(void, duckdb_destroy_logical_type, duckdb_logical_type *)(&tm); API(void, duckdb_destroy_logical_type, duckdb_logical_type *)(&tv);
}

// ---- the device a function runs on, and the one message for "there is none" ---------------------------------------------------------
static inline std::vector<int> device_list() {
    std::vector<int> d;
    if (const char *e = getenv("DHTS_DEVICES")) { for (const char *q = e; *q;) { char *end; long v = strtol(q, &end, 10); if (end == q) break; d.push_back((int)v); q = *end ? end + 1 : end; } }
    if (d.empty()) d.push_back(getenv("DHTS_DEVICE") ? atoi(getenv("DHTS_DEVICE")) : 0);
    return d;
}
// ---- the scan's environment switches, each read once per process -------------------------------------------------------------------
static inline bool env_is_zero(const char *name) { const char *e = getenv(name); return e && atoi(e) == 0; }
static inline int64_t env_batch_blocks(int64_t dflt) {                 // DHTS_BATCH_BLOCKS: BGZF blocks per batch (every caller has its own default)
    static const int64_t v = getenv("DHTS_BATCH_BLOCKS") ? atoll(getenv("DHTS_BATCH_BLOCKS")) : 0;
    return v > 0 ? v : dflt;
}
static inline int env_fill_threads() {                                 // DHTS_THREADS: workers that fill chunks, 1..64 (1: rows in file order)
    const int t = getenv("DHTS_THREADS") ? atoi(getenv("DHTS_THREADS")) : 1;
    return t < 1 ? 1 : t > 64 ? 64 : t;
}
static inline bool env_stream() { static const bool v = !env_is_zero("DHTS_STREAM"); return v; }                       // 0: stage the whole file before the scan starts
static inline bool env_overlap_readback() { static const bool v = !env_is_zero("DHTS_OVERLAP_READBACK"); return v; }   // 0: copy a batch, wait, hand it over
static inline bool env_sparse() { static const bool v = !env_is_zero("DHTS_SPARSE"); return v; }                       // 0: a region query stages the whole file
static inline double now_s() { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec; }

static inline int env_device() { return getenv("DHTS_DEVICE") ? atoi(getenv("DHTS_DEVICE")) : 0; }
static inline std::string no_device_message(const char *fn_name) { return std::string(fn_name) + ": no MI355X (gfx950) device available; this build has no CPU fallback"; }
// a context on `device` (default: the first of device_list()); nullptr with err = the function's no-device message
static inline dhts_ctx *create_ctx(const char *fn_name, std::string &err, int device = -1) {
    dhts_ctx *c = dhts_create(device < 0 ? device_list()[0] : device);
    if (!c) err = no_device_message(fn_name);
    return c;
}

// ---- files ---------------------------------------------------------------------------------------------------------------------------
static inline bool file_exists(const std::string &p) { FILE *f = fopen(p.c_str(), "rb"); if (!f) return false; fclose(f); return true; }
static inline bool read_file(const std::string &path, std::string &out) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    char buf[65536]; size_t n; out.clear();
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) out.append(buf, n);
    fclose(f);
    return true;
}
static inline bool read_file(const std::string &path, std::vector<uint8_t> &out) {
    std::string s; if (!read_file(path, s)) return false;
    out.assign(s.begin(), s.end()); return true;
}
// the 18 bytes of a BGZF block header: gzip, deflate, FEXTRA, subfield 'B' 'C'
static inline bool file_is_bgzf(const std::string &path) {
    uint8_t h[18] = {0}; size_t got = 0;
    if (FILE *f = fopen(path.c_str(), "rb")) { got = fread(h, 1, 18, f); fclose(f); }
    return got == 18 && h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && (h[3] & 4) && h[12] == 'B' && h[13] == 'C';
}
// tbx_index_load3's lookup: index_path, else <path>.tbi, else <path>.csi; a file of fewer than 4 bytes is no index
static inline bool load_tabix_index(const std::string &path, const std::string &index_path, std::string &out) {
    const bool have = index_path.empty() ? (read_file(path + ".tbi", out) || read_file(path + ".csi", out)) : read_file(index_path, out);
    return have && out.size() >= 4;
}
// Stages nothing but the index windows of one region (the reference seeks to them).  *seg_rc = the segment call's code, which the
// caller maps to its own errors; the windows are staged when that code is 0 and it found at least min_count of them.
enum { WINDOWS_NOT_STAGED = 0, WINDOWS_STAGED = 1, WINDOWS_OPEN_FAILED = 2 };
typedef int (*region_segments_fn)(dhts_ctx *, const char *region, const void *index_bytes, uint64_t n, uint64_t *beg, uint64_t *end, int64_t cap, int64_t *count);
static inline int stage_region_windows(dhts_ctx *c, const std::string &path, region_segments_fn segments, const std::string &region, const std::string &index, int64_t min_count, int *seg_rc) {
    uint64_t beg[4096], end[4096]; int64_t cnt = -1;
    *seg_rc = segments(c, region.c_str(), index.data(), index.size(), beg, end, 4096, &cnt);
    if (*seg_rc != 0 || cnt < min_count) return WINDOWS_NOT_STAGED;
    return dhts_open_path_segments(c, path.c_str(), 0, beg, end, cnt) != 0 ? WINDOWS_OPEN_FAILED : WINDOWS_STAGED;
}

// ---- a scan that starts while the file is still being staged (dhts_open_path_async): the block table is built over the resident prefix ----
// The header needs the first blocks only: `want` bytes to start with, four times more whenever open(c) cannot read it from those.
template <class Open>
static inline int stream_open(dhts_ctx *c, uint64_t want, int *staged_all, Open open) {
    for (;;) {
        if (dhts_stage_wait(c, want, staged_all) < 0) return -1;
        if (dhts_bgzf_index_staged(c) > 0 && open(c) == 0) return 0;
        if (*staged_all) return -1;
        want *= 4;
    }
}
// Before a batch: with fewer than max_blocks known blocks ahead, wait for (at least) another 128 MiB of the file, then extend the block
// table.  0: nothing to do, 1: extended (seconds[0] waiting for bytes, seconds[1] in the table), -1: failed (dhts_error).
static inline int stream_extend(dhts_ctx *c, int64_t max_blocks, int *staged_all, double *seconds = nullptr) {
    if (*staged_all || dhts_blocks_ahead(c) >= max_blocks) return 0;
    const double t0 = now_s();
    int64_t f = dhts_stage_wait(c, 0, staged_all);
    if (f >= 0 && !*staged_all) f = dhts_stage_wait(c, (uint64_t)f + (128u << 20), staged_all);
    const double t1 = now_s();
    if (f < 0 || dhts_bgzf_index_staged(c) < 0) return -1;
    if (seconds) { seconds[0] += t1 - t0; seconds[1] += now_s() - t1; }
    return 1;
}

// ---- pinned host memory a batch is read back into; grows with a quarter of slack, kept from batch to batch --------------------------
struct PinnedArena {
    void *p = nullptr; uint64_t cap = 0;
    bool reserve(uint64_t need) {                                      // false: out of pinned host memory
        if (need > cap) { if (p) dhts_host_free(p); cap = need + need / 4 + 4096; p = dhts_host_alloc(cap); if (!p) cap = 0; }
        return need <= cap;
    }
    ~PinnedArena() { if (p) dhts_host_free(p); }
};

// ---- projection: output vector -> schema column id -> position among the distinct projected columns ----------------------------------
// (bam_read_local_init src/bam_reader.c:676-679; ids at or past `limit`, e.g. a row-id pseudo column, get slot -1)
struct Projection { std::vector<idx_t> column_ids; std::vector<int> slot; std::vector<int32_t> proj; };
static inline void map_projection(duckdb_init_info info, idx_t limit, Projection &p) {
    const idx_t n = API(idx_t, duckdb_init_get_column_count, duckdb_init_info)(info);
    for (idx_t i = 0; i < n; i++) {
        const idx_t id = API(idx_t, duckdb_init_get_column_index, duckdb_init_info, idx_t)(info, i);
        p.column_ids.push_back(id);
        int at = -1;
        if (id < limit) {
            for (size_t k = 0; k < p.proj.size(); k++) if (p.proj[k] == (int32_t)id) at = (int)k;
            if (at < 0) { at = (int)p.proj.size(); p.proj.push_back((int32_t)id); }
        }
        p.slot.push_back(at);
    }
}

// ---- the entries of a LIST / MAP vector for rows [s, s + take): row r owns the children off[r] .. off[r + 1] - 1, which the caller appends
// behind the vector's current child size, in row order.  A row whose valid byte is 0 is NULL; its entry {offset, 0} is written all the same,
// unless null_keeps_entry: read_bam's absent B tag sets NULL and leaves the entry untouched (src/bam_reader.c:927-930).
struct ListFrame { idx_t base; uint32_t c0, c1; duckdb_vector child; };      // children c0 .. c1 - 1 go to child rows base ..
static inline ListFrame list_entries(duckdb_vector vec, const uint32_t *off, const uint8_t *valid, int64_t s, idx_t take, idx_t row_count, bool null_keeps_entry = false) {
    duckdb_list_entry *le = (duckdb_list_entry *)API(void *, duckdb_vector_get_data, duckdb_vector)(vec);
    ListFrame f; f.base = API(idx_t, duckdb_list_vector_get_size, duckdb_vector)(vec); f.c0 = off[s]; f.c1 = off[s + (int64_t)take];
    if (f.c1 > f.c0) { API(duckdb_state, duckdb_list_vector_reserve, duckdb_vector, idx_t)(vec, f.base + (f.c1 - f.c0)); API(duckdb_state, duckdb_list_vector_set_size, duckdb_vector, idx_t)(vec, f.base + (f.c1 - f.c0)); }
    f.child = API(duckdb_vector, duckdb_list_vector_get_child, duckdb_vector)(vec);
    for (idx_t r = 0; r < take; r++) {
        if (valid[s + r] || !null_keeps_entry) { le[row_count + r].offset = f.base + (off[s + r] - f.c0); le[row_count + r].length = off[s + r + 1] - off[s + r]; }
        if (!valid[s + r]) set_null(vec, row_count + r);
    }
    return f;
}

// ---- the chunk loop of the one-thread readers over a batch of dhts_col columns read back into host memory ----------------------------
enum ColKind { COL_NULL = 0,        // a slot outside the projection: NULL
               COL_STRING,          // bytes / off, NULL where valid is 0
               COL_FIXED8,          // eight bytes (BIGINT, DOUBLE), NULL where valid is 0
               COL_FIXED8_NOT_NULL, // eight bytes, never NULL
               COL_INT32,           // INTEGER from a 64-bit value: NULL where valid is 0 or the value does not fit
               COL_MAP,             // MAP(VARCHAR, VARCHAR) from a dhts_tabix_map
               COL_WIDEN32,         // BIGINT from a 32-bit value, never NULL
               COL_DICT32,          // VARCHAR, never NULL: fixed holds 32-bit ids, off / bytes the text of every id (off[id] .. off[id + 1])
               COL_CHAR8 };         // VARCHAR of one character, never NULL: fixed holds one byte per row
static inline int kind_of_type(int32_t t) { return t == DHTS_T_VARCHAR ? COL_STRING : t == DHTS_T_INTEGER ? COL_INT32 : COL_FIXED8; }
struct ColBatch {
    std::vector<dhts_col> host; int64_t n = 0, pos = 0; int32_t status = 0; bool done = false;   // HOST pointers; rows [pos, n) are still to be handed out
    std::vector<int> kind;                                             // per output vector: its ColKind
    void init(const Projection &p) { host.resize(p.proj.size() ? p.proj.size() : 1); }
};
// rows [s, s + take) of one column -> rows [row_count, row_count + take) of its vector; one straight loop per kind
static inline void fill_col(duckdb_vector vec, int kind, const dhts_col &hc, const dhts_tabix_map *map, int64_t s, idx_t take, idx_t row_count) {
    auto get_data = API(void *, duckdb_vector_get_data, duckdb_vector);
    auto assign_len = API(void, duckdb_vector_assign_string_element_len, duckdb_vector, idx_t, const char *, idx_t);
    switch (kind) {
    case COL_STRING:
        for (idx_t r = 0; r < take; r++) {
            const int64_t k = s + (int64_t)r;
            if (hc.valid[k]) assign_len(vec, row_count + r, (const char *)hc.bytes + hc.off[k], hc.off[k + 1] - hc.off[k]); else set_null(vec, row_count + r);
        }
        break;
    case COL_FIXED8: {
        int64_t *data = (int64_t *)get_data(vec); const int64_t *src = (const int64_t *)hc.fixed;
        for (idx_t r = 0; r < take; r++) { if (hc.valid[s + r]) data[row_count + r] = src[s + r]; else set_null(vec, row_count + r); }
        break;
    }
    case COL_FIXED8_NOT_NULL: {
        uint64_t *data = (uint64_t *)get_data(vec); const uint64_t *src = (const uint64_t *)hc.fixed;
        for (idx_t r = 0; r < take; r++) data[row_count + r] = src[s + r];
        break;
    }
    case COL_INT32: {
        // the reference declares INTEGER and stores 8-byte values into the 4-byte vector (src/tabix_reader.c:1004-1008); here a value that fits is stored, another is NULL
        int32_t *data = (int32_t *)get_data(vec); const int64_t *src = (const int64_t *)hc.fixed;
        for (idx_t r = 0; r < take; r++) { const int64_t v = src[s + r]; if (hc.valid[s + r] && v >= INT32_MIN && v <= INT32_MAX) data[row_count + r] = (int32_t)v; else set_null(vec, row_count + r); }
        break;
    }
    case COL_MAP: {
        // entries {offset = current child size, length}, keys and values appended in row order (fill_attr_map src/tabix_reader.c:412-494)
        const dhts_tabix_map &m = *map;
        const ListFrame f = list_entries(vec, m.pair_off, m.valid, s, take, row_count);
        duckdb_vector kvec = API(duckdb_vector, duckdb_struct_vector_get_child, duckdb_vector, idx_t)(f.child, 0);
        duckdb_vector vvec = API(duckdb_vector, duckdb_struct_vector_get_child, duckdb_vector, idx_t)(f.child, 1);
        for (uint32_t k = f.c0; k < f.c1; k++) {
            assign_len(kvec, f.base + (k - f.c0), (const char *)m.key_bytes + m.key_off[k], m.key_off[k + 1] - m.key_off[k]);
            assign_len(vvec, f.base + (k - f.c0), (const char *)m.val_bytes + m.val_off[k], m.val_off[k + 1] - m.val_off[k]);
        }
        break;
    }
    case COL_WIDEN32: {
        int64_t *data = (int64_t *)get_data(vec); const int32_t *src = (const int32_t *)hc.fixed;
        for (idx_t r = 0; r < take; r++) data[row_count + r] = (int64_t)src[s + r];
        break;
    }
    case COL_DICT32: {
        const int32_t *src = (const int32_t *)hc.fixed;
        for (idx_t r = 0; r < take; r++) { const int32_t id = src[s + r]; assign_len(vec, row_count + r, (const char *)hc.bytes + hc.off[id], hc.off[id + 1] - hc.off[id]); }
        break;
    }
    case COL_CHAR8: {
        const char *src = (const char *)hc.fixed;
        for (idx_t r = 0; r < take; r++) assign_len(vec, row_count + r, src + s + r, 1);
        break;
    }
    default: for (idx_t r = 0; r < take; r++) set_null(vec, row_count + r); break;
    }
}
// One scan call: up to vector_size rows, 0 = done.  next(err) reads the next batch back into b (called once per batch): false at the end of
// the scan or on a failure (err set).  on_end() is asked once when the scan ends without a failure: a message makes the chunk that error.
template <class Next, class OnEnd>
static inline void scan_chunks(duckdb_function_info info, duckdb_data_chunk output, const Projection &p, ColBatch &b, const dhts_tabix_map *map, Next next, OnEnd on_end) {
    auto set_size = API(void, duckdb_data_chunk_set_size, duckdb_data_chunk, idx_t);
    if (b.done) { set_size(output, 0); return; }
    const idx_t vector_size = API(idx_t, duckdb_vector_size, void)();
    auto get_vec = API(duckdb_vector, duckdb_data_chunk_get_vector, duckdb_data_chunk, idx_t);
    idx_t row_count = 0;
    while (row_count < vector_size) {
        if (b.pos >= b.n) {
            std::string err;
            if (!next(err)) {
                b.done = true;
                if (err.empty()) { if (const char *m = on_end()) err = m; else break; }
                API(void, duckdb_function_set_error, duckdb_function_info, const char *)(info, err.c_str()); set_size(output, 0); return;
            }
        }
        const idx_t take = (idx_t)(b.n - b.pos) < vector_size - row_count ? (idx_t)(b.n - b.pos) : vector_size - row_count;
        for (size_t ci = 0; ci < p.column_ids.size(); ci++) fill_col(get_vec(output, ci), b.kind[ci], b.host[p.slot[ci] < 0 ? 0 : (size_t)p.slot[ci]], map, b.pos, take, row_count);
        b.pos += (int64_t)take; row_count += take;
    }
    set_size(output, row_count);
}
template <class Next>
static inline void scan_chunks(duckdb_function_info info, duckdb_data_chunk output, const Projection &p, ColBatch &b, const dhts_tabix_map *map, Next next) {
    scan_chunks(info, output, p, b, map, next, [] { return (const char *)nullptr; });
}
#endif
