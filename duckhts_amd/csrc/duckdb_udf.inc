// duckdb_udf.inc -- part of duckdb_ext.cpp (included there; not a translation unit of its own): register_kmer_udf_functions
// (src/kmer_udf.c:1223-1254), the reference's 29 scalar functions and the seq_kmers table function over dhts_udf_* (duckhts_amd.h).
// Same names, parameter and return types, order and error strings.  A scalar call packs its chunk into pinned memory, makes one
// upload, the kernel launch and one download, and fills the output vector; the work itself is the device's (csrc/seq_udf.hip).
typedef void *duckdb_scalar_function;
typedef void (*duckdb_scalar_function_t)(duckdb_function_info, duckdb_data_chunk, duckdb_vector);
#define HAS_API(name) (duckdb_ext_api[SLOT_##name] != nullptr)

namespace {
// Contexts for scalar calls: a call takes one for itself (so the thread that executes it owns it for the call's duration), creating it
// on DHTS_DEVICE when none is idle, and gives it back; at most UDF_POOL_MAX stay alive between calls.
enum { UDF_POOL_MAX = 8 };
std::mutex g_udf_mu;
std::vector<dhts_ctx *> g_udf_idle;
dhts_ctx *udf_ctx_take() {
    {
        std::lock_guard<std::mutex> lk(g_udf_mu);
        if (!g_udf_idle.empty()) { dhts_ctx *c = g_udf_idle.back(); g_udf_idle.pop_back(); return c; }
    }
    return dhts_create(env_device());
}
void udf_ctx_give(dhts_ctx *c) {
    {
        std::lock_guard<std::mutex> lk(g_udf_mu);
        if (g_udf_idle.size() < UDF_POOL_MAX) { g_udf_idle.push_back(c); return; }
    }
    dhts_destroy(c);
}
// pinned memory of the calling thread, kept between calls: [0] the packed arguments, [1] the fetched result
struct UdfPinned {
    void *p[2] = {nullptr, nullptr}; uint64_t cap[2] = {0, 0};
    uint8_t *need(int k, uint64_t n) {
        if (n > cap[k]) { if (p[k]) dhts_host_free(p[k]); cap[k] = n + n / 2 + 4096; p[k] = dhts_host_alloc(cap[k]); if (!p[k]) cap[k] = 0; }
        return (uint8_t *)p[k];
    }
    ~UdfPinned() { for (int k = 0; k < 2; k++) if (p[k]) dhts_host_free(p[k]); }
};
thread_local UdfPinned t_udf_pin;

const char *const UDF_SQL_NAMES[DHTS_UDF_OP_COUNT] = {
    "seq_revcomp", "seq_canonical", "seq_hash_2bit", "seq_encode_4bit", "seq_decode_4bit", "seq_gc_content",
    "cigar_has_soft_clip", "cigar_has_hard_clip", "cigar_left_soft_clip", "cigar_right_soft_clip", "cigar_query_length", "cigar_aligned_query_length",
    "cigar_reference_length", "cigar_has_op", "sam_flag_bits", "sam_flag_has", "is_forward_aligned",
    "is_paired", "is_proper_pair", "is_unmapped", "is_next_segment_unmapped", "is_reverse_complemented", "is_next_segment_reverse_complemented",
    "is_first_segment", "is_last_segment", "is_secondary", "is_qc_fail", "is_duplicate", "is_supplementary"};
const char *const UDF_FLAG_FIELDS[12] = {"is_paired", "is_proper_pair", "is_unmapped", "is_next_segment_unmapped", "is_reverse_complemented",
    "is_next_segment_reverse_complemented", "is_first_segment", "is_last_segment", "is_secondary", "is_qc_fail", "is_duplicate", "is_supplementary"};   // :21-34

inline bool udf_row_valid(const uint64_t *v, idx_t r) { return !v || ((v[r / 64] >> (r % 64)) & 1u); }
inline uint64_t udf_up8(uint64_t n) { return (n + 7) & ~7ull; }
inline const char *udf_str(const duckdb_string_t *s, uint32_t *len) { *len = s->value.inlined.length; return *len <= 12 ? s->value.inlined.inlined : s->value.pointer.ptr; }

// the bytes one argument vector needs in the pinned buffer; kind 0 VARCHAR, 1 LIST(UTINYINT), 2 integer
uint64_t udf_arg_bytes(duckdb_vector v, int kind, idx_t n) {
    const uint64_t *val = API(uint64_t *, duckdb_vector_get_validity, duckdb_vector)(v);
    uint64_t need = udf_up8((n + 1) * 4) + udf_up8(n) + 8;
    if (kind == 2) return need + n * 8;
    uint64_t total = 0;
    if (kind == 0) { const duckdb_string_t *s = (const duckdb_string_t *)API(void *, duckdb_vector_get_data, duckdb_vector)(v); for (idx_t r = 0; r < n; r++) if (udf_row_valid(val, r)) total += s[r].value.inlined.length; }
    else { const duckdb_list_entry *e = (const duckdb_list_entry *)API(void *, duckdb_vector_get_data, duckdb_vector)(v); for (idx_t r = 0; r < n; r++) if (udf_row_valid(val, r)) total += e[r].length; }
    return need + 2 * udf_up8(total + 1);
}
// packs the vector at `at` (8-aligned) and describes it in *a (host pointers); returns the end; false when a column would reach 4 GiB
bool udf_pack(duckdb_vector v, int kind, idx_t n, uint8_t *&at, dhts_udf_arg *a) {
    memset(a, 0, sizeof(*a));
    const uint64_t *val = API(uint64_t *, duckdb_vector_get_validity, duckdb_vector)(v);
    const void *data = API(void *, duckdb_vector_get_data, duckdb_vector)(v);
    uint8_t *valid = at; at += udf_up8(n);
    for (idx_t r = 0; r < n; r++) valid[r] = udf_row_valid(val, r) ? 1 : 0;
    a->valid = valid;
    if (kind == 2) {                                                   // get_int64_at :158-195
        duckdb_logical_type lt = API(duckdb_logical_type, duckdb_vector_get_column_type, duckdb_vector)(v);
        const int t = (int)API(int, duckdb_get_type_id, duckdb_logical_type)(lt);
        API(void, duckdb_destroy_logical_type, duckdb_logical_type *)(&lt);
        int64_t *o = (int64_t *)at; at += n * 8;
        for (idx_t r = 0; r < n; r++) {
            int64_t x = 0;
            switch (t) {
            case 2: x = ((const int8_t *)data)[r]; break; case 3: x = ((const int16_t *)data)[r]; break; case 4: x = ((const int32_t *)data)[r]; break;
            case 5: x = ((const int64_t *)data)[r]; break; case 6: x = ((const uint8_t *)data)[r]; break; case 7: x = ((const uint16_t *)data)[r]; break;
            case 8: x = ((const uint32_t *)data)[r]; break; case 9: x = (int64_t)((const uint64_t *)data)[r]; break; default: x = 0; break;
            }
            o[r] = valid[r] ? x : 0;
        }
        a->fixed = o; a->width = -8;
        return true;
    }
    uint32_t *off = (uint32_t *)at; at += udf_up8((n + 1) * 4);
    uint64_t total = 0;
    if (kind == 0) {
        const duckdb_string_t *s = (const duckdb_string_t *)data;
        for (idx_t r = 0; r < n; r++) if (valid[r]) total += s[r].value.inlined.length;
        if (total >> 32) return false;
        uint8_t *b = at; at += udf_up8(total + 1);
        uint64_t w = 0;
        for (idx_t r = 0; r < n; r++) { off[r] = (uint32_t)w; if (valid[r]) { uint32_t l; const char *p = udf_str(&s[r], &l); memcpy(b + w, p, l); w += l; } }
        off[n] = (uint32_t)w; a->bytes = b;
    } else {                                                           // :485-487: the list entries, the child's bytes and validity
        const duckdb_list_entry *e = (const duckdb_list_entry *)data;
        duckdb_vector ch = API(duckdb_vector, duckdb_list_vector_get_child, duckdb_vector)(v);
        const uint8_t *cd = (const uint8_t *)API(void *, duckdb_vector_get_data, duckdb_vector)(ch);
        const uint64_t *cv = API(uint64_t *, duckdb_vector_get_validity, duckdb_vector)(ch);
        for (idx_t r = 0; r < n; r++) if (valid[r]) total += e[r].length;
        if (total >> 32) return false;
        uint8_t *b = at; at += udf_up8(total + 1);
        uint8_t *bv = at; at += udf_up8(total + 1);
        uint64_t w = 0;
        for (idx_t r = 0; r < n; r++) {
            off[r] = (uint32_t)w;
            if (valid[r]) for (uint64_t i = 0; i < e[r].length; i++) { const idx_t ci = e[r].offset + i; b[w] = cd[ci]; bv[w] = udf_row_valid(cv, ci) ? 1 : 0; w++; }
        }
        off[n] = (uint32_t)w; a->bytes = b; a->child_valid = bv;
    }
    a->off = off; a->nbytes = total;
    return true;
}

// one chunk: pack -> one upload per argument, the launch, one download -> the output vector
bool udf_run(dhts_ctx *c, int op, duckdb_data_chunk input, duckdb_vector output, idx_t n, std::string &err) {
    const bool two = op == DHTS_UDF_CIGAR_HAS_OP || op == DHTS_UDF_SAM_FLAG_HAS;
    const int kind0 = op == DHTS_UDF_SEQ_DECODE_4BIT ? 1 : op <= DHTS_UDF_CIGAR_HAS_OP ? 0 : 2, kind1 = op == DHTS_UDF_CIGAR_HAS_OP ? 0 : 2;
    duckdb_vector v0 = API(duckdb_vector, duckdb_data_chunk_get_vector, duckdb_data_chunk, idx_t)(input, 0);
    duckdb_vector v1 = two ? API(duckdb_vector, duckdb_data_chunk_get_vector, duckdb_data_chunk, idx_t)(input, 1) : nullptr;
    const uint64_t need = udf_arg_bytes(v0, kind0, n) + (two ? udf_arg_bytes(v1, kind1, n) : 0);
    uint8_t *at = t_udf_pin.need(0, need);
    if (!at) { err = "out of memory"; return false; }
    dhts_udf_arg h0, h1, d0, d1;
    if (!udf_pack(v0, kind0, n, at, &h0) || (two && !udf_pack(v1, kind1, n, at, &h1))) { err = "the strings of one chunk reach 4 GiB"; return false; }
    dhts_udf_result r, h;
    if (dhts_udf_upload(c, 0, &h0, (int64_t)n, &d0) || (two && dhts_udf_upload(c, 1, &h1, (int64_t)n, &d1)) ||
        dhts_udf_apply(c, op, &d0, two ? &d1 : nullptr, (int64_t)n, &r)) { err = dhts_error(c); return false; }
    const uint64_t cap = dhts_udf_result_host_bytes(&r);
    uint8_t *dst = t_udf_pin.need(1, cap + 8);
    if (!dst) { err = "out of memory"; return false; }
    if (dhts_udf_fetch(c, &r, dst, cap, &h)) { err = dhts_error(c); return false; }
    const uint8_t *valid = h.col.valid;
    void *out = API(void *, duckdb_vector_get_data, duckdb_vector)(output);
    if (op == DHTS_UDF_SAM_FLAG_BITS) {                                // :665-692: 12 BOOLEAN children; a NULL row is NULL in the struct and in every child
        for (int k = 0; k < 12; k++) {
            duckdb_vector ch = API(duckdb_vector, duckdb_struct_vector_get_child, duckdb_vector, idx_t)(output, (idx_t)k);
            bool *cd = (bool *)API(void *, duckdb_vector_get_data, duckdb_vector)(ch);
            const uint8_t *src = (const uint8_t *)h.col.fixed + (uint64_t)k * n;
            for (idx_t i = 0; i < n; i++) { if (valid[i]) cd[i] = src[i] != 0; else set_null(ch, i); }
        }
        for (idx_t i = 0; i < n; i++) if (!valid[i]) set_null(output, i);
        return true;
    }
    if (h.is_list) {                                                   // :432-478: the children go behind those the vector already holds
        duckdb_list_entry *le = (duckdb_list_entry *)out;
        const idx_t base = API(idx_t, duckdb_list_vector_get_size, duckdb_vector)(output), total = (idx_t)h.col.child_n;
        if (API(duckdb_state, duckdb_list_vector_reserve, duckdb_vector, idx_t)(output, base + total) != DuckDBSuccess) { err = "failed to reserve list storage"; return false; }
        if (API(duckdb_state, duckdb_list_vector_set_size, duckdb_vector, idx_t)(output, base + total) != DuckDBSuccess) { err = "failed to grow list storage"; return false; }
        duckdb_vector ch = API(duckdb_vector, duckdb_list_vector_get_child, duckdb_vector)(output);
        uint8_t *cd = (uint8_t *)API(void *, duckdb_vector_get_data, duckdb_vector)(ch);
        if (total) memcpy(cd + base, h.col.bytes, total);
        for (idx_t i = 0; i < n; i++) { le[i].offset = base + h.col.off[i]; le[i].length = h.col.off[i + 1] - h.col.off[i]; if (!valid[i]) set_null(output, i); }
        return true;
    }
    if (h.type == DHTS_T_VARCHAR) {
        for (idx_t i = 0; i < n; i++) {
            if (valid[i]) API(void, duckdb_vector_assign_string_element_len, duckdb_vector, idx_t, const char *, idx_t)(output, i, (const char *)h.col.bytes + h.col.off[i], h.len[i]);
            else set_null(output, i);
        }
        return true;
    }
    if (h.type == DHTS_T_BOOLEAN) { bool *o = (bool *)out; const uint8_t *s = (const uint8_t *)h.col.fixed; for (idx_t i = 0; i < n; i++) { if (valid[i]) o[i] = s[i] != 0; else set_null(output, i); } }
    else { memcpy(out, h.col.fixed, n * 8); for (idx_t i = 0; i < n; i++) if (!valid[i]) set_null(output, i); }      // BIGINT, UBIGINT, DOUBLE
    return true;
}

void udf_scalar(duckdb_function_info info, duckdb_data_chunk input, duckdb_vector output) {
    const int op = (int)(uintptr_t)API(void *, duckdb_scalar_function_get_extra_info, duckdb_function_info)(info) - 1;
    if (op < 0 || op >= DHTS_UDF_OP_COUNT) return;
    const idx_t n = API(idx_t, duckdb_data_chunk_get_size, duckdb_data_chunk)(input);
    if (n == 0) return;
    char msg[640];
    dhts_ctx *c = udf_ctx_take();
    if (!c) { API(void, duckdb_scalar_function_set_error, duckdb_function_info, const char *)(info, no_device_message(UDF_SQL_NAMES[op]).c_str()); return; }
    std::string err;
    const bool ok = udf_run(c, op, input, output, n, err);
    udf_ctx_give(c);
    if (!ok) { snprintf(msg, sizeof(msg), "%s: %s", UDF_SQL_NAMES[op], err.c_str()); API(void, duckdb_scalar_function_set_error, duckdb_function_info, const char *)(info, msg); }
}

// ---- seq_kmers(sequence, k, canonical := false) :820-974 ---------------------------------------------------------------------------
struct KmersBind { std::string seq; int64_t k = 0; int canonical = 0; };
struct KmersInit { uint64_t next = 0; bool done = false; };
void kmers_destroy_bind(void *p) { delete (KmersBind *)p; }
void kmers_destroy_init(void *p) { delete (KmersInit *)p; }
void kmers_bind(duckdb_bind_info info) {
    auto bind_err = [&](const char *m) { API(void, duckdb_bind_set_error, duckdb_bind_info, const char *)(info, m); };
    duckdb_value sv = API(duckdb_value, duckdb_bind_get_parameter, duckdb_bind_info, idx_t)(info, 0), kv = API(duckdb_value, duckdb_bind_get_parameter, duckdb_bind_info, idx_t)(info, 1);
    duckdb_value cv = API(duckdb_value, duckdb_bind_get_named_parameter, duckdb_bind_info, const char *)(info, "canonical");
    auto is_null = [&](duckdb_value v) { return !v || API(bool, duckdb_is_null_value, duckdb_value)(v); };
    const char *early = is_null(sv) ? "seq_kmers: sequence must not be NULL" : is_null(kv) ? "seq_kmers: k must not be NULL" : nullptr;
    char *seq = nullptr; int64_t k = 0; int canonical = 0;
    if (!early) {
        seq = API(char *, duckdb_get_varchar, duckdb_value)(sv); k = API(int64_t, duckdb_get_int64, duckdb_value)(kv);
        if (!is_null(cv)) canonical = API(bool, duckdb_get_bool, duckdb_value)(cv) ? 1 : 0;
    }
    if (sv) API(void, duckdb_destroy_value, duckdb_value *)(&sv);
    if (kv) API(void, duckdb_destroy_value, duckdb_value *)(&kv);
    if (cv) API(void, duckdb_destroy_value, duckdb_value *)(&cv);
    if (early) { bind_err(early); return; }
    if (!seq) { bind_err("seq_kmers: failed to read sequence"); return; }
    KmersBind *b = new KmersBind(); b->seq = seq; b->k = k; b->canonical = canonical;
    API(void, duckdb_free, void *)(seq);
    if (k <= 0) { delete b; bind_err("seq_kmers: k must be > 0"); return; }
    if (dhts_device_count() <= 0) { delete b; bind_err(no_device_message("seq_kmers").c_str()); return; }
    duckdb_logical_type tb = API(duckdb_logical_type, duckdb_create_logical_type, int)(DUCKDB_TYPE_BIGINT), tv = API(duckdb_logical_type, duckdb_create_logical_type, int)(DUCKDB_TYPE_VARCHAR);
    API(void, duckdb_bind_add_result_column, duckdb_bind_info, const char *, duckdb_logical_type)(info, "pos", tb);
    API(void, duckdb_bind_add_result_column, duckdb_bind_info, const char *, duckdb_logical_type)(info, "kmer", tv);
    API(void, duckdb_destroy_logical_type, duckdb_logical_type *)(&tb); API(void, duckdb_destroy_logical_type, duckdb_logical_type *)(&tv);
    const uint64_t len = b->seq.size();
    if (HAS_API(duckdb_bind_set_cardinality)) API(void, duckdb_bind_set_cardinality, duckdb_bind_info, idx_t, bool)(info, len >= (uint64_t)k ? len - (uint64_t)k + 1 : 0, true);   // :882-886
    API(void, duckdb_bind_set_bind_data, duckdb_bind_info, void *, duckdb_delete_callback_t)(info, b, kmers_destroy_bind);
}
void kmers_init(duckdb_init_info info) {
    API(void, duckdb_init_set_max_threads, duckdb_init_info, idx_t)(info, 1);
    API(void, duckdb_init_set_init_data, duckdb_init_info, void *, duckdb_delete_callback_t)(info, new KmersInit(), kmers_destroy_init);
}
void kmers_function(duckdb_function_info info, duckdb_data_chunk output) {
    KmersBind *b = (KmersBind *)API(void *, duckdb_function_get_bind_data, duckdb_function_info)(info);
    KmersInit *st = (KmersInit *)API(void *, duckdb_function_get_init_data, duckdb_function_info)(info);
    auto fn_err = [&](const char *m) { API(void, duckdb_function_set_error, duckdb_function_info, const char *)(info, m); };
    if (!b || !st || st->done || b->seq.size() < (uint64_t)b->k) { API(void, duckdb_data_chunk_set_size, duckdb_data_chunk, idx_t)(output, 0); return; }
    char msg[640];
    dhts_ctx *c = udf_ctx_take();
    if (!c) { fn_err(no_device_message("seq_kmers").c_str()); return; }
    const idx_t vs = API(idx_t, duckdb_vector_size)();
    const uint32_t off[2] = {0, (uint32_t)b->seq.size()};
    dhts_udf_arg h; memset(&h, 0, sizeof(h)); h.off = off; h.bytes = (const uint8_t *)b->seq.data(); h.nbytes = b->seq.size();
    dhts_udf_arg d; dhts_udf_kmers km, hk; memset(&km, 0, sizeof(km));
    bool ok = dhts_udf_upload(c, 0, &h, 1, &d) == 0 && dhts_udf_seq_kmers(c, &d, 1, b->k, b->canonical, 1, 0, (int64_t)vs, st->next, &km) == 0;
    uint8_t *dst = nullptr;
    if (ok && km.n_rows > 0) { const uint64_t cap = dhts_udf_kmers_host_bytes(&km); dst = t_udf_pin.need(1, cap + 8); ok = dst && dhts_udf_kmers_fetch(c, &km, dst, cap, &hk) == 0; }
    if (!ok) { snprintf(msg, sizeof(msg), "seq_kmers: %s", dhts_error(c)); udf_ctx_give(c); fn_err(msg); return; }
    udf_ctx_give(c);
    const idx_t m = (idx_t)km.n_rows;
    if (m) {
        duckdb_vector pv = API(duckdb_vector, duckdb_data_chunk_get_vector, duckdb_data_chunk, idx_t)(output, 0), kv = API(duckdb_vector, duckdb_data_chunk_get_vector, duckdb_data_chunk, idx_t)(output, 1);
        memcpy(API(void *, duckdb_vector_get_data, duckdb_vector)(pv), hk.pos, m * 8);
        for (idx_t i = 0; i < m; i++) {
            if (hk.kmer.valid[i]) API(void, duckdb_vector_assign_string_element_len, duckdb_vector, idx_t, const char *, idx_t)(kv, i, (const char *)hk.kmer.bytes + hk.kmer.off[i], hk.kmer.off[i + 1] - hk.kmer.off[i]);
            else set_null(kv, i);
        }
    }
    st->next = km.next; st->done = km.status != 0;
    API(void, duckdb_data_chunk_set_size, duckdb_data_chunk, idx_t)(output, m);
}
void register_seq_kmers(duckdb_connection connection) {                 // :1199-1221
    register_table_function(connection, "seq_kmers", {{nullptr, DUCKDB_TYPE_BIGINT}, {"canonical", DUCKDB_TYPE_BOOLEAN}}, kmers_bind, kmers_init, nullptr, kmers_function, false);   // (sequence, k, canonical := ...)
}
// one scalar function: name, up to two parameter types, the return type (ret = 0: LIST(UTINYINT) in / out as marked, -1: the flag struct)
void register_udf_scalar(duckdb_connection connection, int op, int p0, int p1, int ret) {
    auto mk = [&](int t) -> duckdb_logical_type {
        if (t > 0) return API(duckdb_logical_type, duckdb_create_logical_type, int)(t);
        if (t == 0) { duckdb_logical_type e = API(duckdb_logical_type, duckdb_create_logical_type, int)(DHTS_T_UTINYINT); duckdb_logical_type l = API(duckdb_logical_type, duckdb_create_list_type, duckdb_logical_type)(e); API(void, duckdb_destroy_logical_type, duckdb_logical_type *)(&e); return l; }
        duckdb_logical_type m[12];                                     // :1138-1144
        for (int i = 0; i < 12; i++) m[i] = API(duckdb_logical_type, duckdb_create_logical_type, int)(DUCKDB_TYPE_BOOLEAN);
        duckdb_logical_type s = API(duckdb_logical_type, duckdb_create_struct_type, duckdb_logical_type *, const char **, idx_t)(m, (const char **)UDF_FLAG_FIELDS, 12);
        for (int i = 0; i < 12; i++) API(void, duckdb_destroy_logical_type, duckdb_logical_type *)(&m[i]);
        return s;
    };
    duckdb_scalar_function fn = API(duckdb_scalar_function, duckdb_create_scalar_function)();
    API(void, duckdb_scalar_function_set_name, duckdb_scalar_function, const char *)(fn, UDF_SQL_NAMES[op]);
    duckdb_logical_type t0 = mk(p0), tr = mk(ret);
    API(void, duckdb_scalar_function_add_parameter, duckdb_scalar_function, duckdb_logical_type)(fn, t0);
    if (p1 != -2) { duckdb_logical_type t1 = mk(p1); API(void, duckdb_scalar_function_add_parameter, duckdb_scalar_function, duckdb_logical_type)(fn, t1); API(void, duckdb_destroy_logical_type, duckdb_logical_type *)(&t1); }
    API(void, duckdb_scalar_function_set_return_type, duckdb_scalar_function, duckdb_logical_type)(fn, tr);
    API(void, duckdb_scalar_function_set_extra_info, duckdb_scalar_function, void *, duckdb_delete_callback_t)(fn, (void *)(uintptr_t)(op + 1), nullptr);
    API(void, duckdb_scalar_function_set_function, duckdb_scalar_function, duckdb_scalar_function_t)(fn, udf_scalar);
    API(duckdb_state, duckdb_register_scalar_function, duckdb_connection, duckdb_scalar_function)(connection, fn);
    API(void, duckdb_destroy_logical_type, duckdb_logical_type *)(&t0); API(void, duckdb_destroy_logical_type, duckdb_logical_type *)(&tr);
    API(void, duckdb_destroy_scalar_function, duckdb_scalar_function *)(&fn);
}
}  // namespace

// The reference's order (:1224-1253).  A host whose table has no scalar-function slots (they are NULL) gets the table function only.
extern "C" __attribute__((visibility("default"))) void register_kmer_udf_functions(duckdb_connection connection) {
    const bool scalars = HAS_API(duckdb_create_scalar_function) && HAS_API(duckdb_destroy_scalar_function) && HAS_API(duckdb_scalar_function_set_name) &&
                         HAS_API(duckdb_scalar_function_add_parameter) && HAS_API(duckdb_scalar_function_set_return_type) && HAS_API(duckdb_scalar_function_set_extra_info) &&
                         HAS_API(duckdb_scalar_function_set_function) && HAS_API(duckdb_register_scalar_function) && HAS_API(duckdb_scalar_function_get_extra_info) &&
                         HAS_API(duckdb_scalar_function_set_error) && HAS_API(duckdb_create_struct_type) && HAS_API(duckdb_vector_get_column_type) && HAS_API(duckdb_get_type_id);
    const int V = DUCKDB_TYPE_VARCHAR, B = DUCKDB_TYPE_BOOLEAN, I = DUCKDB_TYPE_BIGINT, U = DUCKDB_TYPE_USMALLINT, NONE = -2;
    if (scalars) {
        register_udf_scalar(connection, DHTS_UDF_SEQ_REVCOMP, V, NONE, V); register_udf_scalar(connection, DHTS_UDF_SEQ_CANONICAL, V, NONE, V);
        register_udf_scalar(connection, DHTS_UDF_SEQ_HASH_2BIT, V, NONE, DHTS_T_UBIGINT); register_udf_scalar(connection, DHTS_UDF_SEQ_ENCODE_4BIT, V, NONE, 0);
        register_udf_scalar(connection, DHTS_UDF_SEQ_DECODE_4BIT, 0, NONE, V); register_udf_scalar(connection, DHTS_UDF_SEQ_GC_CONTENT, V, NONE, DUCKDB_TYPE_DOUBLE);
    }
    register_seq_kmers(connection);
    if (!scalars) return;
    register_udf_scalar(connection, DHTS_UDF_CIGAR_HAS_SOFT_CLIP, V, NONE, B); register_udf_scalar(connection, DHTS_UDF_CIGAR_HAS_HARD_CLIP, V, NONE, B);
    for (int op = DHTS_UDF_CIGAR_LEFT_SOFT_CLIP; op <= DHTS_UDF_CIGAR_REFERENCE_LENGTH; op++) register_udf_scalar(connection, op, V, NONE, I);
    register_udf_scalar(connection, DHTS_UDF_CIGAR_HAS_OP, V, V, B);
    register_udf_scalar(connection, DHTS_UDF_SAM_FLAG_BITS, U, NONE, -1);
    register_udf_scalar(connection, DHTS_UDF_SAM_FLAG_HAS, U, U, B);
    register_udf_scalar(connection, DHTS_UDF_IS_FORWARD_ALIGNED, I, NONE, B);
    for (int op = DHTS_UDF_IS_PAIRED; op <= DHTS_UDF_IS_SUPPLEMENTARY; op++) register_udf_scalar(connection, op, U, NONE, B);
}
