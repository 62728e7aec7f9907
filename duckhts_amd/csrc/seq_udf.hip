// seq_udf.hip -- the sequence, CIGAR and flag functions of src/kmer_udf.c evaluated on device columns (dhts_udf_* in duckhts_amd.h).
//
// Integer and byte work only.  Three work units, picked by what a row is:
//   * SEQ-like text (reads ~150 bytes, k-mers ~31, contigs much longer): a GROUP of G lanes per row (G = 4, 16 or 64, chosen by the host
//     from the column's mean width).  Lane g of the group takes the 16-byte pieces g, g + G, ... of the row: one (unaligned) 16-byte load
//     per piece, so a wave reads whole cache lines of the arena whatever G is.  Validity, the base counts and the memcmp decision of
//     seq_canonical (the first position where fwd and rev differ) are reduced over the group with log2(G) shuffles -- one reduce step --
//     and the output leaves in 16-byte stores -- one write step.  Functions whose output does not depend on the reduction (seq_revcomp,
//     seq_decode_4bit) write while they validate: a NULL row keeps its reserved bytes with unspecified content.
//   * CIGAR (~4 bytes) and FLAG: a lane per row.
//   * seq_kmers: a lane per k-mer; the output index finds (row, pos) in the prefix sum of max(0, len - k + 1) by bisection and reads its
//     k bytes in 16-byte pieces (neighbouring lanes read overlapping bytes: the loads of a wave cover a few cache lines).
// Pieces live in two 64-bit registers and are indexed with compile-time byte numbers only, the tail of a row is shifted in byte by
// byte; nothing is read or written outside [off[r], off[r] + len[r]) of a row.
#pragma once
#include <stdint.h>

struct Udf16 { uint64_t lo, hi; };
__device__ __forceinline__ uint32_t udf_byte(const Udf16 &v, int j) { return (uint32_t)((j < 8 ? v.lo >> (8 * j) : v.hi >> (8 * (j - 8))) & 0xffu); }
__device__ __forceinline__ void udf_put(Udf16 &v, int j, uint32_t b) { if (j < 8) v.lo |= (uint64_t)b << (8 * j); else v.hi |= (uint64_t)b << (8 * (j - 8)); }
// byte j of the piece = p[j], j < cnt (the rest 0)
__device__ __forceinline__ Udf16 udf_load_left(const uint8_t *p, uint32_t cnt) {
    Udf16 v;
    if (cnt >= 16u) { __builtin_memcpy(&v, p, 16); return v; }
    v.lo = v.hi = 0;
    for (uint32_t i = cnt; i-- > 0;) { v.hi = (v.hi << 8) | (v.lo >> 56); v.lo = (v.lo << 8) | p[i]; }
    return v;
}
// byte 16 - cnt + i of the piece = p[i], i < cnt: the piece a reversed read indexes with 15 - j
__device__ __forceinline__ Udf16 udf_load_right(const uint8_t *p, uint32_t cnt) {
    Udf16 v;
    if (cnt >= 16u) { __builtin_memcpy(&v, p, 16); return v; }
    v.lo = v.hi = 0;
    for (uint32_t i = 0; i < cnt; i++) { v.lo = (v.lo >> 8) | (v.hi << 56); v.hi = (v.hi >> 8) | ((uint64_t)p[i] << 56); }
    return v;
}
__device__ __forceinline__ void udf_store_left(uint8_t *p, uint32_t cnt, Udf16 v) {
    if (cnt >= 16u) { __builtin_memcpy(p, &v, 16); return; }
    for (uint32_t i = 0; i < cnt; i++) { p[i] = (uint8_t)v.lo; v.lo = (v.lo >> 8) | (v.hi << 56); v.hi >>= 8; }
}

// dna_complement (kmer_udf.c:88-97): toupper, then A<->T, C<->G, N->N, anything else 0.  c & 0xdf equals a capital letter only for that
// letter and its lower case, which is all toupper does in the C locale.
__device__ __forceinline__ uint32_t udf_comp(uint32_t c) {
    const uint32_t u = c & 0xdfu;
    return u == 'A' ? 'T' : u == 'C' ? 'G' : u == 'G' ? 'C' : u == 'T' ? 'A' : u == 'N' ? 'N' : 0u;
}
// dna_to_2bit (:99-107); 4 = not ACGT
__device__ __forceinline__ uint32_t udf_2bit(uint32_t c) {
    const uint32_t u = c & 0xdfu;
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 4u;
}
// iupac_to_4bit (:109-128); 0 = no code.  Nibble k of the two constants = the code of the letter 'A' + k.
__device__ __forceinline__ uint32_t udf_iupac(uint32_t c) {
    const uint32_t k = (c & 0xdfu) - 'A';
    if (k > 24u) return 0u;
    return (uint32_t)((k < 16u ? 0x00f30c00b400d2e1ull >> (4u * k) : 0xa09708650ull >> (4u * (k - 16u))) & 15u);
}
// bit4_to_iupac (:130-149); 0 = no base.  "=ACMGRSV" "TWYHKDBN", byte k = the base of code k.
__device__ __forceinline__ uint32_t udf_base_of(uint32_t code) {
    if (code - 1u > 14u) return 0u;
    return (uint32_t)((code < 8u ? 0x565352474d434100ull >> (8u * code) : 0x4e42444b48595754ull >> (8u * (code - 8u))) & 0xffu);
}

template <int G> __device__ __forceinline__ uint32_t udf_and(uint32_t v) { for (int m = G / 2; m > 0; m >>= 1) v &= (uint32_t)__shfl_xor((int)v, m, 64); return v; }
template <int G> __device__ __forceinline__ uint32_t udf_sum(uint32_t v) { for (int m = G / 2; m > 0; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64); return v; }
template <int G> __device__ __forceinline__ uint64_t udf_or64(uint64_t v) { for (int m = G / 2; m > 0; m >>= 1) v |= (uint64_t)__shfl_xor((unsigned long long)v, m, 64); return v; }
template <int G> __device__ __forceinline__ uint64_t udf_min64(uint64_t v) {
    for (int m = G / 2; m > 0; m >>= 1) { const uint64_t t = (uint64_t)__shfl_xor((unsigned long long)v, m, 64); v = t < v ? t : v; }
    return v;
}

// seq_canonical's decision (:361-383) for the row s[0, len), lane g of G: fwd = the upper-cased row, rev = its reverse complement; returns
// 1 when memcmp(fwd, rev) > 0, i.e. rev is chosen (a tie keeps fwd).  ok &= every byte is one of ACGTN in either case.
template <int G> __device__ __forceinline__ uint32_t udf_canon_decide(const uint8_t *s, uint32_t len, uint32_t g, uint32_t &ok) {
    uint32_t bestpos = 0xffffffffu, gt = 0;
    for (uint64_t p = (uint64_t)g * 16u; p < len; p += (uint64_t)G * 16u) {
        const uint32_t cnt = len - p < 16u ? (uint32_t)(len - p) : 16u;
        const Udf16 F = udf_load_left(s + p, cnt), R = udf_load_right(s + (len - p - cnt), cnt);
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t cf = udf_byte(F, j), f = cf & 0xdfu, r = udf_comp(udf_byte(R, 15 - j));
            if ((uint32_t)j < cnt) {
                ok &= udf_comp(cf) != 0u;
                if (f != r && bestpos == 0xffffffffu) { bestpos = (uint32_t)p + (uint32_t)j; gt = f > r; }
            }
        }
    }
    const uint64_t key = udf_min64<G>(((uint64_t)bestpos << 1) | gt);
    ok = udf_and<G>(ok);
    return (uint32_t)(key >> 1) != 0xffffffffu && (key & 1u);
}
// the chosen text of a valid row: fwd upper-cased, or the reverse complement
template <int G> __device__ __forceinline__ void udf_canon_write(const uint8_t *s, uint32_t len, uint32_t g, uint32_t use_rev, uint8_t *d) {
    for (uint64_t p = (uint64_t)g * 16u; p < len; p += (uint64_t)G * 16u) {
        const uint32_t cnt = len - p < 16u ? (uint32_t)(len - p) : 16u;
        Udf16 w = {0, 0};
        if (use_rev) {
            const Udf16 R = udf_load_right(s + (len - p - cnt), cnt);
#pragma unroll
            for (int j = 0; j < 16; j++) udf_put(w, j, udf_comp(udf_byte(R, 15 - j)));
        } else {
            const Udf16 F = udf_load_left(s + p, cnt);
#pragma unroll
            for (int j = 0; j < 16; j++) udf_put(w, j, udf_byte(F, j) & 0xdfu);
        }
        udf_store_left(d + p, cnt, w);
    }
}
// seq_hash_2bit (:409-418) of s[0, len), len <= 32, read forwards or as its reverse complement, by ONE lane; ok &= every base is ACGT
__device__ __forceinline__ uint64_t udf_hash_lane(const uint8_t *s, uint32_t len, uint32_t use_rev, uint32_t &ok) {
    uint64_t h = 0;
    for (uint32_t p = 0; p < len; p += 16u) {
        const uint32_t cnt = len - p < 16u ? len - p : 16u;
        const Udf16 v = use_rev ? udf_load_right(s + (len - p - cnt), cnt) : udf_load_left(s + p, cnt);
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t code = udf_2bit(use_rev ? udf_comp(udf_byte(v, 15 - j)) : udf_byte(v, j));
            if ((uint32_t)j < cnt) { ok &= code < 4u; h = (h << 2) | (code & 3u); }
        }
    }
    return h;
}

// what a string function writes; which members are set depends on the function
struct UdfOut {
    uint8_t *valid;            // n rows, 1 = valid
    uint32_t *len;             // VARCHAR results: the row's length (the offsets are the input's)
    uint8_t *bytes;            // VARCHAR results: the arena, laid out as the input's
    uint64_t *u64; double *f64;
    uint32_t *clen;            // seq_encode_4bit: children of the row (0 for a NULL row)
    const uint32_t *child_off; uint8_t *child;     // seq_encode_4bit, write pass
};
enum { UDF_OP_ENCODE_WRITE = 100 };     // the second pass of seq_encode_4bit, behind the scan of clen

template <int OP, int G>
__global__ void __launch_bounds__(256) udf_seq_rows(dhts_udf_arg a, uint32_t n, UdfOut o) {
    const uint64_t row64 = (uint64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    if (row64 >= n) return;                                  // (whole groups leave: G divides 64)
    const uint32_t row = (uint32_t)row64, g = threadIdx.x % G;
    const bool in_valid = OP == UDF_OP_ENCODE_WRITE ? o.valid[row] != 0 : (!a.valid || a.valid[row]);
    const uint32_t base = a.off[row];
    const uint32_t len = in_valid ? (a.len ? a.len[row] : a.off[row + 1] - base) : 0u;
    const uint8_t *s = a.bytes + base;
    uint32_t ok = in_valid ? 1u : 0u;
    if constexpr (OP == DHTS_UDF_SEQ_REVCOMP) {                                           // :316-324
        uint8_t *d = o.bytes + base;
        for (uint64_t p = (uint64_t)g * 16u; p < len; p += (uint64_t)G * 16u) {
            const uint32_t cnt = len - p < 16u ? (uint32_t)(len - p) : 16u;
            const Udf16 R = udf_load_right(s + (len - p - cnt), cnt);
            Udf16 w = {0, 0};
#pragma unroll
            for (int j = 0; j < 16; j++) { const uint32_t r = udf_comp(udf_byte(R, 15 - j)); if ((uint32_t)j < cnt) ok &= r != 0u; udf_put(w, j, r); }
            udf_store_left(d + p, cnt, w);
        }
        ok = udf_and<G>(ok);
        if (g == 0) { o.valid[row] = (uint8_t)ok; o.len[row] = ok ? len : 0u; }
    } else if constexpr (OP == DHTS_UDF_SEQ_CANONICAL) {
        const uint32_t use_rev = udf_canon_decide<G>(s, len, g, ok);
        if (ok) udf_canon_write<G>(s, len, g, use_rev, o.bytes + base);
        if (g == 0) { o.valid[row] = (uint8_t)ok; o.len[row] = ok ? len : 0u; }
    } else if constexpr (OP == DHTS_UDF_SEQ_HASH_2BIT) {                                  // :404-418
        uint64_t h = 0;
        if (len > 32u) ok = 0;
        else for (uint32_t p = g * 16u; p < len; p += (uint32_t)G * 16u) {
            const uint32_t cnt = len - p < 16u ? len - p : 16u;
            const Udf16 F = udf_load_left(s + p, cnt);
            uint64_t part = 0;
#pragma unroll
            for (int j = 0; j < 16; j++) { const uint32_t code = udf_2bit(udf_byte(F, j)); if ((uint32_t)j < cnt) { ok &= code < 4u; part = (part << 2) | (code & 3u); } }
            h |= part << (2u * (len - p - cnt));                                           // (cnt = 16 bases are 32 bits, shifted by at most 32)
        }
        h = udf_or64<G>(h); ok = udf_and<G>(ok);
        if (g == 0) { o.valid[row] = (uint8_t)ok; o.u64[row] = ok ? h : 0ull; }
    } else if constexpr (OP == DHTS_UDF_SEQ_GC_CONTENT) {                                 // :544-579
        uint32_t gc = 0, called = 0;
        for (uint64_t p = (uint64_t)g * 16u; p < len; p += (uint64_t)G * 16u) {
            const uint32_t cnt = len - p < 16u ? (uint32_t)(len - p) : 16u;
            const Udf16 F = udf_load_left(s + p, cnt);
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const uint32_t u = udf_byte(F, j) & 0xdfu;
                if ((uint32_t)j < cnt) { const uint32_t is_gc = u == 'G' || u == 'C', is_at = u == 'A' || u == 'T'; gc += is_gc; called += is_gc + is_at; ok &= is_gc || is_at || u == 'N'; }
            }
        }
        gc = udf_sum<G>(gc); called = udf_sum<G>(called); ok = udf_and<G>(ok);
        ok = ok && len > 0u && called > 0u;
        if (g == 0) { o.valid[row] = (uint8_t)ok; o.f64[row] = ok ? (double)gc / (double)called : 0.0; }
    } else if constexpr (OP == DHTS_UDF_SEQ_ENCODE_4BIT) {                                // :458-466, the validity and the child count
        for (uint64_t p = (uint64_t)g * 16u; p < len; p += (uint64_t)G * 16u) {
            const uint32_t cnt = len - p < 16u ? (uint32_t)(len - p) : 16u;
            const Udf16 F = udf_load_left(s + p, cnt);
#pragma unroll
            for (int j = 0; j < 16; j++) if ((uint32_t)j < cnt) ok &= udf_iupac(udf_byte(F, j)) != 0u;
        }
        ok = udf_and<G>(ok);
        if (g == 0) { o.valid[row] = (uint8_t)ok; o.clen[row] = ok ? len : 0u; }
    } else if constexpr (OP == UDF_OP_ENCODE_WRITE) {                                     // the children of the valid rows, compacted
        uint8_t *d = o.child + o.child_off[row];
        for (uint64_t p = (uint64_t)g * 16u; p < len; p += (uint64_t)G * 16u) {
            const uint32_t cnt = len - p < 16u ? (uint32_t)(len - p) : 16u;
            const Udf16 F = udf_load_left(s + p, cnt);
            Udf16 w = {0, 0};
#pragma unroll
            for (int j = 0; j < 16; j++) udf_put(w, j, udf_iupac(udf_byte(F, j)));
            udf_store_left(d + p, cnt, w);
        }
    } else if constexpr (OP == DHTS_UDF_SEQ_DECODE_4BIT) {                                // :503-516; the row is a list of 1-byte codes
        uint8_t *d = o.bytes + base;
        const uint8_t *cv = a.child_valid ? a.child_valid + base : nullptr;
        for (uint64_t p = (uint64_t)g * 16u; p < len; p += (uint64_t)G * 16u) {
            const uint32_t cnt = len - p < 16u ? (uint32_t)(len - p) : 16u;
            const Udf16 F = udf_load_left(s + p, cnt);
            Udf16 V = {~0ull, ~0ull}; if (cv) V = udf_load_left(cv + p, cnt);
            Udf16 w = {0, 0};
#pragma unroll
            for (int j = 0; j < 16; j++) { const uint32_t ch = udf_base_of(udf_byte(F, j)); if ((uint32_t)j < cnt) ok &= ch != 0u && udf_byte(V, j) != 0u; udf_put(w, j, ch); }
            udf_store_left(d + p, cnt, w);
        }
        ok = udf_and<G>(ok);
        if (g == 0) { o.valid[row] = (uint8_t)ok; o.len[row] = ok ? len : 0u; }
    }
}

// ---- CIGAR: a lane per row -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool udf_is_cigar_op(uint32_t c) { return c == 'M' || c == 'I' || c == 'D' || c == 'N' || c == 'S' || c == 'H' || c == 'P' || c == '=' || c == 'X'; }
// op: DHTS_UDF_CIGAR_HAS_SOFT_CLIP .. DHTS_UDF_CIGAR_HAS_OP.  BOOLEAN results in b8, BIGINT in i64.  parse_cigar_metrics (:197-269) and
// cigar_has_operator_text (:271-295) byte for byte; a length that leaves int64 wraps (the reference's behaviour there is undefined).
__global__ void __launch_bounds__(256) udf_cigar_rows(dhts_udf_arg a, dhts_udf_arg b, int op, uint32_t n, uint8_t *valid, uint8_t *b8, long long *i64) {
    const uint64_t row64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (row64 >= n) return;
    const uint32_t row = (uint32_t)row64;
    bool ok = !a.valid || a.valid[row];
    const uint32_t base = a.off[row], len = ok ? (a.len ? a.len[row] : a.off[row + 1] - base) : 0u;
    const uint8_t *s = a.bytes + base;
    long long res = 0;
    if (op == DHTS_UDF_CIGAR_HAS_OP) {
        const uint32_t rb = b.is_const ? 0u : row;
        ok = ok && (!b.valid || b.valid[rb]);
        uint32_t want = 0;
        if (ok) {
            const uint32_t bb = b.off[rb], bl = b.len ? b.len[rb] : b.off[rb + 1] - bb;
            ok = bl == 1u;
            if (ok) { want = b.bytes[bb]; if (want >= 'a' && want <= 'z') want -= 32u; ok = udf_is_cigar_op(want); }
        }
        if (ok && !(len == 0u || (len == 1u && s[0] == '*'))) {
            unsigned long long ol = 0; int has = 0;
            for (uint32_t i = 0; i < len; i++) {
                const uint32_t ch = s[i];
                if (ch - '0' < 10u) { ol = ol * 10ull + (ch - '0'); continue; }
                if ((long long)ol <= 0) { has = -1; break; }
                if (ch == want) { has = 1; break; }
                ol = 0;
            }
            if (has == 0 && ol != 0) has = -1;
            ok = has >= 0; res = has > 0;
        }
        valid[row] = ok; b8[row] = ok ? (uint8_t)res : 0;
        return;
    }
    unsigned long long ol = 0, first_len = 0, last_len = 0, qlen = 0, alen = 0, rlen = 0; uint32_t first_op = 0, last_op = 0; bool saw = false, soft = false, hard = false;
    ok = ok && !(len == 0u || (len == 1u && s[0] == '*'));
    for (uint32_t i = 0; ok && i < len; i++) {
        const uint32_t ch = s[i];
        if (ch - '0' < 10u) { ol = ol * 10ull + (ch - '0'); continue; }
        if ((long long)ol <= 0 || !udf_is_cigar_op(ch)) { ok = false; break; }
        if (ch == 'M' || ch == '=' || ch == 'X') { qlen += ol; alen += ol; rlen += ol; }
        else if (ch == 'I') qlen += ol;
        else if (ch == 'S') { qlen += ol; soft = true; }
        else if (ch == 'H') hard = true;
        else if (ch == 'D' || ch == 'N') rlen += ol;
        if (!saw) { first_op = ch; first_len = ol; }
        last_op = ch; last_len = ol; saw = true; ol = 0;
    }
    ok = ok && saw && ol == 0;
    switch (op) {
    case DHTS_UDF_CIGAR_HAS_SOFT_CLIP: res = soft; break;
    case DHTS_UDF_CIGAR_HAS_HARD_CLIP: res = hard; break;
    case DHTS_UDF_CIGAR_LEFT_SOFT_CLIP: res = first_op == 'S' ? (long long)first_len : 0; break;
    case DHTS_UDF_CIGAR_RIGHT_SOFT_CLIP: res = last_op == 'S' ? (long long)last_len : 0; break;
    case DHTS_UDF_CIGAR_QUERY_LENGTH: res = (long long)qlen; break;
    case DHTS_UDF_CIGAR_ALIGNED_QUERY_LENGTH: res = (long long)alen; break;
    default: res = (long long)rlen; break;
    }
    valid[row] = ok;
    if (op <= DHTS_UDF_CIGAR_HAS_HARD_CLIP) b8[row] = ok ? (uint8_t)res : 0; else i64[row] = ok ? res : 0;
}

// ---- FLAG: a lane per row -----------------------------------------------------------------------------------------------------------
// get_int64_at (:158-195): the integer of `width` bytes (negative: signed) at row r
__device__ __forceinline__ long long udf_int_at(const dhts_udf_arg &a, uint32_t r) {
    switch (a.width) {
    case 1: return ((const uint8_t *)a.fixed)[r];
    case -1: return ((const int8_t *)a.fixed)[r];
    case 2: return ((const uint16_t *)a.fixed)[r];
    case -2: return ((const int16_t *)a.fixed)[r];
    case 4: return ((const uint32_t *)a.fixed)[r];
    case -4: return ((const int32_t *)a.fixed)[r];
    default: return ((const long long *)a.fixed)[r];
    }
}
// mask: the predicate's bit (is_paired ...); sam_flag_has takes it from b; sam_flag_bits writes 12 arrays of n bytes behind each other,
// in the order of SAM_FLAG_FIELD_MASKS (:36-49), which is bit 0 .. bit 11
__global__ void __launch_bounds__(256) udf_flag_rows(dhts_udf_arg a, dhts_udf_arg b, int op, uint32_t mask, uint32_t n, uint8_t *valid, uint8_t *b8) {
    const uint64_t row64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (row64 >= n) return;
    const uint32_t row = (uint32_t)row64, ra = a.is_const ? 0u : row;
    bool ok = !a.valid || a.valid[ra];
    long long f = 0;
    if (ok) { f = udf_int_at(a, ra); ok = f >= 0 && f <= 0xffff; }
    if (op == DHTS_UDF_SAM_FLAG_HAS) {
        const uint32_t rb = b.is_const ? 0u : row;
        ok = ok && (!b.valid || b.valid[rb]);
        if (ok) { const long long m = udf_int_at(b, rb); ok = m >= 0 && m <= 0xffff; mask = (uint32_t)m; }
    }
    if (op == DHTS_UDF_SAM_FLAG_BITS) {
        valid[row] = ok;
        for (uint32_t k = 0; k < 12u; k++) b8[(uint64_t)k * n + row] = ok ? (uint8_t)(((uint32_t)f >> k) & 1u) : 0;
        return;
    }
    uint32_t res;
    if (op == DHTS_UDF_IS_FORWARD_ALIGNED) { ok = ok && !((uint32_t)f & 4u); res = !((uint32_t)f & 16u); }
    else res = ((uint32_t)f & mask) != 0u;
    valid[row] = ok; b8[row] = ok ? (uint8_t)res : 0;
}

// ---- seq_kmers ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) udf_kmer_counts(dhts_udf_arg a, uint32_t n, uint32_t k, uint32_t *cnt) {
    const uint64_t row64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (row64 >= n) return;
    const uint32_t row = (uint32_t)row64;
    const bool ok = !a.valid || a.valid[row];
    const uint32_t len = ok ? (a.len ? a.len[row] : a.off[row + 1] - a.off[row]) : 0u;
    cnt[row] = len >= k ? len - k + 1u : 0u;                     // :882-885
}
struct UdfKmerOut {
    long long *row, *pos;          // m entries each
    uint32_t *off; uint8_t *bytes, *kvalid;      // text: off[m + 1] = t * k, k bytes per k-mer; NULL when not wanted
    uint64_t *hash; uint8_t *hvalid;              // NULL when not wanted (k <= 32)
};
// k-mers start .. start + m - 1 of the column, in (row, pos) order; cum[n + 1] = the prefix sum of udf_kmer_counts
__global__ void __launch_bounds__(256) udf_kmers_emit(dhts_udf_arg a, const uint64_t *cum, uint32_t n, uint32_t k, uint64_t start, uint32_t m, int canonical, UdfKmerOut o) {
    const uint64_t t64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t64 >= m) return;
    const uint32_t t = (uint32_t)t64;
    const uint64_t T = start + t;
    uint32_t lo = 0, hi = n;                                      // the first row r with cum[r + 1] > T (T < cum[n])
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; if (cum[mid + 1] > T) hi = mid; else lo = mid + 1u; }
    if (lo >= n) lo = n - 1u;
    const uint32_t p0 = (uint32_t)(T - cum[lo]);
    o.row[t] = (long long)lo; o.pos[t] = (long long)p0 + 1;       // :941
    const uint8_t *s = a.bytes + a.off[lo] + p0;
    uint32_t ok = 1, use_rev = 0;
    if (canonical) use_rev = udf_canon_decide<1>(s, k, 0, ok);   // :948-966
    if (o.bytes) {
        uint8_t *d = o.bytes + (uint64_t)t * k;
        o.off[t] = t * k; if (t == m - 1u) o.off[m] = m * k;
        if (!canonical) for (uint32_t p = 0; p < k; p += 16u) { const uint32_t cnt = k - p < 16u ? k - p : 16u; udf_store_left(d + p, cnt, udf_load_left(s + p, cnt)); }   // :944, the raw bytes
        else if (ok) udf_canon_write<1>(s, k, 0, use_rev, d);
        o.kvalid[t] = (uint8_t)ok;
    }
    if (o.hash) {
        uint32_t hok = ok;
        const uint64_t h = hok ? udf_hash_lane(s, k, use_rev, hok) : 0ull;
        o.hash[t] = hok ? h : 0ull; o.hvalid[t] = (uint8_t)hok;
    }
}

// one text kernel launch: n rows, G lanes each
template <int OP> static void udf_launch_rows(hipStream_t st, int G, const dhts_udf_arg &a, uint32_t n, const UdfOut &o) {
    const unsigned grid = (unsigned)(((uint64_t)n * (uint64_t)G + 255u) / 256u);
    if (G == 4) hipLaunchKernelGGL((udf_seq_rows<OP, 4>), dim3(grid), dim3(256), 0, st, a, n, o);
    else if (G == 16) hipLaunchKernelGGL((udf_seq_rows<OP, 16>), dim3(grid), dim3(256), 0, st, a, n, o);
    else hipLaunchKernelGGL((udf_seq_rows<OP, 64>), dim3(grid), dim3(256), 0, st, a, n, o);
}
