// tabix_text.hip -- tab-delimited text -> the typed columns of read_tabix / read_gtf / read_gff on the device (gfx950).  Included by
// dhts_api.hip after bed_text.hip: the delimiter table (bed_delim_count / bed_delim_fill), bed_field, fq_compact, tabix_intervals,
// vcf_strtoll and vcf_str2dbl_fast are shared as they are.
//
// Restates src/tabix_reader.c on a batch of text:
//   the skip tests of tabix_scan :896-906            -> tabix_classify (one lane per line) + tabix_skip_apply behind a scan of the flags
//   get_field :234-254                               -> two reads of the tab table (bed_field)
//   parse_int64_span / parse_double_span :58-80      -> tabix_fixed; a DOUBLE token the one-operation fast path declines is recorded as a
//                                                       TabixPatch, converted by strtod on the host and written back by tabix_patch_apply
//   duckdb_vector_assign_string_element_len          -> tabix_str_measure, scans (eight columns a launch), tabix_str_gather into ONE arena
//   count_gff_pairs / count_gtf_pairs / fill_attr_map :362-494 -> tabix_attr<false> (measure), three scans, tabix_attr<true> (write): one walk
#pragma once

enum { TABIX_MAX_COLS = 256, TABIX_NUM_BUF = 128, TABIX_GXF_MAP = 9 };
enum { TABIX_K_STR = 0, TABIX_K_INT = 1, TABIX_K_DBL = 2, TABIX_K_MAP = 3 };

// One lane per line.  lend / ntab as bed_classify leaves them (CR dropped, cut at the first NUL).  ne = the line is not empty -- by its
// length BEFORE the NUL cut, line.l -- and is_row = not empty and not a meta line; line_skip and the header line are applied afterwards.
extern "C" __global__ void __launch_bounds__(256)
tabix_classify(BedLines a, uint32_t meta_char, uint32_t *__restrict__ ne) {
    const uint32_t li = blockIdx.x * 256u + threadIdx.x;
    if (li >= a.nlines) return;
    const uint8_t *u = a.u;
    const uint32_t l0 = a.line_off[li];
    const bool open = a.last_open && li + 1 == a.nlines;
    uint32_t l1 = open ? a.text_end : a.line_off[li + 1] - 1u;
    if (l1 > l0 && u[l1 - 1] == '\r') l1--;
    const bool nonempty = l1 > l0;
    uint32_t nt = a.tab0[li + 1] - a.tab0[li];
    if (a.has_nul[li]) {
        uint32_t i = l0; nt = 0;
        for (; i < l1 && u[i] != 0; i++) if (u[i] == '\t') nt++;
        l1 = i;
    }
    a.lend[li] = l1; a.ntab[li] = nt;
    const bool meta = nonempty && meta_char != 0 && u[l0] == (uint8_t)meta_char;
    if (ne) ne[li] = nonempty ? 1u : 0u;
    a.is_row[li] = (nonempty && !meta) ? 1u : 0u;
}
// "the first k lines that carry the flag are no rows": rank = exclusive scan of flag (which may be another array than `keep`)
extern "C" __global__ void __launch_bounds__(256)
tabix_skip_apply(uint32_t *__restrict__ keep, const uint32_t *__restrict__ rank, uint32_t n, uint32_t k) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n && rank[i] < k) keep[i] = 0u;
}
// the line that carries the flag and has rank `want` (the header candidate of the sniff)
extern "C" __global__ void __launch_bounds__(256)
tabix_pick(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ rank, uint32_t n, uint32_t want, uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n && flag[i] && rank[i] == want) *out = i;
}

struct TabixCol { int32_t field, kind, slot, reserved; unsigned long long base; };   // slot: the column's place among the fixed-width / the VARCHAR columns of the
                                                                                    // projection; base: where a VARCHAR column's bytes begin in the arena
struct TabixPatch { uint32_t row, col, pos, len; };             // col = position in the projection; the token is u[pos, pos + len)
struct TabixCols {
    const TabixCol *col; int32_t n, gxf; uint32_t nrows;
    uint8_t *valid;                    // [i * nrows + r], i = position in the projection
    unsigned long long *fixed;         // [slot * nrows + r]: int64, or the bits of a double
    uint32_t *len; const uint32_t *off; uint8_t *bytes;          // [slot * (nrows + 1) + r]; ONE arena, column after column
    TabixPatch *patch; uint32_t *ctr;  // ctr[0] = patches recorded (room for one per row and DOUBLE column), ctr[1] = tokens the fast path converted
};
__device__ __forceinline__ bool tabix_missing(const uint8_t *u, bool have, uint32_t s, uint32_t len) { return !have || len == 0 || (len == 1 && u[s] == '.'); }

// One lane per row, BIGINT and DOUBLE columns: strtoll / strtod over the whole field, NULL from 128 bytes on.  GTF / GFF: a missing start /
// end is 0 and valid.
extern "C" __global__ void __launch_bounds__(256)
tabix_fixed(BedRows a, TabixCols g) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    const bool live = r < a.nrows;
    const uint32_t li = live ? a.row_line[r] : 0u;
    uint32_t nfast = 0;
    if (live) for (int i = 0; i < g.n; i++) {
        const TabixCol c = g.col[i];
        if (c.kind != TABIX_K_INT && c.kind != TABIX_K_DBL) continue;
        uint32_t s = 0, e = 0;
        const bool have = bed_field(a, li, (uint32_t)c.field, false, s, e);
        const uint32_t len = have ? e - s : 0u;
        unsigned long long v = 0; bool ok = false;
        if (tabix_missing(a.u, have, s, len)) ok = g.gxf && c.kind == TABIX_K_INT;
        else if (len < TABIX_NUM_BUF) {
            if (c.kind == TABIX_K_INT) { uint32_t adv = 0; v = (unsigned long long)vcf_strtoll(a.u, s, e, 10, &adv); ok = adv == len; if (!ok) v = 0; }
            else {
                double d = 0.0; uint32_t end = 0;
                if (vcf_str2dbl_fast(a.u + s, len, &d, &end) == 0 && end == len) { v = (unsigned long long)__double_as_longlong(d); ok = true; nfast++; }
                else { const uint32_t k = atomicAdd(g.ctr, 1u); TabixPatch q; q.row = r; q.col = (uint32_t)i; q.pos = s; q.len = len; g.patch[k] = q; }
            }
        }
        g.fixed[(size_t)c.slot * g.nrows + r] = v; g.valid[(size_t)i * g.nrows + r] = ok ? 1 : 0;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) nfast += __shfl_xor(nfast, d, 64);
    if ((threadIdx.x & 63u) == 0 && nfast) atomicAdd(g.ctr + 1, nfast);
}
extern "C" __global__ void __launch_bounds__(256)
tabix_patch_apply(const TabixPatch *__restrict__ patch, const unsigned long long *__restrict__ val, const uint8_t *__restrict__ ok, uint32_t n, TabixCols g) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const TabixPatch q = patch[i];
    g.fixed[(size_t)g.col[q.col].slot * g.nrows + q.row] = ok[i] ? val[i] : 0ull; g.valid[(size_t)q.col * g.nrows + q.row] = ok[i];
}
// the bytes of a VARCHAR value: false = NULL.  GTF / GFF give the one byte "." (dot: written, not copied) where the field is missing.
__device__ __forceinline__ bool tabix_str_span(const BedRows &a, const TabixCols &g, const TabixCol &c, uint32_t li, uint32_t &s, uint32_t &len, bool &dot) {
    uint32_t e = 0; s = 0;
    const bool have = bed_field(a, li, (uint32_t)c.field, false, s, e);
    len = have ? e - s : 0u; dot = false;
    if (!tabix_missing(a.u, have, s, len)) return true;
    len = 0;
    if (!g.gxf) return false;
    dot = true; len = 1;
    return true;
}
extern "C" __global__ void __launch_bounds__(256)
tabix_str_measure(BedRows a, TabixCols g) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.nrows) return;
    const uint32_t li = a.row_line[r];
    for (int i = 0; i < g.n; i++) {
        const TabixCol c = g.col[i];
        if (c.kind != TABIX_K_STR) continue;
        uint32_t s, len; bool dot;
        const bool ok = tabix_str_span(a, g, c, li, s, len, dot);
        g.len[(size_t)c.slot * (g.nrows + 1u) + r] = len; g.valid[(size_t)i * g.nrows + r] = ok ? 1 : 0;
    }
}
// One lane per row copies a short field; a field of more than 64 bytes is copied by the whole wave, 64 bytes per step (as bed_str_gather).
extern "C" __global__ void __launch_bounds__(256)
tabix_str_gather(BedRows a, TabixCols g) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const bool live = r < a.nrows;
    const uint32_t li = live ? a.row_line[r] : 0u;
    for (int i = 0; i < g.n; i++) {
        const TabixCol c = g.col[i];
        if (c.kind != TABIX_K_STR) continue;
        uint8_t *out = g.bytes + c.base;
        uint32_t s = 0, len = 0, d = 0; bool dot = false;
        if (live && tabix_str_span(a, g, c, li, s, len, dot)) d = g.off[(size_t)c.slot * (g.nrows + 1u) + r];
        if (dot) { out[d] = '.'; len = 0; }
        if (len <= 64u) for (uint32_t k = 0; k < len; k++) out[d + k] = a.u[s + k];
        for (unsigned long long m = __ballot(len > 64u); m;) {
            const int src = __builtin_ctzll(m); m &= m - 1;
            const uint32_t ws = __shfl(s, src, 64), wd = __shfl(d, src, 64), wl = __shfl(len, src, 64);
            for (uint32_t k = lane; k < wl; k += 64u) out[wd + k] = a.u[ws + k];
        }
    }
}

// ---- attributes_map ---------------------------------------------------------------------------------------------------------------------
struct TabixAttr {
    int32_t gff;
    uint32_t *npair, *kbytes, *vbytes;                              // measure: per row
    const uint32_t *pair_off, *kb_off, *vb_off;                     // their exclusive scans (nrows + 1 entries)
    uint8_t *valid; uint32_t *key_off, *val_off; uint8_t *key_bytes, *val_bytes;     // write: key_off / val_off have n_pairs + 1 entries
};
__device__ __forceinline__ bool tabix_blank(uint8_t c) { return c == ' ' || c == '\t'; }
__device__ __forceinline__ void tabix_trim(const uint8_t *u, uint32_t &s, uint32_t &l) {      // trim_span
    while (l > 0 && tabix_blank(u[s])) { s++; l--; }
    while (l > 0 && tabix_blank(u[s + l - 1])) l--;
}
// One lane per row walks field 8 once per pass; the measure pass counts what the write pass stores, pair by pair.
template <bool WRITE>
__global__ void __launch_bounds__(256)
tabix_attr(BedRows a, TabixAttr g) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.nrows) return;
    const uint8_t *u = a.u;
    const uint32_t li = a.row_line[r];
    uint32_t p = 0, e = 0;
    const bool have = bed_field(a, li, 8u, false, p, e);
    const bool null = tabix_missing(u, have, p, have ? e - p : 0u);
    uint32_t np = 0, kb = 0, vb = 0;
    if (WRITE) { np = g.pair_off[r]; kb = g.kb_off[r]; vb = g.vb_off[r]; g.valid[r] = null ? 0 : 1; }
    if (!null) while (p < e) {
        while (p < e && (u[p] == ';' || tabix_blank(u[p]))) p++;
        if (p >= e) break;
        uint32_t key = p, klen = 0, val = 0, vlen = 0;
        if (g.gff) {
            while (p < e && u[p] != '=' && u[p] != ';') p++;
            if (p >= e || u[p] != '=') continue;                      // a token without '=': p stands on its ';' (or the end)
            klen = p - key; p++;
            val = p;
            while (p < e && u[p] != ';') p++;
            vlen = p - val;
        } else {
            while (p < e && !tabix_blank(u[p]) && u[p] != ';') p++;
            klen = p - key;
            while (p < e && tabix_blank(u[p])) p++;
            if (p < e && u[p] == '"') {
                p++; val = p;
                while (p < e && u[p] != '"') p++;
                vlen = p - val;
                if (p < e) p++;
            } else {
                val = p;
                while (p < e && u[p] != ';') p++;
                vlen = p - val;
            }
        }
        tabix_trim(u, key, klen); tabix_trim(u, val, vlen);
        if (klen > 0) {
            if (WRITE) {
                g.key_off[np] = kb; g.val_off[np] = vb;
                for (uint32_t k = 0; k < klen; k++) g.key_bytes[kb + k] = u[key + k];
                for (uint32_t k = 0; k < vlen; k++) g.val_bytes[vb + k] = u[val + k];
            }
            np++; kb += klen; vb += vlen;
        }
        while (p < e && u[p] != ';') p++;
        if (p < e) p++;
    }
    if (WRITE) { if (r + 1 == a.nrows) { g.key_off[np] = kb; g.val_off[np] = vb; } }
    else { g.npair[r] = np; g.kbytes[r] = kb; g.vbytes[r] = vb; }
}
