// bed_text.hip -- BED text -> the 13 typed columns of read_bed on the device (gfx950).  Included by dhts_api.hip after vcf_text.hip
// (vcf_strtoll and VCF_CHUNK are shared).
//
// Restates src/interval_udf.c:127-195, 330-426 on a batch of text:
//   hts_getline                               -> bed_delim_count / bed_delim_fill: the line table AND the table of tabs of a batch
//   is_meta_bed_line, count_tab_fields        -> bed_classify (one lane per line)
//   get_field_span / get_extra_span           -> two reads of the tab table (bed_field)
//   parse_int64_span_local                    -> bed_ints
//   duckdb_vector_assign_string_element_len   -> bed_str_measure, an exclusive scan, bed_str_gather (one byte arena per column)
//
// The delimiter table.  One sweep over the text with 16-byte loads counts '\n', '\t' and NUL per 4 KiB chunk; behind a scan of the
// counts a second sweep writes every newline's successor (line_off), every tab's position in order (tab_off), for every line the rank of
// its first tab (tab0: line i owns tabs tab0[i] .. tab0[i + 1] - 1) and a flag on the lines that hold a NUL.  Field k of a line then
// begins behind tab tab0 + k - 1 and ends at tab tab0 + k: no lane walks its line.  A line with a NUL -- the reference reads C strings, so
// the line ends there -- is walked once, by its own lane in bed_classify, to find the NUL and count the tabs in front of it; those are
// the first tabs of the line in the table, so its fields are looked up like any other line's.
#pragma once

enum { BED_N_COLS = 13, BED_N_INT = 5, BED_N_STR = 8 };
// column id -> tab field; the BIGINT columns are 1, 2, 6, 7, 9 (start, end, thick_start, thick_end, block_count), column 12 (extra) is
// everything behind the 12th tab
__host__ __device__ __forceinline__ bool bed_col_is_int(int col) { return col == 1 || col == 2 || col == 6 || col == 7 || col == 9; }

// bit b set: byte b of w equals the byte that `pat` repeats (exact zero-byte test on w ^ pat, the four flags gathered into the low nibble)
__device__ __forceinline__ uint32_t bed_eq4(uint32_t w, uint32_t pat) {
    const uint32_t y = w ^ pat, z = ~(((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y | 0x7f7f7f7fu) >> 7;
    return (z | z >> 7 | z >> 14 | z >> 21) & 0xfu;
}
__device__ __forceinline__ uint32_t bed_eq16(const uint4 v, uint32_t pat) { return bed_eq4(v.x, pat) | bed_eq4(v.y, pat) << 4 | bed_eq4(v.z, pat) << 8 | bed_eq4(v.w, pat) << 12; }
// bit k set: u[p + k] == '\n' / '\t' / 0.  u + p is 16-byte aligned where the whole load lies inside the text.
struct BedMasks { uint32_t nl, tab, nul; };
__device__ __forceinline__ BedMasks bed_masks16(const uint8_t *__restrict__ u, uint64_t p, uint64_t ulen) {
    BedMasks m = {0u, 0u, 0u};
    if (p + 16 <= ulen) {
        const uint4 v = *(const uint4 *)(u + p);
        m.nl = bed_eq16(v, 0x0a0a0a0au); m.tab = bed_eq16(v, 0x09090909u); m.nul = bed_eq16(v, 0u);
    } else for (uint32_t k = 0; k < 16 && p + k < ulen; k++) { const uint32_t c = u[p + k], bit = 1u << k; m.nl |= c == '\n' ? bit : 0u; m.tab |= c == '\t' ? bit : 0u; m.nul |= c == 0 ? bit : 0u; }
    return m;
}
// per chunk: newlines, tabs
extern "C" __global__ void __launch_bounds__(256)
bed_delim_count(const uint8_t *__restrict__ u, uint64_t start, uint64_t ulen, uint32_t *__restrict__ cnt_nl, uint32_t *__restrict__ cnt_tab) {
    __shared__ uint32_t wsum[2][4];
    const uint64_t p = (start & ~(uint64_t)15) + (uint64_t)blockIdx.x * VCF_CHUNK + threadIdx.x * 16u;
    BedMasks m = {0u, 0u, 0u};
    if (p < ulen) m = bed_masks16(u, p, ulen);
    if (p < start) { const uint32_t keep = ~((1u << (start - p)) - 1u); m.nl &= keep; m.tab &= keep; }      // bytes in front of the first line do not count
    const uint32_t m_nl = m.nl, m_tab = m.tab;
    uint32_t a = __popc(m_nl), b = __popc(m_tab);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { a += __shfl_xor(a, d, 64); b += __shfl_xor(b, d, 64); }
    if ((threadIdx.x & 63) == 0) { wsum[0][threadIdx.x >> 6] = a; wsum[1][threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) { cnt_nl[blockIdx.x] = wsum[0][0] + wsum[0][1] + wsum[0][2] + wsum[0][3]; cnt_tab[blockIdx.x] = wsum[1][0] + wsum[1][1] + wsum[1][2] + wsum[1][3]; }
}
// line_off[r + 1] = successor of newline r, tab_off[t] = position of tab t, tab0[r + 1] = tabs in front of newline r, has_nul[line] = 1
// (has_nul is cleared by the caller; nlines_cap = its length).  The lines begin at `start` (a window of a region query begins inside a block).
extern "C" __global__ void __launch_bounds__(256)
bed_delim_fill(const uint8_t *__restrict__ u, uint64_t start, uint64_t ulen, const uint32_t *__restrict__ base_nl, const uint32_t *__restrict__ base_tab,
               uint32_t *__restrict__ line_off, uint32_t *__restrict__ tab_off, uint32_t *__restrict__ tab0, uint32_t *__restrict__ has_nul, uint32_t nlines_cap) {
    __shared__ uint32_t wsum[2][4];
    const uint32_t k = blockIdx.x;
    if (k == 0 && threadIdx.x == 0) { line_off[0] = (uint32_t)start; tab0[0] = 0; }
    const uint64_t p = (start & ~(uint64_t)15) + (uint64_t)k * VCF_CHUNK + threadIdx.x * 16u;
    BedMasks mk = {0u, 0u, 0u};
    if (p < ulen) mk = bed_masks16(u, p, ulen);
    if (p < start) { const uint32_t keep = ~((1u << (start - p)) - 1u); mk.nl &= keep; mk.tab &= keep; mk.nul &= keep; }
    const uint32_t m_nl = mk.nl, m_tab = mk.tab, m_nul = mk.nul;
    const uint32_t n_nl = __popc(m_nl), n_tab = __popc(m_tab);
    uint32_t i_nl = n_nl, i_tab = n_tab;                                        // inclusive scans inside the wave, then across the four waves
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t a = __shfl_up(i_nl, d, 64), b = __shfl_up(i_tab, d, 64);
        if ((int)(threadIdx.x & 63) >= d) { i_nl += a; i_tab += b; }
    }
    if ((threadIdx.x & 63) == 63) { wsum[0][threadIdx.x >> 6] = i_nl; wsum[1][threadIdx.x >> 6] = i_tab; }
    __syncthreads();
    uint32_t r_nl = base_nl[k] + i_nl - n_nl, r_tab = base_tab[k] + i_tab - n_tab;       // newlines / tabs in front of this lane's 16 bytes
    for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) { r_nl += wsum[0][w]; r_tab += wsum[1][w]; }
    for (uint32_t m = m_nul; m;) { const uint32_t b = __ffs(m) - 1; m &= m - 1; const uint32_t li = r_nl + __popc(m_nl & ((1u << b) - 1u)); if (li < nlines_cap) has_nul[li] = 1u; }
    for (uint32_t m = m_tab, t = r_tab; m; t++) { const uint32_t b = __ffs(m) - 1; m &= m - 1; tab_off[t] = (uint32_t)(p + b); }
    for (uint32_t m = m_nl, r = r_nl; m; r++) { const uint32_t b = __ffs(m) - 1; m &= m - 1; line_off[r + 1] = (uint32_t)(p + b + 1); tab0[r + 1] = r_tab + __popc(m_tab & ((1u << b) - 1u)); }
}

struct BedLines {
    const uint8_t *u; const uint32_t *line_off, *tab_off, *tab0; const uint32_t *has_nul;
    uint32_t nlines; uint32_t text_end; int32_t last_open, report_bad;     // line i = u[line_off[i], line_off[i + 1] - 1); the last one ends at text_end when it has no newline
    uint32_t *lend, *ntab, *is_row;                            // per line: where it ends for the reference (CR dropped, cut at a NUL), its tabs in front of that, 1 = a row
    unsigned long long *first_bad;                             // smallest line with fewer than 3 fields (report_bad; a region query reports it for the lines it keeps)
};
// One lane per line: meta or row or error (next_bed_line's skip test, read_bed_scan's field count).
extern "C" __global__ void __launch_bounds__(256)
bed_classify(BedLines a) {
    const uint32_t li = blockIdx.x * 256u + threadIdx.x;
    if (li >= a.nlines) return;
    const uint8_t *u = a.u;
    const uint32_t l0 = a.line_off[li];
    const bool open = a.last_open && li + 1 == a.nlines;
    uint32_t l1 = open ? a.text_end : a.line_off[li + 1] - 1u;
    if (l1 > l0 && u[l1 - 1] == '\r') l1--;                                      // bgzf_getline / hts_getline drop a CR in front of the newline
    uint32_t nt = a.tab0[li + 1] - a.tab0[li];
    if (a.has_nul[li]) {                                                        // rare: the C string ends at the first NUL
        uint32_t i = l0; nt = 0;
        for (; i < l1 && u[i] != 0; i++) if (u[i] == '\t') nt++;
        l1 = i;
    }
    a.lend[li] = l1; a.ntab[li] = nt;
    const uint32_t len = l1 - l0;
    bool meta = len == 0 || u[l0] == '#';
    if (!meta && len >= 5 && u[l0] == 't' && u[l0 + 1] == 'r' && u[l0 + 2] == 'a' && u[l0 + 3] == 'c' && u[l0 + 4] == 'k') meta = true;
    if (!meta && len >= 7 && u[l0] == 'b' && u[l0 + 1] == 'r' && u[l0 + 2] == 'o' && u[l0 + 3] == 'w' && u[l0 + 4] == 's' && u[l0 + 5] == 'e' && u[l0 + 6] == 'r') meta = true;
    a.is_row[li] = meta ? 0u : nt < 2 ? 2u : 1u;                                // 2: fewer than 3 fields, read_bed's error
    if (!meta && nt < 2 && a.report_bad) atomicMin(a.first_bad, (unsigned long long)li);
}
// Region query: a row stays when tabix's interval of its line [beg, end) lies on the queried sequence and end > beg_q and end_q > beg
// (hts_itr_next, hts.c:4287-4300, on what tbx_parse1 made of the line: tabix_intervals).
extern "C" __global__ void __launch_bounds__(256)
bed_region_keep(const uint8_t *__restrict__ u, const TbxLine *__restrict__ t, uint32_t nlines, const uint8_t *__restrict__ name, uint32_t name_len, long long beg_q, long long end_q,
                uint32_t *__restrict__ is_row, unsigned long long *first_bad) {
    const uint32_t li = blockIdx.x * 256u + threadIdx.x;
    if (li >= nlines) return;
    const TbxLine r = t[li];
    bool keep = is_row[li] != 0 && r.flag == 0 && r.name_len == name_len && r.end > beg_q && end_q > r.beg;
    for (uint32_t k = 0; keep && k < name_len; k++) keep = u[r.name_off + k] == name[k];
    if (!keep) is_row[li] = 0;
    else if (is_row[li] == 2u) atomicMin(first_bad, (unsigned long long)li);
}
struct BedRows {
    const uint8_t *u; const uint32_t *line_off, *tab_off, *tab0, *lend, *ntab, *row_line; uint32_t nrows;
};
// field `f` of line `li` = u[s, e); false when the line has no such field.  f = 12 with `rest`: everything behind the 12th tab.
__device__ __forceinline__ bool bed_field(const BedRows &a, uint32_t li, uint32_t f, bool rest, uint32_t &s, uint32_t &e) {
    const uint32_t nt = a.ntab[li], t0 = a.tab0[li];
    if (f > nt) return false;
    s = f == 0 ? a.line_off[li] : a.tab_off[t0 + f - 1] + 1u;
    e = (f < nt && !rest) ? a.tab_off[t0 + f] : a.lend[li];
    return true;
}
struct BedIntArgs { int32_t n; int32_t field[BED_N_INT]; long long *val[BED_N_INT]; uint8_t *valid[BED_N_INT]; };
// One lane per row: strtoll(field, &end, 10) that has to consume the whole field (parse_int64_span_local)
extern "C" __global__ void __launch_bounds__(256)
bed_ints(BedRows a, BedIntArgs g) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.nrows) return;
    const uint32_t li = a.row_line[r];
    for (int k = 0; k < g.n; k++) {
        uint32_t s = 0, e = 0, adv = 0; long long v = 0; bool ok = false;
        if (bed_field(a, li, (uint32_t)g.field[k], false, s, e) && e > s) { v = vcf_strtoll(a.u, s, e, 10, &adv); ok = adv == e - s; }
        g.val[k][r] = ok ? v : 0; g.valid[k][r] = ok ? 1 : 0;
    }
}
struct BedStrArgs { int32_t n; int32_t col[BED_N_STR]; uint32_t *len[BED_N_STR]; const uint32_t *off[BED_N_STR]; uint8_t *bytes[BED_N_STR]; uint8_t *valid[BED_N_STR]; };
extern "C" __global__ void __launch_bounds__(256)
bed_str_measure(BedRows a, BedStrArgs g) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.nrows) return;
    const uint32_t li = a.row_line[r];
    for (int k = 0; k < g.n; k++) {
        uint32_t s = 0, e = 0;
        const bool have = bed_field(a, li, (uint32_t)g.col[k], g.col[k] == 12, s, e) && e > s;
        g.len[k][r] = have ? e - s : 0u; g.valid[k][r] = have ? 1 : 0;
    }
}
// One lane per row copies a short field; a field of more than 64 bytes is copied by the whole wave, 64 bytes per step.
extern "C" __global__ void __launch_bounds__(256)
bed_str_gather(BedRows a, BedStrArgs g) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const bool live = r < a.nrows;
    const uint32_t li = live ? a.row_line[r] : 0u;
    for (int k = 0; k < g.n; k++) {
        uint32_t s = 0, e = 0, len = 0, d = 0;
        if (live && bed_field(a, li, (uint32_t)g.col[k], g.col[k] == 12, s, e) && e > s) { len = e - s; d = g.off[k][r]; }
        uint8_t *out = g.bytes[k];
        if (len <= 64u) for (uint32_t i = 0; i < len; i++) out[d + i] = a.u[s + i];
        for (unsigned long long m = __ballot(len > 64u); m;) {
            const int src = __builtin_ctzll(m); m &= m - 1;
            const uint32_t ws = __shfl(s, src, 64), wd = __shfl(d, src, 64), wl = __shfl(len, src, 64);
            for (uint32_t i = lane; i < wl; i += 64u) out[wd + i] = a.u[ws + i];
        }
    }
}
