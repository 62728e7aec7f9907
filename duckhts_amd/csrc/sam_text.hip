// sam_text.hip -- SAM TEXT lines -> BAM records on the device (gfx950), so that read_bam's record stage (tile scan, bam_read1's checks, the
// CG swap, the 13 columns, tags, aux map) serves text input unchanged.  Included by dhts_api.hip after vcf_text.hip (the line index kernels
// vcf_line_count / vcf_line_fill, the name hash and the decimal fast path are shared).
//
// Replaces:
//   sam_read1_sam / hts_getline     htslib sam.c:4243-4250, bgzf.c:2328   -> vcf_line_count / vcf_line_fill (a trailing '\r' is dropped here)
//   sam_parse1                      sam.c:2657-2838                        -> sam_encode<false> (record sizes, the first rejected line) and
//   aux_parse, sam_parse_B_vals     sam.c:2519-2655, 2360-2517                sam_encode<true> behind an exclusive scan of the sizes
//   bam_parse_cigar                 sam.c:2923+
//   bam_write1                      sam.c:857+                             (bin, l_read_name without extra NULs, > 65535 CIGAR ops as CG:B,I)
//   hts_str2int / hts_str2uint      textutils_internal.h:218-330           (the saturating limits; overflow rejects the line)
// f / d / B:f values go through vcf_str2dbl_fast; what it does not take (exponents beyond 10^22, > 15 digits, inf / nan / hex) becomes a
// SamPatch that the host converts with strtod.
//
// Shape: one wave per line.  The lanes read 64-byte windows of the line and find the tabs by ballot; lane k (k < 11) holds the end of field
// k, so the numeric core fields (FLAG, POS, MAPQ, PNEXT, TLEN), both name lookups and the CIGAR are parsed by different lanes at the same
// time.  SEQ packing, the QUAL subtraction and the QNAME copy run across all 64 lanes.  The aux fields are parsed by lane 0 in order: their
// boundaries are not plain tabs (htslib skips to the next byte <= '\t' of a signed char, so bytes >= 0x80 end a field too), and a short-read
// line holds a handful of them.
#pragma once
#include <string.h>
#include <unordered_map>

#define SAM_ENC_THREADS 256
struct SamPatch { uint32_t line, pos, len, relk; };         // relk = offset of the value in the record << 2 | kind; kind 0: f (float of strtod), 1: d (double),
                                                            // 2: a B:f element (float; strtod must take the whole token)
struct SamArgs {
    const uint8_t *u; const uint32_t *line_off; int64_t nlines;   // line i = u[line_off[i], line_off[i+1] - 1)
    VcfDictDev names; int32_t n_targets;                          // @SQ SN and AN names -> tid (names.id)
    uint32_t *rec_len; const uint32_t *rec_off; uint8_t *out;
    unsigned long long *first_bad;                                // the first line sam_parse1 rejects (atomicMin)
    uint32_t *n_patch; SamPatch *patch; uint32_t patch_cap;
};

__constant__ uint8_t sam_nt16[256] = {                        // seq_nt16_table
    15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15,
    15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15,  0,15,15,15, 15,15,15,15, 15,15,15,15, 15, 0,15,15,
    15, 1,14, 2, 13,15,15, 4, 11,15,15,12, 15, 3,15,15, 15,15, 5, 6,  8,15, 7, 9, 15,10,15,15, 15,15,15,15,
    15, 1,14, 2, 13,15,15, 4, 11,15,15,12, 15, 3,15,15, 15,15, 5, 6,  8,15, 7, 9, 15,10,15,15, 15,15,15,15,
    15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15,
    15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15,
    15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15,
    15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15};

__device__ __forceinline__ bool sam_gt_tab(uint8_t c) { return c > 9 && c < 128; }     // `*q > '\t'` on a signed char
__device__ __forceinline__ bool sam_digit(uint8_t c) { return c >= '0' && c <= '9'; }
// hts_str2uint / hts_str2int over u[i, e): the value saturates at the limit of `bits` and sets ov
__device__ __forceinline__ uint64_t sam_str2uint(const uint8_t *u, uint32_t &i, uint32_t e, int bits, bool &ov) {
    const uint64_t limit = bits < 64 ? (1ull << bits) - 1 : ~0ull;
    if (i < e && u[i] == '+') i++;
    uint64_t n = 0;
    for (; i < e && sam_digit(u[i]); i++) {
        const uint32_t d = u[i] - '0';
        if (n > (limit - d) / 10) { n = limit; ov = true; while (i < e && sam_digit(u[i])) i++; break; }
        n = n * 10 + d;
    }
    return n;
}
__device__ __forceinline__ int64_t sam_str2int(const uint8_t *u, uint32_t &i, uint32_t e, int bits, bool &ov) {
    uint64_t limit = (1ull << (bits - 1)) - 1; bool neg = false;
    if (i < e && u[i] == '-') { neg = true; limit++; i++; } else if (i < e && u[i] == '+') i++;
    uint64_t n = 0;
    for (; i < e && sam_digit(u[i]); i++) {
        const uint32_t d = u[i] - '0';
        if (n > (limit - d) / 10) { n = limit; ov = true; while (i < e && sam_digit(u[i])) i++; break; }
        n = n * 10 + d;
    }
    return neg ? (int64_t)(0ull - n) : (int64_t)n;
}
__device__ __forceinline__ int sam_name(const VcfDictDev &d, const uint8_t *s, uint32_t l) { const int k = vcf_dict_find(d, s, l); return k < 0 ? -1 : d.id[k]; }
__device__ __forceinline__ int64_t sam_shfl64(int64_t v, int src) { return (int64_t)(((uint64_t)(uint32_t)__shfl((int)(uint32_t)((uint64_t)v >> 32), src, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)v, src, 64)); }

// sam_parse_B_vals over u[q, p) (q at the ',' in front of the first value) with subtype `sub`, no stores: -> end, count, overflow; false = malformed
__device__ bool sam_b_pass(const uint8_t *u, uint32_t q, uint32_t p, uint8_t sub, uint32_t &r_out, uint32_t &cnt, bool &ov) {
    uint32_t r = q; cnt = 0; ov = false;
    const bool uns = sub == 'C' || sub == 'S' || sub == 'I';
    const int bits = (sub == 'c' || sub == 'C') ? 8 : (sub == 's' || sub == 'S') ? 16 : 32;
    if (sub != 'A') while (r < p && u[r] == ',') {
        cnt++;
        if (sub == 'f') {
            uint32_t t = r + 1; while (t < p && u[t] != ',' && sam_gt_tab(u[t])) t++;
            double v; uint32_t end = 0;
            if (t > r + 1 && vcf_str2dbl_fast(u + r + 1, t - r - 1, &v, &end) == 0 && end != t - r - 1) return false;   // junk behind the number
            r = t; continue;                                                   // (what the fast path does not take is checked by the host)
        }
        if (uns && r + 1 < p && u[r + 1] == '-') { ov = true; r++; while (r < p && sam_gt_tab(u[r]) && u[r] != ',') r++; continue; }
        r++;
        if (uns) (void)sam_str2uint(u, r, p, bits, ov); else (void)sam_str2int(u, r, p, bits, ov);
    }
    if (r < p && u[r] != '\t') return false;
    r_out = r;
    return true;
}

// aux_parse (lenient = 0) of u[q, p) by one lane; WRITE: stores at dst (the record's aux part, at offset rel of the record).  -> bytes, or -1
template <bool WRITE>
__device__ int64_t sam_aux(const SamArgs &a, int64_t line, uint32_t q, uint32_t p, uint8_t *dst, uint32_t rel) {
    const uint8_t *u = a.u;
    VcfSink<WRITE> o; o.p = dst; o.n = 0;
    bool ov = false;
    auto patch = [&](uint32_t pos, uint32_t len, uint32_t kind) {
        if (WRITE) return;                                                      // (recorded once, by the measure pass)
        const uint32_t k = atomicAdd(a.n_patch, 1u);
        if (k < a.patch_cap) { SamPatch pt; pt.line = (uint32_t)line; pt.pos = pos; pt.len = len; pt.relk = (rel + o.n) << 2 | kind; a.patch[k] = pt; }
    };
    while (q < p) {
        if (p - q < 5) return -1;
        if (u[q] < '!' || u[q] >= 128 || u[q + 1] < '!' || u[q + 1] >= 128) return -1;
        o.b(u[q]); o.b(u[q + 1]);
        const uint8_t ty = u[q + 3]; q += 5;
        if (ty != 'Z' && ty != 'H' && (q >= p || !sam_gt_tab(u[q]))) return -1;
        if (ty == 'A' || ty == 'a' || ty == 'c' || ty == 'C') { o.b('A'); o.b(u[q]); q++; }
        else if (ty == 'i' || ty == 'I') {
            if (u[q] == '-') {
                const int64_t x = sam_str2int(u, q, p, 32, ov);
                if (x >= -128) { o.b('c'); o.b((uint8_t)x); }
                else if (x >= -32768) { o.b('s'); o.b((uint8_t)x); o.b((uint8_t)(x >> 8)); }
                else { o.b('i'); o.w32((uint32_t)x); }
            } else {
                const uint64_t x = sam_str2uint(u, q, p, 32, ov);
                if (x <= 255) { o.b('C'); o.b((uint8_t)x); }
                else if (x <= 65535) { o.b('S'); o.b((uint8_t)x); o.b((uint8_t)(x >> 8)); }
                else { o.b('I'); o.w32((uint32_t)x); }
            }
        } else if (ty == 'f' || ty == 'd') {
            uint32_t t = q; while (t < p && sam_gt_tab(u[t])) t++;               // strtod stops inside [q, t); the rest is skipped as junk
            o.b(ty);
            double v = 0.0; uint32_t end = 0;
            const bool fast = vcf_str2dbl_fast(u + q, t - q, &v, &end) == 0;
            if (!fast) patch(q, t - q, ty == 'f' ? 0u : 1u);
            if (ty == 'f') { const float f = fast ? __double2float_rn(v) : 0.0f; o.w32(__float_as_uint(f)); }
            else { const uint64_t b = fast ? (uint64_t)__double_as_longlong(v) : 0ull; o.w32((uint32_t)b); o.w32((uint32_t)(b >> 32)); }
            q = t;
        } else if (ty == 'Z' || ty == 'H') {
            uint32_t t = q; while (t < p && u[t] != '\t') t++;
            if (ty == 'H' && ((t - q) & 1)) return -1;
            o.b(ty); o.bytes(u + q, t - q); o.b(0);
            q = t;
        } else if (ty == 'B') {
            const uint8_t sub0 = u[q]; q++;
            if (q < p && u[q] != ',' && u[q] != '\t') return -1;
            uint32_t r = 0, cnt = 0; bool bov = false; uint8_t sub = sub0;
            const int size = (sub == 'c' || sub == 'C' || sub == 'A') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
            if (!size || !sam_b_pass(u, q, p, sub, r, cnt, bov)) return -1;
            if (bov) {                                                          // the given type was too narrow: retype from the range (sam.c:2446-2479)
                int64_t lo = 0, hi = 0; bool ov64 = false;
                for (uint32_t t = q; t < r;) { t++; const int64_t v = sam_str2int(u, t, p, 64, ov64); if (v > hi) hi = v; if (v < lo) lo = v; while (t < p && sam_gt_tab(u[t]) && u[t] != ',') t++; }
                if (ov64) return -1;
                if (lo < 0) sub = (lo >= -128 && hi <= 127) ? 'c' : (lo >= -32768 && hi <= 32767) ? 's' : (lo >= -2147483648ll && hi <= 2147483647ll) ? 'i' : 0;
                else sub = hi < 255 ? 'C' : hi <= 65535 ? 'S' : hi <= 4294967295ll ? 'I' : 0;
                if (!sub || !sam_b_pass(u, q, p, sub, r, cnt, bov) || bov) return -1;
            }
            o.b('B'); o.b(sub); o.w32(cnt);
            const uint32_t w = (sub == 'c' || sub == 'C' || sub == 'A') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
            if (sub != 'A') for (uint32_t t = q; t < r && u[t] == ',';) {          // the values, in the final subtype
                if (sub == 'f') {
                    uint32_t e2 = t + 1; while (e2 < p && u[e2] != ',' && sam_gt_tab(u[e2])) e2++;
                    double v = 0.0; uint32_t end = 0;
                    bool fast = e2 == t + 1 || vcf_str2dbl_fast(u + t + 1, e2 - t - 1, &v, &end) == 0;
                    if (e2 == t + 1) v = 0.0;
                    if (!fast) patch(t + 1, e2 - t - 1, 2u);
                    o.w32(__float_as_uint(fast ? __double2float_rn(v) : 0.0f));
                    t = e2; continue;
                }
                t++;
                bool d = false;
                const uint64_t x = (sub == 'C' || sub == 'S' || sub == 'I') ? sam_str2uint(u, t, p, 32, d) : (uint64_t)sam_str2int(u, t, p, 32, d);
                o.b((uint8_t)x); if (w >= 2) o.b((uint8_t)(x >> 8)); if (w == 4) { o.b((uint8_t)(x >> 16)); o.b((uint8_t)(x >> 24)); }
            }
            q = r;
        } else return -1;
        while (q < p && sam_gt_tab(u[q])) q++;
        q++;
    }
    if (ov) return -1;
    return (int64_t)o.n;
}

// hts_reg2bin(beg, end, 14, 5)
__device__ __forceinline__ uint32_t sam_reg2bin(int64_t beg, int64_t end) {
    --end;
    int l = 0, s = 14, t = ((1 << 15) - 1) / 7;
    for (; l < 5; l++, s += 3, t -= 1 << (3 * l)) if ((beg >> s) == (end >> s)) return (uint32_t)(t + (beg >> s));
    return 0;
}

template <bool WRITE>
__global__ void __launch_bounds__(SAM_ENC_THREADS) sam_encode(SamArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * (SAM_ENC_THREADS / 64);
    for (int64_t line = (int64_t)blockIdx.x * (SAM_ENC_THREADS / 64) + (threadIdx.x >> 6); line < a.nlines; line += nw) {
        if (WRITE && (a.rec_len[line] == 0 || (unsigned long long)line >= *a.first_bad)) continue;
        const uint8_t *u = a.u;
        const uint32_t s = a.line_off[line];
        uint32_t e = a.line_off[line + 1] - 1;
        if (e > s && u[e - 1] == '\r') e--;                                     // hts_getline drops one trailing '\r'
        // tabs of the line (lane k < 11 keeps the position of tab k); the parser reads a C string: the line ends at its first NUL
        int ntab = 0; uint32_t my_tab = e;
        for (uint32_t p = s; p < e; p += 64) {
            const uint32_t x = p + lane;
            const uint8_t ch = x < e ? u[x] : 1;
            const uint64_t zm = __ballot(ch == 0);
            uint64_t tm = __ballot(ch == '\t');
            if (zm) { const int z = __ffsll((unsigned long long)zm) - 1; e = p + (uint32_t)z; tm &= z ? ((1ull << z) - 1) : 0ull; }
            const int c = __popcll(tm);
            if (lane >= ntab && lane < ntab + c && lane < 11) { uint64_t m = tm; for (int k = ntab; k < lane; k++) m &= m - 1; my_tab = p + (uint32_t)(__ffsll((unsigned long long)m) - 1); }
            ntab += c;
            if (zm) break;
        }
        if (lane >= ntab) my_tab = e;
        bool reject = ntab < 10;
        // field k = u[fs, fe) on lane k
        const uint32_t prev = (uint32_t)__shfl((int)my_tab, lane > 0 ? lane - 1 : 0, 64);
        const uint32_t fs = lane == 0 ? s : prev + 1, fe = my_tab;
        int64_t v = 0, v2 = 0, v3 = 0; bool bad = false, ov = false;
        if (!reject && lane <= 8) {
            uint32_t i = fs;
            if (lane == 0) bad = fe - fs > 254;
            else if (lane == 1) {                                               // parse_sam_flag
                const uint8_t c0 = fs < fe ? u[fs] : 0;
                if (c0 >= '1' && c0 <= '9') v = (int64_t)sam_str2uint(u, i, fe, 16, ov);
                else if (c0 == '0') {                                           // strtoul(v, rv, 0): "0x" + hex digits, else octal
                    uint64_t n = 0; i++;
                    auto hexd = [](uint8_t h) -> int { return sam_digit(h) ? h - '0' : ((h | 32) >= 'a' && (h | 32) <= 'f') ? (h | 32) - 'a' + 10 : -1; };
                    if (i + 1 < fe && (u[i] | 32) == 'x' && hexd(u[i + 1]) >= 0) { for (i++; i < fe && hexd(u[i]) >= 0; i++) if (n < (1ull << 40)) n = n * 16 + (uint64_t)hexd(u[i]); }
                    else for (; i < fe && u[i] >= '0' && u[i] <= '7'; i++) if (n < (1ull << 40)) n = n * 8 + (u[i] - '0');
                    if (n > 65535) { ov = true; n = 65535; }
                    v = (int64_t)n;
                }
                bad = i != fe;
            } else if (lane == 2 || lane == 6) {                                // RNAME / RNEXT
                const uint32_t l = fe - fs;
                if (l == 1 && u[fs] == '*') v = -1;
                else if (lane == 6 && l == 1 && u[fs] == '=') v = -2;
                else if (lane == 2 && a.n_targets == 0) bad = true;             // "no SQ lines present in the header"
                else v = sam_name(a.names, u + fs, l);
            } else if (lane == 3 || lane == 7) { v = (int64_t)sam_str2uint(u, i, fe, 62, ov) - 1; bad = i != fe; }
            else if (lane == 4) { v = (int64_t)sam_str2uint(u, i, fe, 8, ov); bad = i != fe; }
            else if (lane == 8) { v = sam_str2int(u, i, fe, 63, ov); bad = i != fe; }
            else if (lane == 5) {                                               // CIGAR: v = n_cigar (-1: '*'), v2 = reference length, v3 = query length
                if (fs < fe && u[fs] == '*') v = -1;
                else {
                    uint32_t n = 0; for (uint32_t k = fs; k < fe; k++) n += sam_digit(u[k]) ? 0u : 1u;
                    bad = n == 0;
                    for (uint32_t k = 0; k < n && !bad; k++) {
                        const uint32_t i0 = i; bool o2 = false;
                        const uint64_t len = sam_str2uint(u, i, fe, 28, o2);
                        if (i == i0 || o2 || i >= fe) { bad = true; break; }
                        const uint8_t op = u[i++];
                        const int t = op == 'M' ? 0 : op == 'I' ? 1 : op == 'D' ? 2 : op == 'N' ? 3 : op == 'S' ? 4 : op == 'H' ? 5 : op == 'P' ? 6 : op == '=' ? 7 : op == 'X' ? 8 : op == 'B' ? 9 : -1;
                        if (t < 0) { bad = true; break; }
                        if (t == 0 || t == 1 || t == 4 || t == 7 || t == 8) v3 += (int64_t)len;
                        if (t == 0 || t == 2 || t == 3 || t == 7 || t == 8) v2 += (int64_t)len;
                    }
                    if (!bad && i != fe) bad = true;
                    v = n;
                }
            }
        }
        reject = reject || __ballot(bad) != 0 || __ballot(ov) != 0;
        if (reject) { if (!WRITE && lane == 0) { a.rec_len[line] = 0; atomicMin(a.first_bad, (unsigned long long)line); } continue; }
        uint32_t flag = (uint32_t)__shfl((int)v, 1, 64);
        int64_t tid = sam_shfl64(v, 2), pos = sam_shfl64(v, 3), mapq = sam_shfl64(v, 4);
        const int64_t ncig = sam_shfl64(v, 5), rlen0 = sam_shfl64(v2, 5), qlen = sam_shfl64(v3, 5);
        int64_t mtid = sam_shfl64(v, 6), mpos = sam_shfl64(v, 7);
        const int64_t tlen = sam_shfl64(v, 8);
        const uint32_t fe0 = (uint32_t)__shfl((int)fe, 0, 64), fs9 = (uint32_t)__shfl((int)fs, 9, 64), fe9 = (uint32_t)__shfl((int)fe, 9, 64);
        const uint32_t fs10 = (uint32_t)__shfl((int)fs, 10, 64), fe10 = (uint32_t)__shfl((int)fe, 10, 64);
        if (pos < 0 && tid >= 0) tid = -1;
        if (tid < 0) flag |= 4;
        int64_t rlen;
        const uint32_t n_cigar = ncig > 0 ? (uint32_t)ncig : 0;
        if (ncig > 0) { rlen = (flag & 4) ? 1 : rlen0; if (rlen == 0) rlen = 1; }
        else { flag |= 4; rlen = 1; }
        const uint32_t bin = sam_reg2bin(pos, pos + rlen);
        if (mtid == -2) mtid = tid;
        if (mpos < 0 && mtid >= 0) mtid = -1;
        // SEQ, QUAL
        const bool seq_star = fe9 - fs9 == 1 && u[fs9] == '*';
        const uint32_t l_qseq = seq_star ? 0u : fe9 - fs9;
        if (!seq_star && n_cigar && qlen != (int64_t)l_qseq) reject = true;        // ("CIGAR and query sequence are of different length": SEQ given)
        const bool qual_star = fs10 < e && u[fs10] == '*' && (fs10 + 1 == e || u[fs10 + 1] == '\t');
        if (!qual_star && fe10 - fs10 != l_qseq) reject = true;                // "SEQ and QUAL are of different length"
        if (!reject && !qual_star) {
            bool qb = false;
            for (uint32_t k = lane; k < l_qseq; k += 64) qb |= ((uint8_t)(u[fs10 + k] - 33) & 0x80) != 0;
            reject = __ballot(qb) != 0;
        }
        // bam_write1's limits
        if (pos > 2147483647ll || mpos > 2147483647ll || tlen < -2147483648ll || tlen > 2147483647ll) reject = true;
        if (n_cigar > 65535 && rlen0 >= (1ll << 28)) reject = true;
        const uint32_t l_qname = fe0 - s + 1, ncw = n_cigar > 65535 ? 2u : n_cigar;
        const uint32_t aux_rel = 4u + 32u + l_qname + 4u * ncw + (l_qseq + 1) / 2 + l_qseq;
        const uint32_t a0 = qual_star ? fs10 + 2 : fs10 + l_qseq + 1;
        uint8_t *rec = WRITE ? a.out + a.rec_off[line] : nullptr;
        int64_t aux_len = 0;
        if (!reject && lane == 0) aux_len = sam_aux<WRITE>(a, line, a0, e, WRITE ? rec + aux_rel : nullptr, aux_rel);
        aux_len = sam_shfl64(aux_len, 0);
        if (reject || aux_len < 0) { if (!WRITE && lane == 0) { a.rec_len[line] = 0; atomicMin(a.first_bad, (unsigned long long)line); } continue; }
        const uint32_t total = aux_rel + (uint32_t)aux_len + (n_cigar > 65535 ? 8u + 4u * n_cigar : 0u);
        if (!WRITE) { if (lane == 0) a.rec_len[line] = total; continue; }
        // ---- stores ----
        if (lane < 9) {
            uint32_t w = 0;
            switch (lane) {
                case 0: w = total - 4; break;
                case 1: w = (uint32_t)tid; break;
                case 2: w = (uint32_t)pos; break;
                case 3: w = bin << 16 | (uint32_t)mapq << 8 | l_qname; break;
                case 4: w = flag << 16 | ncw; break;
                case 5: w = l_qseq; break;
                case 6: w = (uint32_t)mtid; break;
                case 7: w = (uint32_t)mpos; break;
                default: w = (uint32_t)tlen; break;
            }
            __builtin_memcpy(rec + 4 * lane, &w, 4);
        }
        for (uint32_t k = lane; k < l_qname - 1; k += 64) rec[36 + k] = u[s + k];
        if (lane == 0) rec[36 + l_qname - 1] = 0;
        if (n_cigar) {
            const uint32_t cdst = n_cigar > 65535 ? total - 4 * n_cigar : 36 + l_qname;
            if (lane == 5) {
                const uint32_t cfs = (uint32_t)fs; uint32_t i = cfs;
                for (uint32_t k = 0; k < n_cigar; k++) {
                    bool o2 = false; const uint64_t len = sam_str2uint(u, i, fe, 28, o2); const uint8_t op = u[i++];
                    const uint32_t t = op == 'M' ? 0 : op == 'I' ? 1 : op == 'D' ? 2 : op == 'N' ? 3 : op == 'S' ? 4 : op == 'H' ? 5 : op == 'P' ? 6 : op == '=' ? 7 : op == 'X' ? 8 : 9;
                    const uint32_t w = (uint32_t)len << 4 | t; __builtin_memcpy(rec + cdst + 4 * k, &w, 4);
                }
            }
            if (n_cigar > 65535 && lane == 0) {
                const uint32_t w0 = l_qseq << 4 | 4u, w1 = (uint32_t)rlen0 << 4 | 3u;
                __builtin_memcpy(rec + 36 + l_qname, &w0, 4); __builtin_memcpy(rec + 40 + l_qname, &w1, 4);
                const uint32_t cg = cdst - 8; rec[cg] = 'C'; rec[cg + 1] = 'G'; rec[cg + 2] = 'B'; rec[cg + 3] = 'I'; __builtin_memcpy(rec + cg + 4, &n_cigar, 4);
            }
        }
        const uint32_t sdst = 36 + l_qname + 4 * ncw, qdst = sdst + (l_qseq + 1) / 2;
        for (uint32_t k = lane; k < (l_qseq + 1) / 2; k += 64) {
            const uint8_t hi = sam_nt16[u[fs9 + 2 * k]], lo = 2 * k + 1 < l_qseq ? sam_nt16[u[fs9 + 2 * k + 1]] : 0;
            rec[sdst + k] = (uint8_t)(hi << 4 | lo);
        }
        for (uint32_t k = lane; k < l_qseq; k += 64) rec[qdst + k] = qual_star ? 0xff : (uint8_t)(u[fs10 + k] - 33);
    }
}

// the host's strtod values go back: value i (8 bytes; 4 are stored for a float) to out[dst[i] ..) (records are byte-packed: no alignment)
extern "C" __global__ void __launch_bounds__(256)
sam_scatter_values(uint8_t *__restrict__ out, const uint32_t *__restrict__ dst, const uint64_t *__restrict__ val, const uint8_t *__restrict__ width, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t v = val[i];
    for (uint32_t k = 0; k < width[i]; k++) out[dst[i] + k] = (uint8_t)(v >> (8 * k));
}

// ---- host: is this stream SAM text?  hts_detect_format2 (htslib hts.c:690-705, 734-743) on its first bytes ------------------------------
// headered: "@HD\t", "@SQ\t", "@RG\t", "@PG\t" or "@CO\t"; headerless: the first line's columns (parse_tabbed_text, hts.c:484-539) match
// "ZiZiiCZiiZZOOOOOOOOOOOOOOOOOOOOO+" (colmatch, hts.c:544-553) for at least 9 columns, 11 when the line ended inside the bytes looked at
static int fastq_text_detect(const uint8_t *s, size_t len);
static bool sam_text_detect(const uint8_t *s, size_t len) {
    if (len > 1024) len = 1024;
    if (len >= 4 && s[0] == '@' && (!memcmp(s, "@HD\t", 4) || !memcmp(s, "@SQ\t", 4) || !memcmp(s, "@RG\t", 4) || !memcmp(s, "@PG\t", 4) || !memcmp(s, "@CO\t", 4))) return true;
    if (fastq_text_detect(s, len)) return false;                                 // ('>' / '@' + is_fastaq come in front of the column rule: fastq_text.hip)
    char cols[24]; int nc = 0, complete = 0;
    const uint8_t *str = s, *end = s + len; unsigned seen = 0;
    for (const uint8_t *p = s; p < end; p++) {
        const uint8_t ch = *p;
        if ((int8_t)ch >= ' ') {
            if (ch >= '0' && ch <= '9') seen |= 1;
            else if ((ch == '+' || ch == '-') && p == str) seen |= 2;
            else if (strchr("MIDNSHP=XB", (char)ch) && p > str && p[-1] >= '0' && p[-1] <= '9') seen |= 4;
            else seen |= 8;
        } else if (ch == '\t' || ch == '\r' || ch == '\n') {
            const size_t l = (size_t)(p - str); char t;
            if (seen == 1 || seen == 3) t = 'i';
            else if (seen == 5) t = 'C';
            else if (l == 1) t = str[0] == '*' ? 'C' : (str[0] == '+' || str[0] == '-' || str[0] == '.') ? 's' : 'Z';
            else if (l >= 5 && str[2] == ':' && str[4] == ':') t = 'O';
            else t = 'Z';
            cols[nc++] = t;
            if (ch != '\t' || nc >= (int)sizeof(cols) - 1) { complete = 1; break; }
            str = p + 1; seen = 0;
        } else return false;
    }
    cols[nc] = 0;
    if (nc <= 0) return false;
    const char *pat = "ZiZiiCZiiZZOOOOOOOOOOOOOOOOOOOOO+";
    int m = 0;
    for (int i = 0; cols[i]; i++) { if (pat[i] == '+') { m = i; break; } if (!(cols[i] == pat[i] || pat[i] == 'Z')) { m = 0; break; } m = i + 1; }
    return m >= 9 + 2 * complete;
}
