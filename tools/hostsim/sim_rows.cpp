// sim_rows.cpp -- host build of the record helpers of the row passes (aux_size, find_nul_t, aux_skip_known, aux_skip_t, aux_find_t, rec_check_t
// with the GSrc and WSrc accessors) under ASAN/UBSAN.  The helper text is cut out of bam_records.hip and bam_tiles_lds.hip by run_rows.sh
// (rows_extract.inc); nothing is duplicated here except the plain serial model the helpers are compared with.
//   sim_rows stream.bin [n_ref] ...   (a stream = BAM records one behind the other, as they lie in the inflated file behind the header)
// Every record is checked through GSrc on an exact-size copy of the stream (+ the 16 bytes of padding the device buffer guarantees), and --
// when it lies inside the window of the tile it starts in -- through WSrc on an exact-size image of that window (+ 16 bytes, as in LDS), so
// that a read the device code may not make is an ASAN error.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define __device__
#define __forceinline__ inline
static inline int __ffsll(unsigned long long v) { return __builtin_ffsll((long long)v); }
#include "rows_extract.inc"

// ---- the plain model: htslib's aux_type2size as a switch, a byte-wise walk (sam.c skip_aux, bam_aux_get), bam_read1's tests ----
static int ref_size(uint8_t t) {
    switch (t) {
    case 'A': case 'c': case 'C': return 1;
    case 's': case 'S': return 2;
    case 'i': case 'I': case 'f': return 4;
    case 'd': return 8;
    default: return 0;
    }
}
static const int64_t NONE = -1;
static int64_t ref_skip(const uint8_t *u, int64_t p, int64_t end) {           // p at the type byte
    if (p >= end) return end;
    const uint8_t t = u[p++];
    if (t == 'Z' || t == 'H') { while (p < end && u[p]) p++; return p < end ? p + 1 : end; }
    if (t == 'B') {
        if (end - p < 5) return NONE;
        const uint8_t sub = u[p++];
        int64_t sz = ref_size(sub); if (sub == 'Z' || sub == 'H' || sub == 'B') sz = sub;
        uint32_t n; memcpy(&n, u + p, 4); p += 4;
        if (sz == 0 || end - p < sz * (int64_t)n) return NONE;
        return p + sz * (int64_t)n;
    }
    const int sz = ref_size(t);
    if (sz == 0 || end - p < sz) return NONE;
    return p + sz;
}
static int64_t ref_find(const uint8_t *u, int64_t aux, int64_t end, char t0, char t1, bool *bad, int64_t sb, int64_t se) {
    *bad = false;
    if ((end - aux) - (se - sb) <= 2) return NONE;
    int64_t p = aux; if (p == sb) p = se;
    for (;;) {
        const uint8_t ty = u[p + 2];
        const int64_t e = ref_skip(u, p + 2, end);
        if (u[p] == (uint8_t)t0 && u[p + 1] == (uint8_t)t1) {
            if (e == NONE) { *bad = true; return NONE; }
            if ((ty == 'Z' || ty == 'H') && u[e - 1] != 0) { *bad = true; return NONE; }
            return p + 2;
        }
        if (e == NONE) { *bad = true; return NONE; }
        int64_t nx = e; if (nx == sb) nx = se;
        if (end - nx <= 2) return NONE;
        p = nx;
    }
}
struct RefRec { int rc; int64_t cig_off, cg_beg, cg_end, rg; uint32_t n_eff; bool rg_bad; };
static uint32_t rd32(const uint8_t *u, int64_t o) { uint32_t v; memcpy(&v, u + o, 4); return v; }
static RefRec ref_check(const uint8_t *u, int64_t ulen, int32_t n_ref, int64_t o) {
    RefRec r = {REC_OK, 0, 0, 0, NONE, 0, false};
    if (ulen - o < 4) { r.rc = REC_INCOMPLETE; return r; }
    const int32_t bl = (int32_t)rd32(u, o);
    if (bl < 32) { r.rc = REC_INVALID; return r; }
    if (ulen - o - 4 < 32) { r.rc = REC_INCOMPLETE; return r; }
    const int32_t tid = (int32_t)rd32(u, o + 4), pos = (int32_t)rd32(u, o + 8), l_seq = (int32_t)rd32(u, o + 20), mtid = (int32_t)rd32(u, o + 24);
    const int64_t l_qname = rd32(u, o + 12) & 0xff, n_cigar = rd32(u, o + 16) & 0xffff, flag = rd32(u, o + 16) >> 16;
    if (l_seq < 0 || l_qname < 1) { r.rc = REC_INVALID; return r; }
    const int64_t core = 4 * n_cigar + l_qname + ((int64_t)l_seq + 1) / 2 + l_seq;
    if (core > (int64_t)bl - 32) { r.rc = REC_INVALID; return r; }
    if (ulen - o - 36 < (int64_t)bl - 32) { r.rc = REC_INCOMPLETE; return r; }
    r.cig_off = o + 36 + l_qname; r.n_eff = (uint32_t)n_cigar;
    const int64_t end = o + 4 + bl, aux = o + 36 + core;
    if (n_cigar > 0 && rd32(u, r.cig_off) == (4u | ((uint32_t)l_seq << 4)) && tid >= 0 && pos >= 0) {
        bool bad; const int64_t cg = ref_find(u, aux, end, 'C', 'G', &bad, 0, 0);
        if (cg == NONE && bad) { r.rc = REC_INVALID; return r; }
        if (cg != NONE && u[cg] == 'B' && (u[cg + 1] == 'I' || u[cg + 1] == 'i')) {
            const uint32_t n = rd32(u, cg + 2);
            if (n >= n_cigar && n < (1u << 29)) { r.cig_off = cg + 6; r.n_eff = n; r.cg_beg = cg - 2; r.cg_end = cg + 6 + 4 * (int64_t)n; }
        }
    }
    int64_t qlen = 0;
    for (uint32_t k = 0; k < r.n_eff; k++) { const uint32_t c = rd32(u, r.cig_off + 4 * (int64_t)k); if (CIG_QUERY(c & 0xf)) qlen += c >> 4; }
    if (r.n_eff > 0 && l_seq > 0 && !(flag & 4) && qlen != l_seq) { r.rc = REC_INVALID; return r; }
    if (tid >= n_ref || tid < -1 || mtid >= n_ref || mtid < -1) { r.rc = REC_INVALID; return r; }
    r.rg = ref_find(u, aux, end, 'R', 'G', &r.rg_bad, r.cg_beg, r.cg_end);
    return r;
}

static long g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_fail++ < 20) { printf("MISMATCH " __VA_ARGS__); printf("\n"); } } } while (0)

// the helpers on one record through accessor S (offsets in S's space: add `base` for the stream's), against the model's result
template <class S> static void one(const BamStream &st, const S &s, typename S::off o, uint64_t base, const RefRec &m, const char *what, int64_t abs_o) {
    typedef typename S::off O;
    RecInfoT<O> r; memset(&r, 0, sizeof r);
    const int rc = rec_check_t(st, s, o, r, true);
    CHECK(rc == m.rc, "%s record at %lld: rec_check_t %d, model %d", what, (long long)abs_o, rc, m.rc);
    if (rc != REC_OK || m.rc != REC_OK) return;
    CHECK((int64_t)(base + r.cig_off) == m.cig_off && r.n_cigar_eff == m.n_eff, "%s record at %lld: effective CIGAR", what, (long long)abs_o);
    CHECK((r.cg_beg == 0 && r.cg_end == 0 && m.cg_end == 0) || ((int64_t)(base + r.cg_beg) == m.cg_beg && (int64_t)(base + r.cg_end) == m.cg_end), "%s record at %lld: CG splice", what, (long long)abs_o);
    const O end = o + 4 + r.block_len, aux = o + 36 + r.l_qname + 4u * r.n_cigar + (((uint32_t)r.l_seq + 1u) >> 1) + (uint32_t)r.l_seq;
    bool bad = false; const O rg = aux_find_t(s, aux, end, 'R', 'G', &bad, r.cg_beg, r.cg_end);
    CHECK(bad == m.rg_bad && ((rg == S::none()) ? m.rg == NONE : (int64_t)(base + rg) == m.rg), "%s record at %lld: RG walk (%lld bad %d, model %lld bad %d)", what, (long long)abs_o,
          rg == S::none() ? -1LL : (long long)(base + rg), (int)bad, (long long)m.rg, (int)m.rg_bad);
    // every field of the record through aux_skip_t as well (the walk of bam_tags.hip), hop by hop against the model
    O p = aux;
    while (end - p > 2) {
        const O e = aux_skip_t(s, p + 2, end);
        const int64_t me = ref_skip(st.u, (int64_t)(base + p) + 2, (int64_t)(base + end));
        CHECK((e == S::none()) ? me == NONE : (int64_t)(base + e) == me, "%s record at %lld: aux_skip_t at %lld", what, (long long)abs_o, (long long)(base + p));
        if (e == S::none() || me == NONE) break;
        p = e;
    }
}

int main(int argc, char **argv) {
    for (int t = 0; t < 256; t++)
        if (aux_size((uint8_t)t) != ref_size((uint8_t)t)) { printf("MISMATCH aux_size(%d) = %d, switch %d\n", t, aux_size((uint8_t)t), ref_size((uint8_t)t)); g_fail++; }
    printf("aux_size: 256 type bytes compared with the switch\n");
    const int32_t n_ref = 1;
    for (int a = 1; a < argc; a++) {
        FILE *f = fopen(argv[a], "rb"); if (!f) { perror(argv[a]); return 2; }
        std::vector<uint8_t> raw; uint8_t tmp[65536]; size_t k;
        while ((k = fread(tmp, 1, sizeof tmp, f)) > 0) raw.insert(raw.end(), tmp, tmp + k);
        fclose(f);
        const int64_t ulen = (int64_t)raw.size();
        uint8_t *g = (uint8_t *)malloc((size_t)ulen + 16); memcpy(g, raw.data(), (size_t)ulen); memset(g + ulen, 0xA5, 16);
        BamStream st; memset(&st, 0, sizeof st); st.u = g; st.ulen = (uint64_t)ulen; st.n_ref = n_ref; st.final_batch = 1; st.want_rg = 1;
        GSrc gs; gs.g = g;
        long recs = 0, inwin = 0, invalid = 0;
        int64_t o = 0;
        while (o < ulen) {
            const RefRec m = ref_check(g, ulen, n_ref, o);
            if (m.rc == REC_INCOMPLETE) break;
            recs++; invalid += m.rc != REC_OK;
            one(st, gs, (uint64_t)o, 0, m, "GSrc", o);
            const int64_t bl = (int32_t)rd32(g, o);
            const int64_t tb = o / (int64_t)TL_TILE * (int64_t)TL_TILE, left = ulen - tb;
            const uint32_t avail = left < (int64_t)(TL_TILE + TL_HALO) ? (uint32_t)left : (TL_TILE + TL_HALO);
            if (bl >= 32 && (o - tb) + 4 + bl <= (int64_t)avail) {            // the row passes' "fast" test: the record lies inside the staged window
                const uint32_t pad = (avail + 15u) & ~15u;
                uint8_t *w = (uint8_t *)malloc(pad + 16);                     // exact size: tile_stage's copy and the 16 bytes behind it
                memcpy(w, g + tb, avail); memset(w + avail, 0x5A, pad + 16 - avail);
                WSrc ws; ws.l = w; ws.base = (uint64_t)tb; ws.len = avail;
                one(st, ws, (uint32_t)(o - tb), (uint64_t)tb, m, "WSrc", o);
                free(w); inwin++;
            }
            if (bl < 32) break;
            o += 4 + bl;
        }
        free(g);
        printf("records %ld in-window %ld invalid %ld mismatching %ld  %s\n", recs, inwin, invalid, g_fail, argv[a]);
    }
    return g_fail ? 1 : 0;
}
