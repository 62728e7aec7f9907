// interval_nearest.hip -- the kernels of interval_nearest, for gfx950.  Included by dhts_api.hip behind interval_algebra.hip (ivl_lower, IvlRight,
// IVL_POS_LIMIT, ivl_page_cut); launched by dhts_interval_nearest.inc.  The contract: include/duckhts_amd.h, "interval nearest"; DESIGN.md 4u.
//
//   end order   ivl_end_input makes the (end, row) pairs of the right file's valid rows; the sort of the index (interval_sort.hip) orders them by
//               (rank, end), so rank_first bounds this order as it bounds the start order; ivl_end_gather keeps the ends alone: e_end.
//   selection   ivl_nearest_cells<false>, one lane per left row, binary searches only.  On the chrom's rows [f0, f1): nb(x) = the rows with
//               rs < x (s_beg), ne(x) = the rows with re < x (e_end); the rows within D number cnt(D) = nb(e + D + 1) - ne(s - D), since a row
//               that ends in front of s - D starts in front of e + D + 1.  The rows farther than 0 are two sequences sorted by distance, downstream
//               s_beg[f0 + nb(e + 1) + j] - e and upstream s - e_end[f0 + ne(s) - 1 - j]; the k-th distance is the (k - cnt(0))-th smallest of
//               the two, found by the partition search of two sorted sequences.  The row's count, its D and its tie quota are stored.
//   emission    ivl_nearest_cells<true>: the 'any' walk of ivl_overlap_cells over the rows that start in front of e + D + 1 and end at or behind
//               s - D, from the first row whose pmax admits one, 64-row blocks skipped by bmax; rows at distance D are kept while the quota lasts.
#pragma once

enum { IVL_TIES_ALL = 0, IVL_TIES_FIRST = 1 };
#define IVL_NEAR_NO_QUOTA 0xffffffffu

// vpos: the valid rows in front of every row (n + 1 entries, as the index build leaves it).  A valid row's pair at vpos[r]
extern "C" __global__ void __launch_bounds__(256)
ivl_end_input(const long long *__restrict__ end, const uint32_t *__restrict__ vpos, uint64_t n, unsigned long long *__restrict__ key, uint32_t *__restrict__ row) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    if (vpos[r + 1] != vpos[r]) { key[vpos[r]] = (unsigned long long)end[r] ^ (1ull << 63); row[vpos[r]] = (uint32_t)r; }
}
// e_end[k] = the end of the k-th row in (rank, end) order
extern "C" __global__ void __launch_bounds__(256)
ivl_end_gather(const uint32_t *__restrict__ row, const long long *__restrict__ end, uint64_t m, long long *__restrict__ e_end) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k < m) e_end[k] = end[row[k]];
}

struct IvlNearest {
    IvlRight R; const long long *e_end;                                       // the right file's index and its ends in (rank, end) order
    long long k, max_distance; int32_t ties;                                  // max_distance < 0: none
    const int32_t *name_id; const long long *start, *end; const uint32_t *vpos; const int32_t *rank_of_left;      // the left table, as in IvlOverlap
    uint64_t i0, n;                                                           // left rows i0 .. i0 + n - 1
    unsigned long long *cnt; long long *dist; uint32_t *quota;               // selection: the row's result rows, its D, the rows at distance D it keeps
    unsigned long long *n_unmatched;                                          // selection: += the valid left rows without a candidate
    const unsigned long long *off; unsigned long long off0;                   // emission: the row's result goes to off[i] - off0
    int32_t *out_chrom; long long *out_start, *out_end, *out_lrow, *out_rstart, *out_rend, *out_rrow, *out_ov, *out_dist;
};
// e + D + 1 and s - D inside the position range: D can approach 2^63, s and e lie in [-2^62, 2^62)
__device__ __forceinline__ long long ivl_near_hi(long long e, long long D) { return D > IVL_POS_LIMIT - 1 - e ? IVL_POS_LIMIT : e + D + 1; }
__device__ __forceinline__ long long ivl_near_lo(long long s, long long D) { return D > s + IVL_POS_LIMIT ? -IVL_POS_LIMIT : s - D; }
// the rows of [f0, f1) within D of [s, e)
__device__ __forceinline__ uint32_t ivl_near_count(const IvlNearest &a, uint32_t f0, uint32_t f1, long long s, long long e, long long D) {
    return ivl_lower(a.R.beg, f0, f1, ivl_near_hi(e, D)) - ivl_lower(a.e_end, f0, f1, ivl_near_lo(s, D));
}
// the selection of left row [s, e) on the chrom's rows [f0, f1), f1 > f0: its D and tie quota; returns its result rows
__device__ __forceinline__ uint32_t ivl_near_select(const IvlNearest &a, uint32_t f0, uint32_t f1, long long s, long long e, long long &D, uint32_t &quota) {
    const uint32_t n = f1 - f0, b0 = ivl_lower(a.R.beg, f0, f1, e + 1), u0 = ivl_lower(a.e_end, f0, f1, s);     // rows b0 .. start behind e, rows .. u0 - 1 end in front of s
    const uint32_t c0 = b0 - u0, nd = f1 - b0, nu = u0 - f0;
    const uint32_t k = a.k < (long long)n ? (uint32_t)a.k : n;
    long long dk = 0;
    if (a.k > (long long)n) dk = LLONG_MAX;                                    // fewer rows than k: every row qualifies
    else if (c0 < k) {
        // the need-th smallest of d[j] = beg[b0 + j] - e (j < nd) and u[j] = s - e_end[u0 - 1 - j] (j < nu): the fewest rows `lo` taken from d
        // such that the last row taken from u is not behind the next of d
        const uint32_t need = k - c0;
        uint32_t lo = need > nu ? need - nu : 0u, hi = need < nd ? need : nd;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1), b = need - mid;
            if (s - a.e_end[u0 - b] > a.R.beg[b0 + mid] - e) lo = mid + 1; else hi = mid;
        }
        const uint32_t b = need - lo;
        const long long dd = lo ? a.R.beg[b0 + lo - 1u] - e : 0, du = b ? s - a.e_end[u0 - b] : 0;
        dk = dd > du ? dd : du;
    }
    D = a.max_distance >= 0 && a.max_distance < dk ? a.max_distance : dk;
    const uint32_t c = D == 0 ? c0 : ivl_near_count(a, f0, f1, s, e, D);
    quota = IVL_NEAR_NO_QUOTA;
    if (a.ties != IVL_TIES_FIRST) return c;
    const uint32_t k32 = a.k < (long long)IVL_NEAR_NO_QUOTA ? (uint32_t)a.k : IVL_NEAR_NO_QUOTA - 1u;
    quota = k32 - (D == 0 ? 0u : ivl_near_count(a, f0, f1, s, e, D - 1));     // (fewer than k rows lie nearer than D)
    return c < k32 ? c : k32;
}
// the emission of left row i = [s, e) on chrom rank rk: its rows to off[i] - off0 .., never past off[i + 1] - off0
__device__ __forceinline__ void ivl_near_emit(const IvlNearest &a, uint64_t i, int32_t rk) {
    const long long s = a.start[i], e = a.end[i], D = a.dist[i];
    const uint32_t f0 = a.R.rank_first[rk], f1 = a.R.rank_first[rk + 1];
    const long long y = ivl_near_lo(s, D);                                    // a row within D starts in front of e + D + 1 and ends at or behind y
    const uint32_t stop = ivl_lower(a.R.beg, f0, f1, ivl_near_hi(e, D));
    unsigned long long w = a.off[i] - a.off0;
    const unsigned long long w1 = a.off[i + 1] - a.off0;
    uint32_t quota = a.quota[i];
    uint32_t lo = f0, hi = stop;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (a.R.pmax[mid] >= y) hi = mid; else lo = mid + 1; }
    for (uint32_t k = lo; k < stop && w < w1;) {
        const uint32_t be = (k | 63u) + 1u < stop ? (k | 63u) + 1u : stop;
        if (a.R.bmax[k >> 6] >= y) {
            for (; k < be && w < w1; k++) {
                const long long re = a.R.end[k];
                if (re < y) continue;
                const long long rs = a.R.beg[k], dn = rs - e, up = s - re, d = dn > up ? (dn > 0 ? dn : 0) : (up > 0 ? up : 0);
                if (d == D) { if (quota == 0) continue; if (quota != IVL_NEAR_NO_QUOTA) quota--; }
                const long long olo = s > rs ? s : rs, ohi = e < re ? e : re;
                if (a.out_chrom) a.out_chrom[w] = a.name_id[i];
                if (a.out_start) a.out_start[w] = s;
                if (a.out_end) a.out_end[w] = e;
                if (a.out_lrow) a.out_lrow[w] = (long long)i;
                if (a.out_rstart) a.out_rstart[w] = rs;
                if (a.out_rend) a.out_rend[w] = re;
                if (a.out_rrow) a.out_rrow[w] = (long long)a.R.id[k];
                if (a.out_ov) a.out_ov[w] = ohi > olo ? ohi - olo : 0;
                if (a.out_dist) a.out_dist[w] = d;
                w++;
            }
        }
        k = be;
    }
}
template <bool WRITE> __global__ void __launch_bounds__(256)
ivl_nearest_cells(IvlNearest a) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t i = a.i0 + j;
    const bool valid = j < a.n && a.vpos[i + 1] != a.vpos[i];
    const int32_t rk = valid ? a.rank_of_left[a.name_id[i]] : -1;
    if (WRITE) {
        if (rk >= 0 && a.off[i + 1] != a.off[i]) ivl_near_emit(a, i, rk);
        return;
    }
    unsigned long long c = 0; long long D = 0; uint32_t quota = 0;
    if (rk >= 0) {
        const uint32_t f0 = a.R.rank_first[rk], f1 = a.R.rank_first[rk + 1];
        if (f1 > f0) c = ivl_near_select(a, f0, f1, a.start[i], a.end[i], D, quota);
    }
    if (j < a.n) { a.cnt[i] = c; a.dist[i] = D; a.quota[i] = quota; }
    const unsigned long long m = __ballot(valid && c == 0);
    if (m && (threadIdx.x & 63u) == 0) atomicAdd(a.n_unmatched, (unsigned long long)__popcll(m));
}
