// interval_algebra.hip -- the kernels of interval_merge and interval_overlap around the sort (interval_sort.hip), for gfx950.  Included by
// dhts_api.hip behind vcf_text.hip (TbxLine, bed_intervals) and interval_sort.hip; launched by dhts_interval.inc.  DESIGN.md 4t.
//
//   load     ivl_lines marks the rows and the heads of name runs among a batch's lines (bed_intervals' TbxLine), ivl_head_meta / ivl_head_names
//            bring the heads' names together for the host, ivl_append adds the batch's rows to the table: name id, start, end and a
//            validity flag per row, in file order; a row's number is its place.
//   index    ivl_sort_input makes the (key, row) pairs of the valid rows and every row's rank; behind the sort ivl_index_gather writes
//            beg / end / id / rank by sorted row (OverlapDev's layout, bam_tiles_lds.hip), the first sorted row of every rank and the
//            (rank, end) pairs whose running maximum (ScanMax through the carry) ivl_index_finish turns into pmax and bmax.
//   merge    ivl_merge_heads flags the first row of every run, ivl_merge_runs notes where run j starts, ivl_merge_emit writes a window of runs.
//   overlap  ivl_overlap_cells counts or writes the pairs of a span of left rows, one lane per left row: a binary search in the chrom's
//            starts, then the walk back while pmax admits a hit, 64-row blocks skipped by bmax (the walk of bam_overlap_cells);
//            ivl_page_cut finds where a page of whole left rows ends.
#pragma once
#include <limits.h>

// the pair whose maximum in lexicographic order (rank, end) runs along the sorted rows: ranks do not decrease, so the end of the maximum
// in front of a row is the largest end of its chrom so far
struct IvlPair {
    long long end; uint32_t rank, pad;
    static __host__ __device__ __forceinline__ IvlPair lowest() { IvlPair p; p.end = LLONG_MIN; p.rank = 0; p.pad = 0; return p; }
    __host__ __device__ __forceinline__ bool operator<(const IvlPair &o) const { return rank != o.rank ? rank < o.rank : end < o.end; }
};
#define IVL_POS_LIMIT (1ll << 62)       /* a valid row has start and end in [-2^62, 2^62) */

// per line: 1 = a row of read_bed, 1 = the head of a name run (a row whose chrom is not known to equal the row in front of it; the first
// row of a batch is one); first_bad = the first line with fewer than 3 fields
extern "C" __global__ void __launch_bounds__(256)
ivl_lines(const TbxLine *__restrict__ t, uint32_t nlines, uint32_t *__restrict__ is_row, uint32_t *__restrict__ head, unsigned long long *first_bad) {
    const uint32_t li = blockIdx.x * 256u + threadIdx.x;
    if (li >= nlines) return;
    const TbxLine r = t[li];
    const bool row = r.flag != 1u && r.flag != 2u;
    is_row[li] = row ? 1u : 0u; head[li] = row && !r.same ? 1u : 0u;
    if (r.flag == 2u) atomicMin(first_bad, (unsigned long long)li);
}
// head h (hpos: the heads in front of a line): where its name lies in the text and how long it is
extern "C" __global__ void __launch_bounds__(256)
ivl_head_meta(const TbxLine *__restrict__ t, uint32_t nlines, const uint32_t *__restrict__ hpos, uint32_t *__restrict__ hoff, uint32_t *__restrict__ hlen) {
    const uint32_t li = blockIdx.x * 256u + threadIdx.x;
    if (li >= nlines || hpos[li + 1] == hpos[li]) return;
    hoff[hpos[li]] = t[li].name_off; hlen[hpos[li]] = t[li].name_len;
}
extern "C" __global__ void __launch_bounds__(256)
ivl_head_names(const uint8_t *__restrict__ u, uint32_t nheads, const uint32_t *__restrict__ hoff, const uint32_t *__restrict__ hdst, uint8_t *__restrict__ names) {
    const uint32_t h = blockIdx.x * 256u + threadIdx.x;
    if (h >= nheads) return;
    const uint32_t s = hoff[h], d = hdst[h], n = hdst[h + 1] - d;
    for (uint32_t i = 0; i < n; i++) names[d + i] = u[s + i];
}
// the batch's rows behind the `base` rows of the table; head_id: the name id the host gave every head; *n_skipped += the invalid rows
struct IvlAppend {
    const TbxLine *t; const uint32_t *rpos, *hpos, *head_id; uint32_t nlines; uint64_t base;
    int32_t *name_id; long long *start, *end; uint32_t *vflag; unsigned long long *n_skipped;
};
extern "C" __global__ void __launch_bounds__(256)
ivl_append(IvlAppend a) {
    const uint32_t li = blockIdx.x * 256u + threadIdx.x;
    bool skipped = false;
    if (li < a.nlines && a.rpos[li + 1] != a.rpos[li]) {
        const TbxLine r = a.t[li];
        const uint64_t o = a.base + a.rpos[li];
        const bool ok = !(r.flag & 12u) && r.end >= r.beg && r.beg >= -IVL_POS_LIMIT && r.beg < IVL_POS_LIMIT && r.end >= -IVL_POS_LIMIT && r.end < IVL_POS_LIMIT;
        a.name_id[o] = (int32_t)a.head_id[a.hpos[li + 1] - 1u];                // (the head at or in front of this line)
        a.start[o] = r.beg; a.end[o] = r.end; a.vflag[o] = ok ? 1u : 0u;
        skipped = !ok;
    }
    const unsigned long long m = __ballot(skipped);
    if (m && (threadIdx.x & 63u) == 0) atomicAdd(a.n_skipped, (unsigned long long)__popcll(m));
}

// vpos: the valid rows in front of every row (n + 1 entries).  rank_row[r] = the rank of row r's chrom; a valid row's pair at vpos[r]
extern "C" __global__ void __launch_bounds__(256)
ivl_sort_input(const int32_t *__restrict__ name_id, const long long *__restrict__ start, const uint32_t *__restrict__ vpos, const uint32_t *__restrict__ rank_of_id, uint64_t n,
               uint32_t *__restrict__ rank_row, unsigned long long *__restrict__ key, uint32_t *__restrict__ row) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    rank_row[r] = rank_of_id[name_id[r]];
    if (vpos[r + 1] != vpos[r]) { key[vpos[r]] = (unsigned long long)start[r] ^ (1ull << 63); row[vpos[r]] = (uint32_t)r; }
}

struct IvlIndex {
    const uint32_t *row, *rank_row; const long long *start, *end; uint64_t m; uint32_t n_chroms;
    long long *s_beg, *s_end; uint32_t *s_id, *s_rank, *rank_first; IvlPair *pair;
};
// sorted row k (thread m closes the table): the interval, its row and rank, rank_first[r] = the first sorted row of rank >= r
extern "C" __global__ void __launch_bounds__(256)
ivl_index_gather(IvlIndex a) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k > a.m) return;
    uint32_t rk = a.n_chroms;                                                 // (behind the last row: every rank left gets m)
    if (k < a.m) {
        const uint32_t r = a.row[k];
        rk = a.rank_row[r];
        a.s_beg[k] = a.start[r]; a.s_end[k] = a.end[r]; a.s_id[k] = r; a.s_rank[k] = rk;
        IvlPair p; p.end = a.end[r]; p.rank = rk; p.pad = 0; a.pair[k] = p;
    }
    const uint32_t from = k == 0 ? 0u : a.rank_row[a.row[k - 1]] + 1u;
    for (uint32_t q = from; q <= rk && q <= a.n_chroms; q++) a.rank_first[q] = (uint32_t)k;
}
// pair: the maximum in FRONT of every sorted row (the carry's exclusive form).  pmax[k] = the largest end of the chrom up to and with row k,
// bmax[b] = the largest end of sorted rows 64 b .. 64 b + 63
extern "C" __global__ void __launch_bounds__(256)
ivl_index_finish(const IvlPair *__restrict__ pair, const long long *__restrict__ s_end, const uint32_t *__restrict__ s_rank, uint64_t m, long long *__restrict__ pmax, long long *__restrict__ bmax) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    long long e = LLONG_MIN;
    if (k < m) {
        e = s_end[k];
        const IvlPair p = pair[k];
        pmax[k] = (k > 0 && p.rank == s_rank[k] && p.end > e) ? p.end : e;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const long long o = __shfl_xor(e, d, 64); e = o > e ? o : e; }
    if ((threadIdx.x & 63u) == 0 && k < m) bmax[k >> 6] = e;
}

// ---- merge ---------------------------------------------------------------------------------------------------------------------------
// head[k] = 1: sorted row k starts a run -- the first of its chrom, or start > the largest end so far + max_gap
extern "C" __global__ void __launch_bounds__(256)
ivl_merge_heads(const long long *__restrict__ s_beg, const long long *__restrict__ pmax, const uint32_t *__restrict__ s_rank, uint64_t m, long long max_gap, uint32_t *__restrict__ head) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= m) return;
    head[k] = (k == 0 || s_rank[k] != s_rank[k - 1] || s_beg[k] > pmax[k - 1] + max_gap) ? 1u : 0u;
}
// hidx: the heads in front of every sorted row (m + 1 entries).  run_head[j] = the first sorted row of run j, run_head[n_runs] = m
extern "C" __global__ void __launch_bounds__(256)
ivl_merge_runs(const uint32_t *__restrict__ hidx, uint64_t m, uint32_t *__restrict__ run_head) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k > m) return;
    if (k == m) run_head[hidx[m]] = (uint32_t)m;
    else if (hidx[k + 1] != hidx[k]) run_head[hidx[k]] = (uint32_t)k;
}
struct IvlMergeEmit {
    const uint32_t *run_head, *s_id; const long long *s_beg, *pmax; const int32_t *name_id; uint64_t r0, n;
    int32_t *out_chrom; long long *out_start, *out_end, *out_n;
};
// runs r0 .. r0 + n - 1: chrom (the name id of the run's first row), its first start, the largest end of the run, its rows
extern "C" __global__ void __launch_bounds__(256)
ivl_merge_emit(IvlMergeEmit a) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= a.n) return;
    const uint32_t k0 = a.run_head[a.r0 + j], k1 = a.run_head[a.r0 + j + 1];
    if (a.out_chrom) a.out_chrom[j] = a.name_id[a.s_id[k0]];
    if (a.out_start) a.out_start[j] = a.s_beg[k0];
    if (a.out_end) a.out_end[j] = a.pmax[k1 - 1u];
    if (a.out_n) a.out_n[j] = (long long)(k1 - k0);
}

// ---- overlap ---------------------------------------------------------------------------------------------------------------------------
enum { IVL_MODE_ANY = 0, IVL_MODE_CONTAIN = 1, IVL_MODE_WITHIN = 2 };
struct IvlRight { const long long *beg, *end, *pmax, *bmax; const uint32_t *id, *rank_first; };     // the right file's index (OverlapDev's layout)
struct IvlOverlap {
    IvlRight R; int32_t mode;
    const int32_t *name_id; const long long *start, *end; const uint32_t *vpos; const int32_t *rank_of_left;      // the left table; the right rank of a left name id, -1: none
    uint64_t i0, n;                                                           // left rows i0 .. i0 + n - 1
    unsigned long long *cnt;                                                  // count: cnt[i] = the row's pairs
    const unsigned long long *off; unsigned long long off0;                   // write: the row's pairs go to off[i] - off0
    int32_t *out_chrom; long long *out_start, *out_end, *out_lrow, *out_rstart, *out_rend, *out_rrow, *out_ov;
};
// first sorted row in [lo, hi) whose start is >= x
__device__ __forceinline__ uint32_t ivl_lower(const long long *__restrict__ beg, uint32_t lo, uint32_t hi, long long x) {
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (beg[mid] >= x) hi = mid; else lo = mid + 1; }
    return lo;
}
template <bool WRITE> __device__ __forceinline__ void ivl_pair(const IvlOverlap &a, uint64_t i, long long s, long long e, uint32_t k, unsigned long long &w) {
    if (WRITE) {
        const long long rs = a.R.beg[k], re = a.R.end[k], lo = s > rs ? s : rs, hi = e < re ? e : re;
        if (a.out_chrom) a.out_chrom[w] = a.name_id[i];
        if (a.out_start) a.out_start[w] = s;
        if (a.out_end) a.out_end[w] = e;
        if (a.out_lrow) a.out_lrow[w] = (long long)i;
        if (a.out_rstart) a.out_rstart[w] = rs;
        if (a.out_rend) a.out_rend[w] = re;
        if (a.out_rrow) a.out_rrow[w] = (long long)a.R.id[k];
        if (a.out_ov) a.out_ov[w] = hi > lo ? hi - lo : 0;
    }
    w++;
}
template <bool WRITE> __global__ void __launch_bounds__(256)
ivl_overlap_cells(IvlOverlap a) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= a.n) return;
    const uint64_t i = a.i0 + j;
    unsigned long long w = WRITE ? a.off[i] - a.off0 : 0ull;
    const unsigned long long w0 = w;
    const int32_t rk = a.vpos[i + 1] != a.vpos[i] ? a.rank_of_left[a.name_id[i]] : -1;
    if (rk >= 0) {
        const long long s = a.start[i], e = a.end[i];
        const uint32_t f0 = a.R.rank_first[rk], f1 = a.R.rank_first[rk + 1];
        if (a.mode == IVL_MODE_CONTAIN) {
            // s <= rs && re <= e && rs < e: the rows whose start lies in [s, e), each tested for its end
            const uint32_t lo = ivl_lower(a.R.beg, f0, f1, s), stop = ivl_lower(a.R.beg, lo, f1, e);
            for (uint32_t k = lo; k < stop; k++) if (a.R.end[k] <= e) ivl_pair<WRITE>(a, i, s, e, k, w);
        } else {
            // any: rs < e && re > s.  within: rs <= s && re >= e && re > s, that is rs < s + 1 && re > max(e - 1, s).  Both: the rows that
            // start in front of `x` and end behind `t` -- [first row whose running maximum end > t, first row whose start >= x), each
            // tested for its own end, 64-row blocks whose largest end does not reach skipped whole
            const long long x = a.mode == IVL_MODE_ANY ? e : s + 1, t = a.mode == IVL_MODE_ANY ? s : (e - 1 > s ? e - 1 : s);
            const uint32_t stop = ivl_lower(a.R.beg, f0, f1, x);
            uint32_t lo = f0, hi = stop;
            while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (a.R.pmax[mid] > t) hi = mid; else lo = mid + 1; }
            for (uint32_t k = lo; k < stop;) {
                const uint32_t be = (k | 63u) + 1u < stop ? (k | 63u) + 1u : stop;
                if (a.R.bmax[k >> 6] > t) { for (; k < be; k++) if (a.R.end[k] > t) ivl_pair<WRITE>(a, i, s, e, k, w); }
                k = be;
            }
        }
    }
    if (!WRITE) a.cnt[i] = w - w0;
}
// off: the pairs in front of every left row (n + 1 entries).  The page that starts at left row i0: out[0] = the row behind its last row -- the
// most whole rows whose pairs fit max_rows, at least one --, out[1] = off[i0], out[2] = off[out[0]]
extern "C" __global__ void ivl_page_cut(const unsigned long long *__restrict__ off, unsigned long long n, unsigned long long i0, unsigned long long max_rows, unsigned long long *out) {
    if (blockIdx.x || threadIdx.x) return;
    const unsigned long long lim = off[i0] + max_rows;
    unsigned long long lo = i0, hi = n;                                         // the last i in [i0, n] with off[i] <= lim
    while (lo < hi) { const unsigned long long mid = lo + (hi - lo + 1) / 2; if (off[mid] <= lim) lo = mid; else hi = mid - 1; }
    if (lo == i0 && i0 < n) lo = i0 + 1;
    out[0] = lo; out[1] = off[i0]; out[2] = off[lo];
}
