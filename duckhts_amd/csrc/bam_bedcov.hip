// bam_bedcov.hip -- bam_bedcov: summed per-base depth and overlapping-read counts per BED interval, accumulated on the device from the columns
// and the binary CIGARs a read_bam batch leaves in HBM.  The contract is in include/duckhts_amd.h; the host side in dhts_bam_bedcov.inc.
//
//   breakpoints  X[M]: per contig the sorted distinct starts and ends of its valid BED rows, concatenated; base[t] = the breakpoints in front
//                of contig t.  Built on the host at open; a BED row keeps the indices ks / ke of its start and end.
//   counters     cnt[4 * (M + 1)] 64-bit words, four per index: C, S (depth segments) and RS, RE (read intervals).  A segment [a, b) adds
//                (+1, +a) at the first breakpoint > a and (-1, -b) at the first breakpoint > b; a read interval [p, q) adds 1 to RS at the
//                first breakpoint > p and 1 to RE at the first breakpoint >= q.  All sums wrap in 64 bits.
//   classify     one lane per row: the step the row falls out at, the reference length and the number of depth segments of its CIGAR
//   add          rounds over the segments of a wave's rows; runs of neighbouring lanes with one counter index become one atomic per word
//   scan         64-bit prefix sums of the four words over the whole concatenation: a copy of cnt, scanned in place by dev_scan.hip's carry_*
//   emit         F[k] = X[k] * sum C[k] - sum S[k]; bases_covered = F[ke] - F[ks], read_count = sum RS[ke] - sum RE[ks]
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_scan.hip"

enum { COV_STEP_FLAG = 0, COV_STEP_UNPLACED, COV_STEP_MAPQ, COV_STEP_COUNTED, COV_N_STEPS, COV_STEP_NONE = 7 };
enum { COV_C = 0, COV_S, COV_RS, COV_RE, COV_WORDS };
#define COV_NO_IDX 0xffffffffu
// the CIGAR operations that consume the reference (bam_cigar_type bit 1): M D N = X
#define COV_REF_OPS ((1u << 0) | (1u << 2) | (1u << 3) | (1u << 7) | (1u << 8))

struct CovArgs {
    const uint8_t *u;                                                       // the batch's inflated stream
    const uint32_t *rec_off, *cig_rel, *ncig_eff;                           // per row: the record, its effective CIGAR (relative), the CIGAR's length
    const uint16_t *flag; const int32_t *tid; const int64_t *pos; const int32_t *mapq;   // POS 1-based
    uint32_t n; int32_t n_ref;
    uint32_t require, exclude, include, min_mapq;
    uint32_t cover_ops;                                                     // bit per CIGAR operation that counts as depth: M = X, D and N by the options
    const uint32_t *base; const long long *X;                               // base[n_ref + 1]
    uint8_t *step; long long *rlen; uint32_t *nseg;                          // per row
};

__device__ __forceinline__ uint32_t cov_ldu32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }

__global__ void __launch_bounds__(256) bam_cov_classify(CovArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t f = a.flag[i];
    const int32_t t = a.tid[i];
    const int64_t p0 = a.pos[i] - 1;
    uint32_t s, ns = 0; long long rl = 0;
    if ((f & a.require) != a.require || (f & a.exclude) != 0 || (a.include != 0 && (f & a.include) == 0)) s = COV_STEP_FLAG;
    else if (t < 0 || t >= a.n_ref || p0 < 0) s = COV_STEP_UNPLACED;
    else if ((uint32_t)a.mapq[i] < a.min_mapq) s = COV_STEP_MAPQ;
    else {
        s = COV_STEP_COUNTED;
        // (a contig without breakpoints adds nothing: its CIGARs are not read)
        if (!(f & 4u) && a.base[t + 1] > a.base[t]) {
            const uint8_t *cig = a.u + a.rec_off[i] + a.cig_rel[i];
            const uint32_t ne = a.ncig_eff[i];
            bool in = false;
            for (uint32_t j = 0; j < ne; j++) {
                const uint32_t op = cov_ldu32(cig + 4ull * j), code = op & 15u, len = op >> 4;
                if (!((COV_REF_OPS >> code) & 1u) || len == 0) continue;
                if ((a.cover_ops >> code) & 1u) { if (!in) { ns++; in = true; } } else in = false;
                rl += len;
            }
        }
    }
    a.step[i] = (uint8_t)s; a.rlen[i] = rl; a.nseg[i] = ns;
}

// first k in [lo, hi) with X[k] > v (strict) or X[k] >= v, else hi
template <bool STRICT> __device__ __forceinline__ uint32_t cov_bisect(const long long *__restrict__ X, uint32_t lo, uint32_t hi, long long v) {
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; const long long x = X[mid]; if (STRICT ? x > v : x >= v) hi = mid; else lo = mid + 1u; }
    return lo;
}
// the same from a start index that is known not to lie behind the answer: reads are short, so the answer is mostly within a few breakpoints
template <bool STRICT> __device__ __forceinline__ uint32_t cov_walk(const long long *__restrict__ X, uint32_t k, uint32_t hi, long long v) {
    for (int s = 0; s < 4 && k < hi; s++, k++) { const long long x = X[k]; if (STRICT ? x > v : x >= v) return k; }
    return cov_bisect<STRICT>(X, k, hi, v);
}

__device__ __forceinline__ unsigned long long cov_wave_scan(unsigned long long x, uint32_t lane) {      // inclusive, over the 64 lanes
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) { const unsigned long long y = __shfl_up(x, d); if (lane >= d) x += y; }
    return x;
}
// Every lane of the wave calls this.  A lane with idx != COV_NO_IDX adds 1 to word kc and, with SUM, v to word ks of counter idx (NEG: subtracts).
// A lane whose index differs from the lane below heads a run of equal indices; it adds the run's length and the run's sum of v once.  The sum
// of a run is the difference of two entries of the wave's inclusive scan of v.  Nothing depends on the order of the rows.
template <bool SUM, bool NEG> __device__ __forceinline__ void cov_merge(uint32_t idx, unsigned long long v, uint32_t lane, unsigned long long *__restrict__ cnt, uint32_t kc, uint32_t ks) {
    const bool on = idx != COV_NO_IDX;
    const uint32_t below = __shfl_up(idx, 1);
    const bool head = on && (lane == 0 || below != idx);
    const unsigned long long heads = __ballot(head), live = __ballot(on);
    const unsigned long long stop = (heads | ~live) & ~((2ull << lane) - 1ull);       // the first lane above that is not part of this run
    const uint32_t end = stop ? (uint32_t)__ffsll((long long)stop) - 1u : 64u;
    unsigned long long sum = 0;
    if (SUM) {
        const unsigned long long mine = on ? v : 0ull, incl = cov_wave_scan(mine, lane);
        sum = __shfl(incl, (int)(end - 1u)) - (incl - mine);
    }
    if (head) {
        const unsigned long long len = (unsigned long long)(end - lane);
        atomicAdd(&cnt[(uint64_t)COV_WORDS * idx + kc], NEG ? 0ull - len : len);
        if (SUM) atomicAdd(&cnt[(uint64_t)COV_WORDS * idx + ks], NEG ? 0ull - sum : sum);
    }
}

// The counters of a batch.  A workgroup walks its share of the rows (the grid is capped); every lane of a wave makes the same number of turns
// and of rounds and takes part in every vote: rows behind n, rows that are not counted and rows on a contig without breakpoints have nothing
// to add.  Round r takes the r-th depth segment of every row that has one; with both options on a row has at most one, [pos0, pos0 + rlen),
// and the CIGAR is not read again.  The step counters: lane k of every wave keeps step k's count, the workgroup adds its sums once.
#define COV_ADD_MAX_BLOCKS 2048u
__global__ void __launch_bounds__(256) bam_cov_add(CovArgs a, unsigned long long *__restrict__ cnt, unsigned long long *__restrict__ steps) {
    __shared__ unsigned long long block_steps[COV_N_STEPS];
    const uint32_t lane = threadIdx.x & 63u;
    if (threadIdx.x < COV_N_STEPS) block_steps[threadIdx.x] = 0;
    __syncthreads();
    const bool whole = (a.cover_ops & COV_REF_OPS) == COV_REF_OPS;          // every reference-consuming operation is depth
    unsigned long long mine = 0;
    for (uint64_t rowbase = (uint64_t)blockIdx.x * 256u; rowbase < a.n; rowbase += (uint64_t)gridDim.x * 256u) {
        const uint64_t i = rowbase + threadIdx.x;
        const uint32_t s = i < a.n ? a.step[i] : (uint32_t)COV_STEP_NONE;
        uint32_t lo = 0, hi = 0, ns = 0; long long p0 = 0, rl = 0;
        if (s == COV_STEP_COUNTED) { const int32_t t = a.tid[i]; lo = a.base[t]; hi = a.base[t + 1]; p0 = a.pos[i] - 1; rl = a.rlen[i]; ns = a.nseg[i]; }
        const bool live = hi > lo;
        // the read interval [p0, p0 + max(1, rlen))
        uint32_t irs = COV_NO_IDX, ire = COV_NO_IDX;
        if (live) { irs = cov_bisect<true>(a.X, lo, hi, p0); ire = cov_walk<false>(a.X, irs, hi, p0 + (rl > 0 ? rl : 1)); }
        cov_merge<false, false>(irs, 0, lane, cnt, COV_RS, 0);
        cov_merge<false, false>(ire, 0, lane, cnt, COV_RE, 0);
        // the depth segments
        const uint8_t *cig = nullptr; uint32_t ne = 0, jop = 0; long long x = p0;
        if (live && ns && !whole) { cig = a.u + a.rec_off[i] + a.cig_rel[i]; ne = a.ncig_eff[i]; }
        for (uint32_t r = 0; __ballot(live && r < ns) != 0ull; r++) {
            uint32_t si = COV_NO_IDX, sj = COV_NO_IDX; long long sa = 0, sb = 0;
            if (live && r < ns) {
                if (whole) { sa = p0; sb = p0 + rl; si = irs; }
                else {
                    bool in = false;
                    while (jop < ne) {
                        const uint32_t op = cov_ldu32(cig + 4ull * jop), code = op & 15u, len = op >> 4;
                        jop++;
                        if (!((COV_REF_OPS >> code) & 1u) || len == 0) continue;
                        if ((a.cover_ops >> code) & 1u) { if (!in) { sa = x; in = true; } x += len; sb = x; }
                        else { x += len; if (in) break; }
                    }
                    si = cov_bisect<true>(a.X, lo, hi, sa);
                }
                sj = cov_walk<true>(a.X, si, hi, sb);
            }
            cov_merge<true, false>(si, (unsigned long long)sa, lane, cnt, COV_C, COV_S);
            cov_merge<true, true>(sj, (unsigned long long)sb, lane, cnt, COV_C, COV_S);
        }
#pragma unroll
        for (uint32_t k = 0; k < COV_N_STEPS; k++) { const unsigned long long m = __ballot(s == k); if (lane == k) mine += (unsigned long long)__popcll(m); }
    }
    if (lane < COV_N_STEPS && mine) atomicAdd(&block_steps[lane], mine);
    __syncthreads();
    if (threadIdx.x < COV_N_STEPS && block_steps[threadIdx.x]) atomicAdd(&steps[threadIdx.x], block_steps[threadIdx.x]);
}

// ---- the prefix sums of the counters: an element is the COV_WORDS words of a breakpoint index, added word by word ------------------------
// The host copies cnt into sums and scans sums in place with the carry in two levels (dev_scan.hip, four elements per thread, so a chunk is
// 1,024 elements): sums[i] = the sum of cnt[0 .. i), so the inclusive sums of index i lie in sums[i + 1].  cnt stays: a later batch adds to it.
struct CovVec { unsigned long long w[COV_WORDS]; };
__device__ __forceinline__ CovVec operator+(const CovVec &a, const CovVec &b) {
    CovVec r;
#pragma unroll
    for (int k = 0; k < COV_WORDS; k++) r.w[k] = a.w[k] + b.w[k];
    return r;
}

// rows [row0, row0 + n) of the BED: ks / ke are the global breakpoint indices of the row's start and end, COV_NO_IDX for a row that answers 0
__global__ void __launch_bounds__(256) bam_cov_emit(const unsigned long long *__restrict__ sums, const long long *__restrict__ X, const uint32_t *__restrict__ ks, const uint32_t *__restrict__ ke,
                                                    uint64_t row0, uint32_t n, long long *__restrict__ bases, long long *__restrict__ reads) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const uint32_t s = ks[row0 + r], e = ke[row0 + r];
    unsigned long long b = 0, c = 0;
    if (s != COV_NO_IDX && e != COV_NO_IDX) {
        const unsigned long long *ps = sums + (uint64_t)COV_WORDS * (s + 1ull), *pe = sums + (uint64_t)COV_WORDS * (e + 1ull);     // (the inclusive sums)
        const unsigned long long fs = (unsigned long long)X[s] * ps[COV_C] - ps[COV_S], fe = (unsigned long long)X[e] * pe[COV_C] - pe[COV_S];
        b = fe - fs; c = pe[COV_RS] - ps[COV_RE];
    }
    bases[r] = (long long)b; reads[r] = (long long)c;
}
