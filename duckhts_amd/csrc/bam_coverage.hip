// bam_coverage.hip -- bam_coverage: numreads, covbases, depth and mean qualities per contig or region (what `samtools coverage` prints),
// accumulated on the device from the columns, the binary CIGARs and the QUAL bytes a read_bam batch leaves in HBM.  The contract is in
// include/duckhts_amd.h; the host side in dhts_bam_coverage.inc.
//
//   target rows  sorted by (contig, start), disjoint, none empty: rbeg / rend, with tid_first[t] rows in front of contig t
//   diff         int32, one span of (end - beg) + 1 slots per row, padded to DEP_TILE (rbase[k] = the row's first slot): the depth's
//                difference table.  With c(x) = "position x of the read is a counted base", a read adds c(x) - c(x - 1) at every x where that
//                is not 0: +1 at the first base of a maximal run of counted bases, -1 behind its last.  Whoever looks at a base needs only
//                the base before it, so nothing is handed from lane to lane: the lane that owns a 16-byte piece of QUAL reads the one byte
//                in front of it, and a CIGAR operation takes the last base of the M before it.
//   words        per row DEP_REPLICAS copies, 64 bytes apart, of four 64-bit words (the layout cov_merge adds to): numreads, sum_mapq,
//                sum_baseq, spare.  A sorted file has every wave of a batch on one row: a workgroup adds to the copy its number picks, so the
//                atomics of a batch spread over 64 lines instead of queueing on one; the result folds the copies.
//   classify     one lane per read: the step it falls out at, the reference length and the rows [k0, k1) its interval overlaps
//   add          eight lanes per read, eight reads per wave.  Every lane walks the read's CIGAR; of an M = X operation lane j takes the
//                16-byte aligned pieces j, j + 8, ... of its qualities, ends masked.  Without min_baseq no quality decides anything: the
//                pieces are only summed and the first lane of the eight sets the runs from the CIGAR alone.
//   result       tile sums of diff, their exclusive scan (the depth in front of every tile), then per tile the scan inside it reduced to
//                #(depth >= min_depth) and sum depth, then per row the sum over its tiles.  diff stays as it is.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bam_bedcov.hip"
#include "dev_scan.hip"

enum { DEP_STEP_FLAG = 0, DEP_STEP_UNPLACED, DEP_STEP_SHORT, DEP_STEP_MAPQ, DEP_STEP_OUTSIDE, DEP_STEP_COUNTED, DEP_N_STEPS, DEP_STEP_NONE = 15 };
enum { DEP_W_READS = 0, DEP_W_MAPQ, DEP_W_BASEQ, DEP_W_SPARE };           // = COV_WORDS words per row
#define DEP_WALK 0x80u                                                      /* step byte: the read has an M = X operation to walk */
#define DEP_TILE 1024u
#define DEP_M_OPS ((1u << 0) | (1u << 7) | (1u << 8))                       /* M = X: counted bases */
#define DEP_GAP_OPS ((1u << 2) | (1u << 3))                                 /* D N: reference positions that never count */
#define DEP_Q_ONLY_OPS ((1u << 1) | (1u << 4))                              /* I S: query bases without a reference position */
#define DEP_LANES 8u                                                        /* lanes per read */
#define DEP_ADD_MAX_BLOCKS 4096u
#define DEP_REPLICAS 64u                                                    /* copies of a row's words, one 64-byte line each */
#define DEP_WORD_IDX(k, rep) (((k) * DEP_REPLICAS + (rep)) * 2u)            /* cov_merge's index (four words each) of copy rep of row k */

struct DepArgs {
    const uint8_t *u;                                                       // the batch's inflated stream
    const uint32_t *rec_off, *cig_rel, *ncig_eff;                           // per read: the record, its effective CIGAR (relative), the CIGAR's length
    const uint16_t *flag; const int32_t *tid; const int64_t *pos; const int32_t *mapq;   // POS 1-based
    uint32_t n; int32_t n_ref;
    uint32_t require, exclude, include, min_mapq, min_baseq; long long min_read_len;
    const uint32_t *tid_first; const long long *rbeg, *rend; const unsigned long long *rbase;   // the sorted rows
    uint8_t *step; long long *rlen; uint32_t *k0, *k1;                      // per read
};

// DEL: a D operation is walked as well (bam_depth's include_deletions); the kernel bam_coverage launches is the body without it
template <bool DEL> __device__ __forceinline__ void dep_classify_body(const DepArgs &a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t f = a.flag[i];
    const int32_t t = a.tid[i];
    const int64_t p0 = a.pos[i] - 1;
    const uint8_t *rec = a.u + a.rec_off[i];
    uint32_t s, k0 = 0, k1 = 0; long long rl = 0; bool walk = false;
    if ((f & a.require) != a.require || (f & a.exclude) != 0 || (a.include != 0 && (f & a.include) == 0)) s = DEP_STEP_FLAG;
    else if (t < 0 || t >= a.n_ref || p0 < 0) s = DEP_STEP_UNPLACED;
    else if ((long long)(int32_t)cov_ldu32(rec + 20) < a.min_read_len) s = DEP_STEP_SHORT;
    else if ((uint32_t)a.mapq[i] < a.min_mapq) s = DEP_STEP_MAPQ;
    else {
        if (!(f & 4u)) {
            const uint8_t *cig = rec + a.cig_rel[i];
            const uint32_t ne = a.ncig_eff[i];
            for (uint32_t j = 0; j < ne; j++) {
                const uint32_t op = cov_ldu32(cig + 4ull * j), code = op & 15u, len = op >> 4;
                if (!((COV_REF_OPS >> code) & 1u) || len == 0) continue;
                if (((DEP_M_OPS >> code) & 1u) || (DEL && code == 2u)) walk = true;
                rl += len;
            }
        }
        // the rows the read interval [p0, p0 + max(1, rlen)) overlaps: the first that ends behind p0, up to the first that starts at or behind its end
        const uint32_t lo = a.tid_first[t], hi = a.tid_first[t + 1];
        k0 = cov_bisect<true>(a.rend, lo, hi, p0);
        k1 = cov_walk<false>(a.rbeg, k0, hi, p0 + (rl > 0 ? rl : 1));
        s = k1 > k0 ? DEP_STEP_COUNTED : DEP_STEP_OUTSIDE;
    }
    a.step[i] = (uint8_t)(s | (walk && s == DEP_STEP_COUNTED ? DEP_WALK : 0u));
    a.rlen[i] = rl; a.k0[i] = k0; a.k1[i] = k1;
}
__global__ void __launch_bounds__(256) bam_depth_classify(DepArgs a) { dep_classify_body<false>(a); }

__device__ __forceinline__ uint32_t dep_byte_mask(uint32_t bits4) {           // bit b of bits4 -> byte b all ones
    return (bits4 & 1u) * 0xffu | ((bits4 >> 1) & 1u) * 0xff00u | ((bits4 >> 2) & 1u) * 0xff0000u | ((bits4 >> 3) & 1u) * 0xff000000u;
}
// the sum of the bytes of w[0 .. 3] whose bit is set in m (16 bits)
__device__ __forceinline__ uint32_t dep_byte_sum(const uint32_t (&w)[4], uint32_t m) {
    uint32_t acc = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) acc = __builtin_amdgcn_sad_u8(w[k] & dep_byte_mask((m >> (4 * k)) & 15u), 0u, acc);
    return acc;
}
// bit i = byte i of w[0 .. 3] is >= t
__device__ __forceinline__ uint32_t dep_ge_mask(const uint32_t (&w)[4], uint32_t t) {
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int b = 0; b < 4; b++) m |= (((w[k] >> (8 * b)) & 255u) >= t ? 1u : 0u) << (4 * k + b);
    return m;
}

// One read against one row [beg, end), as seen by lane `sub` of the read's eight: the difference entries of its runs go to dp (the row's span),
// the return value is this lane's share of the counted bases' qualities.  qual = the read's QUAL (lseq bytes of it lie in the record; a query
// index at or behind lseq passes every threshold and adds 0); ub = the stream's address rounded down to 16 bytes, mis = what was cut off.
// DEL (bam_depth's include_deletions): every position of a D operation inside the row is a counted position without a quality, so a run goes on
// through it (20M3D20M with passing bases around the D is one run, two atomics); the first lane of the eight sets what a D starts and ends.
// SUM = false: nobody wants the quality sum; without min_baseq the pieces are then not read at all.
template <bool BQ, bool DEL = false, bool SUM = true>
__device__ __forceinline__ uint64_t dep_walk_row(const uint8_t *__restrict__ ub, uint32_t mis, uint64_t qoff, long long lseq, uint32_t min_baseq,
                                                 const uint8_t *__restrict__ cig, uint32_t ne, long long p0, long long beg, long long end, int32_t *__restrict__ dp, uint32_t sub) {
    const uint8_t *qual = ub + mis + qoff;
    const long long qbase = (long long)(mis + qoff);                         // position of query index 0 in the 16-byte grid
    auto pass = [&](long long q) -> bool { return !BQ || q >= lseq || (uint32_t)qual[q] >= min_baseq; };
    auto in_row = [&](long long x) -> bool { return x >= beg && x < end; };
    uint64_t sumq = 0;
    long long x = p0, q = 0, last_q = 0; bool adj = false, del = false;      // adj: the reference position before x is the base last_q of an M = X operation; del (DEL): it is a D's
    for (uint32_t j = 0; j < ne; j++) {
        const uint32_t op = cov_ldu32(cig + 4ull * j), code = op & 15u; const long long len = (long long)(op >> 4);
        if (len == 0) continue;
        if (DEL && code == 2u) {
            const bool carry = in_row(x - 1) && (del || (adj && pass(last_q)));                     // c(x - 1)
            const long long dlo = beg > x ? beg : x, dhi = end < x + len ? end : x + len;           // the operation's positions inside the row
            if (sub == 0) {
                if (dhi > dlo) {
                    if (!(carry && dlo == x)) atomicAdd(dp + (dlo - beg), 1);
                    if (dhi < x + len) atomicAdd(dp + (end - beg), -1);                             // the row ends inside the operation
                } else if (carry) atomicAdd(dp + (x - beg), -1);                                    // (then x == end)
            }
            x += len; adj = false; del = true;
            continue;
        }
        if ((DEP_M_OPS >> code) & 1u) {
            const bool carry = in_row(x - 1) && ((DEL && del) || (adj && pass(last_q)));            // c(x - 1)
            const long long jlo = beg > x ? beg - x : 0, jhi = end - x < len ? end - x : len;      // the operation's bases inside the row
            if (!in_row(x)) { if (sub == 0 && carry) atomicAdd(dp + (x - beg), -1); }               // (then x == end: the run stops at the row's end)
            if (jhi > jlo) {
                const long long qlo = q + jlo, qhi = q + jhi;
                const long long c_last = (qbase + qhi - 1) >> 4;
                if (BQ || SUM) for (long long c = ((qbase + qlo) >> 4) + sub; c <= c_last; c += DEP_LANES) {
                    const long long qc0 = (c << 4) - qbase;                  // the query index of the piece's byte 0
                    const uint32_t lo_i = qlo > qc0 ? (uint32_t)(qlo - qc0) : 0u, hi_i = qhi - qc0 < 16 ? (uint32_t)(qhi - qc0) : 16u;
                    const uint32_t valid = ((1u << hi_i) - 1u) & ~((1u << lo_i) - 1u);
                    const long long nr = lseq - qc0;
                    const uint32_t in_rec = nr <= 0 ? 0u : nr >= 16 ? 0xffffu : (1u << (uint32_t)nr) - 1u, real = valid & in_rec;
                    uint32_t w[4] = {0u, 0u, 0u, 0u};
                    if (real) { const uint4 v = *(const uint4 *)(ub + (c << 4)); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
                    if (!BQ) { if (SUM) sumq += dep_byte_sum(w, real); }
                    else {
                        const uint32_t m = (dep_ge_mask(w, min_baseq) & real) | (valid & ~in_rec);
                        if (SUM) sumq += dep_byte_sum(w, m & real);
                        const bool pred = qc0 + lo_i > qlo ? pass(qc0 + lo_i - 1) : (jlo == 0 && carry);
                        const uint32_t p = (m << 1) | ((pred ? 1u : 0u) << lo_i);
                        uint32_t st = m & ~p, en = ~m & p & valid;
                        int32_t *d0 = dp + (x + (qc0 - q) - beg);            // the slot of the piece's byte 0
                        while (st) { atomicAdd(d0 + (__ffs((int)st) - 1), 1); st &= st - 1u; }
                        while (en) { atomicAdd(d0 + (__ffs((int)en) - 1), -1); en &= en - 1u; }
                    }
                }
                if (sub == 0) {
                    if (!BQ && !(jlo == 0 && carry)) atomicAdd(dp + (x + jlo - beg), 1);
                    if (jhi < len && pass(q + jhi - 1)) atomicAdd(dp + (end - beg), -1);          // the row ends inside the operation
                }
            }
            x += len; q += len; adj = true; del = false; last_q = q - 1;
        } else if ((DEP_GAP_OPS >> code) & 1u) {
            if (sub == 0 && in_row(x - 1) && ((DEL && del) || (adj && pass(last_q)))) atomicAdd(dp + (x - beg), -1);
            adj = false; del = false; x += len;
        } else if ((DEP_Q_ONLY_OPS >> code) & 1u) q += len;
    }
    if (sub == 0 && in_row(x - 1) && ((DEL && del) || (adj && pass(last_q)))) atomicAdd(dp + (x - beg), -1);
    return sumq;
}

// The counters of a batch.  A workgroup takes 32 reads a turn (the grid is capped); every lane makes the same number of turns and of rounds
// and takes part in every vote.  Round r is the r-th row a read overlaps (one, for all but the reads that hang over a row's edge into the
// next).  The eight lanes' quality sums are folded, the eight reads of a wave moved to its first eight lanes, and cov_merge adds runs of one
// row index once.  The step counters as in bam_cov_add.
// bam_depth's form: DEL as in dep_walk_row; WORDS = false drops the per-row words and their copies (words is not read): a counted read then
// sets touched[tid] = 1 with a plain store instead (every writer stores the same value, so no atomic is needed).
template <bool BQ, bool DEL, bool WORDS>
__device__ __forceinline__ void dep_add_body(const DepArgs &a, int32_t *__restrict__ diff, unsigned long long *__restrict__ words, uint32_t *__restrict__ touched, unsigned long long *__restrict__ steps) {
    __shared__ unsigned long long block_steps[DEP_N_STEPS];
    const uint32_t lane = threadIdx.x & 63u, sub = threadIdx.x & (DEP_LANES - 1u), grp = threadIdx.x / DEP_LANES;
    if (threadIdx.x < DEP_N_STEPS) block_steps[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t mis = (uint32_t)((uintptr_t)a.u & 15u);
    const uint8_t *ub = a.u - mis;
    unsigned long long mine = 0;
    for (uint64_t rowbase = (uint64_t)blockIdx.x * 32u; rowbase < a.n; rowbase += (uint64_t)gridDim.x * 32u) {
        const uint64_t i = rowbase + grp;
        const uint32_t sb = i < a.n ? a.step[i] : (uint32_t)DEP_STEP_NONE, s = sb & 15u;
        uint32_t k0 = 0, k1 = 0, ne = 0; long long p0 = 0, lseq = 0; uint64_t qoff = 0; unsigned long long mq = 0; const uint8_t *cig = nullptr;
        if (s == DEP_STEP_COUNTED) {
            k0 = a.k0[i]; k1 = a.k1[i]; p0 = a.pos[i] - 1; mq = (unsigned long long)(uint32_t)a.mapq[i];
            if (sb & DEP_WALK) {
                const uint64_t ro = a.rec_off[i];
                const uint8_t *rec = a.u + ro;
                cig = rec + a.cig_rel[i]; ne = a.ncig_eff[i];
                const uint32_t lrn = rec[12], nc = (uint32_t)rec[16] | ((uint32_t)rec[17] << 8);
                const long long ls = (long long)(int32_t)cov_ldu32(rec + 20), rec_len = 4ll + (long long)cov_ldu32(rec);
                const long long qrel = 36ll + lrn + 4ll * nc + ((ls > 0 ? ls : 0) + 1) / 2;
                qoff = ro + (uint64_t)qrel;
                lseq = ls < 0 || qrel >= rec_len ? 0 : ls < rec_len - qrel ? ls : rec_len - qrel;      // (QUAL is never read behind the record)
            }
        }
        for (uint32_t r = 0; __ballot(k0 + r < k1) != 0ull; r++) {
            const bool on = k0 + r < k1;
            const uint32_t k = k0 + r;
            unsigned long long sumq = 0;
            if (on && ne) sumq = dep_walk_row<BQ, DEL, WORDS>(ub, mis, qoff, lseq, a.min_baseq, cig, ne, p0, a.rbeg[k], a.rend[k], diff + a.rbase[k], sub);
            if (!WORDS) continue;
            sumq += __shfl_xor(sumq, 1); sumq += __shfl_xor(sumq, 2); sumq += __shfl_xor(sumq, 4);
            const uint32_t idx = on ? DEP_WORD_IDX(k, blockIdx.x & (DEP_REPLICAS - 1u)) : COV_NO_IDX;
            const int src = (int)((lane & 7u) * DEP_LANES);
            uint32_t idxc = __shfl(idx, src); const unsigned long long mqc = __shfl(mq, src), sqc = __shfl(sumq, src);
            if (lane >= 64u / DEP_LANES) idxc = COV_NO_IDX;
            cov_merge<true, false>(idxc, mqc, lane, words, DEP_W_READS, DEP_W_MAPQ);
            cov_merge<true, false>(idxc, sqc, lane, words, DEP_W_SPARE, DEP_W_BASEQ);
        }
        if (!WORDS && s == DEP_STEP_COUNTED && sub == 0) touched[a.tid[i]] = 1u;
        const uint32_t sv = sub == 0 ? s : (uint32_t)DEP_STEP_NONE;
#pragma unroll
        for (uint32_t k = 0; k < DEP_N_STEPS; k++) { const unsigned long long m = __ballot(sv == k); if (lane == k) mine += (unsigned long long)__popcll(m); }
    }
    if (lane < DEP_N_STEPS && mine) atomicAdd(&block_steps[lane], mine);
    __syncthreads();
    if (threadIdx.x < DEP_N_STEPS && block_steps[threadIdx.x]) atomicAdd(&steps[threadIdx.x], block_steps[threadIdx.x]);
}
template <bool BQ> __global__ void __launch_bounds__(256) bam_depth_add(DepArgs a, int32_t *__restrict__ diff, unsigned long long *__restrict__ words, unsigned long long *__restrict__ steps) {
    dep_add_body<BQ, false, true>(a, diff, words, nullptr, steps);
}

// ---- the result: depth = the inclusive scan of diff; nothing of it is written back ------------------------------------------------------
// (32-bit sums wrap; the depth in front of a tile and inside it is what the contract bounds by 32 bits.  The tile sums become the depth in
// front of every tile by the carry in two levels, dev_scan.hip)
__global__ void __launch_bounds__(256) dep_tile_sum(const int32_t *__restrict__ diff, uint32_t *__restrict__ tsum) {
    __shared__ uint32_t sh[256];
    const int4 v = *(const int4 *)(diff + (uint64_t)blockIdx.x * DEP_TILE + threadIdx.x * 4u);
    const uint32_t tot = block_scan<uint32_t, ScanSum>((uint32_t)v.x + (uint32_t)v.y + (uint32_t)v.z + (uint32_t)v.w, sh);
    if (threadIdx.x == 255u) tsum[blockIdx.x] = tot;
}
// per tile: the positions of its row with depth >= min_depth, and the sum of their depths (a tile belongs to one row: the spans are padded)
__global__ void __launch_bounds__(256) dep_tile_reduce(const int32_t *__restrict__ diff, const uint32_t *__restrict__ tcarry, const uint32_t *__restrict__ tile_row,
                                                       const unsigned long long *__restrict__ rbase, const long long *__restrict__ rbeg, const long long *__restrict__ rend,
                                                       long long min_depth, uint32_t *__restrict__ tcov, unsigned long long *__restrict__ tdepth) {
    __shared__ uint32_t sh[256];
    __shared__ unsigned long long shd[256];
    const uint64_t e0 = (uint64_t)blockIdx.x * DEP_TILE + threadIdx.x * 4u;
    const int4 v = *(const int4 *)(diff + e0);
    const uint32_t d[4] = {(uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w};
    const uint32_t tot = d[0] + d[1] + d[2] + d[3];
    uint32_t run = tcarry[blockIdx.x] + block_scan<uint32_t, ScanSum>(tot, sh) - tot;
    const uint32_t k = tile_row[blockIdx.x];
    const uint64_t len = (uint64_t)(rend[k] - rbeg[k]), p0 = e0 - rbase[k];
    uint32_t cov = 0; unsigned long long sum = 0;
#pragma unroll
    for (uint32_t e = 0; e < 4u; e++) {
        run += d[e];
        if (p0 + e < len) { const long long depth = (long long)(int32_t)run; sum += (unsigned long long)depth; cov += depth >= min_depth ? 1u : 0u; }
    }
    sh[threadIdx.x] = cov; shd[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t s = 128u; s > 0u; s >>= 1) {
        if (threadIdx.x < s) { sh[threadIdx.x] += sh[threadIdx.x + s]; shd[threadIdx.x] += shd[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { tcov[blockIdx.x] = sh[0]; tdepth[blockIdx.x] = shd[0]; }
}
// per row: res[5 k ..] = covbases, sum_depth summed over the row's tiles, and numreads, sum_mapq, sum_baseq folded over the copies of its words
#define DEP_RES_WORDS 5u
__global__ void __launch_bounds__(256) dep_row_sum(const uint32_t *__restrict__ tcov, const unsigned long long *__restrict__ tdepth, const unsigned long long *__restrict__ rbase,
                                                   const long long *__restrict__ rbeg, const long long *__restrict__ rend, const unsigned long long *__restrict__ words, unsigned long long *__restrict__ res) {
    __shared__ unsigned long long shc[256], shd[256];
    const uint32_t k = blockIdx.x;
    const uint64_t t0 = rbase[k] / DEP_TILE, t1 = t0 + ((uint64_t)(rend[k] - rbeg[k]) + 1u + DEP_TILE - 1u) / DEP_TILE;
    unsigned long long cov = 0, sum = 0;
    for (uint64_t t = t0 + threadIdx.x; t < t1; t += 256u) { cov += tcov[t]; sum += tdepth[t]; }
    shc[threadIdx.x] = cov; shd[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t s = 128u; s > 0u; s >>= 1) {
        if (threadIdx.x < s) { shc[threadIdx.x] += shc[threadIdx.x + s]; shd[threadIdx.x] += shd[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { res[(uint64_t)DEP_RES_WORDS * k] = shc[0]; res[(uint64_t)DEP_RES_WORDS * k + 1] = shd[0]; }
    if (threadIdx.x < 3u) {
        unsigned long long v = 0;
        for (uint32_t rep = 0; rep < DEP_REPLICAS; rep++) v += words[(uint64_t)COV_WORDS * DEP_WORD_IDX(k, rep) + threadIdx.x];      // (DEP_W_READS, _MAPQ, _BASEQ = 0, 1, 2)
        res[(uint64_t)DEP_RES_WORDS * k + 2u + threadIdx.x] = v;
    }
}
