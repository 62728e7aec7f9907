// interval_sort.hip -- the sort of the interval functions (interval_merge, interval_overlap): a stable LSD radix sort of
// (key, row) pairs on the device (gfx950), 8 bits a pass.  Included by dhts_api.hip behind dev_scan.hip's users; launched by
// dhts_interval.inc (ivl_sort).
//
//   key      64 bits, compared unsigned: an interval's start with the sign bit flipped.  Passes 0 .. 7 take its bytes from the lowest up.
//   rank     32 bits per ROW (rank[row], not per pair): the chrom's place in byte order.  Passes 8 .. 11 take its bytes, read through the
//            pair's row, so the pairs stay 12 bytes.
//   skipped  a pass whose digit is the same in every pair moves nothing: ivl_sort_bits leaves the OR and the AND of all keys and of all
//            ranks, and a digit in which the two agree is not sorted.  Positions below 2^32 on fewer than 257 chroms: 4 + 1 passes.
//   a pass   ivl_sort_count: one workgroup per tile of IVL_SORT_TILE pairs, a histogram of the digit in LDS (one per wave, LDS atomics),
//            counts[digit * ntiles + tile].  The carry of dev_scan.hip turns counts, read digit-major, into where every (digit, tile) group
//            starts.  ivl_sort_scatter ranks the tile's pairs stably and writes every digit's pairs as one run.
//   ranking  element e of a tile belongs to wave e / 1024, step (e / 64) % 16, lane e % 64: a wave's loads are 64 consecutive pairs.  In a
//            step the lanes of equal digit find each other by eight ballots (a lane keeps the ballot or its complement by its own bit);
//            the rank in the group is the popcount of the group's lanes below, the group's highest lane adds the group's size to the
//            wave's count of that digit in LDS.  Steps follow each other in program order, so a wave's counts grow in element order.  The
//            four waves' counts are then turned into starts, digit by digit (one thread per digit, block_scan across the digits), and
//            every pair goes to its place in the LDS copy of the tile -- 48 KiB, the whole kernel 53 KiB: three workgroups per CU.
//   writing  thread t takes places t, t + 256, ... of the sorted tile: consecutive lanes hold consecutive pairs of one digit's run, bound for
//            consecutive addresses (base[digit] + place in the run), so a wave's store is a few contiguous segments, not 64 scattered ones.
// A tile that is not full (the last one) has its missing pairs masked out of the ballots and the counts.
#pragma once
#include "dev_scan.hip"

#define IVL_SORT_NT 256u
#define IVL_SORT_PER 16u
#define IVL_SORT_TILE (IVL_SORT_NT * IVL_SORT_PER)      /* 4,096 pairs: duckhts_amd.IVL_SORT_TILE */
#define IVL_SORT_KEY_PASSES 8
#define IVL_SORT_MAX_PASSES 12

// the digit of a pair in pass p: a byte of the key, or (p >= 8) of its row's rank
template <bool RANK> __device__ __forceinline__ uint32_t ivl_digit(unsigned long long key, uint32_t row, const uint32_t *__restrict__ rank, uint32_t shift) {
    return RANK ? (rank[row] >> shift) & 255u : (uint32_t)(key >> shift) & 255u;
}

// bits[0] |= every key, bits[1] &= every key, bits[2] |= every rank, bits[3] &= every rank (the caller sets 0, ~0, 0, ~0)
extern "C" __global__ void __launch_bounds__(256)
ivl_sort_bits(const unsigned long long *__restrict__ key, const uint32_t *__restrict__ row, const uint32_t *__restrict__ rank, uint64_t n, unsigned long long *bits) {
    __shared__ unsigned long long sh[4][4];
    unsigned long long ko = 0, ka = ~0ull, ro = 0, ra = ~0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * IVL_SORT_TILE + threadIdx.x; i < n && i < ((uint64_t)blockIdx.x + 1) * IVL_SORT_TILE; i += 256u) {
        const unsigned long long k = key[i], r = rank[row[i]];
        ko |= k; ka &= k; ro |= r; ra &= r;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { ko |= __shfl_xor(ko, d, 64); ka &= __shfl_xor(ka, d, 64); ro |= __shfl_xor(ro, d, 64); ra &= __shfl_xor(ra, d, 64); }
    if ((threadIdx.x & 63u) == 0) { const uint32_t w = threadIdx.x >> 6; sh[0][w] = ko; sh[1][w] = ka; sh[2][w] = ro; sh[3][w] = ra; }
    __syncthreads();
    if (threadIdx.x == 0) {                                     // one atomic of each kind per workgroup
        atomicOr(bits + 0, sh[0][0] | sh[0][1] | sh[0][2] | sh[0][3]); atomicAnd(bits + 1, sh[1][0] & sh[1][1] & sh[1][2] & sh[1][3]);
        atomicOr(bits + 2, sh[2][0] | sh[2][1] | sh[2][2] | sh[2][3]); atomicAnd(bits + 3, sh[3][0] & sh[3][1] & sh[3][2] & sh[3][3]);
    }
}

// counts[digit * ntiles + tile] = the tile's pairs of that digit
template <bool RANK> __global__ void __launch_bounds__(256)
ivl_sort_count(const unsigned long long *__restrict__ key, const uint32_t *__restrict__ row, const uint32_t *__restrict__ rank, uint64_t n, uint32_t shift, uint32_t ntiles,
               uint32_t *__restrict__ counts) {
    __shared__ uint32_t hist[4][256];
    const uint32_t t = threadIdx.x, w = t >> 6;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) hist[k][t] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * IVL_SORT_TILE;
#pragma unroll 4
    for (uint32_t j = 0; j < IVL_SORT_PER; j++) {
        const uint64_t i = base + j * 256u + t;
        if (i < n) atomicAdd(&hist[w][ivl_digit<RANK>(RANK ? 0ull : key[i], RANK ? row[i] : 0u, rank, shift)], 1u);
    }
    __syncthreads();
    counts[(uint64_t)t * ntiles + blockIdx.x] = hist[0][t] + hist[1][t] + hist[2][t] + hist[3][t];
}

// base = counts behind their exclusive scan in digit-major order.  (key, row) -> (key_out, row_out), stable.
template <bool RANK> __global__ void __launch_bounds__(256)
ivl_sort_scatter(const unsigned long long *__restrict__ key, const uint32_t *__restrict__ row, const uint32_t *__restrict__ rank, uint64_t n, uint32_t shift, uint32_t ntiles,
                 const uint32_t *__restrict__ base, unsigned long long *__restrict__ key_out, uint32_t *__restrict__ row_out) {
    __shared__ unsigned long long lkey[IVL_SORT_TILE];
    __shared__ uint32_t lrow[IVL_SORT_TILE];
    __shared__ uint32_t wcnt[4][256];
    __shared__ uint32_t sh[256];
    const uint32_t t = threadIdx.x, w = t >> 6, lane = t & 63u;
    const uint64_t tile0 = (uint64_t)blockIdx.x * IVL_SORT_TILE;
    const uint32_t tile_n = n - tile0 < IVL_SORT_TILE ? (uint32_t)(n - tile0) : IVL_SORT_TILE;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) wcnt[k][t] = 0;
    __syncthreads();
    unsigned long long k_[IVL_SORT_PER]; uint32_t r_[IVL_SORT_PER], at_[IVL_SORT_PER];       // at_: digit << 16 | rank among the wave's pairs of that digit
#pragma unroll
    for (uint32_t j = 0; j < IVL_SORT_PER; j++) {
        const uint32_t e = w * (IVL_SORT_TILE / 4u) + j * 64u + lane;
        const bool live = e < tile_n;
        k_[j] = live ? key[tile0 + e] : 0ull; r_[j] = live ? row[tile0 + e] : 0u;
    }
#pragma unroll
    for (uint32_t j = 0; j < IVL_SORT_PER; j++) {
        const uint32_t e = w * (IVL_SORT_TILE / 4u) + j * 64u + lane;
        const bool live = e < tile_n;
        const uint32_t d = live ? ivl_digit<RANK>(k_[j], r_[j], rank, shift) : 0u;
        unsigned long long m = __ballot(live);
#pragma unroll
        for (uint32_t b = 0; b < 8; b++) { const unsigned long long bal = __ballot((d >> b) & 1u); m &= ((d >> b) & 1u) ? bal : ~bal; }
        uint32_t pre = 0;
        if (live) pre = wcnt[w][d];
        __builtin_amdgcn_wave_barrier();                       // (every lane of the group has read the count before its highest lane replaces it)
        if (live && (m >> lane) == 1ull) wcnt[w][d] = pre + (uint32_t)__popcll(m);
        __builtin_amdgcn_wave_barrier();
        at_[j] = d << 16 | (pre + (uint32_t)__popcll(m & below));
    }
    __syncthreads();
    // digit t: its pairs in the tile, where they start in the sorted tile, where each wave's share starts, and where the run goes in the output
    const uint32_t c0 = wcnt[0][t], c1 = wcnt[1][t], c2 = wcnt[2][t], c3 = wcnt[3][t], tot = c0 + c1 + c2 + c3;
    const uint32_t first = block_scan<uint32_t, ScanSum>(tot, sh) - tot;
    wcnt[0][t] = first; wcnt[1][t] = first + c0; wcnt[2][t] = first + c0 + c1; wcnt[3][t] = first + c0 + c1 + c2;
    sh[t] = base[(uint64_t)t * ntiles + blockIdx.x] - first;                            // + the place in the sorted tile = the place in the output
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < IVL_SORT_PER; j++) {
        const uint32_t e = w * (IVL_SORT_TILE / 4u) + j * 64u + lane;
        if (e < tile_n) { const uint32_t p = wcnt[w][at_[j] >> 16] + (at_[j] & 0xffffu); lkey[p] = k_[j]; lrow[p] = r_[j]; }
    }
    __syncthreads();
    for (uint32_t p = t; p < tile_n; p += 256u) {
        const unsigned long long k = lkey[p]; const uint32_t r = lrow[p];
        const uint32_t o = sh[ivl_digit<RANK>(k, r, rank, shift)] + p;
        key_out[o] = k; row_out[o] = r;
    }
}
