// bam_depth.hip -- bam_depth: chrom, pos, depth per position (what `samtools depth` prints), streamed page by page out of the difference table
// bam_coverage's add pass fills (bam_coverage.hip; the table, the tiles and the target rows are described there).  The contract is in
// include/duckhts_amd.h; the host side in dhts_bam_depth.inc.
//
//   add          dep_add_body without the per-row words, with or without D as counted positions; a counted read marks its contig in touched
//   carry        an exclusive scan in place in two levels, for 32-bit (the depth in front of every tile) and 64-bit words (the result index in
//                front of every tile): dev_scan.hip's carry_* with ScanSum, launched by depth_carry.  The total lands behind the last word.
//   count        per tile the positions it emits: those of its row (none behind the row's end) with depth > 0, or all of them when the mode
//                and touched say so -- then the tile's table is not read
//   emit         a window [o_a, o_b) of result indices and the contiguous tiles that hold it: a workgroup rescans its tile, compacts the
//                emitting positions into LDS by a block-wide exclusive scan of the predicate, and the 256 threads write the part inside the
//                window in result order: consecutive lanes store consecutive rows of tid (4 bytes), pos (8) and depth (4), so a dense tile is
//                written in whole lines.  A sparse tile writes what it has.  Columns whose pointer is null are skipped.
#pragma once
#include "bam_coverage.hip"

template <bool BQ, bool DEL> __global__ void __launch_bounds__(256) bam_depth_add_nowords(DepArgs a, int32_t *__restrict__ diff, uint32_t *__restrict__ touched, unsigned long long *__restrict__ steps) {
    dep_add_body<BQ, DEL, false>(a, diff, nullptr, touched, steps);
}
__global__ void __launch_bounds__(256) bam_depth_classify_del(DepArgs a) { dep_classify_body<true>(a); }

// ---- count and emit ----------------------------------------------------------------------------------------------------------------------------
struct DepEmitArgs {
    const int32_t *diff; const uint32_t *tcarry; const unsigned long long *toff;                  // the table, the depth and the result index in front of every tile
    const uint32_t *tile_row; const unsigned long long *rbase; const long long *rbeg, *rend;        // the sorted rows
    const int32_t *row_tid; const uint32_t *touched; uint32_t mode;                                // 0: depth > 0; 1: all positions of a touched contig; 2: all
    unsigned long long t0, o_a, o_b, dst0;                                                         // the first tile, the window, and the page row of result index o_a
    int32_t *out_tid; long long *out_pos; int32_t *out_depth;                                      // the page (null: the column is not wanted)
};
__device__ __forceinline__ bool dep_emits_all(uint32_t mode, const uint32_t *touched, int32_t tid) { return mode == 2u || (mode == 1u && touched[tid] != 0u); }

__global__ void __launch_bounds__(256) dep_tile_count(const int32_t *__restrict__ diff, const uint32_t *__restrict__ tcarry, const uint32_t *__restrict__ tile_row,
                                                      const unsigned long long *__restrict__ rbase, const long long *__restrict__ rbeg, const long long *__restrict__ rend,
                                                      const int32_t *__restrict__ row_tid, const uint32_t *__restrict__ touched, uint32_t mode, unsigned long long *__restrict__ tcnt) {
    __shared__ uint32_t sh[256];
    const uint32_t k = tile_row[blockIdx.x];
    const uint64_t len = (uint64_t)(rend[k] - rbeg[k]), tp = (uint64_t)blockIdx.x * DEP_TILE - rbase[k];      // the row's length, the tile's first slot in it
    if (dep_emits_all(mode, touched, row_tid[k])) {                                                 // (the same for the whole workgroup)
        if (threadIdx.x == 0) tcnt[blockIdx.x] = tp >= len ? 0ull : len - tp < DEP_TILE ? len - tp : (unsigned long long)DEP_TILE;
        return;
    }
    const int4 v = *(const int4 *)(diff + (uint64_t)blockIdx.x * DEP_TILE + threadIdx.x * 4u);
    const uint32_t d[4] = {(uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w};
    const uint32_t tot = d[0] + d[1] + d[2] + d[3];
    uint32_t run = tcarry[blockIdx.x] + block_scan<uint32_t, ScanSum>(tot, sh) - tot, cnt = 0;
    const uint64_t p0 = tp + threadIdx.x * 4u;
#pragma unroll
    for (uint32_t e = 0; e < 4u; e++) { run += d[e]; cnt += p0 + e < len && (int32_t)run > 0 ? 1u : 0u; }
    const uint32_t incl = block_scan<uint32_t, ScanSum>(cnt, sh);
    if (threadIdx.x == 255u) tcnt[blockIdx.x] = incl;
}
// out[k] = the result index in front of row k (k = n_rows: the number of positions of the whole result)
__global__ void __launch_bounds__(256) dep_row_offsets(const unsigned long long *__restrict__ toff, const unsigned long long *__restrict__ rbase, uint64_t n_rows, uint64_t ntiles, unsigned long long *__restrict__ out) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k <= n_rows) out[k] = toff[k < n_rows ? rbase[k] / DEP_TILE : ntiles];
}
// res[0], res[1] = the tiles that hold result indices o_a and o_b - 1 (o_a < o_b <= toff[ntiles]): the first t with toff[t + 1] > o
__global__ void dep_page_tiles(const unsigned long long *__restrict__ toff, uint64_t ntiles, unsigned long long o_a, unsigned long long o_b, unsigned long long *__restrict__ res) {
    if (threadIdx.x >= 2u || blockIdx.x != 0u) return;
    const unsigned long long o = threadIdx.x == 0u ? o_a : o_b - 1ull;
    uint64_t lo = 0, hi = ntiles;                                                                 // the answer lies in [lo, hi)
    while (hi - lo > 1u) { const uint64_t mid = lo + (hi - lo) / 2u; if (toff[mid] > o) hi = mid; else lo = mid; }
    res[threadIdx.x] = lo;
}
__global__ void __launch_bounds__(256) dep_emit(DepEmitArgs a) {
    __shared__ uint32_t sh[256];
    __shared__ uint32_t ldep[DEP_TILE];
    __shared__ uint16_t lpos[DEP_TILE];
    const uint64_t tile = a.t0 + blockIdx.x;
    const unsigned long long ob = a.toff[tile], oe = a.toff[tile + 1];
    if (oe <= a.o_a || ob >= a.o_b || oe == ob) return;                                           // (the same for the whole workgroup)
    const uint32_t k = a.tile_row[tile];
    const int32_t tid = a.row_tid[k];
    const uint64_t len = (uint64_t)(a.rend[k] - a.rbeg[k]), tp = tile * DEP_TILE - a.rbase[k], p0 = tp + threadIdx.x * 4u;
    const bool all = dep_emits_all(a.mode, a.touched, tid);
    const int4 v = *(const int4 *)(a.diff + tile * DEP_TILE + threadIdx.x * 4u);
    const uint32_t d[4] = {(uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w};
    const uint32_t tot = d[0] + d[1] + d[2] + d[3];
    uint32_t run = a.tcarry[tile] + block_scan<uint32_t, ScanSum>(tot, sh) - tot, dep[4], em = 0, cnt = 0;
#pragma unroll
    for (uint32_t e = 0; e < 4u; e++) { run += d[e]; dep[e] = run; if (p0 + e < len && (all || (int32_t)run > 0)) { em |= 1u << e; cnt++; } }
    uint32_t at = block_scan<uint32_t, ScanSum>(cnt, sh) - cnt;                                                   // (ends in a barrier)
#pragma unroll
    for (uint32_t e = 0; e < 4u; e++) if ((em >> e) & 1u) { ldep[at] = dep[e]; lpos[at] = (uint16_t)(threadIdx.x * 4u + e); at++; }
    __syncthreads();
    const uint32_t n = (uint32_t)(oe - ob);                                                        // (<= DEP_TILE: what dep_tile_count counted by the same rule)
    const long long pos1 = a.rbeg[k] + (long long)tp + 1;                                          // 1-based position of the tile's first slot
    for (uint32_t j = threadIdx.x; j < n && j < DEP_TILE; j += 256u) {
        const unsigned long long o = ob + j;
        if (o < a.o_a || o >= a.o_b) continue;
        const unsigned long long r = a.dst0 + (o - a.o_a);
        if (a.out_tid) a.out_tid[r] = tid;
        if (a.out_pos) a.out_pos[r] = pos1 + (long long)lpos[j];
        if (a.out_depth) a.out_depth[r] = (int32_t)ldep[j];
    }
}
