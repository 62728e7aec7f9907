// bam_bedgraph.hip -- bam_bedgraph: chrom, start, end, depth per run of equal depth class (bedGraph rows, what `bedtools genomecov -bg / -bga`
// and `mosdepth --quantize` print), streamed page by page out of the difference table bam_depth's add pass fills (bam_depth.hip, bam_coverage.hip:
// the table, the tiles and the target rows are described there).  The contract is in include/duckhts_amd.h; the host side in
// dhts_bam_bedgraph.inc.
//
//   class        class(d) = d without breaks, else the number of breaks <= d: one compare per break given, at most 16
//   boundary     a slot p < len of a row that is the row's first or whose class differs from the class of the slot in front of it; the depth in
//                front of a tile is tcarry[tile] (dep_tile_sum + the 32-bit carry).  A boundary is emitted iff its class is > 0 or zero_runs is on.
//   count        per tile the emitted boundaries (tcnt, which the 64-bit carry turns into the result index in front of every tile) and the
//                global slot of its first boundary of any class (tfirst; `none` where it has no boundary)
//   suffix       tfirst[t] becomes tnext[t], the least tfirst behind t, or `none`: dev_scan.hip's carry_* in reverse with ScanMin.  It needs
//                no segmentation: a row's first slot is always a boundary, and the user clips to the end of its own row.
//   emit         a window [o_a, o_b) of result indices and the contiguous tiles that hold it: a workgroup rescans its tile, compacts all
//                boundaries into LDS and of the emitted ones their index among all and their class's depth.  A run ends at the next boundary of
//                any class in the tile, else at min(tnext[tile], rbase[k] + len).  Consecutive lanes store consecutive rows of tid (4 bytes),
//                start (8), end (8) and depth (4).  Columns whose pointer is null are skipped.
#pragma once
#include "bam_depth.hip"

#define BDG_MAX_BREAKS 16u
struct BdgClasses { uint32_t n, zero_runs; uint32_t br[BDG_MAX_BREAKS]; };                        // the first n breaks, ascending
__device__ __forceinline__ uint32_t bdg_class(const BdgClasses &c, uint32_t d) {
    if (c.n == 0u) return d;
    uint32_t k = 0;
    for (uint32_t j = 0; j < c.n; j++) k += d >= c.br[j] ? 1u : 0u;                               // (c is a kernel argument: the trip count is the same in every lane)
    return k;
}
__device__ __forceinline__ uint32_t bdg_class_depth(const BdgClasses &c, uint32_t cls) { return c.n == 0u || cls == 0u ? cls : c.br[cls - 1u]; }

// The four slots of a thread: dep[e] the depth on slot e, bnd / em bit e set where the slot is a boundary / an emitted one.  The depth in
// front of the thread's first slot is the scan's exclusive value, which for thread 0 is the tile's carry.
struct BdgLane { uint32_t cls[4], bnd, em; };
__device__ __forceinline__ BdgLane bdg_lane(const int32_t *__restrict__ diff, uint64_t tile, uint32_t carry, uint64_t tp, uint64_t len, const BdgClasses &c, uint32_t *sh) {
    const int4 v = *(const int4 *)(diff + tile * DEP_TILE + threadIdx.x * 4u);
    const uint32_t d[4] = {(uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w};
    const uint32_t tot = d[0] + d[1] + d[2] + d[3];
    uint32_t run = carry + block_scan<uint32_t, ScanSum>(tot, sh) - tot, prev = bdg_class(c, run);
    const uint64_t p0 = tp + threadIdx.x * 4u;
    BdgLane r; r.bnd = 0; r.em = 0;
#pragma unroll
    for (uint32_t e = 0; e < 4u; e++) {
        run += d[e];
        const uint32_t k = bdg_class(c, run);
        r.cls[e] = k;
        if (p0 + e < len && (p0 + e == 0u || k != prev)) { r.bnd |= 1u << e; if (k > 0u || c.zero_runs) r.em |= 1u << e; }
        prev = k;
    }
    return r;
}

__global__ void __launch_bounds__(256) bdg_tile_count(const int32_t *__restrict__ diff, const uint32_t *__restrict__ tcarry, const uint32_t *__restrict__ tile_row,
                                                      const unsigned long long *__restrict__ rbase, const long long *__restrict__ rbeg, const long long *__restrict__ rend,
                                                      BdgClasses c, unsigned long long none, unsigned long long *__restrict__ tcnt, unsigned long long *__restrict__ tfirst) {
    __shared__ uint32_t sh[256];
    __shared__ uint32_t wmin[4], wcnt[4];
    const uint64_t tile = blockIdx.x;
    const uint32_t k = tile_row[tile];
    const uint64_t len = (uint64_t)(rend[k] - rbeg[k]), tp = tile * DEP_TILE - rbase[k];
    const BdgLane r = bdg_lane(diff, tile, tcarry[tile], tp, len, c, sh);
    // only the tile's totals are wanted here, so no second scan: both are reduced inside the wave, and one thread joins the four waves
    uint32_t first = r.bnd ? threadIdx.x * 4u + (uint32_t)__builtin_ctz(r.bnd) : DEP_TILE, cnt = (uint32_t)__popc(r.em);
#pragma unroll
    for (uint32_t d = 32u; d > 0u; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)first, (int)d, 64);
        first = o < first ? o : first;
        cnt += (uint32_t)__shfl_xor((int)cnt, (int)d, 64);
    }
    if ((threadIdx.x & 63u) == 0u) { wmin[threadIdx.x >> 6] = first; wcnt[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t f = wmin[0], n = wcnt[0];
        for (uint32_t w = 1; w < 4u; w++) { f = wmin[w] < f ? wmin[w] : f; n += wcnt[w]; }
        tcnt[tile] = n;
        tfirst[tile] = f < DEP_TILE ? tile * DEP_TILE + f : none;
    }
}

// ---- emit --------------------------------------------------------------------------------------------------------------------------------------
struct BdgEmitArgs {
    const int32_t *diff; const uint32_t *tcarry; const unsigned long long *toff, *tnext;          // the table; the depth, the result index and the next boundary behind every tile
    const uint32_t *tile_row; const unsigned long long *rbase; const long long *rbeg, *rend;        // the sorted rows
    const int32_t *row_tid; BdgClasses c;
    unsigned long long t0, o_a, o_b, dst0;                                                         // the first tile, the window, and the page row of result index o_a
    int32_t *out_tid; long long *out_start, *out_end; int32_t *out_depth;                           // the page (null: the column is not wanted)
};
__global__ void __launch_bounds__(256) bdg_emit(BdgEmitArgs a) {
    __shared__ uint32_t sh[256];
    __shared__ uint32_t ldep[DEP_TILE];                                                            // of emitted boundary j: its class's depth
    __shared__ uint16_t lsel[DEP_TILE], lpos[DEP_TILE + 1u];                                       // ... its index among all boundaries; of boundary i: its slot in the tile
    const uint64_t tile = a.t0 + blockIdx.x;
    const unsigned long long ob = a.toff[tile], oe = a.toff[tile + 1];
    if (oe <= a.o_a || ob >= a.o_b || oe == ob) return;                                           // (the same for the whole workgroup)
    const uint32_t k = a.tile_row[tile];
    const uint64_t len = (uint64_t)(a.rend[k] - a.rbeg[k]), tp = tile * DEP_TILE - a.rbase[k];
    const BdgLane r = bdg_lane(a.diff, tile, a.tcarry[tile], tp, len, a.c, sh);
    const uint32_t nb = (uint32_t)__popc(r.bnd), ne = (uint32_t)__popc(r.em);
    const uint32_t ib = block_scan<uint32_t, ScanSum>(nb, sh);
    if (threadIdx.x == 255u) lpos[DEP_TILE] = (uint16_t)ib;                                        // the tile's boundaries of any class (<= DEP_TILE)
    uint32_t at_b = ib - nb, at_e = block_scan<uint32_t, ScanSum>(ne, sh) - ne;                                    // (ends in a barrier)
#pragma unroll
    for (uint32_t e = 0; e < 4u; e++) {
        if (!((r.bnd >> e) & 1u)) continue;
        if ((r.em >> e) & 1u) { ldep[at_e] = bdg_class_depth(a.c, r.cls[e]); lsel[at_e] = (uint16_t)at_b; at_e++; }
        lpos[at_b] = (uint16_t)(threadIdx.x * 4u + e); at_b++;
    }
    __syncthreads();
    const uint32_t n = (uint32_t)(oe - ob), n_all = lpos[DEP_TILE];                                // (n <= DEP_TILE: what bdg_tile_count counted by the same rule)
    const unsigned long long row_end = a.rbase[k] + len, nx = a.tnext[tile];
    const long long behind = a.rbeg[k] + (long long)((nx < row_end ? nx : row_end) - a.rbase[k]);  // where the tile's last run ends, as a position
    const long long pos0 = a.rbeg[k] + (long long)tp;                                              // 0-based position of the tile's first slot
    const int32_t tid = a.row_tid[k];
    for (uint32_t j = threadIdx.x; j < n && j < DEP_TILE; j += 256u) {
        const unsigned long long o = ob + j;
        if (o < a.o_a || o >= a.o_b) continue;
        const unsigned long long row = a.dst0 + (o - a.o_a);
        const uint32_t i = lsel[j];
        if (a.out_tid) a.out_tid[row] = tid;
        if (a.out_start) a.out_start[row] = pos0 + (long long)lpos[i];
        if (a.out_end) a.out_end[row] = i + 1u < n_all ? pos0 + (long long)lpos[i + 1u] : behind;
        if (a.out_depth) a.out_depth[row] = (int32_t)ldep[j];
    }
}
