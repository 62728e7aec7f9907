// bam_depth_hist.hip -- bam_depth_hist: per group of target rows the number of positions on every depth (mosdepth's *.dist.txt, the COV section of
// `samtools stats`), binned on the device out of the difference table bam_depth's add pass fills (bam_depth.hip, bam_coverage.hip: the table, the
// tiles and the target rows are described there).  The contract is in include/duckhts_amd.h; the host side in dhts_bam_depth_hist.inc.
//
//   bin          bin(d) = min(d, depth_cap); a group's row of the histogram table has depth_cap + 1 64-bit words
//   hist         one read of the table behind dep_tile_sum + the 32-bit carry.  A workgroup owns a span of consecutive tiles, recovers the depth
//                on its four slots per thread as bdg_lane does, and counts into an LDS histogram of DHI_LDS_BINS 32-bit bins; a bin at or above
//                DHI_LDS_BINS is added to the table at once (64-bit atomic).  Depth is piecewise constant: a thread adds a run of equal slots once,
//                and a wave whose 256 slots are all live and hold one depth adds 256 once.  The LDS histogram is flushed into the table (non-zero
//                bins up to the highest one touched, 64-bit atomics) when the next tile belongs to another group and at the end of the span.
//   group count  per group the non-empty bins; their carry (depth_carry, 64-bit) is the result index in front of every group
//   emit         a window [o_a, o_b) of result indices and the contiguous groups that hold it: a workgroup walks its group's bins from the top
//                down, DHI_EMIT_CHUNK a turn, carries the suffix sum (n_at_least) and the number of non-empty bins above in two block scans, and
//                writes the non-empty bins whose result index lies in the window.  Columns whose pointer is null are skipped.
#pragma once
#include "bam_depth.hip"

#define DHI_LDS_BINS 4096u                                                  /* bins of the workgroup's LDS histogram: 16 KiB */
#define DHI_GRID_TARGET 2048u                                               /* workgroups the spans are cut for: 8 per CU of 256 */
#define DHI_SPAN_MIN_TILES 8u                                               /* a span is never shorter: 32 KiB of the table */
#define DHI_EMIT_CHUNK 1024u                                                /* bins of a turn of the emit walk: four per thread */
// The bound of the LDS counters: a span has ceil(ntiles / DHI_GRID_TARGET) tiles and no fewer than DHI_SPAN_MIN_TILES.  A bin counts at most
// every slot of the span between two flushes, span * DEP_TILE; the host refuses a span of 2^22 tiles or more (dhi_span_tiles' caller), so a
// counter stays below 2^32.  The 16 GiB table cap gives 2^22 tiles and a span of 2,048: 2^21 slots.

// one add of n positions on depth d of group row `grow` of the table (cap + 1 words): LDS below DHI_LDS_BINS, the table at once above
__device__ __forceinline__ void dhi_add(uint32_t *lh, uint32_t &hi, unsigned long long *__restrict__ grow, uint32_t cap, uint32_t d, uint32_t n) {
    const uint32_t bin = d < cap ? d : cap;
    if (bin < DHI_LDS_BINS) { atomicAdd(&lh[bin], n); hi = bin > hi ? bin : hi; }
    else atomicAdd(&grow[bin], (unsigned long long)n);
}
// the LDS histogram into group row `grow`, zeroed behind it; hi: every thread's highest bin since the last flush (the same for the whole workgroup
// on return: 0).  Called by the whole workgroup.
__device__ __forceinline__ void dhi_flush(uint32_t *lh, uint32_t *lhi, uint32_t &hi, unsigned long long *__restrict__ grow) {
    atomicMax(lhi, hi);
    __syncthreads();                                                                               // (every add of the group is in lh, every hi in lhi)
    const uint32_t top = *lhi;
    for (uint32_t b = threadIdx.x; b <= top; b += 256u) {
        const uint32_t v = lh[b];
        if (v) { atomicAdd(&grow[b], (unsigned long long)v); lh[b] = 0u; }
    }
    __syncthreads();
    if (threadIdx.x == 0u) *lhi = 0u;
    hi = 0u;
    __syncthreads();
}

__global__ void __launch_bounds__(256) dhi_hist(const int32_t *__restrict__ diff, const uint32_t *__restrict__ tcarry, const uint32_t *__restrict__ tile_row,
                                                const uint32_t *__restrict__ row_group, const unsigned long long *__restrict__ rbase, const long long *__restrict__ rbeg,
                                                const long long *__restrict__ rend, uint64_t ntiles, uint64_t span, uint32_t cap, unsigned long long *__restrict__ table) {
    __shared__ uint32_t sh[256];
    __shared__ uint32_t lh[DHI_LDS_BINS];
    __shared__ uint32_t lhi;
    const uint64_t t_a = (uint64_t)blockIdx.x * span, t_b = t_a + span < ntiles ? t_a + span : ntiles;
    if (t_a >= t_b) return;                                                                       // (the same for the whole workgroup)
    for (uint32_t b = threadIdx.x; b < DHI_LDS_BINS; b += 256u) lh[b] = 0u;
    if (threadIdx.x == 0u) lhi = 0u;
    __syncthreads();
    const uint64_t words = (uint64_t)cap + 1u;
    uint32_t hi = 0u, g = row_group[tile_row[t_a]];
    for (uint64_t tile = t_a; tile < t_b; tile++) {
        const uint32_t k = tile_row[tile], gt = row_group[k];                                     // (the same for the whole workgroup)
        if (gt != g) { dhi_flush(lh, &lhi, hi, table + (uint64_t)g * words); g = gt; }
        const uint64_t len = (uint64_t)(rend[k] - rbeg[k]), tp = tile * DEP_TILE - rbase[k];
        if (tp >= len) continue;                                                                  // a tile of padding alone (the closing slot of a row of n * 1,024)
        unsigned long long *const grow = table + (uint64_t)g * words;
        const int4 v = *(const int4 *)(diff + tile * DEP_TILE + threadIdx.x * 4u);
        const uint32_t d[4] = {(uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w};
        const uint32_t tot = d[0] + d[1] + d[2] + d[3];
        uint32_t run = tcarry[tile] + block_scan<uint32_t, ScanSum>(tot, sh) - tot, dep[4];
#pragma unroll
        for (uint32_t e = 0; e < 4u; e++) { run += d[e]; dep[e] = run; }
        const uint64_t p0 = tp + threadIdx.x * 4u;
        const uint32_t live = p0 + 4u <= len ? 4u : p0 < len ? (uint32_t)(len - p0) : 0u;         // the thread's slots inside the row: a prefix of the four
        // a wave whose lanes all hold the first lane's depth on four live slots: one add of the whole count
        const uint32_t first = (uint32_t)__shfl((int)dep[0], 0, 64);
        const bool flat = live == 4u && dep[0] == first && dep[1] == first && dep[2] == first && dep[3] == first;
        if (__ballot(flat) == ~0ull) {
            if ((threadIdx.x & 63u) == 0u) dhi_add(lh, hi, grow, cap, first, 256u);
        } else if (live) {                                                                        // a thread merges its equal slots into one add
            uint32_t cur = dep[0], n = 1u;
#pragma unroll
            for (uint32_t e = 1; e < 4u; e++) {
                if (e >= live) break;
                if (dep[e] == cur) n++; else { dhi_add(lh, hi, grow, cap, cur, n); cur = dep[e]; n = 1u; }
            }
            dhi_add(lh, hi, grow, cap, cur, n);
        }
    }
    dhi_flush(lh, &lhi, hi, table + (uint64_t)g * words);
}

// gcnt[g] = the non-empty bins of group g
__global__ void __launch_bounds__(256) dhi_group_count(const unsigned long long *__restrict__ table, uint32_t cap, unsigned long long *__restrict__ gcnt) {
    __shared__ uint32_t sh[256];
    const unsigned long long *row = table + (uint64_t)blockIdx.x * ((uint64_t)cap + 1u);
    uint32_t cnt = 0;
    for (uint64_t b = threadIdx.x; b <= cap; b += 256u) cnt += row[b] != 0ull ? 1u : 0u;
    const uint32_t incl = block_scan<uint32_t, ScanSum>(cnt, sh);
    if (threadIdx.x == 255u) gcnt[blockIdx.x] = incl;
}

struct DhiEmitArgs {
    const unsigned long long *table, *goff;                                                       // the histogram; the result index in front of every group
    const int32_t *g_tid; const long long *g_beg, *g_end, *g_len; uint32_t cap;                    // the groups
    unsigned long long g0, o_a, o_b;                                                               // the first group and the window; result index o_a is page row 0
    int32_t *out_tid; long long *out_start, *out_end; int32_t *out_depth; long long *out_n, *out_at_least, *out_len;      // the page (null: the column is not wanted)
};
__global__ void __launch_bounds__(256) dhi_emit(DhiEmitArgs a) {
    __shared__ uint32_t sh[256];
    __shared__ unsigned long long sh64[256];
    const uint64_t g = a.g0 + blockIdx.x;
    const unsigned long long ob = a.goff[g], oe = a.goff[g + 1];
    if (oe <= a.o_a || ob >= a.o_b || oe == ob) return;                                           // (the same for the whole workgroup)
    const unsigned long long *row = a.table + g * ((uint64_t)a.cap + 1u);
    const int32_t tid = a.g_tid[g];
    const long long beg = a.g_beg[g], end = a.g_end[g], len = a.g_len[g];
    unsigned long long above_sum = 0, above_cnt = 0;                                               // of the bins above this turn's: their positions, and how many are non-empty
    for (long long top = (long long)a.cap; top >= 0; top -= (long long)DHI_EMIT_CHUNK) {
        unsigned long long v[4], tot = 0; uint32_t cnt = 0;
#pragma unroll
        for (uint32_t e = 0; e < 4u; e++) {                                                        // the thread's bins, descending: top - 4 t - e
            const long long b = top - (long long)(threadIdx.x * 4u + e);
            v[e] = b >= 0 ? row[b] : 0ull;
            tot += v[e]; cnt += v[e] != 0ull ? 1u : 0u;
        }
        const unsigned long long incl_sum = block_scan<unsigned long long, ScanSum>(tot, sh64);
        const uint32_t incl_cnt = block_scan<uint32_t, ScanSum>(cnt, sh);
        unsigned long long run_sum = above_sum + incl_sum - tot, run_cnt = above_cnt + incl_cnt - cnt;
#pragma unroll
        for (uint32_t e = 0; e < 4u; e++) {
            if (v[e] == 0ull) continue;
            run_sum += v[e];
            const unsigned long long o = oe - 1ull - run_cnt;                                     // depth ascending: the highest bin is the group's last row
            run_cnt++;
            if (o < a.o_a || o >= a.o_b) continue;
            const unsigned long long r = o - a.o_a;
            if (a.out_tid) a.out_tid[r] = tid;
            if (a.out_start) a.out_start[r] = beg;
            if (a.out_end) a.out_end[r] = end;
            if (a.out_depth) a.out_depth[r] = (int32_t)(top - (long long)(threadIdx.x * 4u + e));
            if (a.out_n) a.out_n[r] = (long long)v[e];
            if (a.out_at_least) a.out_at_least[r] = (long long)run_sum;
            if (a.out_len) a.out_len[r] = len;
        }
        sh64[threadIdx.x] = incl_sum; sh[threadIdx.x] = incl_cnt;
        __syncthreads();
        above_sum += sh64[255]; above_cnt += sh[255];
        __syncthreads();
        if (oe - above_cnt <= a.o_a || above_cnt >= oe - ob) break;                                // what is left lies in front of the window, or is empty
    }
}
