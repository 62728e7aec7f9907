// bam_bins.hip -- bam_bin_counts: read-start counts in fixed-width bins, accumulated on the device from the fixed-width columns a
// read_bam batch leaves in HBM (FLAG, tid, POS, MAPQ, PNEXT).  The contract is in include/duckhts_amd.h; the host side in dhts_bam_bins.inc.
//
//   table     counts[2 * total_bins] of 64-bit words: word 2 * (bin_base[tid] + pos0 / bin_width) + (FLAG & 0x10 ? 1 : 0)
//   classify  one lane per row: the step the row falls out at (BIN_STEP_*), its table word, and whether the duplicate rule sees it
//   dedup     (dedup = adjacent) the rows the rule sees are compacted by a scan of their flags; a row's predecessor is its neighbour in
//             the compacted list, the first row's the last visible row of the batches before (BinCarry, two slots used in turn)
//   add       runs of equal words among neighbouring lanes of a wave become one atomic each; the step counters one add per workgroup
//   mark/emit the bins of a window of the table that become result rows, compacted by a scan, seven 8-byte columns
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

enum { BIN_STEP_FLAG = 0, BIN_STEP_UNPLACED, BIN_STEP_RANGE, BIN_STEP_DUP, BIN_STEP_MAPQ, BIN_STEP_COUNTED, BIN_N_STEPS, BIN_STEP_NONE = 7 };
#define BIN_NO_WORD 0xffffffffu

struct BinArgs {
    const uint16_t *flag; const int32_t *tid; const int64_t *pos; const int32_t *mapq; const int64_t *pnext;   // the batch (POS, PNEXT 1-based)
    uint32_t n;
    const uint32_t *ref_len; const uint32_t *bin_base; int32_t n_ref;      // bin_base[n_ref + 1]: the bins in front of every contig
    uint32_t bin_width;                                                     // 0: wider than any position (every row in bin 0 of its contig)
    uint32_t require, exclude, include, min_mapq;
    uint8_t *step; uint32_t *word; uint32_t *vis;                           // per row
};
// the last row in front of a batch that passed the flag and placement steps
struct BinCarry { int32_t have, tid; int64_t pos0, pnext; };

__global__ void __launch_bounds__(256) bam_bin_classify(BinArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t f = a.flag[i];
    const int32_t t = a.tid[i];
    const int64_t p0 = a.pos[i] - 1;
    uint32_t s, w = BIN_NO_WORD;
    if ((f & a.require) != a.require || (f & a.exclude) != 0 || (a.include != 0 && (f & a.include) == 0)) s = BIN_STEP_FLAG;
    else if (t < 0 || t >= a.n_ref || p0 < 0) s = BIN_STEP_UNPLACED;
    else if ((uint64_t)p0 >= (uint64_t)a.ref_len[t]) s = BIN_STEP_RANGE;
    else {
        const uint32_t b = a.bin_width ? (uint32_t)p0 / a.bin_width : 0u;    // positions are below 2^31: a 32-bit divide
        w = 2u * (a.bin_base[t] + b) + ((f >> 4) & 1u);
        s = (uint32_t)a.mapq[i] < a.min_mapq ? BIN_STEP_MAPQ : BIN_STEP_COUNTED;
    }
    a.step[i] = (uint8_t)s; a.word[i] = w;
    if (a.vis) a.vis[i] = w != BIN_NO_WORD ? 1u : 0u;
}

// rank[n + 1]: exclusive sum of vis; src[rank[i]] = i for the visible rows (fq_compact).  A visible row is a duplicate when its predecessor
// has its contig and start and (it is unpaired, or the predecessor has its PNEXT); the duplicate step comes in front of the MAPQ step.
__global__ void __launch_bounds__(256) bam_bin_dedup(BinArgs a, const uint32_t *__restrict__ rank, const uint32_t *__restrict__ src, const BinCarry *__restrict__ prev, BinCarry *__restrict__ next) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t total = rank[a.n];
    if (i == 0 && total == 0) *next = *prev;
    if (i >= a.n || a.word[i] == BIN_NO_WORD) return;
    const uint32_t r = rank[i];
    const int32_t t = a.tid[i]; const int64_t p0 = a.pos[i] - 1, pn = a.pnext[i];
    int32_t have, pt; int64_t pp, ppn;
    if (r > 0) { const uint32_t j = src[r - 1]; have = 1; pt = a.tid[j]; pp = a.pos[j] - 1; ppn = a.pnext[j]; }
    else { have = prev->have; pt = prev->tid; pp = prev->pos0; ppn = prev->pnext; }
    if (have && pt == t && pp == p0 && ((a.flag[i] & 1u) == 0 || ppn == pn)) a.step[i] = BIN_STEP_DUP;
    if (r + 1 == total) { next->have = 1; next->tid = t; next->pos0 = p0; next->pnext = pn; }
}

// counts[word] += 1 for the counted rows, steps[s] += 1 for every row.  A coordinate-sorted file puts hundreds of consecutive rows into one
// word: a lane whose word differs from the lane below heads a run, and adds the run's length once.  Nothing depends on the order of the
// rows: unsorted input makes every lane a head, a word that comes back later in the wave heads a run of its own.
// The step counters are six addresses for the whole batch: a workgroup walks its share of the rows (the grid is capped), lane k of every wave
// keeps step k's count in a register, and the workgroup adds its six sums once, through LDS.
#define BIN_ADD_MAX_BLOCKS 2048u
__global__ void __launch_bounds__(256) bam_bin_add(const uint8_t *__restrict__ step, const uint32_t *__restrict__ word, uint32_t n, unsigned long long *__restrict__ counts, unsigned long long *__restrict__ steps) {
    __shared__ unsigned long long block_steps[BIN_N_STEPS];
    const uint32_t lane = threadIdx.x & 63u;
    if (threadIdx.x < BIN_N_STEPS) block_steps[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long mine = 0;
    // (every lane of a wave makes the same number of turns and takes part in every vote: rows behind n are rows without a step)
    for (uint64_t base = (uint64_t)blockIdx.x * 256u; base < n; base += (uint64_t)gridDim.x * 256u) {
        const uint64_t i = base + threadIdx.x;
        const uint32_t s = i < n ? step[i] : (uint32_t)BIN_STEP_NONE;
        const bool counted = s == BIN_STEP_COUNTED;
        const uint32_t w = counted ? word[i] : BIN_NO_WORD;
        const uint32_t below = __shfl_up(w, 1);
        const bool head = counted && (lane == 0 || below != w);
        const unsigned long long heads = __ballot(head), live = __ballot(counted);
        if (head) {
            const unsigned long long stop = (heads | ~live) & ~((2ull << lane) - 1ull);     // the first lane above that is not part of this run
            const uint32_t end = stop ? (uint32_t)__ffsll((long long)stop) - 1u : 64u;
            atomicAdd(&counts[w], (unsigned long long)(end - lane));
        }
#pragma unroll
        for (uint32_t k = 0; k < BIN_N_STEPS; k++) { const unsigned long long m = __ballot(s == k); if (lane == k) mine += (unsigned long long)__popcll(m); }
    }
    if (lane < BIN_N_STEPS && mine) atomicAdd(&block_steps[lane], mine);
    __syncthreads();
    if (threadIdx.x < BIN_N_STEPS && block_steps[threadIdx.x]) atomicAdd(&steps[threadIdx.x], block_steps[threadIdx.x]);
}

// bins [b0, b0 + nb) of the table: keep[k] = 1 where bin b0 + k becomes a row (a count, or emit_zero_bins on a contig the scan names)
__device__ __forceinline__ int32_t bin_contig(const uint32_t *__restrict__ bin_base, int32_t n_ref, uint32_t b) {   // the last t with bin_base[t] <= b
    int32_t lo = 0, hi = n_ref;                                             // (contigs without bins share their base with the next one)
    while (hi - lo > 1) { const int32_t mid = lo + (hi - lo) / 2; if (bin_base[mid] <= b) lo = mid; else hi = mid; }
    return lo;
}
__global__ void __launch_bounds__(256) bam_bin_mark(const unsigned long long *__restrict__ counts, const uint32_t *__restrict__ bin_base, int32_t n_ref, const uint8_t *__restrict__ zero_ok,
                                                    uint32_t b0, uint32_t nb, uint32_t *__restrict__ keep) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= nb) return;
    const uint32_t b = b0 + k;
    uint32_t on = (counts[2ull * b] | counts[2ull * b + 1]) != 0 ? 1u : 0u;
    if (!on && zero_ok) on = zero_ok[bin_contig(bin_base, n_ref, b)];
    keep[k] = on;
}
struct BinCols { long long *chrom, *start, *end, *bin_id, *total, *fwd, *rev; };
// the kept bins whose rank lies in [r0, r0 + nrows) -> rows rank - r0 (chrom is the contig's id)
__global__ void __launch_bounds__(256) bam_bin_emit(const unsigned long long *__restrict__ counts, const uint32_t *__restrict__ bin_base, const uint32_t *__restrict__ ref_len, int32_t n_ref, uint64_t bin_width,
                                                    uint32_t b0, uint32_t nb, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ rank, uint32_t r0, uint32_t nrows, BinCols o) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= nb || !keep[k]) return;
    const uint32_t r = rank[k] - r0;
    if (rank[k] < r0 || r >= nrows) return;
    const uint32_t b = b0 + k;
    const int32_t t = bin_contig(bin_base, n_ref, b);
    const uint64_t id = b - bin_base[t], start = id * bin_width, len = ref_len[t];
    const uint64_t fwd = counts[2ull * b], rev = counts[2ull * b + 1];
    o.chrom[r] = t; o.start[r] = (long long)start; o.end[r] = (long long)(len - start < bin_width ? len : start + bin_width); o.bin_id[r] = (long long)id;
    o.total[r] = (long long)(fwd + rev); o.fwd[r] = (long long)fwd; o.rev[r] = (long long)rev;
}
