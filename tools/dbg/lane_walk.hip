// micro-benchmark: one LANE per 8 KiB tile walks a BAM record chain straight from HBM (tools only; needs nothing from the library).
// The question it answers: how long do ~25 dependent, unaligned 4-byte loads per lane take when the 64 lanes of a wave instruction hit 64
// different tiles and every tile of a 1.6 GB batch is in flight at once (3,072 waves)?  That chain is the floor of a lane-per-tile form of
// bam_tile_scan; compare the per-launch time with bam_tile_scan's in a kernel trace of the bench taken in the same session.
//   hipcc --offload-arch=gfx950 -O3 -o lane_walk tools/dbg/lane_walk.hip && ./lane_walk
// The buffer holds back-to-back records of 323 +- 40 bytes of which only the leading block_size word is valid (the rest is zero).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <cstdlib>
#include <vector>
#define TL_TILE 8192u
#define TL_RECS (TL_TILE / 32u)
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

__device__ __forceinline__ uint32_t ldu32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }

// LIST: also store the record starts (u16, relative to the tile) as bam_tile_scan does for bam_tile_unpack
template <bool LIST>
__global__ void __launch_bounds__(64) lane_walk(const uint8_t *u, uint64_t ulen, int64_t ntiles, const uint16_t *start, uint32_t *count, uint64_t *end_next, uint16_t *recs) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= ntiles) return;
    const uint64_t tb = (uint64_t)t * TL_TILE;
    if (tb >= ulen) return;
    const uint64_t left64 = ulen - tb;
    const uint32_t left = left64 > 0xffffffffull ? 0xffffffffu : (uint32_t)left64;
    const uint32_t lim = left < TL_TILE ? left : TL_TILE;
    uint32_t rel = start[t], cnt = 0;
    while (rel < lim) {
        if (left - rel < 4u) break;                                   // fewer than four bytes left: incomplete
        const int32_t b = (int32_t)ldu32(u + tb + rel);               // (tb + rel + 4 <= ulen)
        if (b < 32) break;
        if (left - rel - 4u < (uint32_t)b) break;                     // the record runs past the stream: incomplete
        if (LIST && cnt < TL_RECS) recs[(size_t)t * TL_RECS + cnt] = (uint16_t)rel;
        cnt++; rel += 4u + (uint32_t)b;
    }
    count[t] = cnt; end_next[t] = tb + rel;
}

int main(int argc, char **argv) {
    const int64_t nt = argc > 1 ? atoll(argv[1]) : 3072 * 64;         // 196,608 tiles = 1.61 GB
    const uint64_t ulen = (uint64_t)nt * TL_TILE;
    std::vector<uint8_t> h(ulen + 4096, 0);
    std::vector<uint16_t> hstart(nt, 0xffff);
    std::vector<uint32_t> hcount(nt, 0);
    uint64_t o = 0, nrec = 0, seed = 0x9e3779b97f4a7c15ull;
    while (o + 4 <= ulen) {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        const uint32_t total = 283u + (uint32_t)((seed >> 33) % 81u), b = total - 4u;      // 323 +- 40 bytes with the length word
        memcpy(&h[o], &b, 4);
        const uint64_t t = o / TL_TILE;
        if (hstart[t] == 0xffff) hstart[t] = (uint16_t)(o - t * TL_TILE);
        if (o + total <= ulen) { hcount[t]++; nrec++; }                // the walk stops at a record that runs past the stream
        o += total;
    }
    for (int64_t t = 0; t < nt; t++) if (hstart[t] == 0xffff) hstart[t] = (uint16_t)(TL_TILE - 1);   // (cannot happen at these record sizes)
    uint8_t *u; uint16_t *start, *recs; uint32_t *count; uint64_t *en;
    CK(hipMalloc(&u, ulen + 4096)); CK(hipMalloc(&start, nt * 2)); CK(hipMalloc(&count, nt * 4)); CK(hipMalloc(&en, nt * 8)); CK(hipMalloc(&recs, (size_t)nt * TL_RECS * 2));
    CK(hipMemcpy(u, h.data(), ulen + 4096, hipMemcpyHostToDevice)); CK(hipMemcpy(start, hstart.data(), nt * 2, hipMemcpyHostToDevice));
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    const dim3 grid((unsigned)((nt + 63) / 64)), block(64);
    printf("%lld tiles (%.3f GB), %llu records, %u waves\n", (long long)nt, ulen / 1e9, (unsigned long long)nrec, grid.x);
    for (int list = 0; list < 2; list++) {
        CK(hipMemset(count, 0, nt * 4));
        float sum = 0, mn = 1e9f, mx = 0;
        for (int rep = 0; rep < 22; rep++) {                              // two warm-up launches, then 20 timed
            CK(hipEventRecord(a));
            if (list) hipLaunchKernelGGL(lane_walk<true>, grid, block, 0, 0, u, ulen, nt, start, count, en, recs);
            else hipLaunchKernelGGL(lane_walk<false>, grid, block, 0, 0, u, ulen, nt, start, count, en, recs);
            CK(hipEventRecord(b)); CK(hipEventSynchronize(b)); CK(hipGetLastError());
            float ms; CK(hipEventElapsedTime(&ms, a, b));
            if (rep >= 2) { sum += ms; mn = ms < mn ? ms : mn; mx = ms > mx ? ms : mx; }
        }
        std::vector<uint32_t> got(nt);
        CK(hipMemcpy(got.data(), count, nt * 4, hipMemcpyDeviceToHost));
        int64_t bad = 0; for (int64_t t = 0; t < nt; t++) bad += got[t] != hcount[t];
        printf("lane_walk%s  20 launches: avg %.4f ms  min %.4f  max %.4f   (%lld of %lld tile counts differ from the host walk)\n",
               list ? " + record list" : "              ", sum / 20, mn, mx, (long long)bad, (long long)nt);
        if (bad) return 2;
    }
    return 0;
}
