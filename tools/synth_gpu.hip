// synth_gpu.hip -- the synthetic BAM workload generated on the device, byte for byte the file synth_bam.c writes.
//
// Workload tooling, not part of the scan path: bench.py makes its 10 GB input with it instead of spending a minute of host zlib.
// Segments k0 .. k0+nseg-1 (records [k * n_u, (k+1) * n_u) of a total_n-record file, no header, no EOF block) are produced in groups:
//   1. one thread per record sizes it (synth_bam_model.h gen_record into a private buffer); an exclusive scan gives the offsets;
//   2. one thread per record writes it at its offset: the segment's inflated record stream;
//   3. every 65,280-byte cut is deflated as zlib 1.2.11 level 6 does, in the three phases of zlib6_deflate.h: one thread per cut
//      builds its hash chains, one thread per position runs longest_match for both chain budgets, one thread per cut parses and
//      writes the BGZF block (the header, BSIZE, CRC-32, ISIZE of synth_bam.c bgzf_block); a cut that zlib would not fit in the
//      block comes back with size 0 and is stored on the host with zlib level 0, as bgzf_block does;
//   4. the blocks are packed to their file offsets and copied to the caller's buffer.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <zlib.h>

#pragma clang force_cuda_host_device begin
#include "synth_bam_model.h"
#pragma clang force_cuda_host_device end
#include "zlib6_deflate.h"

#define SG_PAYLOAD 65280u
#define SG_SLOT 65536u
#define SG_REC_CAP 420u
#define SG_MATCH_CHUNK (1ull << 30)          /* positions per sg_match launch */

static char g_err[256];
#define SG_FREE() do { (void)hipFree(d_head); (void)hipFree(d_prev); (void)hipFree(d_m128); (void)hipFree(d_m32); (void)hipFree(d_sz); (void)hipFree(d_off); (void)hipFree(d_raw); (void)hipFree(d_ws); (void)hipFree(d_slots); (void)hipFree(d_bsz); \
                        (void)hipFree(d_boff); (void)hipFree(d_packed); (void)hipFree(d_meta); (void)hipFree(d_tmp); \
                        free(h_meta); free(h_bsz); free(h_boff); free(h_cut); } while (0)
#define SG_CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { snprintf(g_err, sizeof g_err, "%s: %s", #x, hipGetErrorString(e_)); goto fail; } } while (0)

__global__ void sg_sizes(model_t m, uint64_t rec0, uint64_t n, uint64_t *sz) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint8_t tmp[SG_REC_CAP];
    sz[i] = gen_record(&m, rec0 + i, tmp);
}

__global__ void sg_write(model_t m, uint64_t rec0, uint64_t n, const uint64_t *off, uint8_t *raw) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint8_t tmp[SG_REC_CAP];
    size_t l = gen_record(&m, rec0 + i, tmp);
    uint8_t *d = raw + off[i];
    for (size_t k = 0; k < l; k++) d[k] = tmp[k];
}

__constant__ uint32_t c_crc[256];

// the cut of block b: segment s (seg_blk0[s] = its first block, seg_raw0[s] / seg_rawlen[s] its record stream) -> raw offset, length
__device__ __forceinline__ uint64_t sg_cut(uint64_t b, int nseg, const uint64_t *seg_blk0, const uint64_t *seg_raw0, const uint64_t *seg_rawlen, uint32_t *n) {
    int s = 0;
    while (s + 1 < nseg && b >= seg_blk0[s + 1]) s++;
    const uint64_t beg = (b - seg_blk0[s]) * SG_PAYLOAD;
    const uint64_t len = seg_rawlen[s] - beg;
    *n = (uint32_t)(len < SG_PAYLOAD ? len : SG_PAYLOAD);
    return seg_raw0[s] + beg;
}

// phase 1, one thread per cut: prev[] at the cut's raw offsets; head = 32,768 entries per thread
__global__ void __launch_bounds__(64) sg_chain(const uint8_t *raw, int nseg, const uint64_t *seg_blk0, const uint64_t *seg_raw0, const uint64_t *seg_rawlen,
                                               uint64_t nblk, uint16_t *head, uint16_t *prev) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nblk) return;
    uint32_t n;
    const uint64_t o = sg_cut(b, nseg, seg_blk0, seg_raw0, seg_rawlen, &n);
    zd_chain(head + b * 32768u, raw + o, n, prev + o);
}

// phase 2, one thread per raw position r0 + i of the group (lookahead >= 16 in its cut); launched in chunks, as a dispatch covers
// fewer than 2^32 work-items
__global__ void sg_match(const uint8_t *raw, int nseg, const uint64_t *seg_raw0, const uint64_t *seg_rawlen, uint64_t r0, uint64_t raw_len,
                         const uint16_t *prev, uint32_t *m128, uint32_t *m32) {
    const uint64_t r = r0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= raw_len) return;
    int s = 0;
    while (s + 1 < nseg && r >= seg_raw0[s + 1]) s++;
    const uint64_t q = r - seg_raw0[s], o = seg_raw0[s] + q / SG_PAYLOAD * SG_PAYLOAD, len = seg_rawlen[s] - (o - seg_raw0[s]);
    const uint32_t n = (uint32_t)(len < SG_PAYLOAD ? len : SG_PAYLOAD), p = (uint32_t)(r - o);
    if (p + 16 > n) return;
    zd_match_pair(raw + o, n, prev + o, p, m128 + r, m32 + r);
}

// phase 3, one thread per cut: the parse, the blocks, the BGZF wrapping
__global__ void __launch_bounds__(64) sg_parse(const uint8_t *raw, int nseg, const uint64_t *seg_blk0, const uint64_t *seg_raw0, const uint64_t *seg_rawlen,
                                               uint64_t nblk, const uint16_t *prev, const uint32_t *m128, const uint32_t *m32, zd_ws *ws,
                                               uint8_t *slots, uint32_t *sizes) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nblk) return;
    uint32_t n;
    const uint64_t o = sg_cut(b, nseg, seg_blk0, seg_raw0, seg_rawlen, &n);
    const uint8_t *src = raw + o;
    uint8_t *dst = slots + b * SG_SLOT;
    const uint32_t clen = zd_parse(ws + b, src, n, prev + o, m128 + o, m32 + o, dst + 18);
    if (clen == 0) { sizes[b] = 0; return; }
    const uint8_t hdr[16] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0};
    for (int k = 0; k < 16; k++) dst[k] = hdr[k];
    const uint32_t total = 18 + clen + 8;
    dst[16] = (uint8_t)((total - 1) & 0xff); dst[17] = (uint8_t)((total - 1) >> 8);
    uint32_t crc = 0xffffffffu;
    for (uint32_t k = 0; k < n; k++) crc = c_crc[(crc ^ src[k]) & 0xff] ^ (crc >> 8);
    crc ^= 0xffffffffu;
    put32(dst + 18 + clen, crc); put32(dst + 18 + clen + 4, n);
    sizes[b] = total;
}

// one workgroup per block: copy slot b to its packed offset
__global__ void sg_pack(const uint8_t *slots, const uint32_t *sizes, const uint64_t *off, uint8_t *out) {
    uint64_t b = blockIdx.x;
    uint32_t n = sizes[b];
    const uint8_t *s = slots + b * SG_SLOT;
    uint8_t *d = out + off[b];
    for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) d[k] = s[k];
}

// bgzf_block of synth_bam.c for a cut that level 6 cannot fit: the same zlib calls on the host
static size_t stored_block(const uint8_t *src, size_t slen, uint8_t *dst) {
    static const uint8_t HDR[16] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0};
    z_stream zs; memset(&zs, 0, sizeof(zs));
    deflateInit2(&zs, 0, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
    zs.next_in = (Bytef *)src; zs.avail_in = (uInt)slen; zs.next_out = dst + 18; zs.avail_out = 65536 - 18 - 8;
    deflate(&zs, Z_FINISH);
    size_t clen = zs.total_out;
    deflateEnd(&zs);
    memcpy(dst, HDR, 16);
    size_t total = 18 + clen + 8;
    dst[16] = (uint8_t)((total - 1) & 0xff); dst[17] = (uint8_t)((total - 1) >> 8);
    uint32_t crc = (uint32_t)crc32(crc32(0L, NULL, 0), src, (uInt)slen);
    put32(dst + 18 + clen, crc); put32(dst + 18 + clen + 4, (uint32_t)slen);
    return total;
}

extern "C" const char *synth_gpu_error(void) { return g_err; }

// Segments k0 .. k0+nseg-1 of n_u records each of a total_n-record file -> out (concatenated, file order), seg_sizes[k - k0] = bytes
// of segment k, *raw_bytes = their inflated bytes.  group = segments per device pass.  Returns bytes written, or -1 (synth_gpu_error).
extern "C" int64_t synth_gpu_bam_segments(int device, uint64_t seed, uint64_t total_n, uint64_t n_u, uint64_t k0, int nseg, int group,
                                          uint8_t *out, uint64_t out_cap, uint64_t *seg_sizes, uint64_t *raw_bytes) {
    model_t m; model_init(&m, total_n, seed);
    uint64_t written = 0, raw_total = 0;
    uint64_t *d_sz = NULL, *d_off = NULL, *d_meta = NULL, *d_boff = NULL, *h_meta = NULL, *h_boff = NULL;
    uint16_t *d_head = NULL, *d_prev = NULL;
    uint32_t *d_m128 = NULL, *d_m32 = NULL;
    uint8_t *d_raw = NULL, *d_slots = NULL, *d_packed = NULL, *d_tmp = NULL, *h_cut = NULL;
    uint32_t *d_bsz = NULL, *h_bsz = NULL;
    zd_ws *d_ws = NULL;
    size_t tmp_bytes = 0;
    g_err[0] = 0;
    if (group < 1) group = 1;
    if (group > nseg) group = nseg;
    if ((unsigned __int128)total_n * m.genome >> 64) { snprintf(g_err, sizeof g_err, "total_n too large for the device generator"); return -1; }
    {
        const uint64_t recs = n_u * (uint64_t)group, raw_cap = recs * SG_REC_CAP, blk_cap = raw_cap / SG_PAYLOAD + (uint64_t)group + 1;
        uint32_t tab[256];
        for (uint32_t i = 0; i < 256; i++) { uint32_t c = i; for (int k = 0; k < 8; k++) c = c & 1 ? 0xedb88320u ^ (c >> 1) : c >> 1; tab[i] = c; }
        SG_CHK(hipSetDevice(device));
        SG_CHK(hipMemcpyToSymbol(HIP_SYMBOL(c_crc), tab, sizeof tab));
        SG_CHK(hipMalloc(&d_sz, (recs + 1) * 8));
        SG_CHK(hipMalloc(&d_off, (recs + 1) * 8));
        SG_CHK(hipMalloc(&d_raw, raw_cap));
        SG_CHK(hipMalloc(&d_ws, blk_cap * sizeof(zd_ws)));
        SG_CHK(hipMalloc(&d_head, blk_cap * 32768 * sizeof(uint16_t)));
        SG_CHK(hipMalloc(&d_prev, raw_cap * sizeof(uint16_t)));
        SG_CHK(hipMalloc(&d_m128, raw_cap * sizeof(uint32_t)));
        SG_CHK(hipMalloc(&d_m32, raw_cap * sizeof(uint32_t)));
        SG_CHK(hipMalloc(&d_slots, blk_cap * SG_SLOT));
        SG_CHK(hipMalloc(&d_bsz, blk_cap * 4));
        SG_CHK(hipMalloc(&d_boff, blk_cap * 8));
        SG_CHK(hipMalloc(&d_packed, blk_cap * SG_SLOT));
        SG_CHK(hipMalloc(&d_meta, 3 * (size_t)group * 8));
        SG_CHK(hipcub::DeviceScan::ExclusiveSum(NULL, tmp_bytes, d_sz, d_off, (int)(recs + 1)));
        SG_CHK(hipMalloc(&d_tmp, tmp_bytes));
        h_meta = (uint64_t *)malloc(3 * (size_t)group * 8 + 8);
        h_bsz = (uint32_t *)malloc(blk_cap * 4);
        h_boff = (uint64_t *)malloc(blk_cap * 8 + 8);
        h_cut = (uint8_t *)malloc(SG_PAYLOAD);
        if (!h_meta || !h_bsz || !h_boff || !h_cut) { snprintf(g_err, sizeof g_err, "host allocation failed"); goto fail; }
        for (int g0 = 0; g0 < nseg; g0 += group) {
            const int ng = nseg - g0 < group ? nseg - g0 : group;
            const uint64_t n = n_u * (uint64_t)ng, rec0 = (k0 + (uint64_t)g0) * n_u;
            const unsigned tpb = 256;
            sg_sizes<<<(unsigned)((n + tpb - 1) / tpb), tpb>>>(m, rec0, n, d_sz);
            SG_CHK(hipGetLastError());
            SG_CHK(hipMemset(d_sz + n, 0, 8));
            SG_CHK(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp_bytes, d_sz, d_off, (int)(n + 1)));
            sg_write<<<(unsigned)((n + tpb - 1) / tpb), tpb>>>(m, rec0, n, d_off, d_raw);
            SG_CHK(hipGetLastError());
            // segment boundaries in the record stream and in blocks
            uint64_t *blk0 = h_meta, *raw0 = h_meta + group, *rawlen = h_meta + 2 * group, nblk = 0;
            for (int s = 0; s < ng; s++) {
                uint64_t a, e;
                SG_CHK(hipMemcpy(&a, d_off + (uint64_t)s * n_u, 8, hipMemcpyDeviceToHost));
                SG_CHK(hipMemcpy(&e, d_off + (uint64_t)(s + 1) * n_u, 8, hipMemcpyDeviceToHost));
                raw0[s] = a; rawlen[s] = e - a; blk0[s] = nblk;
                nblk += (e - a + SG_PAYLOAD - 1) / SG_PAYLOAD;
                raw_total += e - a;
            }
            if (nblk > blk_cap) { snprintf(g_err, sizeof g_err, "block capacity exceeded"); goto fail; }
            SG_CHK(hipMemcpy(d_meta, h_meta, 3 * (size_t)group * 8, hipMemcpyHostToDevice));
            const uint64_t raw_len = raw0[ng - 1] + rawlen[ng - 1];
            sg_chain<<<(unsigned)((nblk + 63) / 64), 64>>>(d_raw, ng, d_meta, d_meta + group, d_meta + 2 * group, nblk, d_head, d_prev);
            SG_CHK(hipGetLastError());
            for (uint64_t r0 = 0; r0 < raw_len; r0 += SG_MATCH_CHUNK) {
                const uint64_t m = raw_len - r0 < SG_MATCH_CHUNK ? raw_len - r0 : SG_MATCH_CHUNK;
                sg_match<<<(unsigned)((m + 255) / 256), 256>>>(d_raw, ng, d_meta + group, d_meta + 2 * group, r0, raw_len, d_prev, d_m128, d_m32);
                SG_CHK(hipGetLastError());
            }
            sg_parse<<<(unsigned)((nblk + 63) / 64), 64>>>(d_raw, ng, d_meta, d_meta + group, d_meta + 2 * group, nblk, d_prev, d_m128, d_m32, d_ws, d_slots, d_bsz);
            SG_CHK(hipGetLastError());
            SG_CHK(hipMemcpy(h_bsz, d_bsz, nblk * 4, hipMemcpyDeviceToHost));
            // cuts level 6 could not fit: stored on the host, as bgzf_block does
            for (uint64_t b = 0; b < nblk; b++) {
                if (h_bsz[b]) continue;
                int s = 0;
                while (s + 1 < ng && b >= blk0[s + 1]) s++;
                uint64_t beg = (b - blk0[s]) * SG_PAYLOAD, len = rawlen[s] - beg < SG_PAYLOAD ? rawlen[s] - beg : SG_PAYLOAD;
                uint8_t slot[SG_SLOT];
                SG_CHK(hipMemcpy(h_cut, d_raw + raw0[s] + beg, len, hipMemcpyDeviceToHost));
                h_bsz[b] = (uint32_t)stored_block(h_cut, len, slot);
                SG_CHK(hipMemcpy(d_slots + b * SG_SLOT, slot, h_bsz[b], hipMemcpyHostToDevice));
                SG_CHK(hipMemcpy(d_bsz + b, &h_bsz[b], 4, hipMemcpyHostToDevice));
            }
            uint64_t o = 0;
            for (uint64_t b = 0; b < nblk; b++) { h_boff[b] = o; o += h_bsz[b]; }
            for (int s = 0; s < ng; s++) {
                uint64_t e = s + 1 < ng ? h_boff[blk0[s + 1]] : o;
                seg_sizes[g0 + s] = e - h_boff[blk0[s]];
            }
            if (written + o > out_cap) { snprintf(g_err, sizeof g_err, "output capacity too small"); goto fail; }
            SG_CHK(hipMemcpy(d_boff, h_boff, nblk * 8, hipMemcpyHostToDevice));
            sg_pack<<<(unsigned)nblk, 256>>>(d_slots, d_bsz, d_boff, d_packed);
            SG_CHK(hipGetLastError());
            SG_CHK(hipMemcpy(out + written, d_packed, o, hipMemcpyDeviceToHost));
            written += o;
        }
    }
    if (raw_bytes) *raw_bytes = raw_total;
    SG_FREE();
    return (int64_t)written;
fail:
    SG_FREE();
    return -1;
}
