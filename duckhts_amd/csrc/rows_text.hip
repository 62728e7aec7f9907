// rows_text.hip -- typed device columns -> text rows in a device buffer: `name \t c0 \t c1 ... \n` per row, the name looked up by a 32-bit id in a
// table of names (one byte arena plus offsets), the K <= 8 integer columns of 4 or 8 bytes each printed in decimal without padding ('-' in
// front of a negative value).  bam_bedgraph_export is its first front end (K = 3: start, end, depth; dhts_bam_bedgraph_export.inc); the
// encoder itself knows nothing about bedGraph.
//
//   lengths      one lane per row: the name's length + the digits (and signs) of its K values + K + 1, as a 64-bit word per row
//   offsets      the exclusive sum of the lengths in place, the total behind the last: dev_scan.hip's carry_* through depth_carry
//   write        a workgroup of 256 threads owns 256 consecutive rows, whose text is one contiguous span of the output.
//                staged    the span fits RTX_LDS_BYTES: every lane prints its row into LDS at the place it has in the span (the image is shifted
//                          by the span's misalignment, so that byte x of the image is byte A0 + x of the output, A0 = the span's start rounded
//                          down to 16), and behind a barrier the workgroup stores the image in aligned 16-byte pieces, lane after lane; the
//                          pieces the span covers only in part (its ragged head and tail, at most 15 bytes each) leave as single bytes.
//                fallback  the span does not fit (names of hundreds of bytes): 64 rows a turn, a lane each prints the numeric tail of its row
//                          into LDS, then the workgroup copies row after row -- the name from the arena, the tail from LDS -- consecutive
//                          lanes storing consecutive bytes.  Slower, and never taken by the names of a real header.
//                A row whose id is outside the table has an empty name.  which[0] / which[1] count the workgroups of either path when the
//                caller asks for it (the tests do; the export passes null: 42,000 adds to one word per million rows are not free).
//                lane      rtx_write_lane, the form the staged one is measured against (dhts_debug_rows_text_form, tools/bench_bedgraph_export.py): one
//                          lane per row stores its row byte by byte.  Not the product path.
// Nothing is written outside [dst, dst + total); the host sizes the buffer from the total before the write pass is launched.
#pragma once
#include "dev_scan.hip"

#define RTX_MAX_COLS 8u
#define RTX_LDS_BYTES 16384u                                       /* the longest span of 256 rows the staged path takes */
#define RTX_TAIL_MAX (RTX_MAX_COLS * 21u + 1u)                     /* K x (tab, sign, 19 digits) + newline */
#define RTX_FALLBACK_ROWS 64u                                      /* rows a turn of the fallback (their tails fit the staging area) */

struct RtxCols {
    const uint8_t *names; const uint32_t *name_off; uint32_t n_names, k;          // the table; the number of integer columns
    const int32_t *name_id;                                                         // per row
    const void *col[RTX_MAX_COLS]; uint32_t width[RTX_MAX_COLS];                   // per column: its values and 4 or 8
    unsigned long long n;                                                            // rows
};

__device__ const unsigned long long RTX_POW10[20] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull, 1000000000ull,
                                                     10000000000ull, 100000000000ull, 1000000000000ull, 10000000000000ull, 100000000000000ull, 1000000000000000ull,
                                                     10000000000000000ull, 100000000000000000ull, 1000000000000000000ull, 10000000000000000000ull};
// decimal digits of v (1 for 0): the bit length gives the count within one, a compare settles it
__device__ __forceinline__ uint32_t rtx_ndigits(unsigned long long v) {
    const uint32_t t = ((64u - (uint32_t)__clzll((long long)(v | 1ull))) * 1233u) >> 12;
    const uint32_t n = t + (v >= RTX_POW10[t] ? 1u : 0u);
    return n ? n : 1u;
}
__device__ __forceinline__ long long rtx_value(const RtxCols &a, uint32_t j, unsigned long long row) {
    return a.width[j] == 8u ? ((const long long *)a.col[j])[row] : (long long)((const int32_t *)a.col[j])[row];
}
__device__ __forceinline__ uint32_t rtx_name_len(const RtxCols &a, unsigned long long row, uint32_t &off) {
    const int32_t id = a.name_id[row];
    if (id < 0 || (uint32_t)id >= a.n_names) { off = 0; return 0; }
    off = a.name_off[id];
    return a.name_off[id + 1] - off;
}
// the bytes behind the name: K x (tab, value), newline
__device__ __forceinline__ uint32_t rtx_tail_len(const RtxCols &a, unsigned long long row) {
    uint32_t len = a.k + 1u;
    for (uint32_t j = 0; j < a.k; j++) {
        const long long v = rtx_value(a, j, row);
        len += rtx_ndigits(v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v) + (v < 0 ? 1u : 0u);
    }
    return len;
}
// prints the tail at p (LDS); returns the byte behind it.  Digits are written from the last to the first; 32-bit arithmetic once the value fits
__device__ __forceinline__ uint8_t *rtx_put_tail(const RtxCols &a, unsigned long long row, uint8_t *p) {
    for (uint32_t j = 0; j < a.k; j++) {
        const long long v = rtx_value(a, j, row);
        unsigned long long m = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
        *p++ = '\t';
        if (v < 0) *p++ = '-';
        const uint32_t nd = rtx_ndigits(m);
        uint8_t *q = p + nd;
        while (m >> 32) { const unsigned long long d = m / 10ull; *--q = (uint8_t)('0' + (uint32_t)(m - d * 10ull)); m = d; }
        uint32_t w = (uint32_t)m;
        do { const uint32_t d = w / 10u; *--q = (uint8_t)('0' + (w - d * 10u)); w = d; } while (q > p);
        p += nd;
    }
    *p++ = '\n';
    return p;
}

__global__ void __launch_bounds__(256) rtx_lengths(RtxCols a, unsigned long long *__restrict__ off) {
    const unsigned long long row = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (row >= a.n) return;
    uint32_t no;
    off[row] = (unsigned long long)rtx_name_len(a, row, no) + rtx_tail_len(a, row);
}

// off: the exclusive offsets of the rows, off[n] the total.  dst: where byte 0 of the text goes (any alignment)
__global__ void __launch_bounds__(256) rtx_write(RtxCols a, const unsigned long long *__restrict__ off, uint8_t *__restrict__ dst, unsigned long long *__restrict__ which) {
    __shared__ __attribute__((aligned(16))) uint8_t img[RTX_LDS_BYTES + 32u];
    const unsigned long long r0 = (unsigned long long)blockIdx.x * 256u, r1 = r0 + 256u < a.n ? r0 + 256u : a.n;     // (the grid covers the rows: r0 < n)
    const unsigned long long g0 = off[r0], g1 = off[r1];
    const unsigned long long row = r0 + threadIdx.x;
    if (g1 - g0 <= RTX_LDS_BYTES) {
        uint8_t *const A = dst + g0, *const B = dst + g1;
        const uint32_t head = (uint32_t)((uintptr_t)A & 15u);
        if (row < r1) {
            uint32_t no; const uint32_t nl = rtx_name_len(a, row, no);
            uint8_t *p = img + head + (uint32_t)(off[row] - g0);
            for (uint32_t i = 0; i < nl; i++) p[i] = a.names[no + i];
            rtx_put_tail(a, row, p + nl);
        }
        __syncthreads();
        uint8_t *const A0 = A - head;
        const uint32_t npieces = (head + (uint32_t)(g1 - g0) + 15u) / 16u;
        for (uint32_t q = threadIdx.x; q < npieces; q += 256u) {
            uint8_t *const G = A0 + 16u * q;
            if (G >= A && G + 16 <= B) *(uint4 *)G = *(const uint4 *)(img + 16u * q);
            else for (uint32_t i = 0; i < 16u; i++) if (G + i >= A && G + i < B) G[i] = img[16u * q + i];
        }
        if (which && threadIdx.x == 0) atomicAdd(which, 1ull);
        return;
    }
    // the fallback: img holds the tails of 64 rows a turn, RTX_TAIL_MAX bytes apart (64 x 169 < RTX_LDS_BYTES)
    for (unsigned long long b0 = r0; b0 < r1; b0 += RTX_FALLBACK_ROWS) {
        const unsigned long long b1 = b0 + RTX_FALLBACK_ROWS < r1 ? b0 + RTX_FALLBACK_ROWS : r1;
        if (threadIdx.x < (uint32_t)(b1 - b0)) rtx_put_tail(a, b0 + threadIdx.x, img + threadIdx.x * RTX_TAIL_MAX);
        __syncthreads();
        for (unsigned long long r = b0; r < b1; r++) {
            uint32_t no; const uint32_t nl = rtx_name_len(a, r, no);
            const uint32_t len = (uint32_t)(off[r + 1] - off[r]);
            uint8_t *const o = dst + off[r]; const uint8_t *const t = img + (uint32_t)(r - b0) * RTX_TAIL_MAX;
            for (uint32_t i = threadIdx.x; i < len; i += 256u) o[i] = i < nl ? a.names[no + i] : t[i - nl];
        }
        __syncthreads();
    }
    if (which && threadIdx.x == 0) atomicAdd(which + 1, 1ull);
}

// the measuring stick of rtx_write: one lane per row, every byte a store of its own
__global__ void __launch_bounds__(256) rtx_write_lane(RtxCols a, const unsigned long long *__restrict__ off, uint8_t *__restrict__ dst) {
    const unsigned long long row = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (row >= a.n) return;
    uint32_t no; const uint32_t nl = rtx_name_len(a, row, no);
    uint8_t *p = dst + off[row];
    for (uint32_t i = 0; i < nl; i++) p[i] = a.names[no + i];
    rtx_put_tail(a, row, p + nl);
}
