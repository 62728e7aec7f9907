// bam_pileup.hip -- bam_pileup: per position and strand the number of A C G T N = - + that lie on it (an Rsamtools-style pileup), counted into
// a table in HBM and emitted page by page as the compaction of that table.  The contract is in include/duckhts_amd.h; the host side in
// dhts_bam_pileup.inc.  The target rows, the tiles of positions, classify and the step counters are bam_coverage's (bam_coverage.hip), the
// carry in two levels and the page's tiles bam_depth's (bam_depth.hip).
//
//   table        uint32, S = 8 (no strands) or 16 words per position slot of the layout: word (rbase[k] + x - beg) * S + strand * 8 + symbol.
//                In this order the result IS the table's words >= min_nucleotide_depth in address order: row, position, strand, symbol.
//   add          dep_add_body's shape: classified once (bam_depth_classify_del: every read with an M = X or D operation is walked), eight
//                lanes per read, every lane walks the CIGAR.  Of an M = X operation lane j takes the 16-base pieces j, j + 8, ... on QUAL's
//                16-byte grid: QUAL (only with min_baseq) as one aligned 16-byte load with masked ends, SEQ as the up to 9 bytes that hold the
//                same 16 bases, loaded as aligned words that hold a wanted byte and funnel-shifted to the piece's first nibble.  The eight
//                lanes share a D's positions; the first lane sets the I anchors.  A workgroup takes a contiguous run of reads, so on a
//                sorted file its counts stay on neighbouring positions.  Two forms behind the same walk: direct, one return-less atomicAdd
//                per counted base into the table; window, the counts of PIL_WINDOW positions of one row kept in LDS and added to the table
//                as consecutive non-zero words when the window moves, everything outside it direct (at bam_pileup_add)
//   count        per tile of PIL_TILE words the words >= min_nucleotide_depth that lie inside the row (not in the padding)
//   emit         dep_emit's shape on a window of result indices: a tile's emitting words are compacted in LDS by a block scan and the 256
//                threads write rows j, j + 256, ... of the tile's share of the window, only the projected columns, with plain vector stores.
//                The table holds counts, not differences: no depth is carried.
#pragma once
#include "bam_depth.hip"

#define PIL_SYMBOLS 8u                                                      /* A C G T N = - + */
#define PIL_SYM_N 4u
#define PIL_SYM_DEL 6u
#define PIL_SYM_INS 7u
#define PIL_TILE 1024u                                                      /* words per tile of the result pass */
// the symbol of a 4-bit base code, four bits each: 1 2 4 8 -> A C G T, 0 -> '=', every other code -> N
#define PIL_CODE_SYM 0x4444444344424105ull

// The 16 bases whose first has query index qc0 (which may be odd, or negative for a piece that starts in front of the read), as 16 nibbles
// with base i in bits 60 - 4 i.  sbase: SEQ's first byte as an offset from ub (16-byte aligned).  need: bit i = base i is wanted (not 0); only
// aligned words that hold a byte of a wanted base are loaded, so nothing is read behind the record but the rest of such a word.
__device__ __forceinline__ uint64_t pil_seq16(const uint8_t *__restrict__ ub, long long sbase, long long qc0, uint32_t need) {
    const long long nib0 = 2 * sbase + qc0, byte0 = nib0 >> 1;               // (sbase >= 36: never negative)
    const uint32_t par = (uint32_t)(nib0 & 1), m = (uint32_t)(byte0 & 3);
    const uint32_t lo = (uint32_t)__ffs((int)need) - 1u, hi = 32u - (uint32_t)__clz((int)need);         // the wanted bases lie in [lo, hi)
    const int32_t fb = (int32_t)((par + lo) >> 1), lb = (int32_t)((par + hi - 1u) >> 1);                // ... in bytes [fb, lb] behind byte0
    const uint8_t *aw = ub + (byte0 - (long long)m);
    uint32_t w[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {                                            // word k holds bytes 4 k - m .. 4 k - m + 3 (9 bytes + m <= 12)
        const int32_t b0 = 4 * k - (int32_t)m;
        w[k] = (b0 <= lb && b0 + 3 >= fb) ? *(const uint32_t *)(aw + 4 * k) : 0u;
    }
    const uint32_t b0 = __builtin_amdgcn_alignbyte(w[1], w[0], m), b1 = __builtin_amdgcn_alignbyte(w[2], w[1], m), b2 = (w[2] >> (8u * m)) & 255u;
    const uint64_t v = ((uint64_t)__builtin_bswap32(b0) << 32) | (uint64_t)__builtin_bswap32(b1);      // byte0 on top: base i of an even start in bits 60 - 4 i
    return par ? (v << 4) | (uint64_t)(b2 >> 4) : v;
}

// One read against one row [beg, end), as seen by lane `sub` of the read's eight.  put(slot, symbol): slot = the position's index in the row.
// qoff / soff: QUAL's and SEQ's first byte as offsets from ub + mis; lseq: the bases the record holds (clamped: neither is read behind it).
template <bool BQ, bool DEL, bool INS, typename Put>
__device__ __forceinline__ void pil_walk_row(const uint8_t *__restrict__ ub, uint32_t mis, uint64_t qoff, uint64_t soff, long long lseq, uint32_t min_baseq,
                                             const uint8_t *__restrict__ cig, uint32_t ne, long long p0, long long beg, long long end, uint32_t sub, Put put) {
    const long long qbase = (long long)(mis + qoff), sbase = (long long)(mis + soff);
    long long x = p0, q = 0; bool anchored = false;                          // anchored: the last operation that consumed reference was M = X or D
    for (uint32_t j = 0; j < ne; j++) {
        const uint32_t op = cov_ldu32(cig + 4ull * j), code = op & 15u; const long long len = (long long)(op >> 4);
        if (len == 0) continue;
        if ((DEP_M_OPS >> code) & 1u) {
            const long long jlo = beg > x ? beg - x : 0, jhi = end - x < len ? end - x : len;       // the operation's bases inside the row
            if (jhi > jlo) {
                const long long qlo = q + jlo, qhi = q + jhi;
                const long long c_last = (qbase + qhi - 1) >> 4;
                for (long long c = ((qbase + qlo) >> 4) + sub; c <= c_last; c += DEP_LANES) {
                    const long long qc0 = (c << 4) - qbase;                  // the query index of the piece's base 0
                    const uint32_t lo_i = qlo > qc0 ? (uint32_t)(qlo - qc0) : 0u, hi_i = qhi - qc0 < 16 ? (uint32_t)(qhi - qc0) : 16u;
                    const uint32_t valid = ((1u << hi_i) - 1u) & ~((1u << lo_i) - 1u);
                    const long long nr = lseq - qc0;
                    const uint32_t in_rec = nr <= 0 ? 0u : nr >= 16 ? 0xffffu : (1u << (uint32_t)nr) - 1u, real = valid & in_rec;
                    uint32_t m = valid;                                      // the counted bases of the piece
                    if (BQ) {
                        uint32_t w[4] = {0u, 0u, 0u, 0u};
                        if (real) { const uint4 v = *(const uint4 *)(ub + (c << 4)); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
                        m = (dep_ge_mask(w, min_baseq) & real) | (valid & ~in_rec);
                    }
                    const uint64_t bases = (m & in_rec) ? pil_seq16(ub, sbase, qc0, m & in_rec) : 0ull;
                    const long long slot0 = x + (qc0 - q) - beg;             // the slot of the piece's base 0
                    while (m) {
                        const uint32_t i = (uint32_t)__ffs((int)m) - 1u;
                        m &= m - 1u;
                        const uint32_t code4 = (uint32_t)(bases >> (60u - 4u * i)) & 15u;
                        put(slot0 + (long long)i, ((in_rec >> i) & 1u) ? (uint32_t)(PIL_CODE_SYM >> (4u * code4)) & 15u : PIL_SYM_N);
                    }
                }
            }
            x += len; q += len; anchored = true;
        } else if (code == 2u) {
            if (DEL) {
                const long long dlo = beg > x ? beg : x, dhi = end < x + len ? end : x + len;       // the operation's positions inside the row
                for (long long p = dlo + sub; p < dhi; p += DEP_LANES) put(p - beg, PIL_SYM_DEL);
            }
            x += len; anchored = true;
        } else if (code == 3u) { x += len; anchored = false; }
        else if (code == 1u) {
            if (INS && sub == 0 && anchored && x - 1 >= beg && x - 1 < end) put(x - 1 - beg, PIL_SYM_INS);
            q += len;
        } else if (code == 4u) q += len;
    }
}

// The counts of a batch.  A workgroup takes 32 reads a turn and a contiguous run of turns; every lane makes the same number of turns and of
// rounds and takes part in every vote and barrier.  Round r is the r-th row a read overlaps.  The step counters as in dep_add_body.
// WINDOW = false, the direct form: one return-less atomicAdd per counted base into the table.
// WINDOW = true: the workgroup keeps the counts of PIL_WINDOW positions of one target row in LDS (32-bit words, S per position, so no count
// can wrap before the table's own would).  The window is anchored at the first walked read of a turn -- its first position inside its first row --
// and stays while later turns' anchors lie in its row and its first half; otherwise it is flushed and moved.  A count inside it is an LDS atomic,
// every other count -- another row, a read that runs out of the window, an unsorted file, the far side of a long N -- takes the direct form.  A
// flush has consecutive lanes add consecutive non-zero words to the table.  LDS: 32 KiB with strands, 16 KiB without.
#define PIL_WINDOW 512u
#define PIL_NO_ROW 0xffffffffu
template <bool BQ, bool DEL, bool INS, bool STRANDS, bool WINDOW>
__global__ void __launch_bounds__(256) bam_pileup_add(DepArgs a, uint32_t *__restrict__ table, unsigned long long *__restrict__ steps) {
    __shared__ unsigned long long block_steps[DEP_N_STEPS];
    constexpr uint32_t S = STRANDS ? 2u * PIL_SYMBOLS : PIL_SYMBOLS;
    __shared__ uint32_t win[WINDOW ? PIL_WINDOW * S : 1u];
    __shared__ uint32_t wsh[4];                                              // the turn's first walked read, and what its first lane decided: move, row, first slot
    uint32_t cur_k = PIL_NO_ROW, cur_x0 = 0;                                 // the window's row and its first position slot in it (the same in every thread)
    if (WINDOW) for (uint32_t w = threadIdx.x; w < PIL_WINDOW * S; w += 256u) win[w] = 0u;
    auto flush = [&]() {                                                     // (between barriers; every thread takes part)
        uint32_t *dst = table + (a.rbase[cur_k] + cur_x0) * S;
        for (uint32_t w = threadIdx.x; w < PIL_WINDOW * S; w += 256u) { const uint32_t v = win[w]; if (v) { atomicAdd(dst + w, v); win[w] = 0u; } }
    };
    const uint32_t lane = threadIdx.x & 63u, sub = threadIdx.x & (DEP_LANES - 1u), grp = threadIdx.x / DEP_LANES;
    if (threadIdx.x < DEP_N_STEPS) block_steps[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t mis = (uint32_t)((uintptr_t)a.u & 15u);
    const uint8_t *ub = a.u - mis;
    unsigned long long mine = 0;
    const uint64_t turns = ((uint64_t)a.n + 31u) / 32u, per = (turns + gridDim.x - 1u) / gridDim.x;
    const uint64_t t_beg = (uint64_t)blockIdx.x * per, t_end = t_beg + per < turns ? t_beg + per : turns;
    for (uint64_t turn = t_beg; turn < t_end; turn++) {
        const uint64_t i = turn * 32u + grp;
        const uint32_t sb = i < a.n ? a.step[i] : (uint32_t)DEP_STEP_NONE, s = sb & 15u;
        uint32_t k0 = 0, k1 = 0, ne = 0, strand = 0; long long p0 = 0, lseq = 0; uint64_t qoff = 0, soff = 0; const uint8_t *cig = nullptr;
        if (s == DEP_STEP_COUNTED && (sb & DEP_WALK)) {
            k0 = a.k0[i]; k1 = a.k1[i]; p0 = a.pos[i] - 1;
            strand = STRANDS && (a.flag[i] & 16u) ? PIL_SYMBOLS : 0u;
            const uint64_t ro = a.rec_off[i];
            const uint8_t *rec = a.u + ro;
            cig = rec + a.cig_rel[i]; ne = a.ncig_eff[i];
            const uint32_t lrn = rec[12], nc = (uint32_t)rec[16] | ((uint32_t)rec[17] << 8);
            const long long ls = (long long)(int32_t)cov_ldu32(rec + 20), rec_len = 4ll + (long long)cov_ldu32(rec);
            const long long srel = 36ll + lrn + 4ll * nc, qrel = srel + ((ls > 0 ? ls : 0) + 1) / 2;
            soff = ro + (uint64_t)srel; qoff = ro + (uint64_t)qrel;
            lseq = ls < 0 || qrel >= rec_len ? 0 : ls < rec_len - qrel ? ls : rec_len - qrel;          // (SEQ and QUAL are never read behind the record)
        }
        if (WINDOW) {
            if (threadIdx.x == 0) wsh[0] = 0xffffffffu;
            __syncthreads();
            if (k1 > k0 && sub == 0) atomicMin(&wsh[0], grp);
            __syncthreads();
            if (wsh[0] == grp && sub == 0) {                                 // the turn's first walked read anchors the window
                const long long beg = a.rbeg[k0];
                const uint32_t x0 = (uint32_t)(p0 > beg ? p0 - beg : 0);
                wsh[1] = (cur_k != k0 || x0 < cur_x0 || x0 - cur_x0 >= PIL_WINDOW / 2u) ? 1u : 0u; wsh[2] = k0; wsh[3] = x0;
            }
            __syncthreads();
            if (wsh[0] != 0xffffffffu && wsh[1]) {                           // (the same for the whole workgroup)
                if (cur_k != PIL_NO_ROW) flush();
                cur_k = wsh[2]; cur_x0 = wsh[3];
            }
            __syncthreads();
        }
        for (uint32_t k = k0; k < k1; k++) {
            const long long beg = a.rbeg[k];
            uint32_t *row = table + a.rbase[k] * S + strand;
            const bool here = WINDOW && k == cur_k;
            pil_walk_row<BQ, DEL, INS>(ub, mis, qoff, soff, lseq, a.min_baseq, cig, ne, p0, beg, a.rend[k], sub, [&](long long slot, uint32_t sym) {
                const unsigned long long rel = (unsigned long long)(slot - (long long)cur_x0);          // (wraps for a slot in front of the window)
                if (here && rel < PIL_WINDOW) atomicAdd(&win[(uint32_t)rel * S + strand + sym], 1u);
                else atomicAdd(row + (uint64_t)slot * S + sym, 1u);
            });
        }
        const uint32_t sv = sub == 0 ? s : (uint32_t)DEP_STEP_NONE;
#pragma unroll
        for (uint32_t k = 0; k < DEP_N_STEPS; k++) { const unsigned long long m = __ballot(sv == k); if (lane == k) mine += (unsigned long long)__popcll(m); }
    }
    if (lane < DEP_N_STEPS && mine) atomicAdd(&block_steps[lane], mine);
    __syncthreads();
    if (WINDOW && cur_k != PIL_NO_ROW) flush();
    if (threadIdx.x < DEP_N_STEPS && block_steps[threadIdx.x]) atomicAdd(&steps[threadIdx.x], block_steps[threadIdx.x]);
}

// ---- count and emit ----------------------------------------------------------------------------------------------------------------------------
struct PilEmitArgs {
    const uint32_t *table; const unsigned long long *toff;                                         // the counts, and the result index in front of every tile
    const uint32_t *tile_row; const unsigned long long *rbase; const long long *rbeg, *rend;        // the sorted rows (tile_row: per DEP_TILE position slots)
    const int32_t *row_tid; uint32_t sshift, min_count;                                            // S = 1 << sshift words per position
    unsigned long long t0, o_a, o_b, dst0;                                                         // the first tile, the window, and the page row of result index o_a
    int32_t *out_tid; long long *out_pos; uint8_t *out_strand, *out_nuc; int32_t *out_count;       // the page (null: the column is not wanted)
};
// word w of the table lies in the row of its position slot; bit e of the result = word 4 t + e of the tile emits
__device__ __forceinline__ uint32_t pil_emit_mask(const uint4 v, uint64_t w0, uint32_t sshift, uint64_t rbase, uint64_t len, uint32_t min_count) {
    const uint32_t d[4] = {v.x, v.y, v.z, v.w};
    uint32_t em = 0;
#pragma unroll
    for (uint32_t e = 0; e < 4u; e++) if (d[e] >= min_count && ((w0 + e) >> sshift) - rbase < len) em |= 1u << e;
    return em;
}
__global__ void __launch_bounds__(256) pil_tile_count(const uint32_t *__restrict__ table, const uint32_t *__restrict__ tile_row, const unsigned long long *__restrict__ rbase,
                                                      const long long *__restrict__ rbeg, const long long *__restrict__ rend, uint32_t sshift, uint32_t min_count,
                                                      unsigned long long *__restrict__ tcnt) {
    __shared__ uint32_t sh[256];
    const uint64_t w0 = (uint64_t)blockIdx.x * PIL_TILE + threadIdx.x * 4u;
    const uint32_t k = tile_row[((uint64_t)blockIdx.x * PIL_TILE >> sshift) / DEP_TILE];           // (a tile of words lies inside one tile of positions)
    const uint4 v = *(const uint4 *)(table + w0);
    const uint32_t cnt = (uint32_t)__popc(pil_emit_mask(v, w0, sshift, rbase[k], (uint64_t)(rend[k] - rbeg[k]), min_count));
    const uint32_t incl = block_scan<uint32_t, ScanSum>(cnt, sh);
    if (threadIdx.x == 255u) tcnt[blockIdx.x] = incl;
}
// out[k] = the result index in front of row k (k = n_rows: the rows of the whole result)
__global__ void __launch_bounds__(256) pil_row_offsets(const unsigned long long *__restrict__ toff, const unsigned long long *__restrict__ rbase, uint32_t sshift, uint64_t n_rows, uint64_t ntiles,
                                                       unsigned long long *__restrict__ out) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k <= n_rows) out[k] = toff[k < n_rows ? (rbase[k] << sshift) / PIL_TILE : ntiles];
}
__global__ void __launch_bounds__(256) pil_emit(PilEmitArgs a) {
    __shared__ uint32_t sh[256];
    __shared__ uint32_t lcnt[PIL_TILE];
    __shared__ uint16_t lidx[PIL_TILE];
    const uint64_t tile = a.t0 + blockIdx.x;
    const unsigned long long ob = a.toff[tile], oe = a.toff[tile + 1];
    if (oe <= a.o_a || ob >= a.o_b || oe == ob) return;                                           // (the same for the whole workgroup)
    const uint64_t w0 = tile * PIL_TILE + threadIdx.x * 4u;
    const uint32_t k = a.tile_row[(tile * PIL_TILE >> a.sshift) / DEP_TILE];
    const int32_t tid = a.row_tid[k];
    const uint64_t rb = a.rbase[k];
    const uint4 v = *(const uint4 *)(a.table + w0);
    const uint32_t d[4] = {v.x, v.y, v.z, v.w};
    const uint32_t em = pil_emit_mask(v, w0, a.sshift, rb, (uint64_t)(a.rend[k] - a.rbeg[k]), a.min_count), cnt = (uint32_t)__popc(em);
    uint32_t at = block_scan<uint32_t, ScanSum>(cnt, sh) - cnt;                                                   // (ends in a barrier)
#pragma unroll
    for (uint32_t e = 0; e < 4u; e++) if ((em >> e) & 1u) { lcnt[at] = d[e]; lidx[at] = (uint16_t)(threadIdx.x * 4u + e); at++; }
    __syncthreads();
    const uint32_t n = (uint32_t)(oe - ob);                                                        // (<= PIL_TILE: what pil_tile_count counted by the same rule)
    const uint32_t smask = (1u << a.sshift) - 1u;
    const long long pos1 = a.rbeg[k] - (long long)rb + 1;                                          // 1-based position of position slot 0
    for (uint32_t j = threadIdx.x; j < n && j < PIL_TILE; j += 256u) {
        const unsigned long long o = ob + j;
        if (o < a.o_a || o >= a.o_b) continue;
        const unsigned long long r = a.dst0 + (o - a.o_a);
        const uint64_t w = tile * PIL_TILE + lidx[j];
        const uint32_t ss = (uint32_t)w & smask;                                                   // strand * 8 + symbol
        if (a.out_tid) a.out_tid[r] = tid;
        if (a.out_pos) a.out_pos[r] = pos1 + (long long)(w >> a.sshift);
        if (a.out_strand) a.out_strand[r] = a.sshift == 3u ? (uint8_t)'*' : ss >= PIL_SYMBOLS ? (uint8_t)'-' : (uint8_t)'+';
        if (a.out_nuc) a.out_nuc[r] = (uint8_t)(0x2b2d3d4e54474341ull >> (8u * (ss & 7u)));        // "ACGTN=-+"
        if (a.out_count) a.out_count[r] = (int32_t)lcnt[j];
    }
}
