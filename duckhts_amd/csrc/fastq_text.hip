// fastq_text.hip -- FASTQ / FASTA TEXT -> BAM records on the device (gfx950), so that read_bam's record stage serves raw reads unchanged.
// Included by dhts_api.hip after sam_text.hip (the line index kernels vcf_line_count / vcf_line_fill, seq_nt16_table and hts_reg2bin are shared).
//
// Replaces:
//   hts_detect_format2   htslib hts.c:686-745 (is_fastaq :458-477)   -> fastq_text_detect (host)
//   fastq_parse1         sam.c:3919-4120, default options            -> fq_line_props / fq_next (which lines one record takes),
//                                                                       fq_tile / fq_chain (which lines START a record), fq_encode
//   bam_set1, bam_write1 sam.c:526-646, 857+                         -> fq_encode<false> (sizes), <true> (bytes) behind an exclusive scan
//
// A record is a chain over lines: the name line, sequence lines up to the first '+'-led line, then quality lines until their summed length
// reaches the sequence length -- a quality line may itself begin with '@' or '+', so no line can be told to start a record by its own
// bytes.  What CAN be said of every line alone is where the NEXT record would start if a record started here:
//   len[i], and flag[i] = "begins with '+'" ('>' for FASTA)        one lane per line
//   psum = exclusive scan of len, rank = exclusive scan of flag, mark_idx = the flagged lines in order
//   next[i]: the first '+' line behind i is mark_idx[rank[i + 1]]; the sequence length is a difference of psum; the last quality line is
//            found by bisection over psum.  No lane walks lines: O(log n) per line whatever the wrapping.
// The true record starts are the chain 0 -> next[0] -> next[next[0]] ...  It is resolved in tiles of FQ_TILE lines: pointer jumping in
// LDS (2^k-th successors inside the tile) gives every line the place where a chain through it LEAVES its tile (fq_tile<false>); one lane
// then hops from tile to tile (fq_chain: lines / FQ_TILE hops) and notes each tile's entry; fq_tile<true> marks, again by the 2^k-th
// successors, the lines reachable from the entry.  A chain ends at the end of the batch's lines, at a line that cannot start a record
// (rejected: the scan ends there) or at a record whose lines run out of the batch (the carry, or a truncated file).
//
// fq_encode: one wave per record.  The name scan, the SEQ packing (two bases per byte across line breaks) and QUAL - 33 run across the 64
// lanes, a wrapped record line by line.
#pragma once

#define FQ_TILE 2048u
#define FQ_LEVELS 11                                         /* 2^11 = FQ_TILE: a chain inside a tile has fewer than FQ_TILE hops */
#define FQ_STOP 0x80000000u                                  /* next / exit: the chain stops AT line (value & FQ_IDX) ... */
#define FQ_INCOMPLETE 0x40000000u                            /* ... because its record runs out of the batch's lines (else: rejected) */
#define FQ_IDX 0x3fffffffu
#define FQ_NONE 0xffffffffu
#define FQ_ENC_THREADS 256

struct FqArgs {
    const uint8_t *u; const uint32_t *line_off; uint32_t nlines; int fasta, final_batch;   // line i = u[line_off[i], line_off[i+1] - 1)
    uint32_t *len, *flag;                                     // per line: bytes without the trailing '\r'; begins with '+' ('>')
    const uint32_t *psum, *rank; uint32_t *mark_idx; uint32_t nmark;
    uint32_t *next, *plus;                                    // per line: where the next record would start; the '+' line
    uint32_t *exit_, *entry, *stop;                           // per line; per tile; stop[0] = line the chain stopped at, stop[1] = 0 end of lines, 1 rejected, 2 incomplete
    uint32_t *is_start; const uint32_t *rec_rank; uint32_t *rec_line; uint32_t nrec;
    uint32_t *rec_len; const uint32_t *rec_off; uint8_t *out;
    unsigned long long *first_bad;                            // the first record bam_set1 refuses (atomicMin)
};

__global__ void __launch_bounds__(256) fq_line_props(FqArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.nlines) return;
    const uint32_t s = a.line_off[i]; uint32_t e = a.line_off[i + 1] - 1;
    if (e > s && a.u[e - 1] == '\r') e--;                     // bgzf_getline drops one trailing '\r'
    a.len[i] = e - s;
    a.flag[i] = (e > s && a.u[s] == (a.fasta ? '>' : '+')) ? 1u : 0u;
}
// dst[rank[i]] = i for the flagged i
__global__ void __launch_bounds__(256) fq_compact(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ rank, uint32_t n, uint32_t *__restrict__ dst) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n && flag[i]) dst[rank[i]] = i;
}
__global__ void __launch_bounds__(256) fq_next(FqArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.nlines) return;
    const uint32_t n = a.nlines;
    const uint8_t c0 = a.len[i] ? a.u[a.line_off[i]] : 0;
    uint32_t nx = FQ_STOP | i, pl = 0;                        // "*x->name.s != x->nprefix"
    if (a.fasta) {
        if (c0 == '>') {                                      // sequence lines run to the next '>' line, or to the end of the file
            const uint32_t r = a.rank[i + 1];
            nx = r < a.nmark ? a.mark_idx[r] : a.final_batch ? n : (FQ_STOP | FQ_INCOMPLETE | i);
            pl = nx;
        }
    } else if (c0 == '@') {
        const uint32_t r = a.rank[i + 1];
        nx = FQ_STOP | FQ_INCOMPLETE | i;
        if (r < a.nmark) {
            const uint32_t j = a.mark_idx[r], q = j + 1; pl = j;
            const uint32_t S = a.psum[j] - a.psum[i + 1];
            if (q < n) {
                if (S == 0) nx = a.len[q] ? (FQ_STOP | i) : q + 1;      // an empty read takes one, empty, quality line
                else {
                    const uint32_t base = a.psum[q];
                    uint32_t lo = q, hi = n;                            // the first k with psum[k + 1] - psum[q] >= S
                    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (a.psum[mid + 1] - base >= S) hi = mid; else lo = mid + 1; }
                    if (lo < n) nx = a.psum[lo + 1] - base == S ? lo + 1 : (FQ_STOP | i);   // "fp->line.l > remainder"
                }
            }
        }
    }
    a.next[i] = nx; a.plus[i] = pl;
}

// MARK = false: exit_[e] = where a chain through line e leaves e's tile (a line of a later tile, nlines, or a FQ_STOP value)
// MARK = true:  is_start[e] = e is reachable from the tile's entry and its record is whole
template <bool MARK>
__global__ void __launch_bounds__(256) fq_tile(FqArgs a) {
    __shared__ uint16_t lv[FQ_LEVELS][FQ_TILE];
    __shared__ uint8_t mk[MARK ? FQ_TILE : 1];
    const uint32_t base = blockIdx.x * FQ_TILE, n = a.nlines - base < FQ_TILE ? a.nlines - base : FQ_TILE;
    uint32_t ent = FQ_NONE;
    if (MARK) { ent = a.entry[blockIdx.x]; if (ent == FQ_NONE) { for (uint32_t e = threadIdx.x; e < n; e += 256) a.is_start[base + e] = 0; return; } }
    for (uint32_t e = threadIdx.x; e < n; e += 256) {
        const uint32_t x = a.next[base + e];
        lv[0][e] = (!(x & FQ_STOP) && x < base + n) ? (uint16_t)(x - base) : (uint16_t)0xffff;
        if (MARK) mk[e] = (base + e == ent) ? 1 : 0;
    }
    __syncthreads();
    for (int k = 1; k < FQ_LEVELS; k++) {
        for (uint32_t e = threadIdx.x; e < n; e += 256) { const uint16_t h = lv[k - 1][e]; lv[k][e] = h == 0xffff ? h : lv[k - 1][h]; }
        __syncthreads();
    }
    if (!MARK) {
        for (uint32_t e = threadIdx.x; e < n; e += 256) {
            uint32_t cur = e;
            for (int k = FQ_LEVELS - 1; k >= 0; k--) { const uint16_t h = lv[k][cur]; if (h != 0xffff) cur = h; }
            a.exit_[base + e] = a.next[base + cur];
        }
        return;
    }
    // a line d hops behind the entry is marked by the set bits of d, high to low (a mark set in this round may already be passed on in
    // it: that marks a line 2 * 2^k hops on, which the chain reaches as well)
    for (int k = FQ_LEVELS - 1; k >= 0; k--) {
        for (uint32_t e = threadIdx.x; e < n; e += 256) { const uint16_t h = lv[k][e]; if (mk[e] && h != 0xffff) mk[h] = 1; }
        __syncthreads();
    }
    for (uint32_t e = threadIdx.x; e < n; e += 256) a.is_start[base + e] = (mk[e] && !(a.next[base + e] & FQ_STOP)) ? 1u : 0u;
}
// from tile to tile: every hop leaves a tile, so there are at most (tiles) of them.  entry[] is preset to FQ_NONE
__global__ void fq_chain(FqArgs a) {
    if (threadIdx.x || blockIdx.x) return;
    uint32_t e = 0;
    for (;;) {
        if (e >= a.nlines) { a.stop[0] = a.nlines; a.stop[1] = 0; return; }
        a.entry[e / FQ_TILE] = e;
        const uint32_t x = a.exit_[e];
        if (x & FQ_STOP) { a.stop[0] = x & FQ_IDX; a.stop[1] = (x & FQ_INCOMPLETE) ? 2u : 1u; return; }
        e = x;
    }
}

__device__ __forceinline__ bool fq_isspace(uint8_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

template <bool WRITE>
__global__ void __launch_bounds__(FQ_ENC_THREADS) fq_encode(FqArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t nw = gridDim.x * (FQ_ENC_THREADS / 64);
    const uint8_t *u = a.u;
    for (uint32_t r = blockIdx.x * (FQ_ENC_THREADS / 64) + (threadIdx.x >> 6); r < a.nrec; r += nw) {
        if (WRITE && (a.rec_len[r] == 0 || (unsigned long long)r >= *a.first_bad)) continue;
        const uint32_t i = a.rec_line[r], nx = a.next[i], j = a.plus[i];
        // name = the bytes behind '@' / '>' up to the first isspace_c byte
        const uint32_t s = a.line_off[i] + 1, avail = a.len[i] - 1;
        uint32_t nl = avail, z = FQ_NONE;                     // z: the first NUL of the name (bam_set1 copies it with strncpy)
        for (uint32_t p = 0; p < avail; p += 64) {
            const uint8_t ch = p + lane < avail ? u[s + p + lane] : (uint8_t)'x';
            const uint64_t sp = __ballot(fq_isspace(ch)), zm = __ballot(ch == 0);
            if (zm && z == FQ_NONE) z = p + (uint32_t)(__ffsll((unsigned long long)zm) - 1);
            if (sp) { nl = p + (uint32_t)(__ffsll((unsigned long long)sp) - 1); break; }
            if (p >= 320) break;                              // (longer than bam_set1 takes: rejected below whatever follows)
        }
        uint32_t flag = 4;
        if (nl >= 2 && u[s + nl - 2] == '/' && u[s + nl - 1] >= '0' && u[s + nl - 1] <= '9') {     // name.l (with its '@') > 2
            const uint8_t d = u[s + nl - 1];
            flag |= 1 | 8 | (d == '1' ? 64u : d == '2' ? 128u : 192u);
            nl -= 2;
        }
        const bool star = nl == 0;                            // bam_set1: "use a default qname '*' if none is provided"
        if (star) nl = 1;
        if (nl > 254) { if (!WRITE && lane == 0) { a.rec_len[r] = 0; atomicMin(a.first_bad, (unsigned long long)r); } continue; }
        if (z > nl) z = nl;
        const uint32_t S = a.psum[j] - a.psum[i + 1];
        const uint32_t l_qname = nl + 1, sdst = 36 + l_qname, qdst = sdst + (S + 1) / 2, total = qdst + S;
        if (!WRITE) { if (lane == 0) a.rec_len[r] = total; continue; }
        uint8_t *rec = a.out + a.rec_off[r];
        if (lane < 9) {
            uint32_t w = 0;
            switch (lane) {
                case 0: w = total - 4; break;
                case 1: case 2: case 6: case 7: w = 0xffffffffu; break;                     // tid, pos, mtid, mpos = -1
                case 3: w = sam_reg2bin(-1, 0) << 16 | l_qname; break;
                case 4: w = flag << 16; break;
                case 5: w = S; break;
                default: break;                                                              // tlen 0
            }
            __builtin_memcpy(rec + 4 * lane, &w, 4);
        }
        for (uint32_t k = lane; k < l_qname; k += 64) rec[36 + k] = star ? (k == 0 ? (uint8_t)'*' : (uint8_t)0) : k < z ? u[s + k] : (uint8_t)0;
        // SEQ: the lines (i, j), two bases per byte; `pend` is the base an odd count leaves for the next line's first
        uint32_t done = 0; uint8_t pend = 0;
        for (uint32_t m = i + 1; m < j; m++) {
            uint32_t l = a.len[m]; uint32_t t = a.line_off[m];
            if (l == 0) continue;
            if (done & 1) { if (lane == 0) rec[sdst + done / 2] = (uint8_t)(sam_nt16[pend] << 4 | sam_nt16[u[t]]); t++; l--; done++; }
            for (uint32_t k = lane; k < l / 2; k += 64) rec[sdst + done / 2 + k] = (uint8_t)(sam_nt16[u[t + 2 * k]] << 4 | sam_nt16[u[t + 2 * k + 1]]);
            if (l & 1) pend = u[t + l - 1];
            done += l;
        }
        if ((done & 1) && lane == 0) rec[sdst + done / 2] = (uint8_t)(sam_nt16[pend] << 4);
        // QUAL: the lines (j, nx) minus 33 (a first byte 0x20 so becomes 0xff: the record reads as QUAL '*'); FASTA has none
        if (a.fasta) { for (uint32_t k = lane; k < S; k += 64) rec[qdst + k] = 0xff; }
        else {
            uint32_t qd = 0;
            for (uint32_t m = j + 1; m < nx; m++) {
                const uint32_t l = a.len[m], t = a.line_off[m];
                for (uint32_t k = lane; k < l; k += 64) rec[qdst + qd + k] = (uint8_t)(u[t + k] - 33);
                qd += l;
            }
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
// is_fastaq (hts.c:458-477): the first line is text; the second holds base letters only ('=' excluded) up to its end or the end of the bytes
static bool fq_is_fastaq(const uint8_t *u, size_t len) {
    const uint8_t *ulim = u + len, *eol = (const uint8_t *)memchr(u, '\n', len);
    for (const uint8_t *p = u; p < (eol ? eol : ulim); p++) if (!(*p >= ' ' || *p == '\t' || *p == '\r' || *p == '\n')) return false;
    if (!eol) return true;
    static const uint8_t nt16_host[128] = {
        15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15,
        15,15,15,15, 15,15,15,15, 15,15,15,15, 15,15,15,15,  0,15,15,15, 15,15,15,15, 15,15,15,15, 15, 0,15,15,
        15, 1,14, 2, 13,15,15, 4, 11,15,15,12, 15, 3,15,15, 15,15, 5, 6,  8,15, 7, 9, 15,10,15,15, 15,15,15,15,
        15, 1,14, 2, 13,15,15, 4, 11,15,15,12, 15, 3,15,15, 15,15, 5, 6,  8,15, 7, 9, 15,10,15,15, 15,15,15,15};
    const uint8_t *p = eol + 1;
    while (p < ulim && ((*p < 128 && nt16_host[*p] != 15) || *p == 'N' || *p == 'n')) { if (*p == '=') return false; p++; }
    return p == ulim || *p == '\r' || *p == '\n';
}
// hts_detect_format2's order on the first bytes (hts.c:693-733): a SAM header line first, then '>' + is_fastaq (2: FASTA), '@' + is_fastaq
// (1: FASTQ); 0: neither (the SAM column rule of sam_text_detect comes behind these)
static int fastq_text_detect(const uint8_t *s, size_t len) {
    if (len > 1024) len = 1024;
    if (len >= 4 && s[0] == '@' && (!memcmp(s, "@HD\t", 4) || !memcmp(s, "@SQ\t", 4) || !memcmp(s, "@RG\t", 4) || !memcmp(s, "@PG\t", 4) || !memcmp(s, "@CO\t", 4))) return 0;
    if (len >= 1 && s[0] == '>' && fq_is_fastaq(s, len)) return 2;
    if (len >= 1 && s[0] == '@' && fq_is_fastaq(s, len)) return 1;
    return 0;
}
// fastq_parse1 on the first record of h[0, good): 0 it is whole and accepted, 1 it runs beyond `good` and more bytes can be had, -1 rejected
static int fastq_first_record(const uint8_t *h, uint64_t good, bool more, bool fasta) {
    uint64_t p = 0; bool eof = false;
    auto getline = [&](uint64_t &ls, uint64_t &ll) -> int {   // 0 a line, 1 need more bytes, -1 end of file
        if (p >= good) { if (more) return 1; eof = true; return -1; }
        const uint8_t *nl = (const uint8_t *)memchr(h + p, '\n', good - p);
        if (!nl && more) return 1;
        const uint64_t e = nl ? (uint64_t)(nl - h) : good;
        ls = p; ll = e - p; if (ll && h[p + ll - 1] == '\r') ll--;
        p = nl ? e + 1 : good;
        return 0;
    };
    uint64_t ls = 0, ll = 0; int r = getline(ls, ll);
    if (r) return r;
    if (ll == 0 || h[ls] != (fasta ? '>' : '@')) return -1;
    uint64_t nl = 1; while (nl < ll && !(h[ls + nl] == ' ' || (h[ls + nl] >= '\t' && h[ls + nl] <= '\r'))) nl++;
    if (nl > 2 && h[ls + nl - 2] == '/' && h[ls + nl - 1] >= '0' && h[ls + nl - 1] <= '9') nl -= 2;
    if (nl - 1 > 254) return -1;
    if (fasta) return 0;                                      // (nothing else refuses a FASTA record: the next '>' or the end of the file ends it)
    uint64_t S = 0;
    for (;;) {
        r = getline(ls, ll);
        if (r > 0) return 1;
        if (r < 0) { if (fasta) return 0; return -1; }
        if (ll && h[ls] == (fasta ? '>' : '+')) break;
        S += ll;
    }
    if (fasta) return 0;
    uint64_t rem = S;
    do {
        r = getline(ls, ll);
        if (r > 0) return 1;
        if (r < 0 || ll > rem) return -1;
        rem -= ll;
    } while (rem > 0);
    return 0;
}
