// fasta_index.hip -- the FASTA index (.fai) on the device (gfx950): build and region fetch.
// Included by dhts_api.hip after fastq_text.hip (the line index kernels vcf_line_count / vcf_line_fill and fq_compact are shared).
//
// Replaces:
//   fai_build_core   htslib faidx.c:132-349 (a bgzf_getc loop, one character at a time)   -> fa_chunk_props / fa_line_cl (per line),
//                                                                                            fa_short / fa_check / fa_records (per record)
//   fai_retrieve     faidx.c:716-796 (a bgzf_read_small loop, one line at a time)         -> fa_fetch (all regions of a query in one launch)
//
// In FASTA every line that begins with '>' is a header line: OUT_READ and IN_SEQ both go to IN_NAME on it and IN_NAME takes the whole line
// (faidx.c:152-160, 234-236, 195-226).  So the records of a batch are the runs of lines between header lines, and what fai_build_core's
// state machine does inside one run is a function of per-line properties:
//   ll   bytes of the line with its terminator (the difference of two line offsets; the last line of a file counts one more, faidx.c:260)
//   cl   bytes with isgraph (0x21..0x7e)
//   cls  what the first bytes say: header, blank, "\r\n", '\r' + something else, '@', other
//   line_len / line_blen = ll / cl of the run's first line; first_short = the first line that is blank or shorter than line_len;
//   every line in front of first_short has ll == line_len ("Different line length" otherwise), every line behind it is blank or "\r\n"
//   (OUT_READ's errors otherwise); len = the sum of cl (blank lines add nothing).
// fa_chunk_props is the pass that touches every byte: 16 bytes per lane in aligned loads, a newline mask and an isgraph mask per lane, a
// scan of both counts inside the 4 KiB chunk; the lane that holds a newline writes the count of isgraph bytes in front of it and the class
// of the line behind it.  cl is then a difference of two such counts plus the chunks' bases -- no lane walks a line, whatever its width.
// A record crosses batches (a chromosome is many batches): the host carries name, len so far, line_len, line_blen, seq_offset and the
// phase; the run in front of a batch's first header continues the carried record (FaArgs::c_phase / c_line_len).
#pragma once

#define FA_CHUNK VCF_CHUNK
#define FA_NONE 0xffffffffu
enum { FA_CLS_OTHER = 0, FA_CLS_HEADER = 1, FA_CLS_BLANK = 2, FA_CLS_CRBLANK = 3, FA_CLS_CR = 4, FA_CLS_AT = 5 };
enum { FA_ERR_DIFFLEN = 1, FA_ERR_UNEXPECTED = 2, FA_ERR_CR = 3, FA_ERR_AT = 4 };

// what the record between two header lines of a batch came to ([0]: the lines in front of the batch's first header)
struct FaRec { uint32_t hdr_line, nlines, first_ll, first_cl, len, first_short, name_off, name_len, seq_off, pad; };
struct FaArgs {
    const uint8_t *u; uint64_t ulen;
    const uint32_t *line_off; const uint8_t *cls; uint32_t nlines;
    const uint32_t *cl, *csum, *hrank, *hdr_line; uint32_t nhdr;       // hrank[i]: header lines in front of line i = the run line i belongs to
    uint32_t c_phase, c_line_len;                                       // the carried record: 0 IN_SEQ (line_len 0: no sequence line yet), 1 OUT_READ
    uint32_t *first_short; unsigned long long *err; FaRec *rec;
};

__device__ __forceinline__ uint32_t fa_class(const uint8_t *__restrict__ u, uint64_t s, uint64_t ulen) {
    if (s >= ulen) return FA_CLS_OTHER;
    const uint8_t c0 = u[s];
    if (c0 == '>') return FA_CLS_HEADER;
    if (c0 == '\n') return FA_CLS_BLANK;
    if (c0 == '@') return FA_CLS_AT;
    if (c0 == '\r') return (s + 1 < ulen && u[s + 1] == '\n') ? FA_CLS_CRBLANK : FA_CLS_CR;
    return FA_CLS_OTHER;
}
// bit k of nl: u[p + k] == '\n'; bit k of gr: isgraph(u[p + k]).  Four bytes at a time: the high bit of a byte of `ge21` says its low seven
// bits are >= 0x21, of `ge7f` that they are 0x7f; a byte is graphic when the first holds, the second does not and its own high bit is clear.
__host__ __device__ __forceinline__ void fa_masks_word(uint32_t w, uint32_t &nl4, uint32_t &gr4) {
    const uint32_t lo7 = w & 0x7f7f7f7fu;
    const uint32_t g = ((lo7 + 0x5f5f5f5fu) & ~(lo7 + 0x01010101u) & ~w) & 0x80808080u;
    const uint32_t x = w ^ 0x0a0a0a0au;
    const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
    gr4 = (((g >> 7) * 0x01020408u) >> 24) & 0xfu;                      // the four high bits gathered into a nibble (no two partial products meet)
    nl4 = (((z >> 7) * 0x01020408u) >> 24) & 0xfu;
}
// Contract: `u` is the base of a batch buffer (256-byte aligned: DevBuf) and p a multiple of 16, so every load but the text's last is the
// wide one; a caller that handed in an offset pointer would still be right, through the byte loop, and slow.
__device__ __forceinline__ void fa_masks16(const uint8_t *__restrict__ u, uint64_t p, uint64_t ulen, uint32_t &nl, uint32_t &gr) {
    nl = 0; gr = 0;
    if (p + 16 <= ulen && (((uintptr_t)(u + p)) & 15) == 0) {
        const uint4 v = *(const uint4 *)(u + p);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; q++) { uint32_t a, b; fa_masks_word(w[q], a, b); nl |= a << (4 * q); gr |= b << (4 * q); }
    } else for (uint32_t k = 0; k < 16 && p + k < ulen; k++) { const uint8_t b = u[p + k]; if (b == '\n') nl |= 1u << k; if (b >= 0x21 && b <= 0x7e) gr |= 1u << k; }
}
// One workgroup per 4 KiB chunk.  base_of[k] = newlines in front of chunk k (vcf_line_count + scan).  Newline number r (1-based over the
// batch) ends line r - 1 and starts line r:  gtmp[r] = isgraph bytes of the chunk in front of it, cls[r] = class of line r.
// gchunk[k] = isgraph bytes of the chunk.
extern "C" __global__ void __launch_bounds__(256)
fa_chunk_props(const uint8_t *__restrict__ u, uint64_t ulen, const uint32_t *__restrict__ base_of, uint32_t *__restrict__ gtmp, uint32_t *__restrict__ gchunk, uint8_t *__restrict__ cls) {
    __shared__ uint32_t wsum[4];
    const uint64_t p = (uint64_t)blockIdx.x * FA_CHUNK + threadIdx.x * 16u;
    uint32_t nl = 0, gr = 0;
    if (p < ulen) fa_masks16(u, p, ulen, nl, gr);
    const uint32_t v = __popc(nl) | (__popc(gr) << 16);                // both counts in one word: a chunk holds at most 4096 of either
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(incl, d, 64); if ((int)(threadIdx.x & 63) >= d) incl += t; }
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t excl = incl - v;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) excl += wsum[w];
    if (threadIdx.x == 255) gchunk[blockIdx.x] = (excl + v) >> 16;
    if (blockIdx.x == 0 && threadIdx.x == 0) { gtmp[0] = 0; cls[0] = (uint8_t)fa_class(u, 0, ulen); }
    uint32_t rank = base_of[blockIdx.x] + (excl & 0xffffu);
    const uint32_t gex = excl >> 16;
    while (nl) {
        const uint32_t b = __ffs(nl) - 1; nl &= nl - 1; ++rank;
        gtmp[rank] = gex + __popc(gr & ((1u << b) - 1u));
        cls[rank] = (uint8_t)fa_class(u, p + b + 1, ulen);
    }
}
// cl[i] and "line i is a header" (a header line's own bytes are not sequence: its cl is 0).  nl = newlines of the batch; a last line
// without one (nlines = nl + 1) ends where the text ends: gtotal.
__global__ void __launch_bounds__(256)
fa_line_cl(const uint32_t *__restrict__ line_off, const uint32_t *__restrict__ gtmp, const uint32_t *__restrict__ gbase, const uint8_t *__restrict__ cls,
           uint32_t nlines, uint32_t nl, uint32_t gtotal, uint32_t *__restrict__ cl, uint32_t *__restrict__ flag) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nlines) return;
    const uint32_t g0 = i == 0 ? 0u : gbase[(line_off[i] - 1u) / FA_CHUNK] + gtmp[i];
    const uint32_t g1 = i + 1 <= nl ? gbase[(line_off[i + 1] - 1u) / FA_CHUNK] + gtmp[i + 1] : gtotal;
    const bool hdr = cls[i] == FA_CLS_HEADER;
    cl[i] = hdr ? 0u : g1 - g0;
    flag[i] = hdr ? 1u : 0u;
}
// line_len of run `seg`, and whether its lines are all behind a first_short that lies in an earlier batch
__device__ __forceinline__ uint32_t fa_run_line_len(const FaArgs &a, uint32_t seg, bool &all_after) {
    all_after = false;
    uint32_t first = 0;
    if (seg == 0) {
        if (a.c_phase == 1) { all_after = true; return 0; }
        if (a.c_line_len) return a.c_line_len;
    } else first = a.hdr_line[seg - 1] + 1;
    if (first >= a.nlines) return 0;
    const uint32_t cf = a.cls[first];
    if (cf == FA_CLS_HEADER || cf == FA_CLS_BLANK) return 0;
    return a.line_off[first + 1] - a.line_off[first];
}
__global__ void __launch_bounds__(256) fa_short(FaArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.nlines || a.cls[i] == FA_CLS_HEADER) return;
    const uint32_t seg = a.hrank[i]; bool all_after;
    const uint32_t L = fa_run_line_len(a, seg, all_after);
    if (all_after) return;
    if (a.cls[i] == FA_CLS_BLANK || a.line_off[i + 1] - a.line_off[i] < L) atomicMin(&a.first_short[seg], i);
}
// the first line (in file order) at which fai_build_core would stop: err = min over lines of line << 3 | FA_ERR_*
__global__ void __launch_bounds__(256) fa_check(FaArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.nlines || a.cls[i] == FA_CLS_HEADER) return;
    const uint32_t seg = a.hrank[i]; bool all_after;
    const uint32_t L = fa_run_line_len(a, seg, all_after);
    const uint32_t fs = a.first_short[seg], c = a.cls[i];
    uint32_t kind = 0;
    if (all_after || (fs != FA_NONE && i > fs)) {                       // OUT_READ, faidx.c:150-192
        if (c == FA_CLS_AT) kind = FA_ERR_AT; else if (c == FA_CLS_CR) kind = FA_ERR_CR; else if (c != FA_CLS_BLANK && c != FA_CLS_CRBLANK) kind = FA_ERR_UNEXPECTED;
    } else if (i != fs && a.line_off[i + 1] - a.line_off[i] != L) kind = FA_ERR_DIFFLEN;      // IN_SEQ, faidx.c:272-274
    if (kind) atomicMin(a.err, ((unsigned long long)i << 3) | kind);
}
// one lane per run: its numbers, and the name of the header that opens it (faidx.c:205-211: whitespace behind '>' is skipped, the name
// runs to the next whitespace and may be empty)
__global__ void __launch_bounds__(256) fa_records(FaArgs a) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r > a.nhdr) return;
    FaRec o; o.pad = 0; o.hdr_line = FA_NONE; o.name_off = 0; o.name_len = 0; o.seq_off = 0;
    uint32_t start = 0;
    if (r > 0) {
        const uint32_t h = a.hdr_line[r - 1];
        o.hdr_line = h; start = h + 1;
        uint64_t s = (uint64_t)a.line_off[h] + 1, e = (uint64_t)a.line_off[h + 1] - 1;
        if (e > a.ulen) e = a.ulen;
        auto space = [](uint8_t b) { return b == ' ' || (b >= '\t' && b <= '\r'); };
        while (s < e && space(a.u[s])) s++;
        uint64_t q = s;
        while (q < e && !space(a.u[q])) q++;
        o.name_off = (uint32_t)s; o.name_len = (uint32_t)(q - s); o.seq_off = a.line_off[h + 1];
    }
    const uint32_t end = r < a.nhdr ? a.hdr_line[r] : a.nlines;
    o.nlines = end - start;
    o.len = a.csum[end] - a.csum[start];
    o.first_short = a.first_short[r];
    o.first_ll = 0; o.first_cl = 0;
    if (start < end && a.cls[start] != FA_CLS_BLANK) { o.first_ll = a.line_off[start + 1] - a.line_off[start]; o.first_cl = a.cl[start]; }
    a.rec[r] = o;
}
__global__ void __launch_bounds__(256) fa_names(const uint8_t *__restrict__ u, const FaRec *__restrict__ rec, const uint32_t *__restrict__ dst_off, uint32_t nhdr, uint8_t *__restrict__ dst) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x + 1;
    if (r > nhdr) return;
    const uint8_t *s = u + rec[r].name_off; uint8_t *d = dst + dst_off[r];
    for (uint32_t k = 0; k < rec[r].name_len; k++) d[k] = s[k];
}

// ---- region fetch ------------------------------------------------------------------------------------------------------------------
// out[out_off + i] = text[src + (beg + i) / blen * llen + (beg + i) % blen], which is what fai_retrieve's reads leave in its buffer
// (faidx.c:734-787: every line is read with its terminator and the next line overwrites the terminator).  A lane makes 16 output bytes:
// it finds its region by bisection, divides once, and then steps through the line (the column wraps at blen).
struct FaRegion { uint64_t out_off, n, beg; int64_t src; uint32_t blen, llen; };
__global__ void __launch_bounds__(256) fa_fetch(const uint8_t *__restrict__ text, const FaRegion *__restrict__ rg, uint32_t nreg, uint64_t total, uint8_t *__restrict__ out) {
    const uint64_t o0 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 16u;
    if (o0 >= total) return;
    const uint32_t cnt = total - o0 < 16 ? (uint32_t)(total - o0) : 16u;
    uint32_t lo = 0, hi = nreg;                                         // the last region with out_off <= o0 (empty regions share an offset: the last of them is followed by the one that holds the byte)
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (rg[mid].out_off <= o0) lo = mid; else hi = mid; }
    uint64_t w0 = 0, w1 = 0;
    uint32_t k = 0;
    while (k < cnt) {
        while (lo + 1 < nreg && rg[lo].out_off + rg[lo].n <= o0 + k) lo++;
        const FaRegion R = rg[lo];
        const uint64_t i = o0 + k - R.out_off, pos = R.beg + i;
        uint64_t line = pos / R.blen; uint32_t col = (uint32_t)(pos - line * R.blen);
        const uint8_t *s = text + R.src + (int64_t)(line * R.llen);
        uint64_t left = R.n - i;
        for (; k < cnt && left; k++, left--) {
            const uint64_t b = s[col];
            if (k < 8) w0 |= b << (8 * k); else w1 |= b << (8 * (k - 8));
            if (++col == R.blen) { col = 0; s += R.llen; }
        }
    }
    if (cnt == 16) *(uint4 *)(out + o0) = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
    else for (uint32_t q = 0; q < cnt; q++) out[o0 + q] = (uint8_t)((q < 8 ? w0 >> (8 * q) : w1 >> (8 * (q - 8))) & 0xffu);
}
