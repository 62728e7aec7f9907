// fasta_nuc.hip -- fasta_nuc on the device (gfx950): the interval table, the base counts and the finished columns.
// Included by dhts_api.hip after fasta_index.hip (FaRegion / fa_fetch make the seq column) and bed_text.hip (BedRows / bed_field).
//
// Restates src/interval_udf.c:629-836 on a batch of intervals:
//   next_fasta_nuc_bin_interval :684-726   -> nuc_bin_rows   (a closed form of the bin number, one lane per row)
//   next_fasta_nuc_bed_interval :651-682   -> nuc_bed_rows   (one lane per BED line of the delimiter table, then a scan and fq_compact)
//   faidx_adjust_position, htslib faidx.c:914-950, with end_adjust = 1 on (start, end - 1)   -> nuc_resolve
//   count_nucleotides :629-643, one faidx_fetch_seq64 per row :757                          -> nuc_count
//   pct_at / pct_gc :765-768 and the row's columns :771-826                                 -> nuc_finalize
//
// nuc_count divides the work by bases: interval i is cut into pieces of NUC_PIECE bases, the pieces of a batch are numbered by a scan over
// ceil(n_i / NUC_PIECE), a lane takes one piece.  It finds its interval by bisection, divides once for the first base's line and column,
// and then reads the source extent of its piece -- bases and the line terminators between them -- in whole aligned 16-byte loads.  A
// 16-bit mask says which bytes of a load are bases of the piece (inside the extent, column < line_blen); the five letters are recognised
// on the four words of the load at once ((c | 0x20) == 'a' is toupper(c) == 'A' in the C locale, for all 256 byte values), and a
// popcount of mask & hits is the count.  The five counts of a lane (<= NUC_PIECE each) sit in one 64-bit register, 12 bits apiece: a
// wave's 64 pieces hold at most 64 * NUC_PIECE = 3072 < 4096 bases, so the segmented reduction over the lanes of one interval cannot
// carry from one field into the next.  The pieces of an interval are contiguous, so the interval ids of a wave are sorted and the
// segmented reduction is a shuffle-down ladder that adds while the ids agree; the first lane of each run adds the five fields to the
// interval's 64-bit counters with atomicAdd.  Integer addition: the result does not depend on the order.
#pragma once

#define NUC_PIECE 48u
enum { NUC_N_COLS = 13, NUC_COL_CHROM = 0, NUC_COL_START = 1, NUC_COL_END = 2, NUC_COL_PCT_AT = 3, NUC_COL_NUM_A = 5, NUC_COL_NUM_OTHER = 10, NUC_COL_SEQ_LEN = 11, NUC_COL_SEQ = 12 };
enum { NUC_F_FETCHED = 1u, NUC_F_NAME_BED = 2u, NUC_F_NAME_VALID = 4u };

// one sequence of the loaded .fai.  src: where its first base lies in the resident text; avail: the bases of it the text holds (a file
// that ends early holds fewer than len); [lo, hi): the resident bytes a row of this sequence may touch (one staged window, or the text)
struct NucEnt { uint64_t len, avail; int64_t src; uint64_t lo, hi; uint32_t blen, llen, name_off, name_len; };
// one output row.  [beg, beg + n): the bases that are fetched; seq_len: the column (n, or end - start of a row that fetches nothing)
struct NucRow { long long start, end, seq_len; uint64_t beg, n; int64_t src; uint32_t blen, llen, name_off, name_len, flags, pad; };

// The row of (tid, start, end), or false when the reference emits none (interval_udf.c:750-769).  *err is set when the row's bases are not
// resident (a staged window that does not cover them).
__device__ __forceinline__ bool nuc_resolve(const NucEnt *__restrict__ ents, int32_t tid, long long start, long long end, NucRow &r, uint32_t *err) {
    r.start = start; r.end = end; r.beg = 0; r.n = 0; r.src = 0; r.blen = 1; r.llen = 1; r.pad = 0;
    const long long len = (long long)((unsigned long long)end - (unsigned long long)start);
    r.seq_len = len;
    if (len <= 0) return true;                                                   // emitted without any fetch: all counts 0, seq NULL
    if (tid < 0) return false;                                                   // faidx_adjust_position: "The sequence was not found"
    const NucEnt E = ents[tid];
    if (E.blen == 0) return false;                                               // fai_retrieve: "Invalid line length in index"
    const long long L = (long long)E.len;
    long long pb = start, pe = end - 1;                                          // pe >= pb here
    if (pb < 0) pb = 0; else if (L <= pb) pb = L;
    if (pe < 0) pe = 0; else if (L <= pe) pe = L - 1;
    const long long e1 = pe + 1;
    const uint64_t n = e1 > pb ? (uint64_t)(e1 - pb) : 0ull;
    if (n > 0 && (uint64_t)e1 > E.avail) return false;                           // fai_retrieve: "unexpected end of file"
    if (n > 0) {
        const uint64_t last = (uint64_t)e1 - 1;
        const int64_t sa = E.src + (int64_t)((uint64_t)pb / E.blen * E.llen + (uint64_t)pb % E.blen);
        const int64_t sb = E.src + (int64_t)(last / E.blen * E.llen + last % E.blen) + 1;
        if (sa < (int64_t)E.lo || sb > (int64_t)E.hi) { *err = 1u; return false; }
    }
    r.beg = (uint64_t)pb; r.n = n; r.src = E.src; r.blen = E.blen; r.llen = E.llen; r.seq_len = (long long)n; r.flags |= NUC_F_FETCHED;
    return true;
}

// Bins mode.  cum[s] = rows of the sequences in front of s (cum[nseq] = all); row g of sequence s is [beg0 + k * bw, min(.. + bw, end0)).
// With a region there is one "sequence": the region's, with its own [beg0, end0).
extern "C" __global__ void __launch_bounds__(256)
nuc_bin_rows(const NucEnt *__restrict__ ents, const uint64_t *__restrict__ cum, uint32_t nseq, int32_t region_tid, uint64_t beg0, uint64_t end0, uint64_t bw,
             uint64_t g0, uint32_t nrows, NucRow *__restrict__ rows, uint32_t *__restrict__ err) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= nrows) return;
    const uint64_t g = g0 + r;
    uint32_t lo = 0, hi = nseq;                                                  // the last s with cum[s] <= g (sequences without rows share a value)
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (cum[mid] <= g) lo = mid; else hi = mid; }
    const int32_t tid = region_tid >= 0 ? region_tid : (int32_t)lo;
    const uint64_t b = region_tid >= 0 ? beg0 : 0ull, e = region_tid >= 0 ? end0 : ents[tid].len;
    const uint64_t start = b + (g - cum[lo]) * bw;
    const uint64_t end = e - start < bw ? e : start + bw;
    NucRow o; o.flags = NUC_F_NAME_VALID; o.name_off = ents[tid].name_off; o.name_len = ents[tid].name_len;
    (void)nuc_resolve(ents, tid, (long long)start, (long long)end, o, err);      // (the host counted only rows that resolve)
    rows[r] = o;
}
// Intervals from host arrays: tid < 0 is a chrom the index does not know.
extern "C" __global__ void __launch_bounds__(256)
nuc_iv_rows(const NucEnt *__restrict__ ents, uint32_t nseq, const int32_t *__restrict__ tid, const long long *__restrict__ start, const long long *__restrict__ end, uint32_t n,
            NucRow *__restrict__ tmp, uint32_t *__restrict__ keep, uint32_t *__restrict__ err) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const int32_t t = (tid[i] >= 0 && (uint32_t)tid[i] < nseq) ? tid[i] : -1;
    NucRow o; o.flags = t >= 0 ? NUC_F_NAME_VALID : 0u; o.name_off = t >= 0 ? ents[t].name_off : 0u; o.name_len = t >= 0 ? ents[t].name_len : 0u;
    const bool k = nuc_resolve(ents, t, start[i], end[i], o, err);
    tmp[i] = o; keep[i] = k ? 1u : 0u;
}

// the names of the index as an open-addressed table: slot = tid + 1, 0 = empty; linear probing; the table is a power of two and at most
// half full.  FNV-1a over the name's bytes.
__host__ __device__ __forceinline__ uint32_t nuc_hash(const uint8_t *s, uint32_t n) { uint32_t h = 2166136261u; for (uint32_t k = 0; k < n; k++) h = (h ^ s[k]) * 16777619u; return h; }
__device__ __forceinline__ int32_t nuc_lookup(const NucEnt *__restrict__ ents, const uint8_t *__restrict__ names, const uint32_t *__restrict__ table, uint32_t mask, const uint8_t *s, uint32_t n) {
    for (uint32_t h = nuc_hash(s, n) & mask;; h = (h + 1) & mask) {
        const uint32_t v = table[h];
        if (v == 0) return -1;
        const NucEnt &E = ents[v - 1];
        if (E.name_len != n) continue;
        bool eq = true;
        for (uint32_t k = 0; eq && k < n; k++) eq = names[E.name_off + k] == s[k];
        if (eq) return (int32_t)(v - 1);
    }
}
struct NucBedArgs {
    BedRows L; const uint32_t *is_row; uint32_t nlines;
    const NucEnt *ents; const uint8_t *names; const uint32_t *table; uint32_t mask;
    int32_t region_tid; long long region_beg, region_end;                       // bed_overlap_region (interval_udf.c:645-649); region_tid < 0: no region
    NucRow *tmp; uint32_t *keep; uint32_t *err;
};
// BED mode: one lane per line of the batch.  is_row: 1 = a line of three or more fields that is no meta line (and lies in the tabix
// iterator's region where there is one); a line of fewer fields (2) is passed over here, as is one whose start or end strtoll does not
// consume whole.
extern "C" __global__ void __launch_bounds__(256)
nuc_bed_rows(NucBedArgs a) {
    const uint32_t li = blockIdx.x * 256u + threadIdx.x;
    if (li >= a.nlines) return;
    bool k = a.is_row[li] == 1u;
    NucRow o; memset(&o, 0, sizeof(o));
    if (k) {
        uint32_t s0 = 0, e0 = 0, s = 0, e = 0, adv = 0; long long st = 0, en = 0;
        (void)bed_field(a.L, li, 0, false, s0, e0);
        k = bed_field(a.L, li, 1, false, s, e) && e > s;
        if (k) { st = vcf_strtoll(a.L.u, s, e, 10, &adv); k = adv == e - s; }
        k = k && bed_field(a.L, li, 2, false, s, e) && e > s;
        if (k) { en = vcf_strtoll(a.L.u, s, e, 10, &adv); k = adv == e - s; }
        if (k) {
            const int32_t tid = nuc_lookup(a.ents, a.names, a.table, a.mask, a.L.u + s0, e0 - s0);
            if (a.region_tid >= 0) k = tid == a.region_tid && en > a.region_beg && st < a.region_end;
            o.flags = NUC_F_NAME_BED | NUC_F_NAME_VALID; o.name_off = s0; o.name_len = e0 - s0;
            if (k) k = nuc_resolve(a.ents, tid, st, en, o, a.err);
        }
    }
    a.tmp[li] = o; a.keep[li] = k ? 1u : 0u;
}
// rows[r] = tmp[src[r]] (src: fq_compact's list of the kept entries); per row the pieces nuc_count cuts it into, the bytes of its chrom and
// of its seq
extern "C" __global__ void __launch_bounds__(256)
nuc_gather_rows(const NucRow *__restrict__ tmp, const uint32_t *__restrict__ src, uint32_t nrows, NucRow *__restrict__ rows) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r < nrows) rows[r] = tmp[src[r]];
}
extern "C" __global__ void __launch_bounds__(256)
nuc_measure(const NucRow *__restrict__ rows, uint32_t nrows, uint32_t *__restrict__ npieces, uint32_t *__restrict__ name_len, uint32_t *__restrict__ seq_len, uint32_t *__restrict__ big) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= nrows) return;
    const NucRow R = rows[r];
    npieces[r] = (uint32_t)((R.n + NUC_PIECE - 1) / NUC_PIECE);
    name_len[r] = (R.flags & NUC_F_NAME_VALID) ? R.name_len : 0u;
    seq_len[r] = (uint32_t)R.n;
    if (R.n >> 32) *big = 1u;                                                    // (a VARCHAR arena has 32-bit offsets)
}

// bit k: byte k of w (with bit 5 set) is the letter `pat` repeats -- the exact zero-byte test of bed_eq4
__device__ __forceinline__ uint32_t nuc_eq16(const uint4 v, uint32_t pat) {
    const uint32_t c = 0x20202020u;
    return bed_eq4(v.x | c, pat) | bed_eq4(v.y | c, pat) << 4 | bed_eq4(v.z | c, pat) << 8 | bed_eq4(v.w | c, pat) << 12;
}
// piece_off[i] = pieces in front of row i (piece_off[nrows] = total); counts[5 * i + (0..4)] = A, C, G, T, N of row i, zeroed by the caller.
// text + every row's source extent lies in an allocation that is 16-byte aligned at its base and padded behind its end (DevBuf, PAD_BYTES).
extern "C" __global__ void __launch_bounds__(256)
nuc_count(const uint8_t *__restrict__ text, const NucRow *__restrict__ rows, const uint64_t *__restrict__ piece_off, uint32_t nrows, uint64_t total,
          unsigned long long *__restrict__ counts) {
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t iv = 0xffffffffu; unsigned long long packed = 0;
    if (p < total) {
        uint32_t lo = 0, hi = nrows;                                            // the last row with piece_off <= p: the one that owns piece p
        while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (piece_off[mid] <= p) lo = mid; else hi = mid; }
        iv = lo;
        const NucRow R = rows[lo];
        const uint64_t i0 = (p - piece_off[lo]) * NUC_PIECE;                   // first base of the piece inside the row
        const uint32_t cnt = R.n - i0 < NUC_PIECE ? (uint32_t)(R.n - i0) : NUC_PIECE;
        const uint64_t pos = R.beg + i0, line = pos / R.blen;
        uint32_t col = (uint32_t)(pos - line * R.blen);                         // column of the next byte in its line: < blen a base, else a terminator
        const uint64_t last = pos + cnt - 1, lline = last / R.blen;
        const uint8_t *sa = text + R.src + (int64_t)(line * R.llen + col);
        const uint8_t *sb = text + R.src + (int64_t)(lline * R.llen + (last - lline * R.blen)) + 1;
        const uint8_t *w = (const uint8_t *)((uintptr_t)sa & ~(uintptr_t)15);
        uint32_t k = (uint32_t)(sa - w);                                        // first byte of the extent inside the first load
        uint32_t na = 0, nc = 0, ng = 0, nt = 0, nn = 0;
        for (; w < sb; w += 16, k = 0) {
            const uint32_t kend = sb - w < 16 ? (uint32_t)(sb - w) : 16u;
            uint32_t m = 0;                                                     // runs of bases and of terminator columns, alternating
            while (k < kend) {
                if (col < R.blen) { uint32_t run = R.blen - col; if (run > kend - k) run = kend - k; m |= ((1u << run) - 1u) << k; k += run; col += run; }
                else { uint32_t skip = R.llen - col; if (skip > kend - k) skip = kend - k; k += skip; col += skip; }
                if (col == R.llen) col = 0;
            }
            const uint4 v = *(const uint4 *)w;
            na += __popc(m & nuc_eq16(v, 0x61616161u)); nc += __popc(m & nuc_eq16(v, 0x63636363u)); ng += __popc(m & nuc_eq16(v, 0x67676767u));
            nt += __popc(m & nuc_eq16(v, 0x74747474u)); nn += __popc(m & nuc_eq16(v, 0x6e6e6e6eu));
        }
        packed = (unsigned long long)na | (unsigned long long)nc << 12 | (unsigned long long)ng << 24 | (unsigned long long)nt << 36 | (unsigned long long)nn << 48;
    }
    // segmented reduction towards the first lane of each run of equal rows (idle lanes behind the last piece are a run of their own)
    const uint32_t prev = __shfl_up(iv, 1, 64);
    const bool head = lane == 0 || prev != iv;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long t = __shfl_down(packed, d, 64); const uint32_t tiv = __shfl_down(iv, d, 64);
        if (lane + d < 64u && tiv == iv) packed += t;
    }
    if (head && iv != 0xffffffffu) {
#pragma unroll
        for (int f = 0; f < 5; f++) { const unsigned long long c = (packed >> (12 * f)) & 0xfffull; if (c) atomicAdd(&counts[5ull * iv + f], c); }
    }
}

// The columns of a batch, one lane per row.  fixed[id] (ids 1..11) is null where the column is not projected; counts is null when no
// column that needs them is.
struct NucOut { void *fixed[NUC_N_COLS]; uint8_t *ones; uint8_t *name_valid, *seq_valid; };
extern "C" __global__ void __launch_bounds__(256)
nuc_finalize(const NucRow *__restrict__ rows, uint32_t nrows, const unsigned long long *__restrict__ counts, NucOut o) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= nrows) return;
    const NucRow R = rows[r];
    long long c[5] = {0, 0, 0, 0, 0};
    if (counts) for (int f = 0; f < 5; f++) c[f] = (long long)counts[5ull * r + f];
    const long long sl = R.seq_len;
    const long long other = (R.flags & NUC_F_FETCHED) ? sl - (c[0] + c[1] + c[2] + c[3] + c[4]) : 0;
    double at = 0.0, gc = 0.0;
    if ((R.flags & NUC_F_FETCHED) && sl > 0) { at = (double)(c[0] + c[3]) / (double)sl; gc = (double)(c[1] + c[2]) / (double)sl; }   // interval_udf.c:765-768
    if (o.fixed[1]) ((long long *)o.fixed[1])[r] = R.start;
    if (o.fixed[2]) ((long long *)o.fixed[2])[r] = R.end;
    if (o.fixed[3]) ((double *)o.fixed[3])[r] = at;
    if (o.fixed[4]) ((double *)o.fixed[4])[r] = gc;
    for (int f = 0; f < 5; f++) if (o.fixed[5 + f]) ((long long *)o.fixed[5 + f])[r] = c[f];
    if (o.fixed[10]) ((long long *)o.fixed[10])[r] = other;
    if (o.fixed[11]) ((long long *)o.fixed[11])[r] = sl;
    o.ones[r] = 1;
    if (o.name_valid) o.name_valid[r] = (R.flags & NUC_F_NAME_VALID) ? 1 : 0;
    if (o.seq_valid) o.seq_valid[r] = (R.flags & NUC_F_FETCHED) ? 1 : 0;
}
// chrom: the name's bytes from the index's names or from the BED text
extern "C" __global__ void __launch_bounds__(256)
nuc_names(const NucRow *__restrict__ rows, uint32_t nrows, const uint8_t *__restrict__ idx_names, const uint8_t *__restrict__ bed_text, const uint32_t *__restrict__ off, uint8_t *__restrict__ out) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= nrows) return;
    const NucRow R = rows[r];
    if (!(R.flags & NUC_F_NAME_VALID)) return;
    const uint8_t *s = ((R.flags & NUC_F_NAME_BED) ? bed_text : idx_names) + R.name_off; uint8_t *d = out + off[r];
    for (uint32_t k = 0; k < R.name_len; k++) d[k] = s[k];
}
// the seq column is fa_fetch's: its region list from the rows
extern "C" __global__ void __launch_bounds__(256)
nuc_fetch_regions(const NucRow *__restrict__ rows, uint32_t nrows, const uint64_t *__restrict__ seq_off, FaRegion *__restrict__ rg) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= nrows) return;
    const NucRow R = rows[r];
    FaRegion g; g.out_off = seq_off[r]; g.n = R.n; g.beg = R.beg; g.src = R.src; g.blen = R.blen; g.llen = R.llen;
    rg[r] = g;
}
