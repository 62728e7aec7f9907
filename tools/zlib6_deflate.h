/*
 * zlib6_deflate.h -- raw deflate that writes the same bytes as zlib 1.2.11's deflate() at level 6 (windowBits -15, memLevel 8,
 * Z_DEFAULT_STRATEGY) for one input of at most 65,280 bytes fed whole with Z_FINISH: the case of one BGZF block of the synthetic
 * workload.  A restatement of deflate.c (deflate_slow, longest_match, fill_window's slide) and trees.c (_tr_tally, build_tree,
 * gen_bitlen, gen_codes, scan_tree / send_tree, build_bl_tree, _tr_flush_block, compress_block, _tr_stored_block); compiled
 * for the host (tests compare it with libz) and for the device (synth_gpu.hip).
 *
 * The work is split in three phases so that the expensive one runs a thread per input position:
 *   1. zd_chain: every position p <= n-3 is inserted into the hash chains exactly once and in order (deflate_slow inserts the
 *      positions inside a match too), so the head INSERT_STRING reads at p -- prev[p] -- is a function of the input alone;
 *   2. zd_match_pair: longest_match at p depends on the parse only through prev_length (its starting best_len and, at >= 8, a
 *      chain budget of 32 instead of 128).  Where the lookahead is >= 16 the nice length exceeds any prev_length it is called
 *      with (< 16), so its answer is "the first candidate of the longest match among the first 32 / 128 of the chain" when that
 *      length exceeds prev_length, else prev_length: both budgets are computed for every such position;
 *   3. zd_parse: deflate_slow's lazy parse reads those answers (and runs longest_match itself in the last 15 positions), then
 *      trees.c builds and sends the blocks.
 *
 * Level 6: good_length 8, max_lazy 16, nice_length 128, max_chain 128.  Positions are absolute offsets into the block; the one
 * effect of zlib's window slide (at strstart >= 65,274 when the input is 65,280 bytes) that shows in the output is reproduced:
 * afterwards a hash head at position <= 32,768 reads as NIL, and a block that started below 32,768 can no longer be stored.
 * Bytes past the end of the input never change zlib's output (a match is cut to the lookahead, and where a longer one would
 * win on bytes past the end the previous match is emitted anyway), so comparisons stop at the end of the input.
 */
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define ZD_FN __host__ __device__ static inline
#else
#define ZD_FN static inline
#endif

#define ZD_WSIZE 32768u
#define ZD_MAX_DIST (ZD_WSIZE - 262u)      /* MAX_DIST(s) = w_size - MIN_LOOKAHEAD */
#define ZD_MIN_LOOKAHEAD 262u
#define ZD_HASH_MASK 32767u
#define ZD_LIT_BUFSIZE 16384u               /* 1 << (memLevel + 6): a block ends after lit_bufsize - 1 symbols */
#define ZD_HEAP_SIZE 573                     /* 2 * L_CODES + 1 */
#define ZD_MAX_IN 65280u
#define ZD_OUT_CAP (65536u - 18u - 8u)       /* the output room bgzf_block gives deflate(); more means "store the block instead" */

/* per-block scratch of the parse (global memory on the device) */
typedef struct {
    uint32_t sym[ZD_LIT_BUFSIZE];            /* (dist << 8) | lc; dist 0 = literal lc */
    uint32_t freq[ZD_HEAP_SIZE], dad[ZD_HEAP_SIZE];
    uint16_t len[ZD_HEAP_SIZE], code[ZD_HEAP_SIZE];
    uint32_t dfreq[61], ddad[61];
    uint16_t dlen[61], dcode[61];
    uint32_t bfreq[39], bdad[39];
    uint16_t blen[39], bcode[39];
    int heap[ZD_HEAP_SIZE];
    uint8_t depth[ZD_HEAP_SIZE];
    uint16_t bl_count[16];
} zd_ws;

typedef struct { uint32_t *freq, *dad; uint16_t *len, *code; int elems, base, max_length, max_code, kind; } zd_tree;   /* kind 0 lit/len, 1 dist, 2 bl */

typedef struct {
    uint8_t *out; uint32_t pos; uint64_t acc; uint32_t nb; int overflow;
} zd_bits;

ZD_FN void zd_put_bits(zd_bits *b, uint32_t v, uint32_t n) {
    b->acc |= (uint64_t)v << b->nb; b->nb += n;
    while (b->nb >= 8) {
        if (b->pos < ZD_OUT_CAP) b->out[b->pos] = (uint8_t)b->acc; else b->overflow = 1;
        b->pos++; b->acc >>= 8; b->nb -= 8;
    }
}
ZD_FN void zd_windup(zd_bits *b) { if (b->nb) zd_put_bits(b, 0, 8 - b->nb); }
ZD_FN uint32_t zd_rev(uint32_t code, int len) { uint32_t r = 0; do { r |= code & 1; code >>= 1; r <<= 1; } while (--len > 0); return r >> 1; }

ZD_FN int zd_extra_lbits(int c) { return c < 8 || c == 28 ? 0 : (c - 4) >> 2; }
ZD_FN int zd_base_length(int c) { return c < 8 ? c : (4 | (c & 3)) << ((c - 4) >> 2); }      /* code 28 (length 258) has no extra bits */
ZD_FN int zd_extra_dbits(int c) { return c < 4 ? 0 : (c >> 1) - 1; }
ZD_FN int zd_base_dist(int c) { return c < 4 ? c : (2 + (c & 1)) << ((c >> 1) - 1); }
ZD_FN int zd_extra_blbits(int c) { return c == 16 ? 2 : c == 17 ? 3 : c == 18 ? 7 : 0; }
/* _length_code[lc], lc = length - 3 */
ZD_FN int zd_length_code(int lc) {
    if (lc == 255) return 28;
    if (lc < 8) return lc;
    int hb = 31 - __builtin_clz((unsigned)lc), eb = hb - 2;
    return (eb << 2) + ((lc >> eb) & 3) + 4;
}
/* d_code(dist), dist = distance - 1 */
ZD_FN int zd_d_code(uint32_t d) {
    if (d < 4) return (int)d;
    int hb = 31 - __builtin_clz(d), eb = hb - 1;
    return (eb << 1) + (int)((d >> eb) & 1u) + 2;
}
ZD_FN int zd_static_llen(int n) { return n < 144 ? 8 : n < 256 ? 9 : n < 280 ? 7 : 8; }
ZD_FN uint32_t zd_static_lcode(int n) {        /* gen_codes over the static lengths */
    if (n < 144) return zd_rev(0x30u + (uint32_t)n, 8);
    if (n < 256) return zd_rev(0x190u + (uint32_t)(n - 144), 9);
    if (n < 280) return zd_rev((uint32_t)(n - 256), 7);
    return zd_rev(0xc0u + (uint32_t)(n - 280), 8);
}
ZD_FN int zd_stree_len(const zd_tree *t, int n) { return t->kind == 0 ? zd_static_llen(n) : 5; }
ZD_FN int zd_xbits(const zd_tree *t, int n) {
    if (n < t->base) return 0;
    int k = n - t->base;
    return t->kind == 0 ? zd_extra_lbits(k) : t->kind == 1 ? zd_extra_dbits(k) : zd_extra_blbits(k);
}

#define ZD_SMALLER(t, n, m, depth) ((t)->freq[n] < (t)->freq[m] || ((t)->freq[n] == (t)->freq[m] && (depth)[n] <= (depth)[m]))

ZD_FN void zd_pqdownheap(zd_ws *w, const zd_tree *t, int heap_len, int k) {
    int v = w->heap[k], j = k << 1;
    while (j <= heap_len) {
        if (j < heap_len && ZD_SMALLER(t, w->heap[j + 1], w->heap[j], w->depth)) j++;
        if (ZD_SMALLER(t, v, w->heap[j], w->depth)) break;
        w->heap[k] = w->heap[j]; k = j; j <<= 1;
    }
    w->heap[k] = v;
}

ZD_FN void zd_build_tree(zd_ws *w, zd_tree *t, uint64_t *opt_len, uint64_t *static_len) {
    int elems = t->elems, n, m, max_code = -1, node, heap_len = 0, heap_max = ZD_HEAP_SIZE;
    for (n = 0; n < elems; n++) {
        if (t->freq[n] != 0) { w->heap[++heap_len] = max_code = n; w->depth[n] = 0; }
        else t->len[n] = 0;
    }
    while (heap_len < 2) {
        node = w->heap[++heap_len] = (max_code < 2 ? ++max_code : 0);
        t->freq[node] = 1; w->depth[node] = 0;
        (*opt_len)--; if (t->kind != 2) *static_len -= (uint64_t)zd_stree_len(t, node);
    }
    t->max_code = max_code;
    for (n = heap_len / 2; n >= 1; n--) zd_pqdownheap(w, t, heap_len, n);
    node = elems;
    do {
        n = w->heap[1]; w->heap[1] = w->heap[heap_len--]; zd_pqdownheap(w, t, heap_len, 1);
        m = w->heap[1];
        w->heap[--heap_max] = n; w->heap[--heap_max] = m;
        t->freq[node] = t->freq[n] + t->freq[m];
        w->depth[node] = (uint8_t)((w->depth[n] >= w->depth[m] ? w->depth[n] : w->depth[m]) + 1);
        t->dad[n] = t->dad[m] = (uint32_t)node;
        w->heap[1] = node++;
        zd_pqdownheap(w, t, heap_len, 1);
    } while (heap_len >= 2);
    w->heap[--heap_max] = w->heap[1];

    /* gen_bitlen */
    int h, bits, xbits, overflow = 0, max_length = t->max_length;
    for (bits = 0; bits <= 15; bits++) w->bl_count[bits] = 0;
    t->len[w->heap[heap_max]] = 0;
    for (h = heap_max + 1; h < ZD_HEAP_SIZE; h++) {
        n = w->heap[h];
        bits = t->len[t->dad[n]] + 1;
        if (bits > max_length) { bits = max_length; overflow++; }
        t->len[n] = (uint16_t)bits;
        if (n > max_code) continue;
        w->bl_count[bits]++;
        xbits = zd_xbits(t, n);
        uint64_t f = t->freq[n];
        *opt_len += f * (uint64_t)(bits + xbits);
        if (t->kind != 2) *static_len += f * (uint64_t)(zd_stree_len(t, n) + xbits);
    }
    if (overflow) {
        do {
            bits = max_length - 1;
            while (w->bl_count[bits] == 0) bits--;
            w->bl_count[bits]--; w->bl_count[bits + 1] += 2; w->bl_count[max_length]--;
            overflow -= 2;
        } while (overflow > 0);
        for (bits = max_length; bits != 0; bits--) {
            n = w->bl_count[bits];
            while (n != 0) {
                m = w->heap[--h];
                if (m > max_code) continue;
                if ((unsigned)t->len[m] != (unsigned)bits) { *opt_len += ((uint64_t)bits - t->len[m]) * t->freq[m]; t->len[m] = (uint16_t)bits; }
                n--;
            }
        }
    }
    /* gen_codes */
    uint32_t next_code[16], code = 0;
    for (bits = 1; bits <= 15; bits++) { code = (code + w->bl_count[bits - 1]) << 1; next_code[bits] = code; }
    for (n = 0; n <= max_code; n++) {
        int l = t->len[n];
        if (l == 0) continue;
        t->code[n] = (uint16_t)zd_rev(next_code[l]++, l);
    }
}

/* tree[n + 1].Len with scan_tree's guard tree[max_code + 1].Len = 0xffff */
ZD_FN int zd_next_len(const zd_tree *t, int n, int max_code) { return n + 1 > max_code ? 0xffff : t->len[n + 1]; }

ZD_FN void zd_scan_tree(zd_tree *bl, const zd_tree *t, int max_code) {
    int n, prevlen = -1, curlen, nextlen = t->len[0], count = 0, max_count = 7, min_count = 4;
    if (nextlen == 0) { max_count = 138; min_count = 3; }
    for (n = 0; n <= max_code; n++) {
        curlen = nextlen; nextlen = zd_next_len(t, n, max_code);
        if (++count < max_count && curlen == nextlen) continue;
        else if (count < min_count) bl->freq[curlen] += (uint32_t)count;
        else if (curlen != 0) { if (curlen != prevlen) bl->freq[curlen]++; bl->freq[16]++; }
        else if (count <= 10) bl->freq[17]++;
        else bl->freq[18]++;
        count = 0; prevlen = curlen;
        if (nextlen == 0) { max_count = 138; min_count = 3; }
        else if (curlen == nextlen) { max_count = 6; min_count = 3; }
        else { max_count = 7; min_count = 4; }
    }
}

ZD_FN void zd_send_code(zd_bits *b, const zd_tree *t, int c) { zd_put_bits(b, t->code[c], t->len[c]); }

ZD_FN void zd_send_tree(zd_bits *b, const zd_tree *bl, const zd_tree *t, int max_code) {
    int n, prevlen = -1, curlen, nextlen = t->len[0], count = 0, max_count = 7, min_count = 4;
    if (nextlen == 0) { max_count = 138; min_count = 3; }
    for (n = 0; n <= max_code; n++) {
        curlen = nextlen; nextlen = zd_next_len(t, n, max_code);
        if (++count < max_count && curlen == nextlen) continue;
        else if (count < min_count) { do { zd_send_code(b, bl, curlen); } while (--count != 0); }
        else if (curlen != 0) {
            if (curlen != prevlen) { zd_send_code(b, bl, curlen); count--; }
            zd_send_code(b, bl, 16); zd_put_bits(b, (uint32_t)(count - 3), 2);
        } else if (count <= 10) { zd_send_code(b, bl, 17); zd_put_bits(b, (uint32_t)(count - 3), 3); }
        else { zd_send_code(b, bl, 18); zd_put_bits(b, (uint32_t)(count - 11), 7); }
        count = 0; prevlen = curlen;
        if (nextlen == 0) { max_count = 138; min_count = 3; }
        else if (curlen == nextlen) { max_count = 6; min_count = 3; }
        else { max_count = 7; min_count = 4; }
    }
}

ZD_FN void zd_init_block(zd_tree *lt, zd_tree *dt, zd_tree *bt) {
    for (int n = 0; n < 286; n++) lt->freq[n] = 0;
    for (int n = 0; n < 30; n++) dt->freq[n] = 0;
    for (int n = 0; n < 19; n++) bt->freq[n] = 0;
    lt->freq[256] = 1;                                        /* END_BLOCK */
}

/* _tr_flush_block: the block's symbols sym[0, nsym), its input src[0, stored_len) (src = 0: not available -> never stored) */
ZD_FN void zd_flush_block(zd_ws *w, zd_bits *b, zd_tree *lt, zd_tree *dt, zd_tree *bt, uint32_t nsym, const uint8_t *src, uint32_t stored_len, int last) {
    uint64_t opt_len = 0, static_len = 0;
    zd_build_tree(w, lt, &opt_len, &static_len);
    zd_build_tree(w, dt, &opt_len, &static_len);
    zd_scan_tree(bt, lt, lt->max_code);
    zd_scan_tree(bt, dt, dt->max_code);
    zd_build_tree(w, bt, &opt_len, &static_len);
    static const uint8_t bl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    int max_blindex;
    for (max_blindex = 18; max_blindex >= 3; max_blindex--) if (bt->len[bl_order[max_blindex]] != 0) break;
    opt_len += 3 * ((uint64_t)max_blindex + 1) + 5 + 5 + 4;
    uint64_t opt_lenb = (opt_len + 3 + 7) >> 3, static_lenb = (static_len + 3 + 7) >> 3;
    if (static_lenb <= opt_lenb) opt_lenb = static_lenb;
    if ((uint64_t)stored_len + 4 <= opt_lenb && src) {
        zd_put_bits(b, (uint32_t)last, 3);
        zd_windup(b);
        zd_put_bits(b, stored_len & 0xffffu, 16); zd_put_bits(b, ~stored_len & 0xffffu, 16);
        for (uint32_t i = 0; i < stored_len; i++) zd_put_bits(b, src[i], 8);
    } else {
        int fixed = static_lenb == opt_lenb;
        zd_put_bits(b, ((fixed ? 1u : 2u) << 1) + (uint32_t)last, 3);
        if (!fixed) {
            int lcodes = lt->max_code + 1, dcodes = dt->max_code + 1, blcodes = max_blindex + 1;
            zd_put_bits(b, (uint32_t)(lcodes - 257), 5); zd_put_bits(b, (uint32_t)(dcodes - 1), 5); zd_put_bits(b, (uint32_t)(blcodes - 4), 4);
            for (int r = 0; r < blcodes; r++) zd_put_bits(b, bt->len[bl_order[r]], 3);
            zd_send_tree(b, bt, lt, lcodes - 1);
            zd_send_tree(b, bt, dt, dcodes - 1);
        }
        for (uint32_t i = 0; i < nsym; i++) {
            uint32_t s = w->sym[i], dist = s >> 8;
            int lc = (int)(s & 0xff);
            if (dist == 0) {
                if (fixed) zd_put_bits(b, zd_static_lcode(lc), (uint32_t)zd_static_llen(lc)); else zd_send_code(b, lt, lc);
            } else {
                int c = zd_length_code(lc);
                if (fixed) zd_put_bits(b, zd_static_lcode(c + 257), (uint32_t)zd_static_llen(c + 257)); else zd_send_code(b, lt, c + 257);
                int e = zd_extra_lbits(c);
                if (e) zd_put_bits(b, (uint32_t)(lc - zd_base_length(c)), (uint32_t)e);
                dist--;
                c = zd_d_code(dist);
                if (fixed) zd_put_bits(b, zd_rev((uint32_t)c, 5), 5); else zd_send_code(b, dt, c);
                e = zd_extra_dbits(c);
                if (e) zd_put_bits(b, dist - (uint32_t)zd_base_dist(c), (uint32_t)e);
            }
        }
        if (fixed) zd_put_bits(b, zd_static_lcode(256), 7); else zd_send_code(b, lt, 256);
    }
    zd_init_block(lt, dt, bt);
    if (last) zd_windup(b);
}

ZD_FN uint32_t zd_hash(const uint8_t *win, uint32_t p) { return (((uint32_t)win[p] << 10) ^ ((uint32_t)win[p + 1] << 5) ^ win[p + 2]) & ZD_HASH_MASK; }

/* phase 1: prev[p] (p <= n-3) = the last q < p with the same hash, 0 = none (position 0 reads as NIL in zlib too); head: 32768 entries */
ZD_FN void zd_chain(uint16_t *head, const uint8_t *win, uint32_t n, uint16_t *prev) {
    for (uint32_t i = 0; i < 32768; i++) head[i] = 0;
    for (uint32_t p = 0; p + 3 <= n; p++) {
        uint32_t h = zd_hash(win, p);
        prev[p] = head[h];
        head[h] = (uint16_t)p;
    }
}

/* phase 2, at p with lookahead n - p >= 16: (length << 16) | distance of longest_match's answer with a budget of 128 and of 32
 * candidates, best_len starting below any match; 0 = no hash head in reach or no match of length >= 3 */
ZD_FN void zd_match_pair(const uint8_t *win, uint32_t n, const uint16_t *prev, uint32_t p, uint32_t *m128, uint32_t *m32) {
    const uint32_t lookahead = n - p;
    uint32_t cur = prev[p];
    *m128 = *m32 = 0;
    if (cur == 0 || p - cur > ZD_MAX_DIST) return;
    const uint32_t limit = p > ZD_MAX_DIST ? p - ZD_MAX_DIST : 0;
    const uint32_t maxlen = lookahead < 258u ? lookahead : 258u, nice = lookahead < 128u ? lookahead : 128u;
    const uint8_t *scan = win + p;
    uint32_t best = 2, bpos = 0, k = 0;
    int snap = 0;
    for (;;) {
        const uint8_t *match = win + cur;
        int stop = 0;
        if (match[best] == scan[best] && match[best - 1] == scan[best - 1] && match[0] == scan[0] && match[1] == scan[1]) {
            uint32_t len = 2;
            while (len < maxlen && match[len] == scan[len]) len++;
            if (len > best) { best = len; bpos = cur; stop = len >= nice; }
        }
        if (++k == 32 && !stop) { *m32 = best > 2 ? (best << 16) | (p - bpos) : 0; snap = 1; }
        if (stop || k == 128) break;
        cur = prev[cur];
        if (cur <= limit) break;
    }
    *m128 = best > 2 ? (best << 16) | (p - bpos) : 0;
    if (!snap) *m32 = *m128;
}

/* longest_match run live (the last positions of a block, lookahead < 16): chain over the absolute prev[] of phase 1 */
ZD_FN uint32_t zd_longest_match(const uint8_t *win, const uint16_t *prev, uint32_t strstart, uint32_t lookahead, uint32_t prev_length,
                                uint32_t cur_match, uint32_t *match_start) {
    uint32_t chain_length = 128, best_len = prev_length, nice_match = 128;
    uint32_t limit = strstart > ZD_MAX_DIST ? strstart - ZD_MAX_DIST : 0;
    uint32_t maxlen = lookahead < 258u ? lookahead : 258u;
    const uint8_t *scan = win + strstart;
    if (prev_length >= 8) chain_length >>= 2;
    if (nice_match > lookahead) nice_match = lookahead;
    do {
        const uint8_t *match = win + cur_match;
        if (best_len < maxlen && (match[best_len] != scan[best_len] || match[best_len - 1] != scan[best_len - 1] || match[0] != scan[0] || match[1] != scan[1]))
            continue;
        uint32_t len = 2;
        while (len < maxlen && match[len] == scan[len]) len++;
        if (len > best_len) {
            *match_start = cur_match;
            best_len = len;
            if (len >= nice_match) break;
        }
    } while ((cur_match = prev[cur_match]) > limit && --chain_length != 0);
    return best_len <= lookahead ? best_len : lookahead;
}

/* phase 3: deflate_slow over win[0, n) with Z_FINISH, from prev[] (phase 1) and m128[] / m32[] (phase 2, read where n - p >= 16);
 * out: ZD_OUT_CAP bytes.  Returns the compressed size, or 0 when it does not fit (the caller stores the block, as bgzf_block does). */
ZD_FN uint32_t zd_parse(zd_ws *w, const uint8_t *win, uint32_t n, const uint16_t *prev, const uint32_t *m128, const uint32_t *m32, uint8_t *out) {
    zd_tree lt = {w->freq, w->dad, w->len, w->code, 286, 257, 15, 0, 0};
    zd_tree dt = {w->dfreq, w->ddad, w->dlen, w->dcode, 30, 0, 15, 0, 1};
    zd_tree bt = {w->bfreq, w->bdad, w->blen, w->bcode, 19, 0, 7, 0, 2};
    zd_bits b = {out, 0, 0, 0, 0};
    zd_init_block(&lt, &dt, &bt);
    uint32_t strstart = 0, lookahead = n, block_start = 0, nsym = 0;
    uint32_t match_length = 2, prev_length, match_start = 0, prev_match, match_available = 0;
    uint32_t nil_floor = 0; int slid = 0;
#define ZD_FLUSH(last) do { zd_flush_block(w, &b, &lt, &dt, &bt, nsym, (slid && block_start < ZD_WSIZE) ? (const uint8_t *)0 : win + block_start, \
                                           strstart - block_start, last); nsym = 0; block_start = strstart; } while (0)
#define ZD_TALLY_LIT(c) (w->sym[nsym++] = (uint32_t)(c), lt.freq[(c)]++, nsym == ZD_LIT_BUFSIZE - 1)
    for (;;) {
        if (lookahead < ZD_MIN_LOOKAHEAD) {
            if (!slid && strstart >= ZD_WSIZE + ZD_MAX_DIST) { slid = 1; nil_floor = ZD_WSIZE; }    /* fill_window's slide */
            if (lookahead == 0) break;
        }
        uint32_t hash_head = 0;
        if (lookahead >= 3) {
            hash_head = prev[strstart];
            if (hash_head <= nil_floor) hash_head = 0;
        }
        prev_length = match_length; prev_match = match_start;
        match_length = 2;
        if (hash_head != 0 && prev_length < 16 && strstart - hash_head <= ZD_MAX_DIST) {
            if (lookahead >= 16) {
                const uint32_t t = prev_length >= 8 ? m32[strstart] : m128[strstart];
                if ((t >> 16) > prev_length) { match_length = t >> 16; match_start = strstart - (t & 0xffffu); }
                else match_length = prev_length;
            } else {
                match_length = zd_longest_match(win, prev, strstart, lookahead, prev_length, hash_head, &match_start);
            }
            if (match_length <= 5 && match_length == 3 && strstart - match_start > 4096) match_length = 2;
        }
        if (prev_length >= 3 && match_length <= prev_length) {
            uint32_t dist = strstart - 1 - prev_match, lc = prev_length - 3;
            w->sym[nsym++] = (dist << 8) | lc;
            lt.freq[zd_length_code((int)lc) + 257]++;
            dt.freq[zd_d_code(dist - 1)]++;
            int bflush = nsym == ZD_LIT_BUFSIZE - 1;
            lookahead -= prev_length - 1;
            strstart += prev_length - 1;                   /* the positions inside the match were inserted by phase 1 */
            match_available = 0;
            match_length = 2;
            if (bflush) ZD_FLUSH(0);
        } else if (match_available) {
            if (ZD_TALLY_LIT(win[strstart - 1])) ZD_FLUSH(0);
            strstart++;
            lookahead--;
        } else {
            match_available = 1;
            strstart++;
            lookahead--;
        }
    }
    if (match_available) { (void)ZD_TALLY_LIT(win[strstart - 1]); }
    ZD_FLUSH(1);
#undef ZD_FLUSH
#undef ZD_TALLY_LIT
    return b.overflow || b.pos >= ZD_OUT_CAP ? 0u : b.pos;     /* zlib ends with avail_out == 0 -> not Z_STREAM_END */
}
