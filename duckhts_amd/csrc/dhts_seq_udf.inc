// dhts_seq_udf.inc -- part of dhts_api.hip (included there, inside its extern "C" block; not a translation unit of its own):
// the seq_* / cigar_* / SAM flag functions of src/kmer_udf.c on device columns (kernels: seq_udf.hip).  Arguments are device columns --
// a batch's own, or host values brought over by dhts_udf_upload -- results stay on the device until dhts_udf_fetch.
static const char *const UDF_NAMES[DHTS_UDF_OP_COUNT] = {
    "seq_revcomp", "seq_canonical", "seq_hash_2bit", "seq_encode_4bit", "seq_decode_4bit", "seq_gc_content",
    "cigar_has_soft_clip", "cigar_has_hard_clip", "cigar_left_soft_clip", "cigar_right_soft_clip", "cigar_query_length", "cigar_aligned_query_length",
    "cigar_reference_length", "cigar_has_op", "sam_flag_bits", "sam_flag_has", "is_forward_aligned",
    "is_paired", "is_proper_pair", "is_unmapped", "is_next_segment_unmapped", "is_reverse_complemented", "is_next_segment_reverse_complemented",
    "is_first_segment", "is_last_segment", "is_secondary", "is_qc_fail", "is_duplicate", "is_supplementary"};
static const int64_t UDF_MAX_ROWS = 0x7fffff00ll;
static uint64_t udf_pad8(uint64_t n) { return (n + 7) & ~7ull; }
static bool udf_width_ok(int w) { return w == 1 || w == -1 || w == 2 || w == -2 || w == 4 || w == -4 || w == 8 || w == -8; }

int dhts_udf_upload(dhts_ctx *c, int slot, const dhts_udf_arg *h, int64_t n_rows, dhts_udf_arg *dev) {
    if (!c || !h || !dev) return c ? fail(c, "udf: upload without a column") : -1;
    if (slot < 0 || slot > 1) return fail(c, "udf: argument slot %d (0 or 1)", slot);
    if (n_rows < 0 || n_rows > UDF_MAX_ROWS) return fail(c, "udf: bad row count");
    if (h->nbytes >> 32) return fail(c, "udf: a VARCHAR arena holds less than 4 GiB (%llu bytes given)", (unsigned long long)h->nbytes);
    if (h->fixed && !udf_width_ok(h->width)) return fail(c, "udf: integer width %d (1, 2, 4 or 8 bytes; negative = signed)", (int)h->width);
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t rows = h->is_const ? 1u : (uint64_t)n_rows;
    if (h->off) {                                                  // every row inside the arena: the kernels trust the offsets
        if (rows && !h->bytes && h->nbytes) return fail(c, "udf: offsets without bytes");
        for (uint64_t i = 0; i < rows; i++) {
            const uint64_t o = h->off[i], e = h->off[i + 1], l = h->len ? h->len[i] : e - o;
            if (e < o || e > h->nbytes || l > e - o) return fail(c, "udf: row %llu lies outside its column", (unsigned long long)i);
        }
    }
    DevBuf *B = c->udf.up[slot];
    *dev = *h;
    struct { const void *src; size_t n; const void **dst; } cp[6] = {
        {h->off, h->off ? (size_t)(rows + 1) * 4 : 0, (const void **)&dev->off}, {h->len, (size_t)rows * 4, (const void **)&dev->len},
        {h->bytes, (size_t)h->nbytes, (const void **)&dev->bytes}, {h->valid, (size_t)rows, (const void **)&dev->valid},
        {h->child_valid, (size_t)h->nbytes, (const void **)&dev->child_valid}, {h->fixed, (size_t)rows * (size_t)(h->width < 0 ? -h->width : h->width), &dev->fixed}};
    for (int k = 0; k < 6; k++) {
        if (!cp[k].src) { *cp[k].dst = nullptr; continue; }
        ENSURE(c, B[k], cp[k].n + 64);
        if (cp[k].n) HIPCHK(c, hipMemcpyAsync(B[k].p, cp[k].src, cp[k].n, hipMemcpyHostToDevice, c->stream));
        *cp[k].dst = B[k].p;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// lanes per row of the text kernels: by the mean reserved width of the column (4 lanes cover 64 bytes a step, 16 cover a read, a wave a contig)
static int udf_group(const dhts_udf_arg *a, int64_t n) {
    if (const char *e = getenv("DHTS_UDF_GROUP")) { const int g = atoi(e); if (g == 4 || g == 16 || g == 64) return g; }
    const uint64_t mean = n > 0 ? a->nbytes / (uint64_t)n : 0;
    return mean <= 48 ? 4 : mean <= 2048 ? 16 : 64;
}
static int udf_check_text(dhts_ctx *c, const char *name, const dhts_udf_arg *a, int64_t n) {
    if (n == 0 && !a->is_const) return 0;
    if (!a->off || (!a->bytes && a->nbytes)) return fail(c, "%s: the argument is not a VARCHAR column (off / bytes)", name);
    if (a->len && (const void *)a->len == c->seq_chars.p)                    // (the base counts of a packed batch: no text column has them as its lengths)
        return fail(c, "%s: the column is the packed SEQ of a batch (4-bit codes, dhts_bam_set_seq_packed), not text; scan with packed SEQ off", name);
    if (a->nbytes >> 32) return fail(c, "%s: the column is %llu bytes; a VARCHAR arena holds less than 4 GiB (fewer rows per call)", name, (unsigned long long)a->nbytes);
    return 0;
}

int dhts_udf_apply(dhts_ctx *c, int op, const dhts_udf_arg *a0, const dhts_udf_arg *a1, int64_t n_rows, dhts_udf_result *out) {
    if (!c || !out) return c ? fail(c, "udf: no result to fill") : -1;
    memset(out, 0, sizeof(*out));
    if (op < 0 || op >= DHTS_UDF_OP_COUNT) return fail(c, "udf: unknown function id %d", op);
    const char *name = UDF_NAMES[op];
    if (n_rows < 0 || n_rows > UDF_MAX_ROWS) return fail(c, "%s: bad row count", name);
    const bool two = op == DHTS_UDF_CIGAR_HAS_OP || op == DHTS_UDF_SAM_FLAG_HAS, text = op <= DHTS_UDF_CIGAR_HAS_OP;
    if (!a0 || (two && !a1)) return fail(c, "%s takes %d argument column%s", name, two ? 2 : 1, two ? "s" : "");
    out->op = op; out->n_rows = n_rows; out->n_fields = op == DHTS_UDF_SAM_FLAG_BITS ? 12 : 1;
    out->is_list = op == DHTS_UDF_SEQ_ENCODE_4BIT;
    const bool varchar = op == DHTS_UDF_SEQ_REVCOMP || op == DHTS_UDF_SEQ_CANONICAL || op == DHTS_UDF_SEQ_DECODE_4BIT;
    const bool big = op >= DHTS_UDF_CIGAR_LEFT_SOFT_CLIP && op <= DHTS_UDF_CIGAR_REFERENCE_LENGTH;
    out->type = varchar ? DHTS_T_VARCHAR : op == DHTS_UDF_SEQ_HASH_2BIT ? DHTS_T_UBIGINT : op == DHTS_UDF_SEQ_ENCODE_4BIT ? DHTS_T_UTINYINT
              : op == DHTS_UDF_SEQ_GC_CONTENT ? DHTS_T_DOUBLE : big ? DHTS_T_BIGINT : DHTS_T_BOOLEAN;
    if (text) {
        if (udf_check_text(c, name, a0, n_rows)) return -1;
        if (a0->is_const) return fail(c, "%s: the first argument is a column, not a constant", name);
        if (op == DHTS_UDF_CIGAR_HAS_OP && udf_check_text(c, name, a1, n_rows)) return -1;
    } else {
        if (n_rows == 0) return 0;
        if (!a0->fixed || !udf_width_ok(a0->width)) return fail(c, "%s: the argument is not an integer column (fixed / width)", name);
        if (op == DHTS_UDF_SAM_FLAG_HAS && (!a1->fixed || !udf_width_ok(a1->width))) return fail(c, "%s: the mask is not an integer column (fixed / width)", name);
    }
    if (n_rows == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    UdfState &U = c->udf;
    U.cur ^= 1;
    UdfState::Res &R = U.res[U.cur];
    const uint32_t n = (uint32_t)n_rows; const unsigned rgrid = (unsigned)((n_rows + 255) / 256);
    ENSURE(c, R.valid, (size_t)n + 64);
    uint8_t *valid = (uint8_t *)R.valid.p;
    out->col.valid = valid;
    const dhts_udf_arg none = {nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, 0};
    if (op <= DHTS_UDF_SEQ_GC_CONTENT) {
        const int G = udf_group(a0, n_rows);
        UdfOut o; memset(&o, 0, sizeof(o)); o.valid = valid;
        if (varchar) {
            ENSURE(c, R.len, (size_t)n * 4 + 64); ENSURE(c, R.bytes, (size_t)a0->nbytes + 64);
            o.len = (uint32_t *)R.len.p; o.bytes = (uint8_t *)R.bytes.p;
            out->col.off = a0->off; out->col.bytes = o.bytes; out->col.nbytes = a0->nbytes; out->len = o.len;
        } else if (op != DHTS_UDF_SEQ_ENCODE_4BIT) {
            ENSURE(c, R.fixed, (size_t)n * 8 + 64);
            o.u64 = (uint64_t *)R.fixed.p; o.f64 = (double *)R.fixed.p; out->col.fixed = R.fixed.p;
        }
        KTimer tm(c, DHTS_K_STRINGS);
        switch (op) {
        case DHTS_UDF_SEQ_REVCOMP: udf_launch_rows<DHTS_UDF_SEQ_REVCOMP>(c->stream, G, *a0, n, o); break;
        case DHTS_UDF_SEQ_CANONICAL: udf_launch_rows<DHTS_UDF_SEQ_CANONICAL>(c->stream, G, *a0, n, o); break;
        case DHTS_UDF_SEQ_HASH_2BIT: udf_launch_rows<DHTS_UDF_SEQ_HASH_2BIT>(c->stream, G, *a0, n, o); break;
        case DHTS_UDF_SEQ_DECODE_4BIT: udf_launch_rows<DHTS_UDF_SEQ_DECODE_4BIT>(c->stream, G, *a0, n, o); break;
        case DHTS_UDF_SEQ_GC_CONTENT: udf_launch_rows<DHTS_UDF_SEQ_GC_CONTENT>(c->stream, G, *a0, n, o); break;
        default: {                                                 // seq_encode_4bit: validity and child counts, their scan, the children
            ENSURE(c, U.clen, (size_t)(n + 2) * 4 + 64); ENSURE(c, R.off, (size_t)(n + 2) * 4 + 64);
            o.clen = (uint32_t *)U.clen.p;
            udf_launch_rows<DHTS_UDF_SEQ_ENCODE_4BIT>(c->stream, G, *a0, n, o);
            const uint32_t *kin[1] = {(const uint32_t *)U.clen.p}; uint32_t *kout[1] = {(uint32_t *)R.off.p}; uint64_t total = 0;
            if (run_scan(c, 1, kin, kout, nullptr, n_rows, &total)) return -1;
            if (total >> 32) return fail(c, "%s: the list children of one call are %llu bytes; an arena holds less than 4 GiB (fewer rows per call)", name, (unsigned long long)total);
            ENSURE(c, R.bytes, (size_t)total + 64);
            o.child_off = (const uint32_t *)R.off.p; o.child = (uint8_t *)R.bytes.p;
            if (total) udf_launch_rows<UDF_OP_ENCODE_WRITE>(c->stream, G, *a0, n, o);
            out->col.off = o.child_off; out->col.bytes = o.child; out->col.nbytes = total; out->col.child_n = total;
        } break;
        }
    } else if (text) {
        ENSURE(c, R.fixed, (size_t)n * 8 + 64);
        out->col.fixed = R.fixed.p;
        KTimer tm(c, DHTS_K_CORE);
        hipLaunchKernelGGL(udf_cigar_rows, dim3(rgrid), dim3(256), 0, c->stream, *a0, a1 ? *a1 : none, op, n, valid, (uint8_t *)R.fixed.p, (long long *)R.fixed.p);
    } else {
        ENSURE(c, R.fixed, (size_t)n * 12 + 64);
        out->col.fixed = R.fixed.p;
        const uint32_t mask = op >= DHTS_UDF_IS_PAIRED ? 1u << (op - DHTS_UDF_IS_PAIRED) : 0u;       // SAM_FLAG_* (:8-19) are bits 0 .. 11 in registration order
        KTimer tm(c, DHTS_K_CORE);
        hipLaunchKernelGGL(udf_flag_rows, dim3(rgrid), dim3(256), 0, c->stream, *a0, a1 ? *a1 : none, op, mask, n, valid, (uint8_t *)R.fixed.p);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// read-back of one result: every piece queued behind the last at 8-byte steps of the host arena, NULL once a copy failed
struct UdfTake {
    dhts_ctx *c; uint8_t *p;
    const void *take(const void *src, uint64_t nb) {
        const void *at = p;
        if (nb && hipMemcpyAsync(p, src, nb, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return nullptr;
        p += udf_pad8(nb);
        return at;
    }
};
static uint64_t udf_fixed_bytes(const dhts_udf_result *r) {
    const uint64_t n = (uint64_t)r->n_rows;
    return r->type == DHTS_T_BOOLEAN ? n * (uint64_t)(r->n_fields > 0 ? r->n_fields : 1) : n * 8;
}
uint64_t dhts_udf_result_host_bytes(const dhts_udf_result *r) {
    if (!r || r->n_rows <= 0) return 0;
    const uint64_t n = (uint64_t)r->n_rows;
    uint64_t need = udf_pad8(n);
    if (r->is_list) need += udf_pad8((n + 1) * 4) + udf_pad8(r->col.child_n);
    else if (r->type == DHTS_T_VARCHAR) need += udf_pad8((n + 1) * 4) + udf_pad8(n * 4) + udf_pad8(r->col.nbytes);
    else need += udf_pad8(udf_fixed_bytes(r));
    return need;
}
int dhts_udf_fetch(dhts_ctx *c, const dhts_udf_result *r, void *dst, uint64_t cap, dhts_udf_result *out) {
    if (!c || !r || !out || (!dst && cap)) return c ? fail(c, "udf: fetch without a result") : -1;
    HIPCHK(c, hipSetDevice(c->device));
    if (cap < dhts_udf_result_host_bytes(r)) return fail(c, "udf: fetch buffer too small");
    dhts_udf_result o = *r;
    memset(&o.col, 0, sizeof(o.col)); o.len = nullptr; o.col.col = r->col.col;
    const uint64_t n = (uint64_t)(r->n_rows > 0 ? r->n_rows : 0);
    uint8_t *p = (uint8_t *)dst;
    UdfTake cp = {c, p};
    auto take = [&](const void *src, uint64_t nb) { return cp.take(src, nb); };
    bool okc = true;
    if (n) {
        okc = okc && (o.col.valid = (const uint8_t *)take(r->col.valid, n));
        if (r->is_list || r->type == DHTS_T_VARCHAR) {
            okc = okc && (o.col.off = (const uint32_t *)take(r->col.off, (n + 1) * 4));
            if (!r->is_list) okc = okc && (o.len = (const uint32_t *)take(r->len, n * 4));
            const uint64_t nb = r->is_list ? r->col.child_n : r->col.nbytes;
            okc = okc && (o.col.bytes = (const uint8_t *)take(r->col.bytes, nb));
            o.col.nbytes = nb; o.col.child_n = r->col.child_n;
        } else okc = okc && (o.col.fixed = take(r->col.fixed, udf_fixed_bytes(r)));
    }
    if (!okc) { (void)hipStreamSynchronize(c->stream); return fail(c, "udf: the copy to the host failed"); }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *out = o;
    return 0;
}

// ---- seq_kmers over a column -----------------------------------------------------------------------------------------------------------
int dhts_udf_seq_kmers(dhts_ctx *c, const dhts_udf_arg *seq, int64_t n_rows, int64_t k, int canonical, int want_text, int want_hash,
                       int64_t max_rows, uint64_t resume, dhts_udf_kmers *out) {
    if (!c || !out) return c ? fail(c, "seq_kmers: no batch to fill") : -1;
    memset(out, 0, sizeof(*out));
    if (!seq) return fail(c, "seq_kmers: sequence must not be NULL");
    if (k <= 0) return fail(c, "seq_kmers: k must be > 0");
    if (n_rows < 0 || n_rows > UDF_MAX_ROWS) return fail(c, "seq_kmers: bad row count");
    if (udf_check_text(c, "seq_kmers", seq, n_rows)) return -1;
    if (want_hash && k > 32) return fail(c, "seq_kmers: hash needs k <= 32 (seq_hash_2bit holds 32 bases), k = %lld", (long long)k);
    out->k = (int32_t)(k > INT32_MAX ? INT32_MAX : k); out->status = 1; out->next = resume;
    if (n_rows == 0 || k > 0xffffffffll) return 0;                  // (no row of a 32-bit arena is that long)
    HIPCHK(c, hipSetDevice(c->device));
    UdfState &U = c->udf;
    const uint32_t n = (uint32_t)n_rows, kk = (uint32_t)k;
    ENSURE(c, U.cnt, (size_t)(n + 2) * 4 + 64); ENSURE(c, U.cum, (size_t)(n + 2) * 8 + 64);
    KTimer tm(c, DHTS_K_CORE);                                     // the whole call: counts, their scan and the k-mers
    hipLaunchKernelGGL(udf_kmer_counts, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, c->stream, *seq, n, kk, (uint32_t *)U.cnt.p);
    const uint32_t *kin[1] = {(const uint32_t *)U.cnt.p}; uint64_t *kout[1] = {(uint64_t *)U.cum.p}; uint64_t total = 0;
    if (run_scan(c, 1, kin, nullptr, kout, n_rows, &total)) return -1;
    out->total = total;
    if (resume >= total) { out->next = total; return 0; }
    uint64_t m = total - resume;
    if (max_rows <= 0) max_rows = 1 << 22;
    if (m > (uint64_t)max_rows) m = (uint64_t)max_rows;
    if (m > (uint64_t)UDF_MAX_ROWS) m = (uint64_t)UDF_MAX_ROWS;
    if (want_text) {
        const uint64_t lim = 0xfffffff0ull / kk;
        if (lim == 0) return fail(c, "seq_kmers: one k-mer of %lld bytes does not fit a VARCHAR arena of less than 4 GiB", (long long)k);
        if (m > lim) m = lim;
    }
    UdfKmerOut o; memset(&o, 0, sizeof(o));
    ENSURE(c, U.k_row, (size_t)m * 8 + 64); ENSURE(c, U.k_pos, (size_t)m * 8 + 64);
    o.row = (long long *)U.k_row.p; o.pos = (long long *)U.k_pos.p;
    if (want_text) {
        ENSURE(c, U.k_off, (size_t)(m + 2) * 4 + 64); ENSURE(c, U.k_bytes, (size_t)(m * kk) + 64); ENSURE(c, U.k_valid, (size_t)m + 64);
        o.off = (uint32_t *)U.k_off.p; o.bytes = (uint8_t *)U.k_bytes.p; o.kvalid = (uint8_t *)U.k_valid.p;
    }
    if (want_hash) { ENSURE(c, U.k_hash, (size_t)m * 8 + 64); ENSURE(c, U.k_hvalid, (size_t)m + 64); o.hash = (uint64_t *)U.k_hash.p; o.hvalid = (uint8_t *)U.k_hvalid.p; }
    {
        hipLaunchKernelGGL(udf_kmers_emit, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, *seq, (const uint64_t *)U.cum.p, n, kk, resume, (uint32_t)m, canonical ? 1 : 0, o);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out->n_rows = (int64_t)m; out->next = resume + m; out->status = out->next >= total ? 1 : 0;
    out->row = (const int64_t *)o.row; out->pos = (const int64_t *)o.pos;
    out->kmer.valid = o.kvalid; out->kmer.off = o.off; out->kmer.bytes = o.bytes; out->kmer.nbytes = want_text ? m * kk : 0;
    out->hash = o.hash; out->hash_valid = o.hvalid;
    return 0;
}
uint64_t dhts_udf_kmers_host_bytes(const dhts_udf_kmers *b) {
    if (!b || b->n_rows <= 0) return 0;
    const uint64_t n = (uint64_t)b->n_rows;
    uint64_t need = 2 * n * 8;
    if (b->kmer.off) need += udf_pad8(n) + udf_pad8((n + 1) * 4) + udf_pad8(b->kmer.nbytes);
    if (b->hash) need += n * 8 + udf_pad8(n);
    return need;
}
int dhts_udf_kmers_fetch(dhts_ctx *c, const dhts_udf_kmers *b, void *dst, uint64_t cap, dhts_udf_kmers *out) {
    if (!c || !b || !out || (!dst && cap)) return c ? fail(c, "seq_kmers: fetch without a batch") : -1;
    HIPCHK(c, hipSetDevice(c->device));
    if (cap < dhts_udf_kmers_host_bytes(b)) return fail(c, "seq_kmers: fetch buffer too small");
    dhts_udf_kmers o = *b;
    o.row = o.pos = nullptr; memset(&o.kmer, 0, sizeof(o.kmer)); o.hash = nullptr; o.hash_valid = nullptr;
    const uint64_t n = (uint64_t)(b->n_rows > 0 ? b->n_rows : 0);
    uint8_t *p = (uint8_t *)dst;
    UdfTake cp = {c, p};
    auto take = [&](const void *src, uint64_t nb) { return cp.take(src, nb); };
    bool okc = true;
    if (n) {
        okc = okc && (o.row = (const int64_t *)take(b->row, n * 8)); okc = okc && (o.pos = (const int64_t *)take(b->pos, n * 8));
        if (b->kmer.off) {
            okc = okc && (o.kmer.valid = (const uint8_t *)take(b->kmer.valid, n)); okc = okc && (o.kmer.off = (const uint32_t *)take(b->kmer.off, (n + 1) * 4));
            okc = okc && (o.kmer.bytes = (const uint8_t *)take(b->kmer.bytes, b->kmer.nbytes)); o.kmer.nbytes = b->kmer.nbytes;
        }
        if (b->hash) { okc = okc && (o.hash = (const uint64_t *)take(b->hash, n * 8)); okc = okc && (o.hash_valid = (const uint8_t *)take(b->hash_valid, n)); }
    }
    if (!okc) { (void)hipStreamSynchronize(c->stream); return fail(c, "seq_kmers: the copy to the host failed"); }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *out = o;
    return 0;
}
