// dhts_sam_scan.inc -- part of dhts_api.hip (included there, inside its extern "C" block; not a translation unit of its own):
// read_bam on SAM text.  A batch of text (carry + blocks, batch_begin) is cut into lines, the complete lines become BAM records in s_out
// (sam_text.hip: measure, exclusive scan of the sizes, write), and bam_next_batch_one runs its unchanged record stage over those records
// with every record complete.  The text from the first line that was not encoded on is the carry.
//
// out: enc / enc_len (the records), nrec (records = lines in front of the first rejected one), carry_start (text offset of the first line
// not encoded), rejected (a line sam_parse1 refuses ends the scan there: single-threaded sam_read1, sam.c:4243-4250), t0 (text offset of
// the batch's first line).
static int sam_text_records(dhts_ctx *c, const Batch &B, const uint8_t *&enc, uint64_t &enc_len, int64_t &nrec, uint64_t &carry_start, bool &rejected, uint64_t &t0) {
    const uint8_t *u = B.u; const uint64_t ulen = B.ulen, out_base = B.out_base;
    if (!first_line_t0(c, out_base, t0)) return fail(c, "internal: header beyond first batch");
    nrec = 0; enc = nullptr; enc_len = 0; rejected = false;
    c->s_last_nrec = 0; c->s_last_len = 0;                                    // (a batch without a complete line encodes nothing)
    LineTab T;
    if (line_table(c, c->lines, nullptr, u, t0, ulen, batch_clean_end(c, B), ~0ull, -1, T)) return -1;      // (the encoder reads the open last line's end from the sentinel)
    const int64_t nlines = T.nlines;
    carry_start = T.carry_start;
    if (nlines == 0) return 0;
    ENSURE(c, c->v_rec_len, (size_t)(nlines + 1) * 4 + 64); ENSURE(c, c->b_rec_off, (size_t)(nlines + 1) * 4 + 64); ENSURE(c, c->s_ctr, 64);
    // room for the values the host converts: grown (and the measure pass repeated) when a batch needs more.  DHTS_SAM_PATCH_CAP: the
    // starting room (tests: a small one makes the growth path cheap to reach)
    if (c->s_patch_cap == 0) { const char *e = getenv("DHTS_SAM_PATCH_CAP"); const long v = e ? atol(e) : 0; c->s_patch_cap = v > 0 ? (uint32_t)v : (1u << 20); }
    SamArgs a; memset(&a, 0, sizeof(a));
    a.u = u; a.line_off = (const uint32_t *)c->lines.line_off.p; a.nlines = nlines;
    a.names.off = (const uint32_t *)c->s_name_off.p; a.names.bytes = (const uint8_t *)c->s_name_bytes.p; a.names.id = (const int32_t *)c->s_name_id.p;
    a.names.n = c->s_n_names; a.names.hash = (const uint32_t *)c->s_name_hash.p; a.names.hmask = c->s_name_hmask; a.n_targets = (int32_t)c->ref_name.size();
    a.rec_len = (uint32_t *)c->v_rec_len.p; a.rec_off = (const uint32_t *)c->b_rec_off.p;
    a.first_bad = (unsigned long long *)c->s_ctr.p; a.n_patch = (uint32_t *)((uint8_t *)c->s_ctr.p + 8); a.patch = nullptr; a.patch_cap = 0;
    const int64_t waves = SAM_ENC_THREADS / 64;
    const unsigned grid = (unsigned)((nlines + waves - 1) / waves < (1 << 20) ? (nlines + waves - 1) / waves : (1 << 20));
    uint64_t total = 0;
    for (;;) {  // (a read_bam scan runs no BCF kernels: the encoder's two passes are timed in the text encoder's slots)
        ENSURE(c, c->s_patch, (size_t)c->s_patch_cap * sizeof(SamPatch));
        a.patch = (SamPatch *)c->s_patch.p; a.patch_cap = c->s_patch_cap;
        unsigned long long mctr[2] = {0, 0};
        {
            KTimer tm(c, DHTS_K_BCF_MEASURE);
            HIPCHK(c, hipMemsetAsync(c->s_ctr.p, 0xff, 8, c->stream)); HIPCHK(c, hipMemsetAsync((uint8_t *)c->s_ctr.p + 8, 0, 8, c->stream));
            hipLaunchKernelGGL(sam_encode<false>, dim3(grid), dim3(SAM_ENC_THREADS), 0, c->stream, a);
            HIPCHK(c, hipMemcpyAsync(mctr, c->s_ctr.p, 16, hipMemcpyDeviceToHost, c->stream));
            uint32_t *rin = (uint32_t *)c->v_rec_len.p; const uint32_t *in1[1] = {rin}; uint32_t *out1[1] = {(uint32_t *)c->b_rec_off.p};
            if (run_scan(c, 1, in1, out1, nullptr, nlines, &total)) return -1;      // (waits for the stream: mctr has arrived)
        }
        const uint64_t need = (uint32_t)mctr[1];
        if (need <= c->s_patch_cap) break;
        uint64_t cap = (uint64_t)c->s_patch_cap * 2; if (cap < need + need / 8) cap = need + need / 8;
        if (cap > 0xffffffffull) return fail(c, "read_bam: too many floating-point values in one SAM batch");
        c->s_patch_cap = (uint32_t)cap;
    }
    if (total + PAD_BYTES >= (1ull << 32)) return fail(c, "read_bam: a SAM batch encodes to more than 4 GiB: use a smaller max_blocks");
    ENSURE(c, c->s_out, total + PAD_BYTES);
    a.out = (uint8_t *)c->s_out.p;
    unsigned long long ctr[2] = {0, 0};
    {
        KTimer tm(c, DHTS_K_BCF_WRITE);
        hipLaunchKernelGGL(sam_encode<true>, dim3(grid), dim3(SAM_ENC_THREADS), 0, c->stream, a);
        HIPCHK(c, hipMemsetAsync((uint8_t *)c->s_out.p + total, 0, PAD_BYTES, c->stream));
        HIPCHK(c, hipMemcpyAsync(ctr, c->s_ctr.p, 16, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    unsigned long long first_bad = ctr[0];
    const uint32_t npatch = (uint32_t)ctr[1];
    if (npatch > c->s_patch_cap) return fail(c, "internal: SAM patch count changed between the passes");
    if (npatch) {
        // the values the device fast path did not take: strtod on the host; a B:f element strtod does not take whole rejects its line
        std::vector<SamPatch> pt(npatch);
        HIPCHK(c, hipMemcpy(pt.data(), c->s_patch.p, (size_t)npatch * sizeof(SamPatch), hipMemcpyDeviceToHost));
        std::vector<uint32_t> tk_off(npatch + 1, 0);
        for (uint32_t i = 0; i < npatch; i++) tk_off[i + 1] = tk_off[i] + pt[i].len;
        std::vector<char> tk(tk_off[npatch] + 1, 0);
        if (tk_off[npatch]) {
            ENSURE(c, c->v_tok_off, (size_t)npatch * 4 + 64); ENSURE(c, c->v_tok_bytes, (size_t)tk_off[npatch] + 64);
            HIPCHK(c, hipMemcpy(c->v_tok_off.p, tk_off.data(), (size_t)npatch * 4, hipMemcpyHostToDevice));
            hipLaunchKernelGGL(vcf_gather_tokens, dim3((npatch + 255) / 256), dim3(256), 0, c->stream, u, (const uint32_t *)c->s_patch.p, 1, 2, (const uint32_t *)c->v_tok_off.p, npatch, (uint8_t *)c->v_tok_bytes.p);
            HIPCHK(c, hipMemcpyAsync(tk.data(), c->v_tok_bytes.p, tk_off[npatch], hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        std::vector<uint32_t> roff((size_t)nlines + 1);
        HIPCHK(c, hipMemcpy(roff.data(), c->b_rec_off.p, ((size_t)nlines + 1) * 4, hipMemcpyDeviceToHost));
        std::vector<uint32_t> dst; std::vector<uint64_t> val; std::vector<uint8_t> wid;
        for (uint32_t i = 0; i < npatch; i++) {
            const SamPatch &q = pt[i];
            if (q.line >= first_bad) continue;
            std::string t(tk.data() + tk_off[i], q.len);
            char *endp = nullptr; const double d = strtod(t.c_str(), &endp);
            const uint32_t kind = q.relk & 3u;
            if (kind == 2 && (size_t)(endp - t.c_str()) != t.size()) { if (q.line < first_bad) first_bad = q.line; continue; }
            uint64_t bits = 0;
            if (kind == 1) memcpy(&bits, &d, 8); else { const float f = (float)d; uint32_t b32; memcpy(&b32, &f, 4); bits = b32; }
            dst.push_back(roff[q.line] + (q.relk >> 2)); val.push_back(bits); wid.push_back(kind == 1 ? 8 : 4);
        }
        if (!dst.empty()) {
            const uint32_t n = (uint32_t)dst.size();
            ENSURE(c, c->s_pdst, (size_t)n * 4 + 64); ENSURE(c, c->s_pval, (size_t)n * 8 + 64); ENSURE(c, c->s_pwid, (size_t)n + 64);
            HIPCHK(c, hipMemcpy(c->s_pdst.p, dst.data(), (size_t)n * 4, hipMemcpyHostToDevice)); HIPCHK(c, hipMemcpy(c->s_pval.p, val.data(), (size_t)n * 8, hipMemcpyHostToDevice));
            HIPCHK(c, hipMemcpy(c->s_pwid.p, wid.data(), n, hipMemcpyHostToDevice));
            hipLaunchKernelGGL(sam_scatter_values, dim3((n + 255) / 256), dim3(256), 0, c->stream, (uint8_t *)c->s_out.p, (const uint32_t *)c->s_pdst.p, (const uint64_t *)c->s_pval.p, (const uint8_t *)c->s_pwid.p, n);
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
    }
    nrec = first_bad < (unsigned long long)nlines ? (int64_t)first_bad : nlines;
    rejected = nrec < nlines;
    enc_len = total;
    if (rejected) {
        uint32_t w = 0;
        HIPCHK(c, hipMemcpy(&w, (const uint32_t *)c->b_rec_off.p + nrec, 4, hipMemcpyDeviceToHost));
        enc_len = w;
        if (line_start(c, c->lines, nrec, carry_start)) return -1;
    }
    enc = (const uint8_t *)c->s_out.p;
    c->s_last_nrec = nrec; c->s_last_len = enc_len;
    return 0;
}
extern "C" int dhts_bam_is_text(const dhts_ctx *c) { return (!c || !c->bam_open || !c->sam_text) ? 0 : (c->plain_text ? 2 : 1) + 2 * c->fastq; }
// debugging aid (include/duckhts_amd_debug.h): the BAM records the encoder made of the last SAM text batch
extern "C" int64_t dhts_debug_sam_records(dhts_ctx *c, uint8_t *dst, uint64_t cap, int64_t *nrec) {
    if (!c || !c->sam_text) return -1;
    if (nrec) *nrec = c->s_last_nrec;
    const uint64_t n = cap < c->s_last_len ? cap : c->s_last_len;
    if (n && dst) HIPCHK(c, hipMemcpy(dst, c->s_out.p, n, hipMemcpyDeviceToHost));
    return (int64_t)c->s_last_len;
}
