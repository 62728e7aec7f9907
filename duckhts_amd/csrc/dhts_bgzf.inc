// dhts_bgzf.inc -- part of dhts_api.hip (included there, inside its extern "C" block; not a translation unit of its own):
// device scans, the BGZF block table (bgzf_sig_* / chain check), inflate launches (phase A over the shard, phase B per batch).
// ---- scans --------------------------------------------------------------------------------
static int run_scan(dhts_ctx *c, int narr, const uint32_t **in, uint32_t **out32, uint64_t **out64, int64_t n, uint64_t *totals_host, const unsigned long long *n_dev = nullptr) {
    ScanArgs a; memset(&a, 0, sizeof(a));
    int64_t nparts = (n + 1 + SCAN_ITEMS - 1) / SCAN_ITEMS;      // +1: the apply pass also writes off[n]
    if (nparts < 1) nparts = 1;
    ENSURE(c, c->scan_partial, (size_t)narr * (size_t)nparts * 8);
    ENSURE(c, c->scan_total, 8 * 8);
    for (int k = 0; k < narr; k++) {
        a.in[k] = in[k]; a.out32[k] = out32 ? out32[k] : nullptr; a.out64[k] = out64 ? out64[k] : nullptr;
        a.partial[k] = (uint64_t *)c->scan_partial.p + (size_t)k * nparts; a.total[k] = (uint64_t *)c->scan_total.p + k;
    }
    a.n = n; a.narr = narr; a.n_dev = n_dev;
    hipLaunchKernelGGL(scan_reduce, dim3((unsigned)nparts, narr), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(scan_partials, dim3(narr), dim3(1024), 0, c->stream, a, nparts);
    hipLaunchKernelGGL(scan_apply, dim3((unsigned)nparts, narr), dim3(256), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    if (totals_host) {
        HIPCHK(c, hipMemcpyAsync(totals_host, c->scan_total.p, 8 * narr, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return 0;
}

// ---- BGZF index -------------------------------------------------------------------------------
int64_t dhts_bgzf_index(dhts_ctx *c) { return c ? index_impl(c, false) : -1; }
// extend: the resident bytes have grown since the last call (a file that is still being staged): the table is rebuilt over the longer
// prefix -- the blocks known before keep their numbers, offsets and scratch -- and the scan position is left alone
// device buffer that keeps its first `keep` bytes when it has to grow
static int ensure_keep(dhts_ctx *c, DevBuf &b, size_t need, size_t keep) {
    if (need <= b.cap) return 0;
    DevBuf nb; if (nb.ensure(need + need / 2)) return fail(c, "hipMalloc failed");
    if (keep) HIPCHK(c, hipMemcpyAsync(nb.p, b.p, keep, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    b.swap(nb);
    return 0;
}
// index_impl(extend): append the blocks that start behind block keep-1 to the table.  Returns 1 when done, 0 when the caller should run
// the full pass instead, -1 on failure.
static int index_extend_tail(dhts_ctx *c, int64_t keep) {
    const uint64_t endk = c->h_coff[keep - 1] + c->h_clen[keep - 1];          // first byte behind the last complete block
    if (endk > c->comp_len) return 0;
    if (endk == c->comp_len) return 1;                                          // nothing new
    const uint64_t base = endk & ~(uint64_t)15;                                // the sweep reads 16 bytes per lane: keep its alignment
    const uint8_t *d2 = (const uint8_t *)c->comp.p + base; const uint64_t n2 = c->comp_len - base;
    const int64_t nspans = (int64_t)((n2 + 65535) / 65536);
    DevBuf &cnt = c->sg_cnt, &sbase = c->sg_base, &hits = c->sg_hits; uint64_t total = 0;
    if (cnt.ensure((size_t)nspans * 4 + 64) || sbase.ensure((size_t)(nspans + 1) * 4 + 64) || hits.ensure((size_t)nspans * SIG_SLOTS * 2 + 64) || c->d_nfixed.ensure(64)) return fail(c, "hipMalloc failed");
    (void)hipMemsetAsync(c->d_nfixed.p, 0, 4, c->stream);
    {
        KTimer t(c, DHTS_K_SIGSCAN);
        hipLaunchKernelGGL(bgzf_sig_count, dim3((unsigned)((nspans * 64 + 255) / 256)), dim3(256), 0, c->stream, d2, n2, (uint32_t *)cnt.p, (uint16_t *)hits.p, (uint32_t *)c->d_nfixed.p);
    }
    const uint32_t *in[1] = {(const uint32_t *)cnt.p}; uint32_t *o32[1] = {(uint32_t *)sbase.p};
    if (run_scan(c, 1, in, o32, nullptr, nspans, &total)) return -1;
    const int64_t ncand = (int64_t)total;
    // no candidate: fewer than 18 bytes have arrived behind the last complete block (a signature is recognised with its 18-byte header in
    // view), so there is nothing new yet -- a slowly arriving file must not cost a pass over the whole prefix every time it is asked; with
    // 18 bytes or more and no signature at `endk` the stream is damaged there and the full pass reports it
    if (ncand == 0) return c->comp_len - endk < 18 ? 1 : 0;
    if (ensure_keep(c, c->coff, (size_t)(keep + ncand) * 8 + 64, (size_t)keep * 8) || ensure_keep(c, c->clen, (size_t)(keep + ncand) * 4 + 64, (size_t)keep * 4) ||
        ensure_keep(c, c->isize, (size_t)(keep + ncand) * 4 + 64, (size_t)keep * 4)) return -1;
    uint32_t ovf = 0;
    HIPCHK(c, hipMemcpyAsync(&ovf, c->d_nfixed.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint64_t *coff_new = (uint64_t *)c->coff.p + keep;
    {
        KTimer t(c, DHTS_K_SIGSCAN);
        if (ovf) hipLaunchKernelGGL(bgzf_sig_write, dim3((unsigned)((nspans * 64 + 255) / 256)), dim3(256), 0, c->stream, d2, n2, (const uint32_t *)sbase.p, coff_new, base);
        else hipLaunchKernelGGL(bgzf_sig_gather, dim3((unsigned)((nspans + 255) / 256)), dim3(256), 0, c->stream, (const uint32_t *)cnt.p, (const uint32_t *)sbase.p, (const uint16_t *)hits.p, nspans, coff_new, base);
    }
    (void)hipMemsetAsync(c->d_nfixed.p, 0, 8, c->stream);
    hipLaunchKernelGGL(bgzf_chain_check, dim3((unsigned)((ncand + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t *)c->comp.p, c->comp_len, (const uint64_t *)coff_new, ncand,
                       (uint32_t *)c->clen.p + keep, (uint32_t *)c->isize.p + keep, (uint32_t *)c->d_nfixed.p, c->partial_tail ? 1 : 0, endk);
    uint32_t bad[2] = {0, 0}; uint64_t first = 0;
    HIPCHK(c, hipMemcpyAsync(bad, c->d_nfixed.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&first, coff_new, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (bad[0] != 0 || first != endk) return 0;                 // the chain does not prove itself from the expected offset: full pass
    const int64_t nnew = ncand - (int64_t)bad[1];                // (cut candidates are the last ones: a block that is not complete yet)
    if (nnew < 0) return 0;
    const int64_t nb = keep + nnew;
    c->h_coff.resize(nb); c->h_clen.resize(nb); c->h_isize.resize(nb); c->h_uoff.resize(nb + 1);
    if (nnew) {
        HIPCHK(c, hipMemcpy(c->h_coff.data() + keep, coff_new, (size_t)nnew * 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(c->h_clen.data() + keep, (uint32_t *)c->clen.p + keep, (size_t)nnew * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(c->h_isize.data() + keep, (uint32_t *)c->isize.p + keep, (size_t)nnew * 4, hipMemcpyDeviceToHost));
    }
    for (int64_t i = keep; i < nb; i++) c->h_uoff[i + 1] = c->h_uoff[i] + c->h_isize[i];      // (the recorded ISIZE is already the placed one: <= 65,537)
    if (ensure_keep(c, c->uoff, (size_t)(nb + 1) * 8 + 64, (size_t)(keep + 1) * 8)) return -1;
    if (nnew) HIPCHK(c, hipMemcpy((uint64_t *)c->uoff.p + keep + 1, c->h_uoff.data() + keep + 1, (size_t)nnew * 8, hipMemcpyHostToDevice));
    ENSURE(c, c->blk_status, (size_t)(nb + 1) * 4);
    c->n_blocks = nb; c->bgzf_status = 0;
    return 1;
}
// host side of crc_mulmod / crc_xpow8 (bgzf_inflate.hip): polynomials mod the reflected CRC-32 polynomial
static uint32_t h_crc_mulmod(uint32_t a, uint32_t b) { uint32_t p = 0; for (int i = 0; i < 32; i++) { if (b & 0x80000000u) p ^= a; a = (a >> 1) ^ ((a & 1u) ? 0xEDB88320u : 0u); b <<= 1; } return p; }
static uint32_t h_crc_xpow8(uint64_t nbytes) { uint32_t pw = 0x80000000u, sq = 0x00800000u; while (nbytes) { if (nbytes & 1) pw = h_crc_mulmod(pw, sq); sq = h_crc_mulmod(sq, sq); nbytes >>= 1; } return pw; }
// The resident bytes are plain gzip: inflate every member into c->gz_out (gz_inflate_serial: one launch when the guessed capacity holds, a
// second one when it does not), check CRC-32 and ISIZE of every member in parallel, and set c->gz_len to the bytes a reader of the reference
// would have been handed: htslib hands them out in chunks of 64 KiB (inflate_gzip_block, bgzf.c:828-893) and a call that meets an error --
// invalid data, a CRC / length that does not match (zlib finds it at the member's end), trailing bytes that are not a member, a file that
// ends inside a member -- returns nothing, so the stream ends at the last chunk boundary in front of the error (c->gz_error).  A context that
// holds only the head of a file (bind) keeps everything it could decode and no error.
static int gz_plain_inflate(dhts_ctx *c) {
    const bool partial = c->partial_tail || (c->file_size > 0 && c->comp_len < c->file_size);
    // a context that holds the head of a file wants the header: an eighth of the head is inflated (the decoder is serial; a header that does not
    // fit makes the caller stage four times more, as for BGZF)
    const uint64_t n = partial && c->comp_len > (1u << 17) ? c->comp_len / 8 : c->comp_len;
    // the inflated bytes of a whole file stay in the pool beside the file's own (DHTS_FILE_CACHE): the serial decoder takes seconds, the next
    // query of the same unchanged file takes them back
    const std::string ztag = (!partial && !c->comp.tag.empty()) ? c->comp.tag + "|gunzip" : std::string();
    if (!ztag.empty()) {
        for (int e = 0; e < 2; e++) {
            const int64_t got = c->gz_out.adopt(ztag + (e ? "|err" : "|ok"));
            if (got >= 0) { c->gz_plain = true; c->gz_error = e != 0; c->gz_len = (uint64_t)got; return 0; }
        }
    }
    DevBuf d_res, d_mem; const uint32_t mem_cap = 1u << 16;
    ENSURE(c, d_res, sizeof(GzResult) + 64); ENSURE(c, d_mem, (size_t)mem_cap * sizeof(GzMember) + 64);
    uint64_t cap = n * 8 + (1u << 20);
    if (!partial && n >= 18) {                                                     // a file of one member says what it inflates to (ISIZE, mod 2^32): a guess that saves the second launch
        uint8_t t4[4]; HIPCHK(c, hipMemcpy(t4, (const uint8_t *)c->comp.p + n - 4, 4, hipMemcpyDeviceToHost));
        const uint64_t hint = (uint64_t)t4[0] | (uint64_t)t4[1] << 8 | (uint64_t)t4[2] << 16 | (uint64_t)t4[3] << 24;
        if (hint + (1u << 20) > cap && hint < n * 1100) cap = hint + (1u << 20);  // (DEFLATE cannot expand more than 1032 : 1)
    }
    GzResult r; memset(&r, 0, sizeof(r));
    for (int attempt = 0; attempt < 2; attempt++) {
        ENSURE(c, c->gz_out, cap + PAD_BYTES + 64);
        hipLaunchKernelGGL(gz_inflate_serial, dim3(1), dim3(128), 0, c->stream, (const uint8_t *)c->comp.p, (unsigned long long)n, (uint8_t *)c->gz_out.p, (unsigned long long)cap, (GzMember *)d_mem.p, mem_cap, (GzResult *)d_res.p);
        HIPCHK(c, hipMemcpyAsync(&r, d_res.p, sizeof(r), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (r.out_len <= cap) break;
        cap = r.out_len;
    }
    if (getenv("DHTS_TRACE")) fprintf(stderr, "[dhts] plain gzip: %llu -> %llu bytes, %u members, status %u; the decoder ran %.1f M shader cycles in %.3f s (%.0f MHz)\n", (unsigned long long)n, (unsigned long long)r.out_len, r.n_members, r.status,
                                     r.pad[0] * 1024.0 / 1e6, r.pad[1] * 1024.0 / 1e8, r.pad[1] ? (r.pad[0] * 1024.0) / (r.pad[1] * 1024.0 / 1e8) / 1e6 : 0.0);
    if (r.out_len > cap) return fail(c, "plain gzip: the output did not fit the second time");
    uint64_t err_at = ~0ull;                                                      // output position at which the reference's reader meets an error
    if (r.status == 3) return fail(c, "plain gzip: more than %u members", mem_cap);
    if (r.status == 2 || (r.status == 1 && !partial)) err_at = r.out_len;
    else if (r.status == 0 && !partial && r.in_used < n) err_at = r.out_len;      // bytes behind the last member that are not a member ("incorrect header check")
    // CRC-32 / ISIZE of the complete members: pieces of at most 64 KiB, a lane each; folded here
    const uint32_t nm = r.n_members < mem_cap ? r.n_members : mem_cap;
    if (nm) {
        std::vector<GzMember> mem(nm);
        HIPCHK(c, hipMemcpy(mem.data(), d_mem.p, (size_t)nm * sizeof(GzMember), hipMemcpyDeviceToHost));
        std::vector<unsigned long long> off; std::vector<uint32_t> len;
        for (auto &m : mem) for (uint64_t o = m.out_beg; o < m.out_end; o += 65536) { off.push_back(o); len.push_back((uint32_t)(m.out_end - o < 65536 ? m.out_end - o : 65536)); }
        std::vector<uint32_t> st(off.size() + 1, 0);
        if (!off.empty()) {
            DevBuf d_off, d_len, d_st;
            ENSURE(c, d_off, off.size() * 8 + 64); ENSURE(c, d_len, len.size() * 4 + 64); ENSURE(c, d_st, off.size() * 4 + 64);
            HIPCHK(c, hipMemcpy(d_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice)); HIPCHK(c, hipMemcpy(d_len.p, len.data(), len.size() * 4, hipMemcpyHostToDevice));
            hipLaunchKernelGGL(gz_crc_ranges, dim3((unsigned)((off.size() + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t *)c->gz_out.p, (const unsigned long long *)d_off.p, (const uint32_t *)d_len.p, (uint32_t)off.size(), (uint32_t *)d_st.p);
            HIPCHK(c, hipMemcpyAsync(st.data(), d_st.p, off.size() * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        size_t k = 0;
        for (auto &m : mem) {
            const uint64_t ml = m.out_end - m.out_beg;
            uint32_t s = h_crc_mulmod(0xffffffffu, h_crc_xpow8(ml));               // the initial state carried over the member's bytes
            uint32_t acc = 0;                                                      // the bytes' own contribution: piece after piece
            for (uint64_t o = m.out_beg; o < m.out_end; o += 65536, k++) acc = h_crc_mulmod(acc, h_crc_xpow8(len[k])) ^ st[k];
            const uint32_t crc = ~(s ^ acc);
            if (crc != m.crc || (uint32_t)ml != m.isize) { if (m.out_end < err_at) err_at = m.out_end; break; }
        }
    }
    c->gz_plain = true; c->gz_error = err_at != ~0ull;
    c->gz_len = c->gz_error ? (err_at / 65536) * 65536 : r.out_len;
    HIPCHK(c, hipMemsetAsync((uint8_t *)c->gz_out.p + c->gz_len, 0, PAD_BYTES, c->stream));
    if (!ztag.empty()) { c->gz_out.tag = ztag + (c->gz_error ? "|err" : "|ok"); c->gz_out.tag_len = c->gz_len; }
    return 0;
}
static int64_t index_impl(dhts_ctx *c, bool extend) {
    HIPCHK(c, hipSetDevice(c->device));
    discard_prefetch(c);
    const int64_t old_nb = c->n_blocks;
    if (!extend) c->huff_b0 = c->huff_nb = 0;
    if (c->comp_len == 0) { c->n_blocks = 0; return 0; }
    if (!extend && !c->growing && c->comp_len >= 1) {                      // (a FASTQ / FASTA file may be a few bytes long)
        // not gzip at all but VCF text (hts_detect_format: "##fileformat=VCF"): the bytes are the stream; pieces of 65,280 bytes stand in for blocks
        uint8_t head[1024] = {0};                              // (hts_detect_format looks at up to 1 KiB: a headerless SAM line is recognised by its columns)
        size_t nhead = c->comp_len < sizeof(head) ? (size_t)c->comp_len : sizeof(head);
        HIPCHK(c, hipMemcpy(head, c->comp.p, nhead, hipMemcpyDeviceToHost));
        uint64_t text_len = c->comp_len;
        // gzip, but not BGZF (no FEXTRA, or an extra field that does not start with the BC subfield: bgzf.c check_header :896-905): the members are
        // inflated by the serial decoder (gzip_serial.hip) and what they hold is read as the uncompressed file would be
        if (c->comp_len >= 16 && head[0] == 0x1f && head[1] == 0x8b && head[2] == 8 && !((head[3] & 4) && head[10] == 6 && head[11] == 0 && head[12] == 'B' && head[13] == 'C' && head[14] == 2 && head[15] == 0)) {
            if (gz_plain_inflate(c)) return -1;
            text_len = c->gz_len;
            memset(head, 0, sizeof(head));
            nhead = text_len < sizeof(head) ? (size_t)text_len : sizeof(head);
            if (nhead) HIPCHK(c, hipMemcpy(head, c->gz_out.p, nhead, hipMemcpyDeviceToHost));
            if (memcmp(head, "##fileformat=VCF", 16) != 0 && !sam_text_detect(head, nhead) && !fastq_text_detect(head, nhead) && !c->gz_any && !c->text_any) return fail(c, "read_bcf: a plain-gzip file is read when it holds VCF text; this one does not (BAM / BCF inside plain gzip is not read by this build)");
        }
        // VCF text, SAM text (hts_detect_format: an @HD / @SQ / @RG / @PG / @CO line, or a first line whose columns look like SAM), FASTQ / FASTA
        const bool text_fmt = memcmp(head, "##fileformat=VCF", 16) == 0 || sam_text_detect(head, nhead) || fastq_text_detect(head, nhead);
        if ((c->gz_plain && (c->gz_any || c->text_any)) || ((c->gz_plain || !(head[0] == 0x1f && head[1] == 0x8b)) && (text_fmt || c->text_any))) {      // (gz_any: bgunzip wants the bytes, whatever they are)
            const uint64_t P = 65280; const int64_t nb = (int64_t)((text_len + P - 1) / P);
            c->h_coff.resize(nb); c->h_clen.resize(nb); c->h_isize.resize(nb); c->h_uoff.resize(nb + 1);
            for (int64_t i = 0; i < nb; i++) { c->h_coff[i] = (uint64_t)i * P; c->h_uoff[i] = (uint64_t)i * P; const uint64_t l = text_len - (uint64_t)i * P < P ? text_len - (uint64_t)i * P : P; c->h_clen[i] = (uint32_t)l; c->h_isize[i] = (uint32_t)l; }
            c->h_uoff[nb] = text_len;
            ENSURE(c, c->coff, (size_t)nb * 8 + 64); ENSURE(c, c->clen, (size_t)nb * 4 + 64); ENSURE(c, c->isize, (size_t)nb * 4 + 64); ENSURE(c, c->uoff, (size_t)(nb + 1) * 8 + 64); ENSURE(c, c->blk_status, (size_t)(nb + 1) * 4);
            HIPCHK(c, hipMemcpy(c->coff.p, c->h_coff.data(), nb * 8, hipMemcpyHostToDevice)); HIPCHK(c, hipMemcpy(c->clen.p, c->h_clen.data(), nb * 4, hipMemcpyHostToDevice));
            HIPCHK(c, hipMemcpy(c->isize.p, c->h_isize.data(), nb * 4, hipMemcpyHostToDevice)); HIPCHK(c, hipMemcpy(c->uoff.p, c->h_uoff.data(), (nb + 1) * 8, hipMemcpyHostToDevice));
            HIPCHK(c, hipMemset(c->blk_status.p, 0, (size_t)(nb + 1) * 4));
            c->n_blocks = nb; c->bgzf_status = c->gz_error ? -2 : 0; c->plain_text = true;      // (a plain-gzip stream that ends in an error: the scan reports it behind the rows in front of it)
            c->shard_b0 = 0; c->shard_b1 = nb; c->shard_rank = 0; c->shard_world = 1;
            return nb;
        }
    }
    // Extension of a table that already covers a prefix (a file that is still being staged): only the bytes behind the last complete block
    // are swept -- the sweep, the chain check and the copies to the host used to run over the whole resident prefix every ~128 MiB, i.e.
    // quadratic work in the file size (round-2 advisor).  The blocks known before keep their entries; the new ones are appended on the
    // device and on the host.  Anything unusual (no candidate at the expected offset, a chain that does not prove itself) falls back to
    // the full pass below.
    if (extend && old_nb > 0 && !c->plain_text && (int64_t)c->h_coff.size() == old_nb) {
        const int r_inc = index_extend_tail(c, old_nb);
        if (r_inc < 0) return -1;
        if (r_inc > 0) {
            if (c->shard_b1 == old_nb) c->shard_b1 = c->n_blocks;            // a whole-file scan follows the table
            return c->n_blocks;
        }
    }
    const uint8_t *d = (const uint8_t *)c->comp.p; const uint64_t n = c->comp_len;
    int64_t nspans = (int64_t)((n + 65535) / 65536);
    DevBuf &cnt = c->sg_cnt, &base = c->sg_base, &cand = c->sg_cand, &hits = c->sg_hits; uint64_t total = 0; int rc = 0;   // kept across calls
    auto cleanup = [&]() {};
    if (cnt.ensure((size_t)nspans * 4 + 64) || base.ensure((size_t)(nspans + 1) * 4 + 64) || hits.ensure((size_t)nspans * SIG_SLOTS * 2 + 64) || c->d_nfixed.ensure(64)) { cleanup(); return fail(c, "hipMalloc failed"); }
    (void)hipMemsetAsync(c->d_nfixed.p, 0, 4, c->stream);
    {
        KTimer t(c, DHTS_K_SIGSCAN);
        hipLaunchKernelGGL(bgzf_sig_count, dim3((unsigned)((nspans * 64 + 255) / 256)), dim3(256), 0, c->stream, d, n, (uint32_t *)cnt.p, (uint16_t *)hits.p, (uint32_t *)c->d_nfixed.p);
    }
    const uint32_t *in[1] = {(const uint32_t *)cnt.p}; uint32_t *o32[1] = {(uint32_t *)base.p};
    rc = run_scan(c, 1, in, o32, nullptr, nspans, &total);
    if (rc) { cleanup(); return -1; }
    int64_t ncand = (int64_t)total;
    bool need_seq = (ncand == 0);
    if (!need_seq) {
        if (cand.ensure((size_t)ncand * 8) || c->coff.ensure((size_t)ncand * 8) || c->clen.ensure((size_t)ncand * 4) || c->isize.ensure((size_t)ncand * 4) ||
            c->d_nfixed.ensure(64)) { cleanup(); return fail(c, "hipMalloc failed"); }
        uint32_t ovf = 0;
        if (hipMemcpyAsync(&ovf, c->d_nfixed.p, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { cleanup(); return fail(c, "bgzf index sync failed"); }
        {
            KTimer t(c, DHTS_K_SIGSCAN);
            if (ovf) hipLaunchKernelGGL(bgzf_sig_write, dim3((unsigned)((nspans * 64 + 255) / 256)), dim3(256), 0, c->stream, d, n, (const uint32_t *)base.p, (uint64_t *)c->coff.p, (uint64_t)0);
            else hipLaunchKernelGGL(bgzf_sig_gather, dim3((unsigned)((nspans + 255) / 256)), dim3(256), 0, c->stream, (const uint32_t *)cnt.p, (const uint32_t *)base.p, (const uint16_t *)hits.p, nspans, (uint64_t *)c->coff.p, (uint64_t)0);
        }
        (void)hipMemsetAsync(c->d_nfixed.p, 0, 8, c->stream);
        hipLaunchKernelGGL(bgzf_chain_check, dim3((unsigned)((ncand + 255) / 256)), dim3(256), 0, c->stream, d, n, (const uint64_t *)c->coff.p, ncand,
                           (uint32_t *)c->clen.p, (uint32_t *)c->isize.p, (uint32_t *)c->d_nfixed.p, c->partial_tail ? 1 : 0, (uint64_t)0);
        uint32_t bad[2] = {0, 0};
        if (hipMemcpyAsync(bad, c->d_nfixed.p, 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { cleanup(); return fail(c, "bgzf index sync failed"); }
        need_seq = bad[0] != 0;
        c->n_blocks = ncand - (int64_t)bad[1]; c->bgzf_status = 0;       // (cut candidates are the last ones: chain proof)
    }
    if (need_seq) {
        // unusual / corrupt container: restate htslib's sequential walk on the device
        int64_t cap = (int64_t)(n / 26) + 2;
        if (c->coff.ensure((size_t)cap * 8) || c->clen.ensure((size_t)cap * 4) || c->isize.ensure((size_t)cap * 4) || c->d_res.ensure(64)) { cleanup(); return fail(c, "hipMalloc failed"); }
        hipLaunchKernelGGL(bgzf_chain_walk_seq, dim3(1), dim3(1), 0, c->stream, d, n, (uint64_t *)c->coff.p, (uint32_t *)c->clen.p, (uint32_t *)c->isize.p, cap, (int64_t *)c->d_res.p);
        int64_t res[2] = {0, 0};
        if (hipMemcpyAsync(res, c->d_res.p, 16, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { cleanup(); return fail(c, "bgzf index sync failed"); }
        c->n_blocks = res[0]; c->bgzf_status = (int)res[1];
        if (c->partial_tail && c->bgzf_status == -2) c->bgzf_status = 0;      // the window ends inside a block: expected, the block belongs to the next window
    }
    cleanup();
    // uoff = exclusive prefix of the recorded ISIZE values (each <= 65,537: isize_placed)
    const int64_t nb = c->n_blocks;
    ENSURE(c, c->uoff, (size_t)(nb + 1) * 8 + 64);
    ENSURE(c, c->blk_status, (size_t)(nb + 1) * 4);
    if (nb > 0) {
        const uint32_t *in2[1] = {(const uint32_t *)c->isize.p}; uint64_t *o64[1] = {(uint64_t *)c->uoff.p};
        uint64_t tot2 = 0;
        if (run_scan(c, 1, in2, nullptr, o64, nb, &tot2)) return -1;
    } else { uint64_t z = 0; HIPCHK(c, hipMemcpy(c->uoff.p, &z, 8, hipMemcpyHostToDevice)); }
    c->h_coff.resize(nb); c->h_clen.resize(nb); c->h_isize.resize(nb); c->h_uoff.resize(nb + 1);
    if (nb) {
        HIPCHK(c, hipMemcpy(c->h_coff.data(), c->coff.p, nb * 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(c->h_clen.data(), c->clen.p, nb * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(c->h_isize.data(), c->isize.p, nb * 4, hipMemcpyDeviceToHost));
    }
    HIPCHK(c, hipMemcpy(c->h_uoff.data(), c->uoff.p, (nb + 1) * 8, hipMemcpyDeviceToHost));
    if (extend) {
        if (nb < old_nb) return fail(c, "internal: the block table shrank while the file was being staged");
        if (c->shard_b1 == old_nb) c->shard_b1 = nb;            // a whole-file scan follows the table
        return nb;
    }
    c->shard_b0 = 0; c->shard_b1 = nb; c->shard_rank = 0; c->shard_world = 1;
    return nb;
}

// test aid (not part of the public header): index the first `nbytes` of the resident bytes as if the rest had not arrived yet -- the
// first call builds the table, later calls extend it behind its last complete block (what dhts_bgzf_index_staged does while a file is
// being staged); nbytes >= the resident length ends the pretence
extern "C" int64_t dhts_debug_index_prefix(dhts_ctx *c, uint64_t nbytes) {
    if (!c) return -1;
    if (c->debug_full_len == 0) c->debug_full_len = c->comp_len;
    const bool all = nbytes >= c->debug_full_len;
    const bool extend = c->n_blocks > 0 && c->debug_prefix;
    c->comp_len = all ? c->debug_full_len : nbytes; c->partial_tail = !all; c->growing = !all; c->debug_prefix = true;
    const int64_t r = index_impl(c, extend);
    if (all) { c->debug_prefix = false; c->debug_full_len = 0; }
    return r;
}
int dhts_bgzf_table(const dhts_ctx *c, uint64_t *coff, uint32_t *clen, uint32_t *isize, int64_t cap) {
    if (!c) return -1;
    int64_t n = c->n_blocks < cap ? c->n_blocks : cap;
    if (coff) memcpy(coff, c->h_coff.data(), n * 8);
    if (clen) memcpy(clen, c->h_clen.data(), n * 4);
    if (isize) memcpy(isize, c->h_isize.data(), n * 4);
    return c->bgzf_status;
}

static BgzfTable dev_table(dhts_ctx *c) {
    BgzfTable t; t.coff = (const uint64_t *)c->coff.p; t.clen = (const uint32_t *)c->clen.p; t.isize = (const uint32_t *)c->isize.p;
    t.uoff = (const uint64_t *)c->uoff.p; t.n = c->n_blocks; return t;
}

// workgroups of the persistent inflate kernels that the device holds at once (occupancy query, first use)
static int wave_slots(dhts_ctx *c) {
    if (c->wave_slots == 0) {
        static const int64_t env_wg = getenv("DHTS_WAVE_WG_PER_CU") ? atoll(getenv("DHTS_WAVE_WG_PER_CU")) : 0;      // tuning knob
        int per_cu = 0, per_cu2 = 0; hipDeviceProp_t pr;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)bgzf_inflate_fused, 64, 0) != hipSuccess || per_cu < 1) per_cu = 8;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu2, (const void *)bgzf_huff_decode_wave, 64, 0) != hipSuccess || per_cu2 < 1) per_cu2 = 8;
        if (per_cu2 > per_cu) per_cu = per_cu2;
        if (hipGetDeviceProperties(&pr, c->device) != hipSuccess) return fail(c, "hipGetDeviceProperties failed");
        if (env_wg > 0) per_cu = (int)env_wg;
        c->wave_slots = (int64_t)per_cu * pr.multiProcessorCount;
    }
    return 0;
}
// phase A over [b0, b0+nb): tokens + literals into the scratch
static int huff_blocks(dhts_ctx *c, int64_t b0, int64_t nb, int force = -1) {      // force: -1 default choice, 0 / 1 lane kernel (all symbols in LDS / far table), 2 / 3 wave kernel into fixed slots / the packed pool
    ENSURE(c, c->meta, (size_t)nb * sizeof(InflateMeta));
    BgzfTable t = dev_table(c);
    // Two kernels fill the scratch (same format, cross-checked by the tests):
    //   wave: one WAVE per BGZF block, table-driven, persistent (bgzf_huff_wave.hip): the product path for every launch size since round 3
    //         (measured on MI355X per 65,536 blocks in launches of 131,072: 9.5 ms; the round-2 version of it took 16.3 ms);
    //   lane: one LANE per block, canonical arithmetic (bgzf_inflate.hip): 13.0 ms per 65,536 blocks in long launches and never less than one
    //         lane's serial decode of a whole block (13-15 ms) in short ones; kept as the cross-check of the wave kernel (DHTS_PHASE_A=lane).
    static const char *env_a = getenv("DHTS_PHASE_A");
    const bool env_lane = force >= 0 ? (force != 2 && force != 3) : (env_a && !strcmp(env_a, "lane"));
    if (!env_lane) {
        // persistent launch: as many workgroups (one wave each) as the device holds at once, each with its own staging slices and block
        // assembly area; the workgroups take blocks from a counter that starts behind the blocks they begin with.  `packed`: the blocks'
        // tokens and literals go to a pool, each block exactly the room it needs (force == 2, the tests' cross-check: fixed slots)
        const bool packed = force < 0 || force == 3;
        if (wave_slots(c)) return -1;
        {   // DHTS_POOL_PER_BLOCK: room per block in the packed scratch (tuning knob; the tests use a tiny value to exercise the retry)
            const int64_t env_ppb = getenv("DHTS_POOL_PER_BLOCK") ? atoll(getenv("DHTS_POOL_PER_BLOCK")) : 0;        // (read per launch: a test sets it)
            if (env_ppb > 0 && c->pool_per_block == 65536 + 4096) c->pool_per_block = env_ppb;
        }
        const int64_t grid = nb < c->wave_slots ? nb : c->wave_slots;
        ENSURE(c, c->stg_lit, (size_t)grid * HW_STAGE_LIT_BYTES + 64);
        ENSURE(c, c->stg_tok, (size_t)grid * HW_STAGE_TOK_WORDS * 4 + 64);
        ENSURE(c, c->wave_ctr, 64);
        HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)c->wave_ctr.p, (int)grid, 1, c->stream));
        uint64_t pool_cap = 0;
        if (packed) {
            pool_cap = (uint64_t)nb * (uint64_t)c->pool_per_block;
            ENSURE(c, c->lit, pool_cap + 8192);
            ENSURE(c, c->blk_off, (size_t)nb * 8 + 64);
            ENSURE(c, c->wg_lit[0], (size_t)grid * (DHTS_LIT_STRIDE + 64) + 8192);
            ENSURE(c, c->wg_tok[0], (size_t)grid * DHTS_TOK_STRIDE * 4 + 64);
            HIPCHK(c, hipMemsetAsync((uint8_t *)c->wave_ctr.p + 16, 0, 8, c->stream));
        } else {
            ENSURE(c, c->lit, (size_t)nb * DHTS_LIT_STRIDE + 8192);
            ENSURE(c, c->tok, (size_t)nb * DHTS_TOK_STRIDE * 4 + 64);
        }
        c->huff_packed = packed;
        KTimer tm(c, DHTS_K_HUFF);
        hipLaunchKernelGGL(bgzf_huff_decode_wave, dim3((unsigned)grid), dim3(64), 0, c->stream, (const uint8_t *)c->comp.p, t, b0, (int32_t)nb,
                           (uint8_t *)c->lit.p, (uint32_t *)c->tok.p, (InflateMeta *)c->meta.p, (uint8_t *)c->stg_lit.p, (uint32_t *)c->stg_tok.p, (uint32_t *)c->wave_ctr.p,
                           packed ? (uint8_t *)c->lit.p : (uint8_t *)nullptr, (unsigned long long)pool_cap, (unsigned long long *)((uint8_t *)c->wave_ctr.p + 16),
                           (unsigned long long *)c->blk_off.p, (uint8_t *)c->wg_lit[0].p, (uint32_t *)c->wg_tok[0].p);
    } else {
        ENSURE(c, c->lit, (size_t)nb * DHTS_LIT_STRIDE + 8192);
        ENSURE(c, c->tok, (size_t)nb * DHTS_TOK_STRIDE * 4 + 64);
        c->huff_packed = false;
        KTimer tm(c, DHTS_K_HUFF);
        // a launch that six waves per CU can hold at once keeps every symbol in LDS; a longer one runs eight waves per CU
        static const int64_t env_nlo = getenv("DHTS_PHASE_A_NLO") ? atoll(getenv("DHTS_PHASE_A_NLO")) : 0;     // tuning knob: 196 or 288
        const uint32_t nlo = force == 0 ? A_NLO_ALL : force == 1 ? A_NLO_FAR : env_nlo == 196 ? A_NLO_FAR : env_nlo == 288 ? A_NLO_ALL : (nb > 98304 ? A_NLO_FAR : A_NLO_ALL);
        hipLaunchKernelGGL(bgzf_huff_decode, dim3((unsigned)((nb + A_SL - 1) / A_SL)), dim3(64), A_LDS_BYTES_FOR(nlo), c->stream, (const uint8_t *)c->comp.p, t, b0, (int32_t)nb,
                           (uint8_t *)c->lit.p, (uint32_t *)c->tok.p, (InflateMeta *)c->meta.p, nlo);
    }
    HIPCHK(c, hipGetLastError());
    c->huff_b0 = b0; c->huff_nb = nb;
    return 0;
}

// inflate blocks [b0, b0+nb) into `out` (device) so that block b lands at out + (uoff[b] - out_base)
static int launch_lz(dhts_ctx *c, int64_t b0, int64_t nb, uint8_t *out, uint64_t out_base, hipStream_t s) {
    BgzfTable t = dev_table(c);
    {
        KTimer tm(c, DHTS_K_LZ, s);
        hipLaunchKernelGGL(bgzf_lz_resolve, dim3((unsigned)((nb + B_NW - 1) / B_NW)), dim3(64 * B_NW), B_LDS_BYTES_NW, s, (const uint8_t *)c->comp.p, t, b0, (int32_t)nb,
                           (const uint8_t *)c->lit.p, (const uint32_t *)c->tok.p, (const InflateMeta *)c->meta.p, c->huff_b0, out, out_base, (int32_t *)c->blk_status.p,
                           c->huff_packed ? (const unsigned long long *)c->blk_off.p : (const unsigned long long *)nullptr);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}
// the product path of the inflate stage: ONE persistent launch decodes and resolves blocks [b0, b0+nb) (bgzf_inflate_fused); `alt` selects the
// second set of workgroup areas (a launch on stream_b may run beside one on the main stream)
static int launch_fused(dhts_ctx *c, int64_t b0, int64_t nb, uint8_t *out, uint64_t out_base, hipStream_t s, int alt) {
    if (wave_slots(c)) return -1;
    const int64_t grid = nb < c->wave_slots ? nb : c->wave_slots;
    DevBuf &sl = alt ? c->stg2_lit : c->stg_lit, &stk = alt ? c->stg2_tok : c->stg_tok;
    ENSURE(c, sl, (size_t)grid * HW_STAGE_LIT_BYTES + 64);
    ENSURE(c, stk, (size_t)grid * HW_STAGE_TOK_WORDS * 4 + 64);
    ENSURE(c, c->wg_lit[alt], (size_t)grid * (DHTS_LIT_STRIDE + 64) + 8192);
    ENSURE(c, c->wg_tok[alt], (size_t)grid * DHTS_TOK_STRIDE * 4 + 64);
    ENSURE(c, c->wave_ctr, 64);
    uint32_t *ctr = (uint32_t *)c->wave_ctr.p + (alt ? 8 : 0);
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)ctr, (int)grid, 1, s));
    BgzfTable t = dev_table(c);
    {
        KTimer tm(c, DHTS_K_LZ, s);
        hipLaunchKernelGGL(bgzf_inflate_fused, dim3((unsigned)grid), dim3(64), 0, s, (const uint8_t *)c->comp.p, t, b0, (int32_t)nb,
                           (uint8_t *)c->wg_lit[alt].p, (uint32_t *)c->wg_tok[alt].p, (uint8_t *)sl.p, (uint32_t *)stk.p, ctr, out, out_base, (int32_t *)c->blk_status.p);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}
static bool inflate_split() {       // default: phase A over the shard into the packed scratch, phase B per batch; DHTS_INFLATE=fused: one launch per batch does both
    static const bool v = !(getenv("DHTS_INFLATE") && !strcmp(getenv("DHTS_INFLATE"), "fused"));
    return v;
}
static int huff_ensure(dhts_ctx *c, int64_t b0, int64_t nb, int64_t ahead_limit);
static int inflate_blocks(dhts_ctx *c, int64_t b0, int64_t nb, uint8_t *out, uint64_t out_base, int64_t ahead_limit) {
    if (nb <= 0) return 0;
    if (c->plain_text) {                                     // nothing to inflate: the pieces are copied to their place in the stream
        HIPCHK(c, hipMemcpyAsync(out + (c->h_uoff[b0] - out_base), (const uint8_t *)(c->gz_plain ? c->gz_out.p : c->comp.p) + c->h_coff[b0], c->h_uoff[b0 + nb] - c->h_uoff[b0], hipMemcpyDeviceToDevice, c->stream));
        return 0;
    }
    discard_prefetch(c);                                   // (phase A below may reallocate the scratch a prefetched phase B reads)
    if (!inflate_split()) return launch_fused(c, b0, nb, out, out_base, c->stream, 0);
    if (huff_ensure(c, b0, nb, ahead_limit)) return -1;    // (callers that size `out` from the block table have called it before they looked)
    return launch_lz(c, b0, nb, out, out_base, c->stream);
}
// Phase A over a range that covers blocks [b0, b0 + nb) (and runs ahead of them, up to `ahead_limit`), unless the scratch already holds them;
// then the block table is made to agree with what the blocks really inflate to (isize_repair).  Callers that derive buffer sizes or stream
// offsets from h_uoff call this FIRST: the table may change here.
static int isize_repair(dhts_ctx *c);
static int huff_ensure(dhts_ctx *c, int64_t b0, int64_t nb, int64_t ahead_limit) {
    if (nb <= 0 || c->plain_text || !inflate_split()) return 0;
    if (!(b0 >= c->huff_b0 && b0 + nb <= c->huff_b0 + c->huff_nb)) {
        discard_prefetch(c);
        // (a range that overflowed the packed scratch is decoded again with 152 KiB per block; the NEXT range goes back to the packed size)
        if (c->pool_full_pending) c->pool_full_pending = false; else c->pool_per_block = 65536 + 4096;
        static const int64_t env_super = getenv("DHTS_SUPER_BLOCKS") ? atoll(getenv("DHTS_SUPER_BLOCKS")) : 0;   // tuning knob
        int64_t sb = env_super > 0 ? env_super : c->super_blocks;
        {
            // the token/literal scratch of a super-batch may take at most 45 % of the HBM that is free (or already ours)
            size_t fr = 0, tot = 0;
            if (hipMemGetInfo(&fr, &tot) == hipSuccess) {
                const double per_block = ((double)c->pool_per_block + 8.0 + sizeof(InflateMeta)) * 1.125;
                size_t pooled = 0; { std::lock_guard<std::mutex> lk(g_pool_mu); pooled = g_pool_bytes; }       // (idle buffers of earlier contexts can be taken back)
                const int64_t fit = (int64_t)(0.45 * ((double)fr + (double)pooled + (double)c->lit.cap + (double)c->tok.cap) / per_block);
                if (sb > fit) sb = fit;
            }
            if (sb < 16384) sb = 16384;
        }
        int64_t want = sb > nb ? sb : nb;
        if (b0 + want > ahead_limit) want = ahead_limit - b0;
        if (want < nb) want = nb;
        if (huff_blocks(c, b0, want)) return -1;
        if (isize_repair(c)) return -1;
    }
    return 0;
}
// htslib never reads the ISIZE field of a BGZF trailer: a block is whatever its DEFLATE stream inflates to (at most 64 KiB), valid when the
// CRC-32 agrees (bgzf.c:762-824).  The scan here PLACES every block at the prefix sum of the ISIZE fields -- that is what lets a shard start
// without decoding its predecessors -- so a file whose ISIZE fields are wrong (no tool writes such a file; the reference reads it) needs its
// table corrected: phase A has just decoded blocks [huff_b0, huff_b0 + huff_nb) and knows their true lengths; where they differ from the
// table, the table takes the decoded length, every offset behind the first change moves, and the positions the context remembers (first
// record, scan window ends) move with their blocks.  Costs one small kernel and one 4-byte read per phase-A launch.
static int isize_repair(dhts_ctx *c) {
    const int64_t b0 = c->huff_b0, n = c->huff_nb;
    if (n <= 0) return 0;
    ENSURE(c, c->d_nfixed, 64);
    HIPCHK(c, hipMemsetAsync((uint8_t *)c->d_nfixed.p + 32, 0, 4, c->stream));
    hipLaunchKernelGGL(bgzf_len_check, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const InflateMeta *)c->meta.p, (const uint32_t *)c->isize.p, b0, (int32_t)n, (uint32_t *)((uint8_t *)c->d_nfixed.p + 32));
    uint32_t cnt = 0;
    HIPCHK(c, hipMemcpyAsync(&cnt, (uint8_t *)c->d_nfixed.p + 32, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (cnt == 0) return 0;
    std::vector<InflateMeta> m((size_t)n);
    HIPCHK(c, hipMemcpy(m.data(), c->meta.p, (size_t)n * sizeof(InflateMeta), hipMemcpyDeviceToHost));
    int64_t first = -1, placed = 0;
    const std::vector<uint64_t> old_uoff = c->h_uoff;
    for (int64_t k = 0; k < n; k++) if (m[(size_t)k].status == 0 && m[(size_t)k].outlen != c->h_isize[(size_t)(b0 + k)] && m[(size_t)k].outlen <= 65536u) {
        c->h_isize[(size_t)(b0 + k)] = m[(size_t)k].outlen; if (first < 0) first = b0 + k; placed++;
    }
    if (first < 0) return 0;
    const int64_t nbk = c->n_blocks;
    for (int64_t i = first; i < nbk; i++) c->h_uoff[(size_t)i + 1] = c->h_uoff[(size_t)i] + c->h_isize[(size_t)i];
    HIPCHK(c, hipMemcpy((uint32_t *)c->isize.p + b0, c->h_isize.data() + b0, (size_t)n * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy((uint64_t *)c->uoff.p + first + 1, c->h_uoff.data() + first + 1, (size_t)(nbk - first) * 8, hipMemcpyHostToDevice));
    // remembered stream positions move with the block they lie in
    auto remap = [&](uint64_t u) -> uint64_t {
        if (u == ~0ull || u <= old_uoff[(size_t)first]) return u;
        int64_t lo = first, hi = nbk;                           // last block j with old_uoff[j] <= u
        while (lo < hi) { const int64_t mid = (lo + hi + 1) / 2; if (old_uoff[(size_t)mid] <= u) lo = mid; else hi = mid - 1; }
        uint64_t w = u - old_uoff[(size_t)lo]; const uint64_t room = c->h_uoff[(size_t)lo + (lo < nbk ? 1 : 0)] - c->h_uoff[(size_t)lo];
        if (lo < nbk && w > room) w = room;
        return c->h_uoff[(size_t)lo] + w;
    };
    // a position that was computed as h_uoff[blk] + an offset inside block blk (an index's virtual offset) moves with block blk: when that
    // block, or one in front of it inside the window, understated its length, the old table would place the offset in a later block
    auto remap_at = [&](uint64_t u, int64_t blk) -> uint64_t {
        if (u == ~0ull || blk < first || blk > nbk || u < old_uoff[(size_t)blk]) return remap(u);
        return c->h_uoff[(size_t)blk] + (u - old_uoff[(size_t)blk]);
    };
    const bool in_win = !c->wins.empty() && c->win_cur < c->wins.size();
    const bool first_is_win = in_win && c->scan_first_uoff == c->wins[c->win_cur].first_uoff, end_is_win = in_win && c->scan_end_uoff == c->wins[c->win_cur].end_uoff;
    const bool first_anchored = !first_is_win && c->scan_first_blk >= 0 && c->scan_first_uoff == c->scan_first_anchor;
    c->first_rec_uoff = remap(c->first_rec_uoff);
    for (auto &w : c->wins) { w.first_uoff = remap_at(w.first_uoff, w.first_blk); w.end_uoff = remap_at(w.end_uoff, w.end_blk); }
    c->scan_first_uoff = first_is_win ? c->wins[c->win_cur].first_uoff : first_anchored ? remap_at(c->scan_first_uoff, c->scan_first_blk) : remap(c->scan_first_uoff);
    c->scan_end_uoff = end_is_win ? c->wins[c->win_cur].end_uoff : remap(c->scan_end_uoff);
    if (first_anchored) c->scan_first_anchor = c->scan_first_uoff;
    for (auto &w : c->wins) if (w.first_uoff < c->first_rec_uoff) w.first_uoff = c->first_rec_uoff;
    c->isize_repaired += placed; if (c->in_scratch_retry) c->isize_repaired_retry += placed;
    if (g_debug) fprintf(stderr, "[dhts] %u blocks inflate to another length than their ISIZE field says: block table re-placed from block %lld on\n", cnt, (long long)first);
    return 0;
}
// Some block of [b0, b0 + nb) found the packed scratch exhausted (DHTS_BLK_ERR_SCRATCH): phase A runs over the range again with the full
// 152 KiB per block.  The first isize_repair passed over those blocks (their status was not 0); this one sees their decoded lengths, so the
// block table MAY MOVE here: the caller reads its sizes and offsets from h_uoff again before it launches phase B.
static int scratch_retry_phase_a(dhts_ctx *c, int64_t b0, int64_t nb, int64_t ahead_limit) {
    discard_prefetch(c);
    c->pool_per_block = (int64_t)DHTS_LIT_STRIDE + (int64_t)DHTS_TOK_STRIDE * 4; c->pool_full_pending = true; c->huff_b0 = c->huff_nb = 0;
    c->scratch_retries++; c->in_scratch_retry = true;
    const int rc = huff_ensure(c, b0, nb, ahead_limit);
    c->in_scratch_retry = false;
    return rc;
}
int dhts_bgzf_repair_stats(const dhts_ctx *c, int64_t out[3]) {
    if (!c || !out) return -1;
    out[0] = c->isize_repaired; out[1] = c->scratch_retries; out[2] = c->isize_repaired_retry;
    return 0;
}

// how many blocks phase A may decode ahead of the batch that needs them (default 524,288: a whole 10 GB file in one launch, 67 GB of token /
// literal scratch).  A caller that serves many queries from one process wants a scratch the device pool can keep: 196,608 blocks = two full
// rounds of the 1,536 resident waves, 29 GB.
extern "C" void dhts_set_super_blocks(dhts_ctx *c, int64_t n) { if (c && n >= 16384) c->super_blocks = n; }
// SEQ as the file's 4-bit codes: seq.bytes holds (l + 1) / 2 bytes per row at seq.off, seq.len the number of bases (0: "*"); the batch says so
// in seq_packed.  Saves 18 % of an all-column read-back; the consumer expands with "=ACMGRSVTWYHKDBN" (high nibble first).
extern "C" void dhts_bam_set_seq_packed(dhts_ctx *c, int on) { if (c) c->seq_packed = on != 0; }
extern "C" void dhts_bam_set_qual_packed(dhts_ctx *c, int on) { if (c) c->qual_packed = on != 0; }
int64_t dhts_bgzf_inflate_to_host(dhts_ctx *c, int64_t blk0, int64_t nblk, uint8_t *out, uint64_t cap, int32_t *blk_status) {
    if (!c) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    if (blk0 < 0 || nblk < 0 || blk0 + nblk > c->n_blocks) return fail(c, "block range out of bounds");
    if (nblk == 0) return 0;
    if (huff_ensure(c, blk0, nblk, blk0 + nblk)) return -1;          // (the table may be corrected here: sizes are read behind it)
    uint64_t base = c->h_uoff[blk0], total = c->h_uoff[blk0 + nblk] - base;
    if (total > cap) return fail(c, "output capacity too small (%llu needed)", (unsigned long long)total);
    ENSURE(c, c->ubuf[0], total + PAD_BYTES);
    HIPCHK(c, hipMemsetAsync(c->ubuf[0].p, 0, total + PAD_BYTES, c->stream));
    std::vector<int32_t> bs((size_t)nblk);
    for (int attempt = 0; ; attempt++) {
        if (inflate_blocks(c, blk0, nblk, (uint8_t *)c->ubuf[0].p, base, blk0 + nblk)) return -1;
        HIPCHK(c, hipMemcpyAsync(bs.data(), (int32_t *)c->blk_status.p + blk0, nblk * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        bool scratch = false;
        for (int64_t k = 0; k < nblk; k++) if (bs[(size_t)k] == DHTS_BLK_ERR_SCRATCH) { scratch = true; break; }
        if (!scratch) break;
        if (attempt > 0) return fail(c, "internal: phase-A scratch exhausted twice");
        // (see batch_begin) the repeat of phase A may move the table: the range is sized and placed again from what it says now
        if (scratch_retry_phase_a(c, blk0, nblk, blk0 + nblk)) return -1;
        base = c->h_uoff[blk0]; total = c->h_uoff[blk0 + nblk] - base;
        if (total > cap) return fail(c, "output capacity too small (%llu needed)", (unsigned long long)total);
        ENSURE(c, c->ubuf[0], total + PAD_BYTES);
        HIPCHK(c, hipMemsetAsync(c->ubuf[0].p, 0, total + PAD_BYTES, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(out, c->ubuf[0].p, total, hipMemcpyDeviceToHost, c->stream));
    if (blk_status) memcpy(blk_status, bs.data(), (size_t)nblk * 4);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    timing_collect(c);
    return (int64_t)total;
}
