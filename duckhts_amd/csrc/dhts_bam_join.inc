// dhts_bam_join.inc -- part of dhts_api.hip (included there, inside its extern "C" block; not a translation unit of its own):
// interval overlap join (interval arrays or BED), typed tag columns.
// ---- interval overlap join ------------------------------------------------------------------------------------------------
int dhts_bam_set_overlap_intervals(dhts_ctx *c, const int32_t *tid, const int64_t *beg, const int64_t *end, int64_t n) {
    if (!c) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    c->ov_active = false; c->ov_n = 0;
    if (n <= 0) return 0;
    if (!c->bam_open) return fail(c, "dhts_bam_open not called");      // the intervals are resolved against the header's reference table
    if (!tid || !beg || !end) return fail(c, "overlap intervals: null array");
    if (n > 0xfffffff0ll) return fail(c, "overlap intervals: too many intervals");
    const int32_t n_ref = (int32_t)c->ref_name.size();
    std::vector<uint32_t> order; order.reserve((size_t)n);
    for (int64_t i = 0; i < n; i++) if (tid[i] >= 0 && tid[i] < n_ref) order.push_back((uint32_t)i);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return tid[a] != tid[b] ? tid[a] < tid[b] : beg[a] < beg[b]; });
    const size_t m = order.size();
    std::vector<int64_t> sb(m), se(m), pm(m), bm((m + 63) / 64 + 1, INT64_MIN); std::vector<uint32_t> first((size_t)n_ref + 1, 0);
    for (size_t k = 0; k < m; k++) {
        const uint32_t i = order[k];
        sb[k] = beg[i]; se[k] = end[i];
        pm[k] = (k > 0 && tid[order[k - 1]] == tid[i] && pm[k - 1] > end[i]) ? pm[k - 1] : end[i];
        if (end[i] > bm[k >> 6]) bm[k >> 6] = end[i];
        first[(size_t)tid[i] + 1]++;
    }
    for (int32_t t = 0; t < n_ref; t++) first[(size_t)t + 1] += first[t];
    ENSURE(c, c->ov_beg, m * 8 + 64); ENSURE(c, c->ov_end, m * 8 + 64); ENSURE(c, c->ov_pmax, m * 8 + 64); ENSURE(c, c->ov_bmax, bm.size() * 8 + 64); ENSURE(c, c->ov_id, m * 4 + 64); ENSURE(c, c->ov_first, ((size_t)n_ref + 1) * 4 + 64);
    if (m) {
        HIPCHK(c, hipMemcpy(c->ov_beg.p, sb.data(), m * 8, hipMemcpyHostToDevice)); HIPCHK(c, hipMemcpy(c->ov_end.p, se.data(), m * 8, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->ov_pmax.p, pm.data(), m * 8, hipMemcpyHostToDevice)); HIPCHK(c, hipMemcpy(c->ov_id.p, order.data(), m * 4, hipMemcpyHostToDevice));
    }
    HIPCHK(c, hipMemcpy(c->ov_bmax.p, bm.data(), bm.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->ov_first.p, first.data(), ((size_t)n_ref + 1) * 4, hipMemcpyHostToDevice));
    c->ov_active = true; c->ov_n = (int64_t)m;
    return 0;
}

// read_bed rows as the join's intervals (src/interval_udf.c:330-426): the device splits the text into lines and parses chrom / start / end of
// every row (bed_intervals); the host only maps the chrom names, where they change, to the header's reference ids.  Interval id = row number of
// read_bed (meta lines do not count).  A row whose start or end is NULL, or whose chrom the BAM header does not have, never matches.  text = the
// (uncompressed) BED bytes.  Returns the number of rows, < 0 on error (a line with fewer than 3 fields: read_bed's error).
extern "C" int64_t dhts_bam_set_overlap_bed(dhts_ctx *c, const uint8_t *text, uint64_t n) {
    if (!c) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    c->ov_active = false; c->ov_n = 0;
    if (!c->bam_open) return fail(c, "dhts_bam_open not called");
    if (n && !text) return fail(c, "overlap bed: null text");
    if (n >= 0xfffffff0ull) return fail(c, "overlap bed: text of 4 GiB or more");
    if (n == 0) return 0;
    DevBuf d_text, d_rows; LineBufs lines;                                      // (buffers of its own: the context's belong to its scan)
    ENSURE(c, d_text, n + 64);
    HIPCHK(c, hipMemcpyAsync(d_text.p, text, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync((uint8_t *)d_text.p + n, 0, 64, c->stream));
    const uint8_t *u = (const uint8_t *)d_text.p;
    LineTab T;                                                                  // the text is whole: its last line counts when it has no newline
    if (line_table(c, lines, nullptr, u, 0, n, text[n - 1] != '\n', ~0ull, -1, T)) return -1;
    const int64_t nlines = T.nlines; const int last_open = T.last_open;      // (n > 0: at least one line)
    ENSURE(c, d_rows, (size_t)nlines * sizeof(TbxLine) + 64);
    hipLaunchKernelGGL(bed_intervals, dim3((unsigned)((nlines + 255) / 256)), dim3(256), 0, c->stream, u, (const uint32_t *)lines.line_off.p, nlines, n, last_open, (TbxLine *)d_rows.p);
    HIPCHK(c, hipGetLastError());
    std::vector<TbxLine> rows((size_t)nlines);
    HIPCHK(c, hipMemcpyAsync(rows.data(), d_rows.p, (size_t)nlines * sizeof(TbxLine), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::map<std::string, int32_t> tid_of;
    for (size_t t = 0; t < c->ref_name.size(); t++) tid_of.emplace(c->ref_name[t], (int32_t)t);   // (a name listed twice: the first @SQ, as sam_hdr_name2tid's hash keeps)
    std::vector<int32_t> tid; std::vector<int64_t> beg, end; tid.reserve((size_t)nlines); beg.reserve((size_t)nlines); end.reserve((size_t)nlines);
    int32_t cur = -1; int64_t lineno = 0;
    for (const TbxLine &r : rows) {
        ++lineno;
        if (r.flag == 1) continue;
        if (r.flag == 2) return fail(c, "read_bed: BED line has fewer than 3 tab-delimited fields (line %lld)", (long long)lineno);
        if (!r.same || tid.empty()) { auto it = tid_of.find(std::string((const char *)text + r.name_off, r.name_len)); cur = it == tid_of.end() ? -1 : it->second; }
        tid.push_back((r.flag & 12u) ? -1 : cur); beg.push_back(r.beg); end.push_back(r.end);
    }
    const int64_t m = (int64_t)tid.size();
    if (m && dhts_bam_set_overlap_intervals(c, tid.data(), beg.data(), end.data(), m)) return -1;
    return m;
}
// the same from a file: plain text, or BGZF / gzip members (inflated by a context of its own on the same device)
extern "C" int64_t dhts_bam_set_overlap_bed_path(dhts_ctx *c, const char *path) {
    if (!c) return -1;
    if (!path) return fail(c, "overlap bed: null path");
    std::vector<uint8_t> raw;
    {
        FILE *f = fopen(path, "rb");
        if (!f) return fail(c, "overlap bed: cannot open %s", path);
        uint8_t buf[1 << 16]; size_t got;
        while ((got = fread(buf, 1, sizeof(buf), f)) > 0) raw.insert(raw.end(), buf, buf + got);
        fclose(f);
    }
    if (raw.size() >= 18 && raw[0] == 0x1f && raw[1] == 0x8b) {
        dhts_ctx *t = dhts_create(c->device);
        if (!t) return fail(c, "overlap bed: no context for %s", path);
        std::vector<uint8_t> text; std::string err; bool ok = false;
        do {
            if (dhts_open_host(t, raw.data(), raw.size())) { err = dhts_error(t); break; }
            const int64_t nb = dhts_bgzf_index(t);
            if (nb < 0) { err = dhts_error(t); break; }
            if (nb && huff_ensure(t, 0, nb, nb)) { err = dhts_error(t); break; }      // (the table may be corrected from the decoded lengths: sizes are read behind it)
            text.resize((size_t)t->h_uoff[(size_t)nb] + 64);
            std::vector<int32_t> st((size_t)nb + 1, 0);
            int64_t got = nb ? dhts_bgzf_inflate_to_host(t, 0, nb, text.data(), text.size(), st.data()) : 0;
            if (got < 0 && t->h_uoff[(size_t)nb] + 64 != text.size()) {      // a scratch retry inside moved the block table: once more with its sizes
                text.resize((size_t)t->h_uoff[(size_t)nb] + 64);
                got = dhts_bgzf_inflate_to_host(t, 0, nb, text.data(), text.size(), st.data());
            }
            if (got < 0) { err = dhts_error(t); break; }
            text.resize((size_t)got); ok = true;
        } while (0);
        dhts_destroy(t);
        HIPCHK(c, hipSetDevice(c->device));
        if (!ok) return fail(c, "overlap bed: %s: %s", path, err.c_str());
        return dhts_bam_set_overlap_bed(c, text.data(), text.size());
    }
    return dhts_bam_set_overlap_bed(c, raw.data(), raw.size());
}

static int bam_overlap_join(dhts_ctx *c, const BamStream &st, const BamCols &bc, int64_t nrows, dhts_bam_batch *out) {
    out->ov_off = nullptr; out->ov_ids = nullptr; out->n_ov = 0;
    if (!c->ov_active) return 0;
    const size_t n = (size_t)(nrows > 0 ? nrows : 0);
    ENSURE(c, c->ov_cnt, (n + 1) * 4 + 64); ENSURE(c, c->ov_off, (n + 1) * 4 + 64);
    uint64_t total = 0;
    OverlapDev ov; ov.beg = (const int64_t *)c->ov_beg.p; ov.end = (const int64_t *)c->ov_end.p; ov.pmax = (const int64_t *)c->ov_pmax.p; ov.bmax = (const int64_t *)c->ov_bmax.p; ov.id = (const uint32_t *)c->ov_id.p;
    ov.tid_first = (const uint32_t *)c->ov_first.p; ov.n_ref = (int32_t)c->ref_name.size(); ov.pad = 0;
    if (nrows > 0) {
        {
            KTimer tm(c, DHTS_K_CORE);
            hipLaunchKernelGGL(bam_overlap_cells<false>, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, c->stream, st, ov, (const uint32_t *)c->rec_off.p, bc, nrows,
                               (uint32_t *)c->ov_cnt.p, (const uint32_t *)nullptr, (uint32_t *)nullptr);
        }
        const uint32_t *in[1] = {(const uint32_t *)c->ov_cnt.p}; uint32_t *o32[1] = {(uint32_t *)c->ov_off.p};
        { KTimer tm(c, DHTS_K_SCAN); if (run_scan(c, 1, in, o32, nullptr, nrows, &total)) return -1; }
        if (total > 0xfffffff0ull) return fail(c, "overlap join: more than 2^32 pairs in one batch");
        ENSURE(c, c->ov_ids, total * 4 + 64);
        if (total) {
            KTimer tm(c, DHTS_K_CORE);
            hipLaunchKernelGGL(bam_overlap_cells<true>, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, c->stream, st, ov, (const uint32_t *)c->rec_off.p, bc, nrows,
                               (uint32_t *)nullptr, (const uint32_t *)c->ov_off.p, (uint32_t *)c->ov_ids.p);
        }
        HIPCHK(c, hipGetLastError());
    } else {
        HIPCHK(c, hipMemsetAsync(c->ov_off.p, 0, 4, c->stream));
        ENSURE(c, c->ov_ids, 64);
    }
    out->ov_off = (const uint32_t *)c->ov_off.p; out->ov_ids = (const uint32_t *)c->ov_ids.p; out->n_ov = total;
    return 0;
}

static int bam_tag_columns(dhts_ctx *c, const BamStream &st, int64_t nrows, dhts_bam_batch *out) {
    const int nt = (int)c->tag_sel.size();
    c->tag_out.assign(nt, dhts_col());
    for (int i = 0; i < nt; i++) { memset(&c->tag_out[i], 0, sizeof(dhts_col)); c->tag_out[i].col = c->tag_sel[i]; c->tag_out[i].child_width = 8; }
    out->n_tag_cols = nt; out->tag_cols = c->tag_out.data();
    if (nt == 0 || nrows <= 0) return 0;
    const size_t n = (size_t)nrows;
    const uint32_t stride = (uint32_t)((n + 63) & ~(size_t)63), ostride = (uint32_t)((n + 1 + 63) & ~(size_t)63);
    std::vector<uint16_t> codes(nt);
    std::vector<TagColDev> cd(nt);
    int nsa = 0; size_t nfixed = 0; std::vector<size_t> fixed_at(nt, 0);
    for (int i = 0; i < nt; i++) {
        const StdTag &t = kStdTags[c->tag_sel[i]];
        codes[i] = (uint16_t)((uint8_t)t.tag[0] | ((uint8_t)t.tag[1] << 8));
        memset(&cd[i], 0, sizeof(TagColDev));
        cd[i].kind = t.type == 'H' ? 'Z' : t.type; cd[i].slot = i; cd[i].sa_cnt = cd[i].sa_bytes = -1;
        if (t.type == 'B') cd[i].sa_cnt = nsa++;
        else if (t.type == 'i') { fixed_at[i] = nfixed; nfixed += (n * 8 + 63) & ~(size_t)63; }
        else cd[i].sa_bytes = nsa++;
    }
    ENSURE(c, c->t_codes, nt * 2 + 16); ENSURE(c, c->t_dir, (size_t)nt * stride * 4 + 16); ENSURE(c, c->t_valid, (size_t)nt * n + 64); ENSURE(c, c->t_fixed, nfixed + 64);
    ENSURE(c, c->t_lens, (size_t)(nsa ? nsa : 1) * ostride * 4 + 64); ENSURE(c, c->t_offs, (size_t)(nsa ? nsa : 1) * ostride * 4 + 64); ENSURE(c, c->t_coldev, sizeof(TagColDev) * nt);
    for (int i = 0; i < nt; i++) { cd[i].valid = (uint8_t *)c->t_valid.p + (size_t)i * n; if (cd[i].kind == 'i') cd[i].fixed = (int64_t *)((uint8_t *)c->t_fixed.p + fixed_at[i]); }
    HIPCHK(c, hipMemcpyAsync(c->t_codes.p, codes.data(), nt * 2, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->t_coldev.p, cd.data(), sizeof(TagColDev) * nt, hipMemcpyHostToDevice, c->stream));
    TagCellArgs ta; memset(&ta, 0, sizeof(ta));
    ta.rec_off = (const uint32_t *)c->rec_off.p; ta.dir = (const uint32_t *)c->t_dir.p; ta.stride = stride; ta.nrows = nrows;
    ta.lens = (uint32_t *)c->t_lens.p; ta.offs = (const uint32_t *)c->t_offs.p; ta.ostride = ostride; ta.cols = (const TagColDev *)c->t_coldev.p;
    {
        KTimer tm(c, DHTS_K_CORE);
        hipLaunchKernelGGL(bam_tag_dir, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, c->stream, st, (const uint32_t *)c->rec_off.p, nrows, (const uint16_t *)c->t_codes.p, nt,
                           (uint32_t *)c->t_dir.p, stride);
        hipLaunchKernelGGL(bam_tag_cells<false>, dim3((unsigned)((nrows + 255) / 256), (unsigned)nt), dim3(256), 0, c->stream, st, ta);
    }
    std::vector<uint64_t> tot(nsa ? nsa : 1, 0);
    if (nsa > 0) {
        MScanArgs ma; ma.in = (const uint32_t *)c->t_lens.p; ma.out = (uint32_t *)c->t_offs.p; ma.stride = ostride; ma.n = nrows;
        ma.nparts = (nrows + 1 + SCAN_ITEMS - 1) / SCAN_ITEMS; if (ma.nparts < 1) ma.nparts = 1;
        ENSURE(c, c->t_partial, (size_t)nsa * ma.nparts * 8 + 64); ENSURE(c, c->t_total, (size_t)nsa * 8 + 64);
        ma.partial = (uint64_t *)c->t_partial.p; ma.total = (uint64_t *)c->t_total.p;
        {
            KTimer tm(c, DHTS_K_SCAN);
            hipLaunchKernelGGL(mscan_reduce, dim3((unsigned)ma.nparts, (unsigned)nsa), dim3(256), 0, c->stream, ma);
            hipLaunchKernelGGL(mscan_partials, dim3((unsigned)nsa), dim3(1024), 0, c->stream, ma);
            hipLaunchKernelGGL(mscan_apply, dim3((unsigned)ma.nparts, (unsigned)nsa), dim3(256), 0, c->stream, ma);
        }
        HIPCHK(c, hipMemcpyAsync(tot.data(), c->t_total.p, (size_t)nsa * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        size_t var = 0; std::vector<size_t> at(nt, 0);
        for (int i = 0; i < nt; i++) {
            if (cd[i].sa_cnt >= 0) { if (tot[cd[i].sa_cnt] >= (1ull << 32)) return fail(c, "tag column too large for one batch"); at[i] = var; var += (tot[cd[i].sa_cnt] * 8 + 63) & ~(size_t)63; }
            if (cd[i].sa_bytes >= 0) { if (tot[cd[i].sa_bytes] >= (1ull << 32)) return fail(c, "tag column too large for one batch"); at[i] = var; var += (tot[cd[i].sa_bytes] + 63) & ~(size_t)63; }
        }
        ENSURE(c, c->t_var, var + 64);
        for (int i = 0; i < nt; i++) {
            if (cd[i].sa_cnt >= 0) cd[i].child = (uint64_t *)((uint8_t *)c->t_var.p + at[i]);
            if (cd[i].sa_bytes >= 0) cd[i].bytes = (uint8_t *)c->t_var.p + at[i];
        }
        HIPCHK(c, hipMemcpyAsync(c->t_coldev.p, cd.data(), sizeof(TagColDev) * nt, hipMemcpyHostToDevice, c->stream));
        {
            KTimer tm(c, DHTS_K_STRINGS);
            hipLaunchKernelGGL(bam_tag_cells<true>, dim3((unsigned)((nrows + 255) / 256), (unsigned)nt), dim3(256), 0, c->stream, st, ta);
        }
    }
    HIPCHK(c, hipGetLastError());
    for (int i = 0; i < nt; i++) {
        dhts_col &o = c->tag_out[i];
        o.valid = cd[i].valid; o.fixed = cd[i].fixed;
        if (cd[i].sa_cnt >= 0) { o.off = (const uint32_t *)c->t_offs.p + (size_t)cd[i].sa_cnt * ostride; o.child_n = tot[cd[i].sa_cnt]; o.child_fixed = (const uint32_t *)cd[i].child; }
        if (cd[i].sa_bytes >= 0) { o.off = (const uint32_t *)c->t_offs.p + (size_t)cd[i].sa_bytes * ostride; o.bytes = cd[i].bytes; o.nbytes = tot[cd[i].sa_bytes]; }
    }
    return 0;
}
