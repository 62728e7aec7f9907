// dhts_bcf_scan.inc -- part of dhts_api.hip (included there, inside its extern "C" block; not a translation unit of its own):
// read_bcf: dictionaries, projection, regions, VCF text batches, dhts_bcf_next_batch.
// ---- read_bcf ---------------------------------------------------------------------------------------
// (re)builds everything derived from the header dictionaries: the name arrays of dhts_bcf_info, the validity / slot tables of bcf_rec_check
// and, for VCF text, the sorted name tables the text encoder looks names up in.  Called again when a text scan has added names.
static int bcf_upload_dicts(dhts_ctx *c) {
    c->proj_gen++;                                                              // (the key set of the text encoder is sized by the dictionary)
    const size_t nc = c->bh.ctg.size(), ni = c->bh.ids.size();
    if (c->vcf_text && (nc > c->bcf_ctg_p.capacity() || ni > c->bcf_dict_p.capacity())) return fail(c, "read_bcf: too many names without a header definition");
    c->bcf_ctg_p.clear(); c->bcf_dict_p.clear();
    for (size_t i = 0; i < nc; i++) c->bcf_ctg_p.push_back(c->bh.ctg_present[i] ? c->bh.ctg[i].c_str() : nullptr);
    for (auto &e : c->bh.ids) c->bcf_dict_p.push_back(e.present ? e.key.c_str() : nullptr);
    std::vector<uint8_t> ctg_ok(nc + 1, 0), id_ok(ni + 1, 0); std::vector<int16_t> islot(ni + 1, -1), fslot(ni + 1, -1);
    for (size_t i = 0; i < nc; i++) ctg_ok[i] = c->bh.ctg_present[i] ? 1 : 0;
    for (size_t i = 0; i < ni; i++) id_ok[i] = c->bh.ids[i].present ? 1 : 0;
    for (size_t f = 0; f < c->bsch.info_fields.size(); f++) islot[c->bsch.info_fields[f].id] = (int16_t)f;
    for (size_t f = 0; f < c->bsch.format_fields.size(); f++) if (c->bsch.format_fields[f].id >= 0) fslot[c->bsch.format_fields[f].id] = (int16_t)f;
    ENSURE(c, c->d_ctg_ok, nc + 16); ENSURE(c, c->d_id_ok, ni + 16); ENSURE(c, c->d_info_slot, ni * 2 + 16); ENSURE(c, c->d_fmt_slot, ni * 2 + 16);
    HIPCHK(c, hipMemcpy(c->d_ctg_ok.p, ctg_ok.data(), nc + 1, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_id_ok.p, id_ok.data(), ni + 1, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_info_slot.p, islot.data(), (ni + 1) * 2, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_fmt_slot.p, fslot.data(), (ni + 1) * 2, hipMemcpyHostToDevice));
    if (!c->vcf_text) return 0;
    auto upload = [&](std::vector<std::pair<std::string, int32_t>> &names, const std::vector<uint8_t> *typ_of_id, DevBuf &d_off, DevBuf &d_bytes, DevBuf &d_id, DevBuf *d_typ, DevBuf &d_hash, uint32_t &hmask, const std::vector<uint8_t> *ftyp_of_id = nullptr, DevBuf *d_ftyp = nullptr) -> int {
        std::sort(names.begin(), names.end(), [](const std::pair<std::string, int32_t> &a, const std::pair<std::string, int32_t> &b) {
            const size_t n = a.first.size() < b.first.size() ? a.first.size() : b.first.size();
            const int cmp = memcmp(a.first.data(), b.first.data(), n);
            return cmp != 0 ? cmp < 0 : a.first.size() < b.first.size(); });
        std::vector<uint32_t> off(names.size() + 1, 0); std::string bytes; std::vector<int32_t> ids(names.size() + 1, 0); std::vector<uint8_t> typ(names.size() + 1, 15);
        for (size_t i = 0; i < names.size(); i++) { off[i] = (uint32_t)bytes.size(); bytes += names[i].first; ids[i] = names[i].second; if (typ_of_id) typ[i] = (*typ_of_id)[names[i].second]; }
        off[names.size()] = (uint32_t)bytes.size();
        if (d_off.ensure(off.size() * 4 + 64) || d_bytes.ensure(bytes.size() + 64) || d_id.ensure(ids.size() * 4 + 64) || (d_typ && d_typ->ensure(typ.size() + 64))) return fail(c, "hipMalloc failed");
        HIPCHK(c, hipMemcpy(d_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice));
        if (!bytes.empty()) HIPCHK(c, hipMemcpy(d_bytes.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(d_id.p, ids.data(), ids.size() * 4, hipMemcpyHostToDevice));
        if (d_typ) HIPCHK(c, hipMemcpy(d_typ->p, typ.data(), typ.size(), hipMemcpyHostToDevice));
        {   // the lookup table of vcf_dict_find: at most half full, linear probing
            uint32_t cap = 16; while (cap < names.size() * 2 + 2) cap <<= 1;
            std::vector<uint32_t> tab(cap, 0); hmask = cap - 1;
            for (size_t i = 0; i < names.size(); i++) {
                uint32_t h = vcf_name_hash((const uint8_t *)names[i].first.data(), (uint32_t)names[i].first.size()) & hmask;
                while (tab[h]) h = (h + 1) & hmask;
                tab[h] = (uint32_t)i + 1;
            }
            if (d_hash.ensure((size_t)cap * 4 + 64)) return fail(c, "hipMalloc failed");
            HIPCHK(c, hipMemcpy(d_hash.p, tab.data(), (size_t)cap * 4, hipMemcpyHostToDevice));
        }
        if (d_ftyp) {
            std::vector<uint8_t> ft(names.size() + 1, 15);
            for (size_t i = 0; i < names.size(); i++) ft[i] = (*ftyp_of_id)[names[i].second];
            if (d_ftyp->ensure(ft.size() + 64)) return fail(c, "hipMalloc failed");
            HIPCHK(c, hipMemcpy(d_ftyp->p, ft.data(), ft.size(), hipMemcpyHostToDevice));
        }
        return 0;
    };
    std::vector<std::pair<std::string, int32_t>> cn, in; std::vector<uint8_t> ityp(ni + 1, 15), ftyp(ni + 1, 15);
    for (size_t i = 0; i < nc; i++) if (c->bh.ctg_present[i]) cn.push_back({c->bh.ctg[i], (int32_t)i});
    for (size_t i = 0; i < ni; i++) if (c->bh.ids[i].present) {
        in.push_back({c->bh.ids[i].key, (int32_t)i});
        if (c->bh.ids[i].has[dhts::BCF_HL_INFO]) ityp[i] = (uint8_t)c->bh.ids[i].type[dhts::BCF_HL_INFO];
        if (c->bh.ids[i].has[dhts::BCF_HL_FMT]) ftyp[i] = (uint8_t)c->bh.ids[i].type[dhts::BCF_HL_FMT];
    }
    if (upload(cn, nullptr, c->vd_ctg_off, c->vd_ctg_bytes, c->vd_ctg_id, nullptr, c->vd_ctg_hash, c->vd_ctg_hmask) || upload(in, &ityp, c->vd_id_off, c->vd_id_bytes, c->vd_id_id, &c->vd_id_typ, c->vd_id_hash, c->vd_id_hmask, &ftyp, &c->vd_id_ftyp)) return -1;
    return 0;
}

int dhts_bcf_open(dhts_ctx *c, int tidy_format) {
    if (!c) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    c->bcf_open = false;
    if (c->n_blocks <= 0) return fail(c, "Failed to read BCF/VCF header");
    int64_t k = c->n_blocks < 4 ? c->n_blocks : 4;
    std::vector<uint8_t> h; std::vector<int32_t> bs;
    uint64_t text_end = 0; bool is_text = false;
    for (;;) {
        if (huff_ensure(c, 0, k, k)) return -1;              // (phase A first: the block table may be corrected from the decoded lengths)
        uint64_t total = c->h_uoff[k];
        h.assign(total + 16, 0); bs.resize(k);
        if (dhts_bgzf_inflate_to_host(c, 0, k, h.data(), total, bs.data()) < 0) {
            if (c->h_uoff[k] != total) continue;             // a scratch retry inside moved the block table: size the buffer from it again
            return -1;
        }
        total = c->h_uoff[k];                                // (an overstated ISIZE behind a scratch retry: the stream is shorter than the buffer)
        uint64_t good = total;
        for (int64_t b = 0; b < k; b++) if (bs[b] != 0) { good = c->h_uoff[b]; break; }
        const bool more = (good == total && k < c->n_blocks);
        if (good < 9) { if (more) { k = (k * 4 < c->n_blocks) ? k * 4 : c->n_blocks; continue; } return fail(c, "Failed to read BCF/VCF header"); }
        if (good >= 16 && memcmp(h.data(), "##fileformat=VCF", 16) == 0) {
            // VCF text (vcf_hdr_read vcf.c:2594-2680): lines up to and including the first one that does not start with "##"; empty lines are
            // skipped, a line that does not start with '#' before that is "No sample line"
            std::string text; uint64_t p = 0; bool found = false, broken = false;
            while (p < good) {
                const uint8_t *nl = (const uint8_t *)memchr(h.data() + p, '\n', good - p);
                if (!nl && (more || good < total)) break;                       // the line may continue in blocks not read yet
                const uint64_t ls = p, e = nl ? (uint64_t)(nl - h.data()) : good;
                uint64_t l = e - ls;
                if (l && h[e - 1] == '\r') l--;
                { uint64_t z = 0; while (z < l && h[ls + z]) z++; l = z; }    // (a C string to the parser)
                p = nl ? e + 1 : good;
                if (l == 0) continue;
                if (h[ls] != '#') { broken = true; break; }
                text.append((const char *)h.data() + ls, l); text.push_back('\n');
                if (l < 2 || h[ls + 1] != '#') { found = true; break; }
            }
            if (broken) return fail(c, "Failed to read BCF/VCF header");
            if (!found) { if (more) { k = (k * 4 < c->n_blocks) ? k * 4 : c->n_blocks; continue; } return fail(c, "Failed to read BCF/VCF header"); }
            std::string perr;
            if (!dhts::bcf_parse_header(text.c_str(), c->bh, &perr)) return fail(c, "Failed to read BCF/VCF header");
            text_end = p; is_text = true;
            break;
        }
        if (memcmp(h.data(), "BCF\2\2", 5) != 0) return fail(c, "Failed to read BCF/VCF header");       // vcf.c:1733-1740
        const uint64_t l_text = hle32(h.data() + 5);
        if (9 + l_text > good) { if (more) { k = (k * 4 < c->n_blocks) ? k * 4 : c->n_blocks; continue; } return fail(c, "Failed to read BCF/VCF header"); }
        text_end = 9 + l_text;
        std::string text((const char *)h.data() + 9, l_text);      // bcf_hdr_parse works on the NUL-terminated text (vcf.c:1752-1753)
        std::string perr;
        if (!dhts::bcf_parse_header(text.c_str(), c->bh, &perr)) return fail(c, "Failed to read BCF/VCF header");
        break;
    }
    dhts::bcf_build_schema(c->bh, tidy_format != 0, c->bsch);
    c->bcf_tidy_req = tidy_format != 0;
    c->first_rec_uoff = text_end; c->scan_first_uoff = text_end;
    c->vcf_text = is_text;
    if (is_text) {
        // names a record uses without a definition are added to the dictionaries while scanning (vcf_parse): room is reserved now so that
        // the name arrays handed out by dhts_bcf_info_get never move
        c->bh.ctg.reserve(c->bh.ctg.size() + 65536); c->bh.ctg_present.reserve(c->bh.ctg.size() + 65536); c->bh.ids.reserve(c->bh.ids.size() + 65536);
        c->bcf_ctg_p.clear(); c->bcf_dict_p.clear();
        c->bcf_ctg_p.reserve(c->bh.ctg.size() + 65536); c->bcf_dict_p.reserve(c->bh.ids.size() + 65536);
    }
    // host-visible dictionaries
    c->bcf_colinfo.clear(); c->bcf_smp_p.clear();
    for (auto &col : c->bsch.cols) {
        dhts_bcf_colinfo ci; ci.name = col.name.c_str(); ci.type = col.duck_type; ci.is_list = col.is_list ? 1 : 0; ci.reserved = 0;
        ci.encoding = col.kind == dhts::BK_CHROM ? DHTS_ENC_CONTIG : col.kind == dhts::BK_FILTER ? DHTS_ENC_DICT : col.kind == dhts::BK_SAMPLE_ID ? DHTS_ENC_SAMPLE :
                      (col.kind == dhts::BK_VEP && col.duck_type == dhts::DT_FLOAT) ? DHTS_ENC_FLOAT_TEXT : DHTS_ENC_PLAIN;
        c->bcf_colinfo.push_back(ci);
    }
    for (auto &sm : c->bh.samples) c->bcf_smp_p.push_back(sm.c_str());
    if (c->bsch.info_fields.size() > 30000 || c->bsch.format_fields.size() > 30000) return fail(c, "read_bcf: too many INFO/FORMAT fields");
    if (bcf_upload_dicts(c)) return -1;
    c->bcf_proj.clear();
    for (size_t i = 0; i < c->bsch.cols.size(); i++) c->bcf_proj.push_back((int32_t)i);
    c->shard_b0 = 0; c->shard_b1 = c->n_blocks; c->shard_rank = 0; c->shard_world = 1;
    c->bcf_open = true;
    return dhts_bcf_rewind(c);
}

extern "C" int dhts_bcf_is_text(const dhts_ctx *c) { return (!c || !c->bcf_open || !c->vcf_text) ? 0 : c->plain_text ? 2 : 1; }
int dhts_bcf_info_get(const dhts_ctx *c, dhts_bcf_info *out) {
    if (!c || !c->bcf_open || !out) return -1;
    out->n_cols = (int32_t)c->bcf_colinfo.size(); out->cols = c->bcf_colinfo.data();
    out->n_contigs = (int32_t)c->bcf_ctg_p.size(); out->contig_name = c->bcf_ctg_p.data();
    out->n_dict = (int32_t)c->bcf_dict_p.size(); out->dict_name = c->bcf_dict_p.data();
    out->n_samples = (int32_t)c->bcf_smp_p.size(); out->sample_name = c->bcf_smp_p.data();
    out->tidy = c->bsch.tidy ? 1 : 0; out->first_rec_uoff = c->first_rec_uoff;
    return 0;
}

int dhts_bcf_set_projection(dhts_ctx *c, const int32_t *col_ids, int32_t n) {
    if (!c || !c->bcf_open) return -1;
    std::vector<int32_t> pr;
    for (int32_t i = 0; i < n; i++) { if (col_ids[i] < 0 || col_ids[i] >= (int32_t)c->bsch.cols.size()) return fail(c, "projection column %d out of range", col_ids[i]); pr.push_back(col_ids[i]); }
    c->bcf_proj = pr; c->proj_gen++;
    return 0;
}

// one region of read_bcf(region := ...): bcf_itr_querys (htslib vcf.h:1391 -> hts_itr_querys hts.c:4179-4200, "." = everything).
// Returns 0, 1 when the region yields no iterator (unknown contig / malformed: the reference skips it, bcf_reader.c:935-953), <0 on error.
int dhts_bcf_set_region(dhts_ctx *c, const char *region) {
    if (!c || !c->bcf_open) return -1;
    c->bcf_rg_active = false; c->bcf_rg_all = false; c->rg_empty_window = false; c->bcf_rg_pending = false;
    c->wins.clear(); c->win_cur = 0; c->scan_end_uoff = ~0ull;
    c->shard_b0 = 0; c->shard_b1 = c->n_blocks; c->shard_rank = 0; c->shard_world = 1; c->scan_first_uoff = c->first_rec_uoff;
    if (!region || !*region) return dhts_bcf_rewind(c);
    std::string tok(region);
    if (tok == ".") { c->bcf_rg_active = true; c->bcf_rg_all = true; return dhts_bcf_rewind(c); }
    if (c->vcf_text) {                                                          // names are the index's (tbx_itr_querys): resolved by dhts_bcf_load_index
        c->bcf_rg_active = true; c->bcf_rg_pending = true; c->bcf_rg_tok = tok; c->bcf_rg_tid = c->bcf_rg_itid = -1;
        return dhts_bcf_rewind(c);
    }
    std::vector<std::string> names;
    for (size_t i = 0; i < c->bh.ctg.size(); i++) names.push_back(c->bh.ctg_present[i] ? c->bh.ctg[i] : std::string("\x01"));
    int tid; int64_t b, e;
    if (!parse_region_token(names, tok, tid, b, e)) return 1;
    c->bcf_rg_active = true; c->bcf_rg_tid = tid; c->bcf_rg_beg = b; c->bcf_rg_end = e;
    return dhts_bcf_rewind(c);
}

int dhts_bcf_set_block_range(dhts_ctx *c, int64_t b0, int64_t b1, int speculative_start) {
    BED_REFUSE(c, "a block range");
    if (!c || !c->bcf_open) return -1;
    if (b0 < 0 || b1 > c->n_blocks || b0 > b1) return fail(c, "bad block range");
    c->shard_b0 = b0; c->shard_b1 = b1; c->shard_rank = speculative_start ? 1 : 0; c->shard_world = 2;
    return dhts_bcf_rewind(c);
}

int dhts_bcf_rewind(dhts_ctx *c) {
    if (!c) return -1;
    discard_prefetch(c);
    if (!c->wins.empty()) enter_window(c, 0);
    c->next_block = c->shard_b0; c->carry_len = 0; c->stream_done = c->rg_empty_window; c->first_batch = true; c->ucur = 0;
    c->huff_b0 = c->huff_nb = 0; memset(c->tile_stats, 0, sizeof(c->tile_stats));
    skip_header_blocks(c);
    if (c->vcf_text && c->shard_rank != 0 && c->shard_b0 > 0 && c->wins.empty()) c->next_block = c->shard_b0 - 1;   // (the byte in front of the shard: see vcf_text_records)
    return 0;
}

static size_t fixed_width(const dhts::BcfColumn &col) {
    if (col.is_list) return 0;
    switch (col.kind) {
    case dhts::BK_CHROM: case dhts::BK_SAMPLE_ID: return 4;
    case dhts::BK_POS: case dhts::BK_QUAL: return 8;
    case dhts::BK_ID: case dhts::BK_REF: return 0;
    default: break;
    }
    return col.duck_type == dhts::DT_BOOLEAN ? 1 : col.duck_type == dhts::DT_VARCHAR ? 0 : 4;
}

// debugging aid (not part of the public header): the BCF2 records the last VCF text batch was turned into
extern "C" int64_t dhts_debug_vcf_records(dhts_ctx *c, uint8_t *dst, uint64_t cap, uint32_t *rec_off, int64_t nrec) {
    if (!c || !c->v_out.p) return -1;
    const uint64_t n = cap < c->v_out.cap ? cap : c->v_out.cap;
    HIPCHK(c, hipMemcpy(dst, c->v_out.p, n, hipMemcpyDeviceToHost));
    if (rec_off && nrec > 0) HIPCHK(c, hipMemcpy(rec_off, c->b_rec_off.p, (size_t)nrec * 4, hipMemcpyDeviceToHost));
    return (int64_t)n;
}

// ---- VCF text batches (vcf_text.hip): the lines of the batch become BCF2 records in v_out; rec_off / dir as for binary input ----------
// out: nrec, carry_start (start of the incomplete last line), rec_err (a line failed: the scan ends before it), rec0_text (text offset of
// the first line), st re-pointed at the records.  Names without a definition are added to the header and the batch is measured again.
// lim: lines that start at or behind this text offset belong to the next shard / lie behind the index window (finished = one was met).
static int vcf_text_records(dhts_ctx *c, const Batch &B, BcfStream &st, int64_t &nrec, uint64_t &carry_start, bool &rec_err, uint32_t &rec0_text, uint32_t &stride, unsigned long long &bad_rec,
                            uint64_t lim, bool &finished) {
    const uint8_t *u = B.u; const uint64_t ulen = B.ulen, out_base = B.out_base;
    uint64_t t0 = 0;
    if (!c->first_batch || c->shard_rank == 0) { if (!first_line_t0(c, out_base, t0)) return fail(c, "internal: header beyond first batch"); }
    else {
        // a block-range shard that starts inside the file owns the lines that START at or behind its first block: lines synchronise on the
        // newline, so the start is the byte behind the first newline at or after (shard start - 1); the batch begins one block early for that byte
        const uint64_t U0 = c->h_uoff[c->shard_b0];
        uint64_t q = U0 > out_base ? U0 - 1 - out_base : 0; bool found = U0 <= out_base;
        std::vector<uint8_t> piece(1u << 16);
        while (!found && q < ulen) {
            const uint64_t k = ulen - q < piece.size() ? ulen - q : piece.size();
            HIPCHK(c, hipMemcpy(piece.data(), u + q, k, hipMemcpyDeviceToHost));
            const void *nl = memchr(piece.data(), '\n', k);
            if (nl) { q += (uint64_t)((const uint8_t *)nl - piece.data()) + 1; found = true; } else q += k;
        }
        t0 = found ? q : ulen;
        if (c->first_rec_uoff > out_base + t0) t0 = c->first_rec_uoff - out_base;     // (a shard that starts inside the header)
    }
    nrec = 0; carry_start = ulen; rec_err = false; rec0_text = (uint32_t)t0; bad_rec = ~0ull;
    if (c->first_batch) {
        // a scan range that ends before its first line starts (a shard inside the header, a shard swallowed by one long line) owns no line
        uint64_t end_abs = c->shard_b1 < c->n_blocks ? c->h_uoff[c->shard_b1] : ~0ull;
        if (c->scan_end_uoff < end_abs) end_abs = c->scan_end_uoff;
        if (out_base + t0 >= end_abs) { finished = true; carry_start = t0 < ulen ? t0 : ulen; return 0; }
    }
    // (differs from batch_clean_end: B.blk_err is not looked at, so the cut line in front of a damaged BGZF block counts as well -- only a
    // failed gzip stream drops it, as a line the reader never saw whole; DESIGN.md 4s)
    LineTab T;
    if (line_table(c, c->lines, nullptr, u, t0, ulen, B.final_batch && !c->gz_error, lim, -1, T)) return -1;
    int64_t nlines = T.nlines; const int last_open = T.last_open;
    carry_start = T.carry_start; if (T.finished) finished = true;
    if (nlines == 0) return 0;
    ENSURE(c, c->v_rec_len, (size_t)(nlines + 1) * 4 + 64); ENSURE(c, c->b_rec_off, (size_t)(nlines + 1) * 4 + 64); ENSURE(c, c->v_ctr, 64);
    if (const char *e = getenv("DHTS_VCF_CAPS")) { const uint32_t v = (uint32_t)atoi(e); if (v > 0 && c->v_undef_cap == 65536 && c->v_patch_cap == (1u << 20)) c->v_undef_cap = c->v_patch_cap = v; }   // (tests: small caps make the growth path cheap to reach)
    ENSURE(c, c->v_undef, (size_t)c->v_undef_cap * sizeof(VcfUndef)); ENSURE(c, c->v_patch, (size_t)c->v_patch_cap * sizeof(VcfPatch));
    // the tokens of `n` recorded entries (VcfUndef / VcfPatch: pos and len in words pos_w / len_w), fetched with one gather and one copy
    std::vector<uint32_t> tk_off; std::vector<char> tk_bytes;
    auto fetch_tokens = [&](const void *ent_dev, const uint32_t *ent_host, int pos_w, int len_w, uint32_t n) -> int {
        tk_off.assign((size_t)n + 1, 0);
        for (uint32_t i = 0; i < n; i++) tk_off[(size_t)i + 1] = tk_off[i] + ent_host[4u * i + (uint32_t)len_w];
        tk_bytes.assign((size_t)tk_off[n] + 1, 0);
        if (tk_off[n] == 0) return 0;
        ENSURE(c, c->v_tok_off, (size_t)n * 4 + 64); ENSURE(c, c->v_tok_bytes, (size_t)tk_off[n] + 64);
        HIPCHK(c, hipMemcpyAsync(c->v_tok_off.p, tk_off.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(vcf_gather_tokens, dim3((n + 255) / 256), dim3(256), 0, c->stream, u, (const uint32_t *)ent_dev, pos_w, len_w, (const uint32_t *)c->v_tok_off.p, n, (uint8_t *)c->v_tok_bytes.p);
        HIPCHK(c, hipMemcpyAsync(tk_bytes.data(), c->v_tok_bytes.p, tk_off[n], hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return 0;
    };
    VcfArgs a; memset(&a, 0, sizeof(a));
    a.u = u; a.line_off = (const uint32_t *)c->lines.line_off.p; a.nlines = nlines; a.text_end = ulen; a.last_open = last_open;
    a.n_smp = (int32_t)c->bh.samples.size(); a.v44 = c->bh.version >= 4004000 ? 1 : 0;
    {
        // LDS a workgroup of the lane-per-line encoder stages its 64 lines in: what the batch's lines need (average line x 64, half as much again, in
        // steps of 4 KiB), not the maximum -- the LDS a workgroup asks for is what limits the waves per CU of the sites-only kernels now that they
        // take 46 / 81 registers (40 KiB: four workgroups = one wave per SIMD).  A span that does not fit is parsed from HBM by its workgroup.
        // DHTS_VCF_STAGE=0: no staging; =2: an odd budget (tests); DHTS_VCF_LDS=<bytes>: a fixed budget.
        const char *e = getenv("DHTS_VCF_STAGE"); const int mode = e ? atoi(e) : 1;
        uint64_t want = nlines > 0 ? ((ulen - t0) / (uint64_t)nlines + 1) * VCF_ENC_THREADS * 3 / 2 : VCF_LDS_BYTES;
        want = (want + 4095) & ~(uint64_t)4095;
        if (want < 8192) want = 8192;
        if (want > VCF_LDS_BYTES) want = VCF_LDS_BYTES;
        if (const char *f = getenv("DHTS_VCF_LDS")) { const long v = atol(f); if (v >= 0 && v <= (long)VCF_LDS_BYTES) want = (uint64_t)v; }
        a.lds_budget = mode == 0 ? 0u : mode == 2 ? VCF_LDS_BYTES - 15u : (uint32_t)want;
    }
    a.rec_len = (uint32_t *)c->v_rec_len.p; a.rec_off = (const uint32_t *)c->b_rec_off.p; a.first_bad = (unsigned long long *)((uint64_t *)c->v_ctr.p + 2);
    a.counters = (uint32_t *)c->v_ctr.p; a.undef = (VcfUndef *)c->v_undef.p; a.undef_cap = c->v_undef_cap; a.patch = (VcfPatch *)c->v_patch.p; a.patch_cap = c->v_patch_cap;
    // The INFO keys the projected columns read (INFO_<key> columns, and the annotation tag of VEP_<field> columns): the encoder leaves the
    // others out of the records it makes.  DHTS_VCF_KEEP=0: every key is encoded whatever is projected.
    auto keep_set = [&]() -> int {
        if (c->keep_gen != c->proj_gen) {
            const bool off = getenv("DHTS_VCF_KEEP") && atoi(getenv("DHTS_VCF_KEEP")) == 0;
            const size_t ni = c->bh.ids.size(), nw = ni / 32 + 2;
            std::vector<uint32_t> bits(nw, 0); size_t n_keys = 0, n_kept = 0;
            for (auto &f : c->bsch.info_fields) n_keys += f.id >= 0 ? 1 : 0;
            for (const int32_t ci : c->bcf_proj) {
                const dhts::BcfColumn &col = c->bsch.cols[(size_t)ci];
                const int fld = col.kind == dhts::BK_INFO ? col.field : col.kind == dhts::BK_VEP ? c->bsch.vep_info_field : -1;
                if (fld < 0) continue;
                const int id = c->bsch.info_fields[(size_t)fld].id;
                if (id >= 0 && (size_t)id < ni && !((bits[(size_t)id >> 5] >> (id & 31)) & 1u)) { bits[(size_t)id >> 5] |= 1u << (id & 31); n_kept++; }
            }
            c->keep_all = off || n_kept == n_keys; c->keep_none = (!off && n_kept == 0 && n_keys > 0) ? 1 : 0;
            bool any_fmt = false; std::vector<uint32_t> fbits(nw, 0); size_t f_keys = 0, f_kept = 0;
            for (auto &f : c->bsch.format_fields) f_keys += f.id >= 0 ? 1 : 0;
            for (const int32_t ci : c->bcf_proj) {
                const dhts::BcfColumn &col = c->bsch.cols[(size_t)ci];
                if (col.kind != dhts::BK_FORMAT) continue;
                any_fmt = true;
                const int id = c->bsch.format_fields[(size_t)col.field].id;
                if (id >= 0 && (size_t)id < ni && !((fbits[(size_t)id >> 5] >> (id & 31)) & 1u)) { fbits[(size_t)id >> 5] |= 1u << (id & 31); f_kept++; }
            }
            c->fmt_none = (!off && !any_fmt && !c->bh.samples.empty()) ? 1 : 0;
            c->fmt_keep_all = off || !any_fmt || f_kept == f_keys;                   // (no FORMAT column at all: fmt_none says so)
            if (!c->fmt_keep_all) {
                ENSURE(c, c->v_fkeep, nw * 4 + 64);
                HIPCHK(c, hipMemcpy(c->v_fkeep.p, fbits.data(), nw * 4, hipMemcpyHostToDevice));
            }
            if (!c->keep_all) {
                ENSURE(c, c->v_keep, nw * 4 + 64);
                HIPCHK(c, hipMemcpy(c->v_keep.p, bits.data(), nw * 4, hipMemcpyHostToDevice));
            }
            c->keep_gen = c->proj_gen;
        }
        a.info_keep = c->keep_all ? nullptr : (const uint32_t *)c->v_keep.p; a.info_none = c->keep_all ? 0 : c->keep_none; a.fmt_none = c->fmt_none; a.fmt_keep = c->fmt_keep_all ? nullptr : (const uint32_t *)c->v_fkeep.p;
        return 0;
    };
    if (keep_set()) return -1;
    // Lines so long that 64 of them overflow a workgroup's LDS staging get a wave each (vcf_encode_wave): INFO fields parsed one per lane.
    // DHTS_VCF_WAVE=0 / 1 forces the choice (tests run both ways).
    bool wave_lines = nlines > 0 && ((ulen - t0) / (uint64_t)nlines) * VCF_ENC_THREADS > VCF_LDS_BYTES;
    if (const char *e = getenv("DHTS_VCF_WAVE")) wave_lines = atoi(e) != 0;
    if (wave_lines) { ENSURE(c, c->v_endsv, (size_t)nlines * 8 + 64); a.endsv = (uint32_t *)c->v_endsv.p; }
    ENSURE(c, c->v_pos_hi, (size_t)nlines * 4 + 64); a.pos_hi = (int32_t *)c->v_pos_hi.p;
    auto launch_encode = [&](bool write, int64_t n) {                             // measure / write pass over n lines, with or without the sample columns' code
        const dim3 gw((unsigned)n), gl((unsigned)((n + VCF_ENC_THREADS - 1) / VCF_ENC_THREADS)); const bool smp = a.n_smp > 0;
        const uint32_t lds_dyn = (a.lds_budget + 15u) & ~15u;
        if (wave_lines) {
            if (write) { if (smp) hipLaunchKernelGGL((vcf_encode_wave<true, true>), gw, dim3(64), 0, c->stream, a); else hipLaunchKernelGGL((vcf_encode_wave<true, false>), gw, dim3(64), 0, c->stream, a); }
            else { if (smp) hipLaunchKernelGGL((vcf_encode_wave<false, true>), gw, dim3(64), 0, c->stream, a); else hipLaunchKernelGGL((vcf_encode_wave<false, false>), gw, dim3(64), 0, c->stream, a); }
        } else {
            if (write) { if (smp) hipLaunchKernelGGL((vcf_encode<true, true>), gl, dim3(VCF_ENC_THREADS), lds_dyn, c->stream, a); else hipLaunchKernelGGL((vcf_encode<true, false>), gl, dim3(VCF_ENC_THREADS), lds_dyn, c->stream, a); }
            else { if (smp) hipLaunchKernelGGL((vcf_encode<false, true>), gl, dim3(VCF_ENC_THREADS), lds_dyn, c->stream, a); else hipLaunchKernelGGL((vcf_encode<false, false>), gl, dim3(VCF_ENC_THREADS), lds_dyn, c->stream, a); }
        }
    };
    unsigned long long first_bad = ~0ull;
    for (int round = 0;; round++) {
        if (round > 1000) return fail(c, "read_bcf: too many names without a header definition");
        if (round && keep_set()) return -1;                                     // (names were added: the dictionary, and with it the key set, has grown)
        a.ctg = {(const uint32_t *)c->vd_ctg_off.p, (const uint8_t *)c->vd_ctg_bytes.p, (const int32_t *)c->vd_ctg_id.p, nullptr, nullptr, 0, (const uint32_t *)c->vd_ctg_hash.p, c->vd_ctg_hmask};
        a.ids = {(const uint32_t *)c->vd_id_off.p, (const uint8_t *)c->vd_id_bytes.p, (const int32_t *)c->vd_id_id.p, (const uint8_t *)c->vd_id_typ.p, (const uint8_t *)c->vd_id_ftyp.p, 0, (const uint32_t *)c->vd_id_hash.p, c->vd_id_hmask};
        { int32_t n1 = 0, n2 = 0; for (size_t i = 0; i < c->bh.ctg.size(); i++) n1 += c->bh.ctg_present[i] ? 1 : 0; for (auto &e : c->bh.ids) n2 += e.present ? 1 : 0; a.ctg.n = n1; a.ids.n = n2; }
        HIPCHK(c, hipMemsetAsync(c->v_ctr.p, 0, 16, c->stream)); HIPCHK(c, hipMemsetAsync((uint64_t *)c->v_ctr.p + 2, 0xff, 8, c->stream));
        launch_encode(false, nlines);
        uint64_t ctr[3] = {0, 0, 0};
        HIPCHK(c, hipMemcpyAsync(ctr, c->v_ctr.p, 24, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (!wave_lines && (ctr[1] & 0xffffffffu)) {                              // a line with more FORMAT keys than the lane-per-line encoder keeps tables for: the wave encoder takes the batch
            wave_lines = true;
            ENSURE(c, c->v_endsv, (size_t)nlines * 8 + 64); a.endsv = (uint32_t *)c->v_endsv.p;
            round--;
            continue;
        }
        first_bad = ctr[2];
        const uint32_t n_undef = (uint32_t)(ctr[0] & 0xffffffffu);
        if (n_undef == 0) break;
        // names used without a definition: htslib adds dummy definitions as it meets them, so ids follow the order of first appearance;
        // FORMAT Floats in strtod's forms are checked here (the number has to end where the token ends)
        if (n_undef > c->v_undef_cap) {                                          // more than there was room to record: make room, measure again
            c->v_undef_cap = n_undef + n_undef / 4 + 1024;
            ENSURE(c, c->v_undef, (size_t)c->v_undef_cap * sizeof(VcfUndef));
            a.undef = (VcfUndef *)c->v_undef.p; a.undef_cap = c->v_undef_cap;
            continue;
        }
        const uint32_t got = n_undef;
        std::vector<VcfUndef> ud(got);
        HIPCHK(c, hipMemcpy(ud.data(), c->v_undef.p, (size_t)got * sizeof(VcfUndef), hipMemcpyDeviceToHost));
        if (fetch_tokens(c->v_undef.p, (const uint32_t *)ud.data(), 1, 2, got)) return -1;
        std::vector<uint32_t> order(got); for (uint32_t i = 0; i < got; i++) order[i] = i;
        std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return ud[x].line != ud[y].line ? ud[x].line < ud[y].line : ud[x].pos < ud[y].pos; });
        bool added = false; unsigned long long cut = first_bad;
        for (const uint32_t oi : order) {
            const VcfUndef &x = ud[oi];
            if ((unsigned long long)x.line >= cut) break;                        // lines behind the first bad one are never parsed
            std::string name(tk_bytes.data() + tk_off[oi], x.len);
            if (x.cls == 4) {
                char *end = nullptr; (void)strtod(name.c_str(), &end);
                if (strlen(name.c_str()) != name.size() || end != name.c_str() + name.size()) { cut = x.line; break; }      // "Invalid character": the record is an error
                continue;
            }
            const int hl = x.cls == 3 ? dhts::BCF_HL_FMT : dhts::BCF_HL_INFO;
            auto defined = [&]() {
                if (x.cls == 0) { for (size_t i = 0; i < c->bh.ctg.size(); i++) if (c->bh.ctg_present[i] && c->bh.ctg[i] == name) return true; return false; }
                const int id = c->bh.find_id(name); return id >= 0 && (x.cls == 1 || c->bh.ids[id].has[hl]);
            };
            if (defined()) continue;
            const std::string line = x.cls == 0 ? "##contig=<ID=" + name + ">" : x.cls == 1 ? "##FILTER=<ID=" + name + ",Description=\"Dummy\">"
                                   : x.cls == 2 ? "##INFO=<ID=" + name + ",Number=1,Type=String,Description=\"Dummy\">" : "##FORMAT=<ID=" + name + ",Number=1,Type=String,Description=\"Dummy\">";
            if (name.find('\n') != std::string::npos || !dhts::bcf_header_add_line(c->bh, line.c_str()) || !defined()) { cut = x.line; break; }   // "Could not add dummy header": the record is an error
            added = true;
        }
        if (added && bcf_upload_dicts(c)) return -1;
        const bool shortened = cut < (unsigned long long)nlines;
        if (shortened) {
            first_bad = cut; a.nlines = nlines = (int64_t)cut; rec_err = true; a.last_open = 0;
            if (nlines == 0) { nrec = 0; return 0; }
        }
        if (!added && !shortened) break;                                         // only float checks are left, and they passed
        st.n_ctg = (int32_t)c->bh.ctg.size(); st.n_ids = (int32_t)c->bh.ids.size();
        st.ctg_ok = (const uint8_t *)c->d_ctg_ok.p; st.id_ok = (const uint8_t *)c->d_id_ok.p; st.info_slot = (const int16_t *)c->d_info_slot.p; st.fmt_slot = (const int16_t *)c->d_fmt_slot.p;
    }
    nrec = nlines;
    if (first_bad < (unsigned long long)nlines) { nrec = (int64_t)first_bad; rec_err = true; }
    if (nrec == 0) return 0;
    const uint32_t *lin[1] = {(const uint32_t *)c->v_rec_len.p}; uint32_t *lout[1] = {(uint32_t *)c->b_rec_off.p}; uint64_t total = 0;
    if (run_scan(c, 1, lin, lout, nullptr, nrec, &total)) return -1;
    if (total + PAD_BYTES >= (1ull << 32)) return fail(c, "batch too large");
    ENSURE(c, c->v_out, total + PAD_BYTES + 64);
    a.nlines = nrec; a.out = (uint8_t *)c->v_out.p;
    if (nrec < nlines) { a.last_open = 0; }
    HIPCHK(c, hipMemsetAsync(c->v_ctr.p, 0, 16, c->stream));
    launch_encode(true, nrec);
    HIPCHK(c, hipMemsetAsync((uint8_t *)c->v_out.p + total, 0, PAD_BYTES, c->stream));
    uint32_t ctr2[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(ctr2, c->v_ctr.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (ctr2[1] > c->v_patch_cap) {                          // more numbers for the host than there was room to record: make room, write again
        c->v_patch_cap = ctr2[1] + ctr2[1] / 4 + 1024;
        ENSURE(c, c->v_patch, (size_t)c->v_patch_cap * sizeof(VcfPatch));
        a.patch = (VcfPatch *)c->v_patch.p; a.patch_cap = c->v_patch_cap;
        HIPCHK(c, hipMemsetAsync(c->v_ctr.p, 0, 16, c->stream));
        launch_encode(true, nrec);
        HIPCHK(c, hipMemcpyAsync(ctr2, c->v_ctr.p, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (ctr2[1] > c->v_patch_cap) return fail(c, "read_bcf: the write pass recorded %u numbers for the host, room for %u", ctr2[1], c->v_patch_cap);
    }
    if (ctr2[1]) {
        // numbers hts_str2dbl hands to strtod (exponents, > 14 digits, inf / nan / hex) and QUAL values outside that form: converted here.
        // One gather + one copy brings the tokens, one copy + one scatter takes the words back.
        const uint32_t np = ctr2[1];
        std::vector<VcfPatch> pt(np); std::vector<uint32_t> words(np);
        HIPCHK(c, hipMemcpy(pt.data(), c->v_patch.p, (size_t)np * sizeof(VcfPatch), hipMemcpyDeviceToHost));
        if (fetch_tokens(c->v_patch.p, (const uint32_t *)pt.data(), 0, 1, np)) return -1;
        std::string tok;
        for (uint32_t i = 0; i < np; i++) {
            const VcfPatch &x = pt[i];
            tok.assign(tk_bytes.data() + tk_off[i], x.len);
            uint32_t bits;
            if (x.kind == 0) { const float f = (float)atof(tok.c_str()); memcpy(&bits, &f, 4); }
            else {
                char *end = nullptr; const double d = strtod(tok.c_str(), &end);
                if (end == tok.c_str() && x.kind == 1) bits = 0x7F800001u;                     // INFO: a failed conversion is a missing value
                else { const float f = (end == tok.c_str()) ? 0.0f : (float)d; memcpy(&bits, &f, 4); }   // (FORMAT stores what strtod returned: 0.0)
            }
            words[i] = bits;
        }
        ENSURE(c, c->v_tok_bits, (size_t)np * 4 + 64);
        HIPCHK(c, hipMemcpyAsync(c->v_tok_bits.p, words.data(), (size_t)np * 4, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(vcf_scatter_words, dim3((np + 255) / 256), dim3(256), 0, c->stream, (uint8_t *)c->v_out.p, (const VcfPatch *)c->v_patch.p, (const uint32_t *)c->v_tok_bits.p, np);
        HIPCHK(c, hipStreamSynchronize(c->stream));          // (`words` is pageable host memory: the copy must have left it before it goes out of scope)
    }
    HIPCHK(c, hipMemcpyAsync(&rec0_text, c->lines.line_off.p, 4, hipMemcpyDeviceToHost, c->stream));
    st.u = (const uint8_t *)c->v_out.p; st.ulen = total; st.pos_hi = (const int32_t *)c->v_pos_hi.p;
    st.n_ctg = (int32_t)c->bh.ctg.size(); st.n_ids = (int32_t)c->bh.ids.size();
    st.ctg_ok = (const uint8_t *)c->d_ctg_ok.p; st.id_ok = (const uint8_t *)c->d_id_ok.p; st.info_slot = (const int16_t *)c->d_info_slot.p; st.fmt_slot = (const int16_t *)c->d_fmt_slot.p;
    const size_t n = (size_t)nrec; const int D = 2 + st.n_info_f + st.n_fmt_f;
    stride = (uint32_t)((n + 63) & ~(size_t)63);
    ENSURE(c, c->b_dir, (size_t)D * stride * 4 + 16); ENSURE(c, c->d_res, 256);
    HIPCHK(c, hipMemsetAsync((uint64_t *)c->d_res.p + 4, 0xff, 8, c->stream));
    {
        KTimer tm(c, DHTS_K_BCF_CHECK);
        hipLaunchKernelGGL(bcf_rec_check, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, c->stream, st, (const uint32_t *)c->b_rec_off.p, nrec, (uint32_t *)c->b_dir.p, stride,
                           (unsigned long long *)((uint64_t *)c->d_res.p + 4));
    }
    HIPCHK(c, hipMemcpyAsync(&bad_rec, (uint64_t *)c->d_res.p + 4, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

static int bcf_next_batch_one(dhts_ctx *c, int64_t max_blocks, dhts_bcf_batch *out);
int dhts_bcf_next_batch(dhts_ctx *c, int64_t max_blocks, dhts_bcf_batch *out) {
    if (!c || !out) return -1;
    for (;;) {
        if (bcf_next_batch_one(c, max_blocks, out)) return -1;
        // a region query with several index windows: the end of one window is the start of the next, not the end of the scan
        if (next_window(c, out->status) && out->n_rows == 0) continue;
        return 0;
    }
}
static int bcf_next_batch_one(dhts_ctx *c, int64_t max_blocks, dhts_bcf_batch *out) {
    if (!c || !out) return -1;
    memset(out, 0, sizeof(*out));
    for (auto &a : c->bcf_ar) { a.p = nullptr; a.n = 0; }
    if (!c->bcf_open) return fail(c, "dhts_bcf_open not called");
    HIPCHK(c, hipSetDevice(c->device));
    const int ncols = (int)c->bcf_proj.size();
    c->bcf_out.assign(ncols, dhts_bcf_col());
    for (int i = 0; i < ncols; i++) { memset(&c->bcf_out[i], 0, sizeof(dhts_bcf_col)); c->bcf_out[i].col = c->bcf_proj[i]; }
    out->n_cols = ncols; out->cols = c->bcf_out.data();
    if (c->stream_done) { out->status = 1; return 0; }
    Batch B;
    if (batch_begin(c, max_blocks, B)) return -1;
    uint8_t *u = B.u; uint64_t ulen = B.ulen; const uint64_t out_base = B.out_base;
    BcfStream st; memset(&st, 0, sizeof(st));
    st.u = u; st.ulen = ulen; st.n_ctg = (int32_t)c->bh.ctg.size(); st.n_ids = (int32_t)c->bh.ids.size(); st.n_smp = c->bsch.n_samples;
    st.final_batch = B.final_batch ? 1 : 0; st.n_info_f = (int32_t)c->bsch.info_fields.size(); st.n_fmt_f = (int32_t)c->bsch.format_fields.size();
    st.ctg_ok = (const uint8_t *)c->d_ctg_ok.p; st.id_ok = (const uint8_t *)c->d_id_ok.p;
    st.info_slot = (const int16_t *)c->d_info_slot.p; st.fmt_slot = (const int16_t *)c->d_fmt_slot.p;

    // ---- tiles: record chain ----
    int64_t ntiles = (int64_t)((ulen + TILE_BYTES - 1) / TILE_BYTES); if (ntiles < 1) ntiles = 1;
    ENSURE(c, c->t_first, ntiles * 8); ENSURE(c, c->t_end, ntiles * 8); ENSURE(c, c->t_count, ntiles * 4); ENSURE(c, c->t_err, ntiles * 4);
    ENSURE(c, c->t_rowbase, ntiles * 4 + 16); ENSURE(c, c->d_res, 256); ENSURE(c, c->d_nfixed, 64);
    ENSURE(c, c->t2_first, ntiles * 8); ENSURE(c, c->t2_end, ntiles * 8); ENSURE(c, c->t2_count, ntiles * 4); ENSURE(c, c->t2_err, ntiles * 4);
    TileOut to; to.first = (uint64_t *)c->t_first.p; to.end_next = (uint64_t *)c->t_end.p; to.count = (uint32_t *)c->t_count.p; to.err = (int32_t *)c->t_err.p;
    TileOut to2; to2.first = (uint64_t *)c->t2_first.p; to2.end_next = (uint64_t *)c->t2_end.p; to2.count = (uint32_t *)c->t2_count.p; to2.err = (int32_t *)c->t2_err.p;
    uint64_t start0;
    if (c->first_batch) start0 = (c->shard_rank == 0) ? c->scan_first_uoff - out_base : NONE64;
    else start0 = 0;
    if (c->first_batch && c->shard_rank == 0 && c->scan_first_uoff < out_base) return fail(c, "internal: header beyond first batch");
    uint64_t res[4] = {0, 0, 0, 0};
    // (same false-start retry as in dhts_bam_next_batch: a speculated shard start whose chain breaks inside the batch, or whose
    //  "records" fail bcf_record_check, is replaced by the next candidate that is no member of a failed chain; when none is left the
    //  damage is real and the first attempt stands)
    const bool speculative = (start0 == NONE64);
    uint64_t first0 = NONE64, en0 = NONE64, spec_from = 0; int spec_tries = 0; bool restoring = false;
    SpecSkip sk; memset(&sk, 0, sizeof(sk));
    int64_t nrec = 0; uint64_t carry_start = 0; bool rec_err = false;
    // the scan range ends with its last block (later shards / the rest of the file exist) or, for one of several index windows, exactly
    // at the window's end: windows are disjoint, so no record is delivered twice
    uint64_t shard_end_u = B.sharded_tail ? c->h_uoff[c->shard_b1] : ~0ull;
    if (c->scan_end_uoff < shard_end_u) shard_end_u = c->scan_end_uoff;
    const bool cut_tail = B.sharded_tail || c->scan_end_uoff != ~0ull;
    bool shard_finished = false;
    const int reps = c->bsch.tidy ? c->bsch.n_samples : 1;
    const int D = 2 + st.n_info_f + st.n_fmt_f;
    uint32_t rec0_off = 0;
    unsigned long long bad = ~0ull;
    uint32_t stride = 64;
    if (c->vcf_text) {
        if (c->bcf_rg_pending) return fail(c, "read_bcf: a region query on VCF text needs the tabix index (dhts_bcf_load_index) before the scan");
        uint32_t rec0_text = 0;
        const uint64_t lim = (cut_tail && out_base + ulen > shard_end_u) ? shard_end_u - out_base : ~0ull;
        if (vcf_text_records(c, B, st, nrec, carry_start, rec_err, rec0_text, stride, bad, lim, shard_finished)) return -1;
        rec0_off = rec0_text;
    } else
    for (;;) {
        to.first = (uint64_t *)c->t_first.p; to.end_next = (uint64_t *)c->t_end.p; to.count = (uint32_t *)c->t_count.p; to.err = (int32_t *)c->t_err.p;
        to2.first = (uint64_t *)c->t2_first.p; to2.end_next = (uint64_t *)c->t2_end.p; to2.count = (uint32_t *)c->t2_count.p; to2.err = (int32_t *)c->t2_err.p;
        uint64_t start_eff = start0;
        if (speculative && !restoring && spec_tries > 0) {
            uint64_t *d_cand = (uint64_t *)c->d_nfixed.p + 2, cand = NONE64;
            hipLaunchKernelGGL(bcf_spec_next, dim3(1), dim3(64), 0, c->stream, st, spec_from, sk, d_cand);
            HIPCHK(c, hipMemcpyAsync(&cand, d_cand, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (cand == NONE64) { spec_from = 0; restoring = true; c->tile_stats[DHTS_TS_GAVE_UP]++; }
            else { start_eff = cand; c->tile_stats[DHTS_TS_RETRIES]++; }
        }
        {
            KTimer tm(c, DHTS_K_TILES);
            hipLaunchKernelGGL(bcf_tile_scan, dim3((unsigned)ntiles), dim3(64), 0, c->stream, st, start_eff, ntiles, to, spec_from);
            int rounds = 0; bool seq_fallback = false;
            for (;;) {
                (void)hipMemsetAsync(c->d_nfixed.p, 0, 4, c->stream);
                hipLaunchKernelGGL(bcf_tile_fix, dim3((unsigned)((ntiles + 255) / 256)), dim3(256), 0, c->stream, st, TILE_BYTES, ntiles, to, to2, (uint32_t *)c->d_nfixed.p);
                { TileOut tmp = to; to = to2; to2 = tmp; }
                uint32_t nfixed = 0;
                HIPCHK(c, hipMemcpyAsync(&nfixed, c->d_nfixed.p, 4, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                if (g_debug) fprintf(stderr, "[dhts] bcf tiles=%lld round=%d nfixed=%u\n", (long long)ntiles, rounds, nfixed);
                if (nfixed == 0) break;
                c->tile_stats[DHTS_TS_REPAIRED] += nfixed; c->tile_stats[DHTS_TS_ROUNDS]++;
                if (++rounds > 256) {
                    (void)hipMemsetAsync(c->d_nfixed.p, 0, 4, c->stream);
                    hipLaunchKernelGGL(bcf_tile_fix_seq, dim3(1), dim3(1), 0, c->stream, st, TILE_BYTES, ntiles, to, (uint32_t *)c->d_nfixed.p);
                    seq_fallback = true; break;
                }
            }
            hipLaunchKernelGGL(bam_tile_finalize, dim3(1), dim3(1024), 0, c->stream, ntiles, to, (uint32_t *)c->t_rowbase.p, (uint64_t *)c->d_res.p);
            if (seq_fallback) {
                uint32_t nseq = 0;
                HIPCHK(c, hipMemcpyAsync(&nseq, c->d_nfixed.p, 4, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                c->tile_stats[DHTS_TS_REPAIRED] += nseq; c->tile_stats[DHTS_TS_SEQ]++;
            }
        }
        HIPCHK(c, hipMemcpyAsync(res, c->d_res.p, 32, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&first0, to.first, 8, hipMemcpyDeviceToHost, c->stream));
        if (speculative) HIPCHK(c, hipMemcpyAsync(&en0, to.end_next, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        nrec = (int64_t)res[0]; carry_start = res[1]; rec_err = res[2] != 0;
        if (carry_start == NONE64) carry_start = ulen;
        bad = ~0ull; rec0_off = 0;
        if (nrec > 0) {
            const size_t n = (size_t)nrec;
            stride = (uint32_t)((n + 63) & ~(size_t)63);
            ENSURE(c, c->b_rec_off, n * 4 + 16); ENSURE(c, c->b_dir, (size_t)D * stride * 4 + 16);
            hipLaunchKernelGGL(bcf_tile_offsets, dim3((unsigned)((ntiles + 255) / 256)), dim3(256), 0, c->stream, st, TILE_BYTES, ntiles, to, (const uint32_t *)c->t_rowbase.p,
                               (const uint64_t *)c->d_res.p, nrec, (uint32_t *)c->b_rec_off.p);
            HIPCHK(c, hipMemsetAsync((uint64_t *)c->d_res.p + 4, 0xff, 8, c->stream));
            {
                KTimer tm(c, DHTS_K_BCF_CHECK);
                hipLaunchKernelGGL(bcf_rec_check, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, c->stream, st, (const uint32_t *)c->b_rec_off.p, nrec, (uint32_t *)c->b_dir.p, stride,
                                   (unsigned long long *)((uint64_t *)c->d_res.p + 4));
            }
            HIPCHK(c, hipMemcpyAsync(&bad, (uint64_t *)c->d_res.p + 4, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(&rec0_off, c->b_rec_off.p, 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        if (!speculative || restoring) break;
        if (first0 == NONE64) first0 = en0;                     // (the candidate lies behind tile 0: see dhts_bam_next_batch)
        if (start_eff != NONE64) first0 = start_eff;
        const bool invalid_rec = bad < (unsigned long long)nrec;
        const bool false_start = first0 != NONE64 && (res[2] != 0 || invalid_rec);
        if (!false_start) break;
        if (invalid_rec) c->tile_stats[DHTS_TS_VALIDATE]++;
        // the records that lead to the same failure: all of a chain that broke, else those up to the refused one
        const int64_t nskip = res[2] != 0 ? nrec : (int64_t)bad + 1;
        if (nskip > 0 && sk.lists < SPEC_LISTS) {
            DevBuf &sb = c->spec_skip[sk.lists];
            ENSURE(c, sb, (size_t)nskip * 4 + 16);
            HIPCHK(c, hipMemcpyAsync(sb.p, c->b_rec_off.p, (size_t)nskip * 4, hipMemcpyDeviceToDevice, c->stream));
            sk.off[sk.lists] = (const uint32_t *)sb.p; sk.n[sk.lists] = (uint32_t)nskip; sk.lists++;
        }
        spec_from = first0 + 1; spec_tries++;
    }
    if (nrec > 0) {
        if (bad < (unsigned long long)nrec) { nrec = (int64_t)bad; rec_err = true; }    // the first bad record ends the scan (bcf_reader.c:1319-1349)
        if (nrec > 0 && !c->vcf_text && cut_tail && out_base + ulen > shard_end_u) {
            std::vector<uint32_t> ro(nrec);
            HIPCHK(c, hipMemcpyAsync(ro.data(), c->b_rec_off.p, nrec * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            const uint64_t lim = shard_end_u - out_base;
            int64_t lo = 0, hi = nrec;
            while (lo < hi) { int64_t mid = (lo + hi) / 2; if (ro[mid] < lim) lo = mid + 1; else hi = mid; }
            if (lo < nrec) { carry_start = ro[lo]; nrec = lo; shard_finished = true; }
            else if (carry_start >= lim) shard_finished = true;
        }
        const uint32_t *sel = nullptr;
        if (nrec > 0 && c->bcf_rg_active && !c->bcf_rg_all) {
            // region predicate per record -> compacted list of kept record ids (validation above covered every record read)
            const size_t nn = (size_t)nrec;
            ENSURE(c, c->b_keep, nn * 4 + 16); ENSURE(c, c->b_map, (nn + 1) * 4 + 16); ENSURE(c, c->b_sel, nn * 4 + 16);
            hipLaunchKernelGGL(bcf_region_keep, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, c->stream, st, (const uint32_t *)c->b_rec_off.p, (const uint32_t *)c->b_dir.p, nrec,
                               c->bcf_rg_tid, c->bcf_rg_beg, c->bcf_rg_end, 0, (uint32_t *)c->b_keep.p);
            const uint32_t *kin[1] = {(const uint32_t *)c->b_keep.p}; uint32_t *kout[1] = {(uint32_t *)c->b_map.p}; uint64_t kept = 0;
            if (run_scan(c, 1, kin, kout, nullptr, nrec, &kept)) return -1;
            hipLaunchKernelGGL(bcf_select, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, c->stream, (const uint32_t *)c->b_map.p, nrec, (uint32_t *)c->b_sel.p);
            sel = (const uint32_t *)c->b_sel.p;
            nrec = (int64_t)kept;
        }
        if (nrec > 0 && ncols > 0) {
            const int64_t nrows = nrec * reps;
            const uint32_t ostride = (uint32_t)(((size_t)nrows + 1 + 63) & ~(size_t)63);
            // column program for this projection
            std::vector<BcfColDev> cd(ncols);
            int nsa = 0; size_t fixed_bytes = 0;
            std::vector<size_t> fixed_at(ncols, 0);
            for (int i = 0; i < ncols; i++) {
                const dhts::BcfColumn &col = c->bsch.cols[c->bcf_proj[i]];
                BcfColDev &d = cd[i]; memset(&d, 0, sizeof(d));
                d.kind = col.kind; d.is_list = col.is_list ? 1 : 0; d.sample = col.sample; d.slot = col.field < 0 ? 0 : col.field; d.flags = 0; d.sa_cnt = d.sa_bytes = -1;
                if (col.kind == dhts::BK_INFO) d.htype = c->bsch.info_fields[col.field].htype;
                if (col.kind == dhts::BK_VEP) {                                                      // one field of every transcript of the annotation tag
                    d.slot = c->bsch.vep_info_field; d.vep_field = col.field; d.htype = c->bsch.vep_fields[col.field].htype;
                    if (c->bsch.info_fields[c->bsch.vep_info_field].htype != dhts::BCF_HT_STR) d.flags |= BF_NULL_ALWAYS;   // bcf_get_info_string's type check (vcf.c:6056-6066)
                }
                if (col.kind == dhts::BK_FORMAT) {
                    const dhts::BcfField &f = c->bsch.format_fields[col.field];
                    d.htype = f.htype;
                    if (f.htype == dhts::BCF_HT_FLAG || f.id < 0) d.flags |= BF_NULL_ALWAYS;          // no getter yields a value for a FORMAT Flag; default GT column (bcf_reader.c:683-692)
                    if (f.htype == dhts::BCF_HT_STR && f.name == "GT") { d.flags |= BF_GT; if (!c->bsch.gt_string_ok) d.flags |= BF_NULL_ALWAYS; if (c->bh.version < 4004000 && f.id == c->bsch.gt_id) d.flags |= BF_GT_FIX; }
                    else if (f.htype == dhts::BCF_HT_STR && f.is_list) d.flags |= BF_NULL_ALWAYS;       // LIST(VARCHAR) FORMAT strings: undefined in the reference, NULL here
                    if (f.name == "GT" && f.htype != dhts::BCF_HT_STR) d.flags |= BF_NULL_ALWAYS;      // getter type check vcf.c:6183-6187
                }
                const bool varchar = (col.duck_type == dhts::DT_VARCHAR && col.kind != dhts::BK_CHROM && col.kind != dhts::BK_SAMPLE_ID && col.kind != dhts::BK_FILTER) ||
                                     (col.kind == dhts::BK_VEP && col.duck_type == dhts::DT_FLOAT);      // Float fields of a transcript travel as text (DHTS_ENC_FLOAT_TEXT)
                if (col.is_list) { d.sa_cnt = nsa++; if (varchar) d.sa_bytes = nsa++; }
                else if (varchar) d.sa_bytes = nsa++;
                const size_t w = fixed_width(col);
                fixed_at[i] = fixed_bytes; fixed_bytes += (w * (size_t)nrows + 63) & ~(size_t)63;
            }
            ENSURE(c, c->b_valid, (size_t)ncols * nrows + 64); ENSURE(c, c->b_fixed, fixed_bytes + 64);
            ENSURE(c, c->b_lens, (size_t)(nsa ? nsa : 1) * ostride * 4 + 64); ENSURE(c, c->b_offs, (size_t)(nsa ? nsa : 1) * ostride * 4 + 64);
            // VEP_<field> columns of long records: a wave per row and column (bcf_vep_wave) instead of a lane per row.  DHTS_VEP_WAVE=0 / 1 forces the choice.
            std::vector<uint32_t> vep_cols;
            for (int i = 0; i < ncols; i++) if (cd[i].kind == dhts::BK_VEP) vep_cols.push_back((uint32_t)i);
            bool vep_wave = !vep_cols.empty() && nrec > 0 && st.ulen / (uint64_t)nrec >= 1024;
            if (const char *e = getenv("DHTS_VEP_WAVE")) vep_wave = !vep_cols.empty() && atoi(e) != 0;
            const size_t coldev_bytes = (sizeof(BcfColDev) * ncols + 63) & ~(size_t)63;
            ENSURE(c, c->b_coldev, coldev_bytes + vep_cols.size() * 4 + 64);
            for (int i = 0; i < ncols; i++) {
                cd[i].valid = (uint8_t *)c->b_valid.p + (size_t)i * nrows;
                cd[i].fixed = fixed_width(c->bsch.cols[c->bcf_proj[i]]) ? (void *)((uint8_t *)c->b_fixed.p + fixed_at[i]) : nullptr;
            }
            HIPCHK(c, hipMemcpyAsync(c->b_coldev.p, cd.data(), sizeof(BcfColDev) * ncols, hipMemcpyHostToDevice, c->stream));
            BcfCellArgs ca; memset(&ca, 0, sizeof(ca));
            ca.rec_off = (const uint32_t *)c->b_rec_off.p; ca.dir = (const uint32_t *)c->b_dir.p; ca.stride = stride; ca.nrows = nrows; ca.tidy = c->bsch.tidy ? 1 : 0;
            ca.n_smp = c->bsch.n_samples > 0 ? c->bsch.n_samples : 1; ca.lens = (uint32_t *)c->b_lens.p; ca.offs = (const uint32_t *)c->b_offs.p; ca.ostride = ostride;
            ca.cols = (const BcfColDev *)c->b_coldev.p; ca.sel = sel; ca.ncols = (uint32_t)ncols;
            if (vep_wave) {
                if ((uint64_t)nrows * vep_cols.size() >= (1ull << 31)) return fail(c, "read_bcf: too many rows x VEP columns in one batch; use a smaller max_blocks");
                HIPCHK(c, hipMemcpyAsync((uint8_t *)c->b_coldev.p + coldev_bytes, vep_cols.data(), vep_cols.size() * 4, hipMemcpyHostToDevice, c->stream));
                ca.n_vep = (uint32_t)vep_cols.size(); ca.vep_cols = (const uint32_t *)((uint8_t *)c->b_coldev.p + coldev_bytes);
            }
            {
                KTimer tm(c, DHTS_K_BCF_MEASURE);
                hipLaunchKernelGGL(bcf_cells<false>, dim3((unsigned)(((nrows + 255) / 256) * ncols)), dim3(256), 0, c->stream, st, ca);
                if (vep_wave) hipLaunchKernelGGL(bcf_vep_wave<false>, dim3((unsigned)(nrows * (int64_t)vep_cols.size())), dim3(64), 0, c->stream, st, ca);
            }
            std::vector<uint64_t> tot(nsa ? nsa : 1, 0);
            uint64_t var_total = 0;
            if (nsa > 0) {
                MScanArgs ma; ma.in = (const uint32_t *)c->b_lens.p; ma.out = (uint32_t *)c->b_offs.p; ma.stride = ostride; ma.n = nrows;
                ma.nparts = (nrows + 1 + SCAN_ITEMS - 1) / SCAN_ITEMS; if (ma.nparts < 1) ma.nparts = 1;
                ENSURE(c, c->b_partial, (size_t)nsa * ma.nparts * 8 + 64); ENSURE(c, c->b_total, (size_t)nsa * 8 + 64);
                ma.partial = (uint64_t *)c->b_partial.p; ma.total = (uint64_t *)c->b_total.p;
                {
                    KTimer tm(c, DHTS_K_SCAN);
                    hipLaunchKernelGGL(mscan_reduce, dim3((unsigned)ma.nparts, (unsigned)nsa), dim3(256), 0, c->stream, ma);
                    hipLaunchKernelGGL(mscan_partials, dim3((unsigned)nsa), dim3(1024), 0, c->stream, ma);
                    hipLaunchKernelGGL(mscan_apply, dim3((unsigned)ma.nparts, (unsigned)nsa), dim3(256), 0, c->stream, ma);
                }
                HIPCHK(c, hipMemcpyAsync(tot.data(), c->b_total.p, (size_t)nsa * 8, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                for (int k = 0; k < nsa; k++) if (tot[k] >= (1ull << 32)) return fail(c, "read_bcf: a column exceeds 4 GiB in one batch; use a smaller max_blocks");
                // arena for children / bytes
                size_t var_bytes = 0; std::vector<size_t> at_child(ncols, 0), at_coff(ncols, 0), at_bytes(ncols, 0), at_cvalid(ncols, 0);
                for (int i = 0; i < ncols; i++) {
                    if (cd[i].kind == dhts::BK_VEP) { at_cvalid[i] = var_bytes; var_bytes += (tot[cd[i].sa_cnt] + 63) & ~(size_t)63; }
                    if (cd[i].sa_cnt >= 0 && cd[i].sa_bytes < 0) { at_child[i] = var_bytes; var_bytes += (tot[cd[i].sa_cnt] * 4 + 63) & ~(size_t)63; }
                    if (cd[i].sa_cnt >= 0 && cd[i].sa_bytes >= 0) { at_coff[i] = var_bytes; var_bytes += ((tot[cd[i].sa_cnt] + 1) * 4 + 63) & ~(size_t)63; }
                    if (cd[i].sa_bytes >= 0) { at_bytes[i] = var_bytes; var_bytes += (tot[cd[i].sa_bytes] + 63) & ~(size_t)63; }
                }
                ENSURE(c, c->b_var, var_bytes + 64); var_total = var_bytes;
                for (int i = 0; i < ncols; i++) {
                    uint8_t *base = (uint8_t *)c->b_var.p;
                    if (cd[i].sa_cnt >= 0 && cd[i].sa_bytes < 0) cd[i].child_fixed = (uint32_t *)(base + at_child[i]);
                    if (cd[i].sa_cnt >= 0 && cd[i].sa_bytes >= 0) cd[i].child_off = (uint32_t *)(base + at_coff[i]);
                    if (cd[i].sa_bytes >= 0) cd[i].bytes = base + at_bytes[i];
                    if (cd[i].kind == dhts::BK_VEP) cd[i].child_valid = base + at_cvalid[i];
                }
                HIPCHK(c, hipMemcpyAsync(c->b_coldev.p, cd.data(), sizeof(BcfColDev) * ncols, hipMemcpyHostToDevice, c->stream));
                {
                    KTimer tm(c, DHTS_K_BCF_WRITE);
                    hipLaunchKernelGGL(bcf_cells<true>, dim3((unsigned)(((nrows + 255) / 256) * ncols)), dim3(256), 0, c->stream, st, ca);
                    if (vep_wave) hipLaunchKernelGGL(bcf_vep_wave<true>, dim3((unsigned)(nrows * (int64_t)vep_cols.size())), dim3(64), 0, c->stream, st, ca);
                }
            }
            HIPCHK(c, hipGetLastError());
            c->bcf_ar[0].p = (const uint8_t *)c->b_valid.p; c->bcf_ar[0].n = (uint64_t)ncols * (uint64_t)nrows;
            c->bcf_ar[1].p = (const uint8_t *)c->b_fixed.p; c->bcf_ar[1].n = fixed_bytes;
            c->bcf_ar[2].p = (const uint8_t *)c->b_offs.p; c->bcf_ar[2].n = (uint64_t)nsa * ostride * 4;
            c->bcf_ar[3].p = (const uint8_t *)c->b_var.p; c->bcf_ar[3].n = var_total;
            for (int i = 0; i < ncols; i++) {
                dhts_bcf_col &o = c->bcf_out[i];
                o.valid = cd[i].valid; o.fixed = cd[i].fixed;
                if (cd[i].sa_cnt >= 0) { o.off = (const uint32_t *)c->b_offs.p + (size_t)cd[i].sa_cnt * ostride; o.child_n = tot[cd[i].sa_cnt]; o.child_fixed = cd[i].child_fixed; o.child_off = cd[i].child_off; o.child_valid = cd[i].child_valid; }
                else if (cd[i].sa_bytes >= 0) o.off = (const uint32_t *)c->b_offs.p + (size_t)cd[i].sa_bytes * ostride;
                if (cd[i].sa_bytes >= 0) { o.bytes = cd[i].bytes; o.nbytes = tot[cd[i].sa_bytes]; }
            }
        }
    }
    out->n_rows = nrec * reps; c->last_bcf_u = st.u;
    out->end_uoff = out_base + carry_start;
    out->first_rec_uoff = nrec > 0 ? out_base + rec0_off : NONE64;
    return batch_end(c, B, carry_start, rec_err, shard_finished, &out->status);
}

#ifdef DHTS_DIAG
int dhts_debug_diag(dhts_ctx *c, unsigned long long *out8) {
    if (!c) return -1;
    HIPCHK(c, hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_diag), 64));
    HIPCHK(c, hipMemcpyFromSymbol(out8 + 8, HIP_SYMBOL(g_diagt), 64));
    HIPCHK(c, hipMemcpyFromSymbol(out8 + 16, HIP_SYMBOL(g_diagA), 64));
    return 0;
}
#endif
#ifdef HW_DIAG
extern "C" int dhts_debug_hw_diag(dhts_ctx *c, unsigned long long *out16, int reset) {
    if (!c) return -1;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_hw_diag), 128));
    if (reset) { unsigned long long z[16] = {0}; HIPCHK(c, hipMemcpyToSymbol(HIP_SYMBOL(g_hw_diag), z, 128)); }
    return 0;
}
#endif
#ifdef TR_DIAG
extern "C" int dhts_debug_tr_diag(dhts_ctx *c, unsigned long long *out16, int reset) {
    if (!c) return -1;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_tr_diag), 128));
    if (reset) { unsigned long long z[16] = {0}; HIPCHK(c, hipMemcpyToSymbol(HIP_SYMBOL(g_tr_diag), z, 128)); }
    return 0;
}
#endif
// debugging aid (not part of the public header): phase-A metadata of scratch slot s
// kernel experiments (tools/dbg): phase A alone over blocks [b0, b0+nb), `reps` launches; returns ms per launch
extern "C" double dhts_debug_time_huff(dhts_ctx *c, int64_t b0, int64_t nb, int reps) {
    if (!c || hipSetDevice(c->device) != hipSuccess) return -1;
    if (huff_blocks(c, b0, nb)) return -1;
    (void)hipStreamSynchronize(c->stream);
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, c->stream);
    for (int r = 0; r < reps; r++) if (huff_blocks(c, b0, nb)) return -1;
    (void)hipEventRecord(e1, c->stream); (void)hipEventSynchronize(e1);
    float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return ms / reps;
}
// kernel experiments (tools/dbg/time_lz.py): phase A once, then phase B alone over blocks [b0, b0+nb), `reps` launches; returns ms per launch
// (the blocks' status is not looked at: knock-out builds produce wrong bytes on purpose)
extern "C" double dhts_debug_time_lz(dhts_ctx *c, int64_t b0, int64_t nb, int reps) {
    if (!c || hipSetDevice(c->device) != hipSuccess || b0 < 0 || nb <= 0 || b0 + nb > c->n_blocks) return -1;
    discard_prefetch(c);
    if (huff_blocks(c, b0, nb)) return -1;
    const uint64_t ulen = c->h_uoff[b0 + nb] - c->h_uoff[b0];
    if (c->ubuf[0].ensure(ulen + PAD_BYTES)) return -1;
    if (launch_lz(c, b0, nb, (uint8_t *)c->ubuf[0].p, c->h_uoff[b0], c->stream)) return -1;
    (void)hipStreamSynchronize(c->stream);
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, c->stream);
    for (int r = 0; r < reps; r++) if (launch_lz(c, b0, nb, (uint8_t *)c->ubuf[0].p, c->h_uoff[b0], c->stream)) return -1;
    (void)hipEventRecord(e1, c->stream); (void)hipEventSynchronize(e1);
    float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return ms / reps;
}
// cross-check aid for the tests (not part of the public header): run ONE phase-A kernel over blocks [b0, b0+nb) (kernel: 0 / 1 = lane
// per block with all symbols in LDS / with the far table, 2 = wave per block), then read a scratch slot back
extern "C" int dhts_debug_huff_run(dhts_ctx *c, int64_t b0, int64_t nb, int kernel) {
    if (!c || b0 < 0 || nb <= 0 || b0 + nb > c->n_blocks || kernel < 0 || kernel > 3) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    discard_prefetch(c);
    if (huff_blocks(c, b0, nb, kernel)) return -1;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
extern "C" int dhts_debug_scratch_get(dhts_ctx *c, int64_t s, uint32_t *meta4, uint8_t *lit, uint32_t *tok) {
    if (!c || s < 0 || s >= c->huff_nb) return -1;
    HIPCHK(c, hipMemcpy(meta4, (InflateMeta *)c->meta.p + s, 16, hipMemcpyDeviceToHost));
    if (meta4[3] != 0u) return 0;                                     // failed block: the scratch content is unspecified
    if (meta4[1] > DHTS_LIT_STRIDE || meta4[0] > DHTS_TOK_STRIDE) return fail(c, "scratch counts out of range");
    if (c->huff_packed) {
        unsigned long long off = 0;
        HIPCHK(c, hipMemcpy(&off, (unsigned long long *)c->blk_off.p + s, 8, hipMemcpyDeviceToHost));
        const uint8_t *lp = (const uint8_t *)c->lit.p + off;
        if (lit && meta4[1]) HIPCHK(c, hipMemcpy(lit, lp, meta4[1], hipMemcpyDeviceToHost));
        if (tok && meta4[0]) HIPCHK(c, hipMemcpy(tok, lp + ((meta4[1] + 15u) & ~15u), (size_t)meta4[0] * 4, hipMemcpyDeviceToHost));
        return 0;
    }
    if (lit && meta4[1]) HIPCHK(c, hipMemcpy(lit, (uint8_t *)c->lit.p + (size_t)s * DHTS_LIT_STRIDE, meta4[1], hipMemcpyDeviceToHost));
    if (tok && meta4[0]) HIPCHK(c, hipMemcpy(tok, (uint32_t *)c->tok.p + (size_t)s * DHTS_TOK_STRIDE, (size_t)meta4[0] * 4, hipMemcpyDeviceToHost));
    return 0;
}
int dhts_debug_meta(dhts_ctx *c, int64_t s, uint32_t *out4) {
    if (!c || s < 0 || s >= c->huff_nb) return -1;
    HIPCHK(c, hipMemcpy(out4, (InflateMeta *)c->meta.p + s, 16, hipMemcpyDeviceToHost));
    return 0;
}
