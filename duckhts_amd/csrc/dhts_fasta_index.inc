// dhts_fasta_index.inc -- part of dhts_api.hip (included there, inside its extern "C" block; not a translation unit of its own):
// fasta_index and read_fasta(region := ...): the .fai / .gzi builder over the batches of the text readers, the .fai reader, the region fetch.
// Kernels: fasta_index.hip.

// ---- build (fai_build_core, faidx.c:132-349; fai_save :352-377; the .gzi of bgzf_index_dump_hfile, bgzf.c:2382-2408) ---------------
// The block table of bytes that are neither gzip nor a text format index_impl knows by its first lines: pieces of 65,280 bytes
static int fasta_plain_table(dhts_ctx *c) {
    const uint64_t text_len = c->comp_len, P = 65280; const int64_t nb = (int64_t)((text_len + P - 1) / P);
    c->h_coff.resize(nb); c->h_clen.resize(nb); c->h_isize.resize(nb); c->h_uoff.resize(nb + 1);
    for (int64_t i = 0; i < nb; i++) { c->h_coff[i] = (uint64_t)i * P; c->h_uoff[i] = (uint64_t)i * P; const uint64_t l = text_len - (uint64_t)i * P < P ? text_len - (uint64_t)i * P : P; c->h_clen[i] = (uint32_t)l; c->h_isize[i] = (uint32_t)l; }
    c->h_uoff[nb] = text_len;
    ENSURE(c, c->coff, (size_t)nb * 8 + 64); ENSURE(c, c->clen, (size_t)nb * 4 + 64); ENSURE(c, c->isize, (size_t)nb * 4 + 64); ENSURE(c, c->uoff, (size_t)(nb + 1) * 8 + 64); ENSURE(c, c->blk_status, (size_t)(nb + 1) * 4);
    if (nb) { HIPCHK(c, hipMemcpy(c->coff.p, c->h_coff.data(), nb * 8, hipMemcpyHostToDevice)); HIPCHK(c, hipMemcpy(c->clen.p, c->h_clen.data(), nb * 4, hipMemcpyHostToDevice)); HIPCHK(c, hipMemcpy(c->isize.p, c->h_isize.data(), nb * 4, hipMemcpyHostToDevice)); }
    HIPCHK(c, hipMemcpy(c->uoff.p, c->h_uoff.data(), (nb + 1) * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(c->blk_status.p, 0, (size_t)(nb + 1) * 4));
    c->n_blocks = nb; c->bgzf_status = 0; c->plain_text = true;
    c->shard_b0 = 0; c->shard_b1 = nb; c->shard_rank = 0; c->shard_world = 1;
    return 0;
}
// the resident bytes begin like a gzip member (1f 8b); *bgzf: with the BC extra field of a BGZF block (bgzf.c check_header :896-905)
static int fasta_head_is_gzip(dhts_ctx *c, bool &gz, bool &bgzf) {
    uint8_t h[16] = {0}; gz = bgzf = false;
    if (c->comp_len < 2) return 0;
    HIPCHK(c, hipMemcpy(h, c->comp.p, c->comp_len < 16 ? (size_t)c->comp_len : 16, hipMemcpyDeviceToHost));
    gz = h[0] == 0x1f && h[1] == 0x8b;
    bgzf = gz && c->comp_len >= 16 && h[2] == 8 && (h[3] & 4) && h[10] == 6 && h[11] == 0 && h[12] == 'B' && h[13] == 'C' && h[14] == 2 && h[15] == 0;
    return 0;
}
static void fasta_scan_reset(dhts_ctx *c) {
    discard_prefetch(c);
    c->shard_b0 = 0; c->shard_b1 = c->n_blocks; c->shard_rank = 0; c->shard_world = 1; c->wins.clear(); c->win_cur = 0; c->scan_end_uoff = ~0ull; c->rg_empty_window = false;
    c->next_block = 0; c->carry_len = 0; c->stream_done = false; c->first_batch = true; c->ucur = 0; c->huff_b0 = c->huff_nb = 0; c->scan_first_uoff = 0;
}

extern "C" int64_t dhts_fasta_build_index(dhts_ctx *c) {
    if (!c) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    FastaState &F = c->fa;
    F.fai_text.clear(); F.gzi.clear();
    if (!c->segs.empty() || c->growing) return fail(c, "fasta_index: the whole file has to be resident");
    if (c->gz_plain) return fail(c, "Cannot index files compressed with gzip, please use bgzip");
    if (c->n_blocks == 0 && !c->plain_text && c->comp_len > 0) {
        bool gz, bgzf; if (fasta_head_is_gzip(c, gz, bgzf)) return -1;
        if (gz && !bgzf) return fail(c, "Cannot index files compressed with gzip, please use bgzip");
        if (gz) return fail(c, "fasta_index: no BGZF block table (dhts_bgzf_index comes first)");
        if (fasta_plain_table(c)) return -1;
    }
    fasta_scan_reset(c);
    const int64_t max_blocks = getenv("DHTS_BATCH_BLOCKS") ? atoll(getenv("DHTS_BATCH_BLOCKS")) : 0;
    // the record the batches carry (fai_build_core's name / seq_len / line_len / char_len / seq_offset / state / read_done)
    struct Cur { bool active = false, has_seq = false; int phase = 1; std::string name; uint64_t len = 0, seq_off = 0; uint32_t line_len = 0, line_blen = 0; } cur;
    struct Ent { std::string name; uint64_t len, off; uint32_t blen, llen; };
    std::vector<Ent> ents; std::map<std::string, int> seen;
    auto finish = [&]() {                                                       // fai_insert_index: the first of equal names stays (faidx.c:104-109)
        if (cur.active && cur.has_seq && seen.emplace(cur.name, 1).second) ents.push_back({cur.name, cur.len, cur.seq_off, cur.line_blen, cur.line_len});
        cur = Cur();
    };
    int64_t lineno = 0; bool any_header = false;
    std::vector<FaRec> recs; std::vector<uint32_t> ndst; std::vector<uint8_t> names;
    std::string eof_hdr; int64_t eof_hdr_line = 0;                              // a header line the end of the file cuts short
    while (c->n_blocks > 0) {
        Batch B;
        if (batch_begin(c, max_blocks, B)) return -1;
        if (B.blk_err) return fail(c, "fasta_index: the BGZF stream ended on an error");
        const uint8_t *u = B.u; const uint64_t ulen = B.ulen, out_base = B.out_base;
        uint64_t lines_end = ulen;
        if (ulen > 0) {
            const int64_t nchunks = (int64_t)((ulen + FA_CHUNK - 1) / FA_CHUNK);      // (the line table's chunks from 0: FA_CHUNK is VCF_CHUNK by definition, fasta_index.hip)
            // the last line of the file need not end in a newline; it counts one byte more all the same (faidx.c:260).  batch_clean_end is
            // B.final_batch here: a damaged block has returned above, and plain gzip, which alone sets gz_error, was refused before the scan
            LineTab T;
            if (line_table(c, c->lines, nullptr, u, 0, ulen, batch_clean_end(c, B), ~0ull, -1, T)) return -1;
            const uint64_t nl = T.nl; const int64_t nlines = T.nlines; const bool open_last = T.last_open != 0;
            lines_end = T.carry_start;
            if (nlines > 0) {
                const size_t ln = (size_t)(nlines + 2) * 4 + 64; const unsigned lgrid = (unsigned)((nlines + 255) / 256);
                ENSURE(c, F.gtmp, ln); ENSURE(c, F.cls, (size_t)nlines + 2 + 64); ENSURE(c, F.gchunk, (size_t)nchunks * 4 + 64); ENSURE(c, F.gbase, (size_t)(nchunks + 1) * 4 + 64);
                ENSURE(c, F.cl, ln); ENSURE(c, F.flag, ln); ENSURE(c, F.csum, ln); ENSURE(c, F.hrank, ln); ENSURE(c, F.err, 64);
                hipLaunchKernelGGL(fa_chunk_props, dim3((unsigned)nchunks), dim3(256), 0, c->stream, u, ulen, (const uint32_t *)c->lines.base.p, (uint32_t *)F.gtmp.p, (uint32_t *)F.gchunk.p, (uint8_t *)F.cls.p);
                const uint32_t *gin[1] = {(const uint32_t *)F.gchunk.p}; uint32_t *gout[1] = {(uint32_t *)F.gbase.p}; uint64_t gtotal = 0;
                if (run_scan(c, 1, gin, gout, nullptr, nchunks, &gtotal)) return -1;
                hipLaunchKernelGGL(fa_line_cl, dim3(lgrid), dim3(256), 0, c->stream, (const uint32_t *)c->lines.line_off.p, (const uint32_t *)F.gtmp.p, (const uint32_t *)F.gbase.p, (const uint8_t *)F.cls.p,
                                   (uint32_t)nlines, (uint32_t)nl, (uint32_t)gtotal, (uint32_t *)F.cl.p, (uint32_t *)F.flag.p);
                const uint32_t *in2[2] = {(const uint32_t *)F.cl.p, (const uint32_t *)F.flag.p}; uint32_t *out2[2] = {(uint32_t *)F.csum.p, (uint32_t *)F.hrank.p}; uint64_t tot2[2] = {0, 0};
                if (run_scan(c, 2, in2, out2, nullptr, nlines, tot2)) return -1;
                const uint32_t nhdr = (uint32_t)tot2[1];
                ENSURE(c, F.hdr, (size_t)(nhdr + 1) * 4 + 64); ENSURE(c, F.fshort, (size_t)(nhdr + 1) * 4 + 64); ENSURE(c, F.rec, (size_t)(nhdr + 1) * sizeof(FaRec) + 64);
                FaArgs a; memset(&a, 0, sizeof(a));
                a.u = u; a.ulen = ulen; a.line_off = (const uint32_t *)c->lines.line_off.p; a.cls = (const uint8_t *)F.cls.p; a.nlines = (uint32_t)nlines;
                a.cl = (const uint32_t *)F.cl.p; a.csum = (const uint32_t *)F.csum.p; a.hrank = (const uint32_t *)F.hrank.p; a.hdr_line = (const uint32_t *)F.hdr.p; a.nhdr = nhdr;
                a.c_phase = (cur.active && cur.phase == 0) ? 0u : 1u; a.c_line_len = cur.line_len;
                a.first_short = (uint32_t *)F.fshort.p; a.err = (unsigned long long *)F.err.p; a.rec = (FaRec *)F.rec.p;
                if (nhdr) hipLaunchKernelGGL(fq_compact, dim3(lgrid), dim3(256), 0, c->stream, (const uint32_t *)F.flag.p, (const uint32_t *)F.hrank.p, (uint32_t)nlines, (uint32_t *)F.hdr.p);
                HIPCHK(c, hipMemsetAsync(F.fshort.p, 0xff, (size_t)(nhdr + 1) * 4, c->stream));
                HIPCHK(c, hipMemsetAsync(F.err.p, 0xff, 8, c->stream));
                hipLaunchKernelGGL(fa_short, dim3(lgrid), dim3(256), 0, c->stream, a);
                hipLaunchKernelGGL(fa_check, dim3(lgrid), dim3(256), 0, c->stream, a);
                hipLaunchKernelGGL(fa_records, dim3((nhdr + 1 + 255) / 256), dim3(256), 0, c->stream, a);
                recs.resize((size_t)nhdr + 1); unsigned long long err = ~0ull;
                HIPCHK(c, hipMemcpyAsync(recs.data(), F.rec.p, ((size_t)nhdr + 1) * sizeof(FaRec), hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipMemcpyAsync(&err, F.err.p, 8, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                ndst.assign((size_t)nhdr + 2, 0);
                for (uint32_t r = 1; r <= nhdr; r++) ndst[r + 1] = ndst[r] + recs[r].name_len;
                names.resize(ndst[nhdr + 1]);
                if (nhdr) {
                    ENSURE(c, F.ndst, ((size_t)nhdr + 2) * 4 + 64); ENSURE(c, F.names, (size_t)ndst[nhdr + 1] + 64);
                    HIPCHK(c, hipMemcpyAsync(F.ndst.p, ndst.data(), ((size_t)nhdr + 2) * 4, hipMemcpyHostToDevice, c->stream));
                    hipLaunchKernelGGL(fa_names, dim3((nhdr + 255) / 256), dim3(256), 0, c->stream, u, (const FaRec *)F.rec.p, (const uint32_t *)F.ndst.p, nhdr, (uint8_t *)F.names.p);
                    if (!names.empty()) HIPCHK(c, hipMemcpyAsync(names.data(), F.names.p, names.size(), hipMemcpyDeviceToHost, c->stream));
                    HIPCHK(c, hipStreamSynchronize(c->stream));
                }
                auto name_of = [&](uint32_t r) { return std::string((const char *)names.data() + ndst[r], recs[r].name_len); };
                if (err != ~0ull) {                                              // the first line fai_build_core stops at
                    const uint32_t e = (uint32_t)(err >> 3), kind = (uint32_t)(err & 7);
                    uint32_t seg = 0; while (seg < nhdr && recs[seg + 1].hdr_line < e) seg++;
                    const std::string nm = seg ? name_of(seg) : cur.name;
                    const long long ln1 = (long long)(lineno + e + 1);
                    if (seg == 0 && !any_header && kind == FA_ERR_AT) return fail(c, "fasta_index: the first record starts with '@': this is FASTQ, and FASTQ indexes (six columns, qual_offset) are not built");
                    if (kind == FA_ERR_DIFFLEN) return fail(c, "Different line length in sequence '%s' at line %lld", nm.c_str(), ln1);
                    if (kind == FA_ERR_AT) return fail(c, "Found '@' in a FASTA file, error at line %lld", ln1);
                    if (kind == FA_ERR_CR) return fail(c, "Format error, carriage return not followed by new line at line %lld", ln1);
                    uint64_t lo = 0; uint8_t ch = 0;
                    if (line_start(c, c->lines, e, lo)) return -1;
                    HIPCHK(c, hipMemcpy(&ch, u + lo, 1, hipMemcpyDeviceToHost));
                    if (ch >= 0x20 && ch <= 0x7e) return fail(c, "Format error, unexpected \"%c\" at line %lld", (char)ch, ln1);
                    return fail(c, "Format error, unexpected character at line %lld", ln1);
                }
                // the lines in front of the first header continue the carried record
                if (cur.active && cur.phase == 0 && recs[0].nlines > 0) {
                    if (cur.line_len == 0 && recs[0].first_ll) { cur.line_len = recs[0].first_ll; cur.line_blen = recs[0].first_cl; cur.has_seq = true; }
                    cur.len += recs[0].len;
                    if (recs[0].first_short != FA_NONE) cur.phase = 1;
                }
                for (uint32_t r = 1; r <= nhdr; r++) {
                    const FaRec &R = recs[r];
                    if (open_last && R.hdr_line + 1 == (uint32_t)nlines) {       // the file ends inside this header line
                        eof_hdr_line = lineno + R.hdr_line + 1;
                        uint64_t lo = 0; if (line_start(c, c->lines, R.hdr_line, lo)) return -1;
                        eof_hdr.assign((size_t)(ulen - lo), '\0');
                        HIPCHK(c, hipMemcpy(&eof_hdr[0], u + lo, (size_t)(ulen - lo), hipMemcpyDeviceToHost));
                        if (eof_hdr.size() == 1) break;                          // a bare '>' as the last byte: IN_NAME is never entered, the record in front of it is still open
                    }
                    finish();
                    cur.active = true; cur.name = name_of(r); cur.seq_off = out_base + R.seq_off; cur.len = R.len; cur.line_len = R.first_ll; cur.line_blen = R.first_cl;
                    cur.has_seq = R.first_ll != 0; cur.phase = R.first_short != FA_NONE ? 1 : 0;
                    any_header = true;
                }
                lineno += nlines;
            }
        }
        int32_t status = 0;
        if (batch_end(c, B, lines_end, false, false, &status)) return -1;
        if (status == 1) break;
        if (status < 0) return fail(c, "fasta_index: the BGZF stream ended on an error");
    }
    fasta_scan_reset(c);
    if (!eof_hdr.empty()) {
        if (eof_hdr.size() == 1) {                                              // faidx.c:334-340 with the state of the record in front
            if (!(cur.active && cur.has_seq)) return fail(c, "File truncated at line %lld", (long long)eof_hdr_line);
        } else {
            std::string nm; size_t k = 1; bool broke = false;                   // faidx.c:205-218
            for (; k < eof_hdr.size(); k++) { const uint8_t b = (uint8_t)eof_hdr[k]; const bool sp = b == ' ' || (b >= '\t' && b <= '\r'); if (!sp) nm.push_back((char)b); else if (!nm.empty()) { broke = true; break; } }
            if (!broke) return fail(c, "The last entry '%s' has no sequence at line %lld", nm.c_str(), (long long)eof_hdr_line);
            return fail(c, "File truncated at line %lld", (long long)eof_hdr_line + 1);
        }
    } else if (!(cur.active && cur.has_seq)) return fail(c, "File truncated at line %lld", (long long)lineno + 1);
    finish();
    for (auto &e : ents) {
        char buf[128]; snprintf(buf, sizeof(buf), "\t%llu\t%llu\t%u\t%u\n", (unsigned long long)e.len, (unsigned long long)e.off, e.blen, e.llen);
        F.fai_text += e.name; F.fai_text += buf;
    }
    if (!c->plain_text) {                                                       // one record per non-empty block behind the first (bgzf.c:1225-1236, 2402-2407)
        std::vector<uint64_t> g; int64_t seen_blocks = 0;
        for (int64_t b = 0; b < c->n_blocks; b++) { if (c->h_isize[b] == 0) continue; if (seen_blocks++ > 0) { g.push_back(c->h_coff[b]); g.push_back(c->h_uoff[b]); } }
        const uint64_t cnt = g.size() / 2;
        F.gzi.resize(8 + g.size() * 8);
        memcpy(F.gzi.data(), &cnt, 8); if (!g.empty()) memcpy(F.gzi.data() + 8, g.data(), g.size() * 8);
    }
    return (int64_t)F.fai_text.size();
}
extern "C" int dhts_fasta_index_bytes(dhts_ctx *c, void *dst, uint64_t n) {
    if (!c) return -1;
    if (n < c->fa.fai_text.size()) return fail(c, "dhts_fasta_index_bytes: %llu bytes are needed", (unsigned long long)c->fa.fai_text.size());
    if (!c->fa.fai_text.empty()) memcpy(dst, c->fa.fai_text.data(), c->fa.fai_text.size());
    return 0;
}
extern "C" int64_t dhts_fasta_gzi_bytes(dhts_ctx *c, void *dst, uint64_t n) {
    if (!c) return -1;
    if (n == 0) return (int64_t)c->fa.gzi.size();
    if (n < c->fa.gzi.size()) return fail(c, "dhts_fasta_gzi_bytes: %llu bytes are needed", (unsigned long long)c->fa.gzi.size());
    if (!c->fa.gzi.empty()) memcpy(dst, c->fa.gzi.data(), c->fa.gzi.size());
    return (int64_t)c->fa.gzi.size();
}

// ---- .fai reader (fai_read, faidx.c:380-446) and regions (fai_parse_region = hts_parse_region with flags 0; fai_get_val :798-827) -------
extern "C" int dhts_fasta_load_index(dhts_ctx *c, const void *fai, uint64_t n) {
    if (!c) return -1;
    FastaState &F = c->fa;
    F.idx_names.clear(); F.ents.clear(); F.by_name.clear(); F.loaded = false;
    const char *p = (const char *)fai, *end = p + n; long lnum = 1;
    while (p < end) {
        const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
        std::string line(p, nl ? (size_t)(nl - p) + 1 : (size_t)(end - p));
        p += line.size();
        size_t k = 0; while (k < line.size() && line[k] && !(line[k] == ' ' || (line[k] >= '\t' && line[k] <= '\r'))) k++;
        const std::string name = line.substr(0, k);
        unsigned long long len = 0, off = 0; unsigned blen = 0, llen = 0;
        if (sscanf(k < line.size() ? line.c_str() + k + 1 : "", "%llu%llu%u%u", &len, &off, &blen, &llen) != 4) return fail(c, "Could not understand FASTA index line %ld", lnum);
        // (fai_read takes any four numbers; a line shorter than its bases makes fai_retrieve's read lengths negative there -- refused here)
        if (llen < blen) return fail(c, "FASTA index line %ld: line_len %u is smaller than line_blen %u", lnum, llen, blen);
        if (F.by_name.emplace(name, (int)F.ents.size()).second) { F.idx_names.push_back(name); F.ents.push_back({len, off, blen, llen}); }
        if (nl) lnum++;
    }
    F.loaded = true;
    return 0;
}
// "a:1-10, b" -> the regions in the order given (split at commas, blanks trimmed, empty pieces dropped: parse_regions_duckdb,
// src/seq_reader.c:192-229), each resolved and clamped.  `need`: the bytes fai_retrieve reads from `start` on (every line it crosses with
// its terminator, faidx.c:752-785).
struct FaQuery { std::string text; int id; uint64_t beg, n, start, need; };
static int fasta_parse_regions(dhts_ctx *c, const char *regions, std::vector<FaQuery> &q, bool skip_unknown) {
    FastaState &F = c->fa;
    if (!F.loaded) return fail(c, "read_fasta: no FASTA index is loaded (dhts_fasta_load_index comes first)");
    std::string all(regions ? regions : ""); size_t p = 0;
    while (p <= all.size()) {
        size_t e = all.find(',', p); if (e == std::string::npos) e = all.size();
        std::string tok = all.substr(p, e - p); p = e + 1;
        size_t a = 0; while (a < tok.size() && (tok[a] == ' ' || tok[a] == '\t')) a++;
        size_t b = tok.size(); while (b > a && (tok[b - 1] == ' ' || tok[b - 1] == '\t')) b--;
        tok = tok.substr(a, b - a);
        if (tok.empty()) continue;
        int tid = -1; int64_t beg = 0, end = 0;
        auto getid = [&](const std::string &nm) { auto it = F.by_name.find(nm); return it == F.by_name.end() ? -1 : it->second; };
        if (!parse_region_token_fn(getid, tok, tid, beg, end)) { if (skip_unknown) continue; return fail(c, "Reference %s not found in FASTA file", tok.c_str()); }
        const FastaState::Ent &v = F.ents[(size_t)tid];
        if ((uint64_t)beg >= v.len) beg = (int64_t)v.len;
        if ((uint64_t)end >= v.len) end = (int64_t)v.len;
        if (beg > end) beg = end;
        FaQuery x; x.text = tok; x.id = tid; x.beg = (uint64_t)beg; x.n = (uint64_t)(end - beg); x.start = 0; x.need = 0;
        if (v.blen == 0) { if (skip_unknown) continue; return fail(c, "Invalid line length in index: %u", v.blen); }
        x.start = v.off + x.beg / v.blen * v.llen + x.beg % v.blen;
        const uint64_t first_blen = v.blen - x.beg % v.blen, first_len = v.llen - x.beg % v.blen;
        if (x.n <= first_blen) x.need = x.n;
        else {
            uint64_t rem = x.n - first_blen; x.need = first_len;
            const uint64_t full = (rem - 1) / v.blen;                           // "while (remaining > line_blen)"
            x.need += full * v.llen + (rem - full * v.blen);
        }
        q.push_back(x);
    }
    return 0;
}
// Stages what a region query reads: of an uncompressed file only the byte windows of the regions (merged where they touch), of a
// BGZF file everything (no .gzi is needed that way).  dhts_fasta_fetch follows.
extern "C" int dhts_fasta_open_regions(dhts_ctx *c, const char *path, const char *regions) {
    if (!c || !path) return -1;
    std::vector<FaQuery> q;
    if (fasta_parse_regions(c, regions, q, true)) return -1;                    // (a region that does not resolve is dhts_fasta_fetch's to report)
    uint8_t h[2] = {0, 0};
    { int fd = open(path, O_RDONLY); if (fd < 0) return fail(c, "cannot open %s", path); const ssize_t r = pread(fd, h, 2, 0); close(fd); if (r < 0) return fail(c, "read error on %s", path); }
    if (h[0] == 0x1f && h[1] == 0x8b) {
        if (dhts_open_path(c, path) != 0 || dhts_bgzf_index(c) < 0) return -1;
        return 0;
    }
    std::vector<uint64_t> beg, end;
    for (auto &x : q) if (x.need) { beg.push_back(x.start); end.push_back(x.start + x.need); }
    if (open_path_ranges(c, path, 0, beg.data(), end.data(), (int64_t)beg.size(), true)) return -1;
    if (getenv("DHTS_TRACE")) fprintf(stderr, "[dhts] read_fasta: %zu regions, %llu of %llu bytes staged\n", q.size(), (unsigned long long)c->comp_len, (unsigned long long)c->file_size);
    return 0;
}
// the uncompressed text the index speaks of: the resident bytes themselves, or what the BGZF blocks inflate to (the whole file, once)
static int fasta_text(dhts_ctx *c, const uint8_t *&text, uint64_t &text_len) {
    FastaState &F = c->fa;
    if (c->gz_plain) return fail(c, "Failed to retrieve block. (Seeking in a compressed, .gzi unindexed, file?)");
    if (!c->segs.empty()) { text = (const uint8_t *)c->comp.p; text_len = c->file_size; return 0; }
    if (c->n_blocks == 0 && !c->plain_text) {
        bool gz, bgzf; if (fasta_head_is_gzip(c, gz, bgzf)) return -1;
        if (gz) { if (dhts_bgzf_index(c) < 0) return -1; if (c->gz_plain) return fail(c, "Failed to retrieve block. (Seeking in a compressed, .gzi unindexed, file?)"); }
    }
    if (c->plain_text || c->n_blocks == 0) { text = (const uint8_t *)c->comp.p; text_len = c->comp_len; return 0; }
    if (!F.text_ready) {
        fasta_scan_reset(c);
        for (;;) {
            Batch B;
            if (batch_begin(c, 0, B)) return -1;
            if (B.blk_err) return fail(c, "read_fasta: the BGZF stream ended on an error");
            const uint64_t total = c->h_uoff[c->n_blocks];                      // (read behind batch_begin: phase A may correct the table)
            if (F.text.cap < total + PAD_BYTES) { if (ensure_keep(c, F.text, total + PAD_BYTES, B.out_base)) return -1; }
            if (B.ulen) HIPCHK(c, hipMemcpyAsync((uint8_t *)F.text.p + B.out_base, B.u, B.ulen, hipMemcpyDeviceToDevice, c->stream));
            int32_t status = 0;
            if (batch_end(c, B, B.ulen, false, false, &status)) return -1;
            if (status == 1) break;
            if (status < 0) return fail(c, "read_fasta: the BGZF stream ended on an error");
        }
        F.text_len = c->h_uoff[c->n_blocks]; F.text_ready = true;
        fasta_scan_reset(c);
    }
    text = (const uint8_t *)F.text.p; text_len = F.text_len;
    return 0;
}
extern "C" int dhts_fasta_fetch(dhts_ctx *c, const char *regions, dhts_fasta_batch *out) {
    if (!c || !out) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    memset(out, 0, sizeof(*out));
    FastaState &F = c->fa;
    std::vector<FaQuery> q;
    if (fasta_parse_regions(c, regions, q, false)) return -1;
    const uint8_t *text = nullptr; uint64_t text_len = 0;
    if (fasta_text(c, text, text_len)) return -1;
    const size_t n = q.size();
    std::vector<FaRegion> rg(n); std::vector<uint64_t> noff(n + 1, 0), soff(n + 1, 0); std::string nbytes;
    for (size_t i = 0; i < n; i++) {
        const FaQuery &x = q[i]; const FastaState::Ent &v = F.ents[(size_t)x.id];
        if (x.need && x.start + x.need > text_len) return fail(c, "Failed to retrieve block: unexpected end of file");
        int64_t delta = 0;                                                      // resident offset - file offset of the region's bytes
        if (!c->segs.empty() && x.need) {
            bool found = false;
            for (auto &s : c->segs) if (x.start >= s.file_off && x.start + x.need <= s.file_off + s.len) { delta = (int64_t)s.res_off - (int64_t)s.file_off; found = true; break; }
            if (!found) return fail(c, "read_fasta: region '%s' was not staged (dhts_fasta_open_regions takes the same regions)", x.text.c_str());
        }
        rg[i].out_off = soff[i]; rg[i].n = x.n; rg[i].beg = x.beg; rg[i].src = (int64_t)v.off + delta; rg[i].blen = v.blen; rg[i].llen = v.llen;
        soff[i + 1] = soff[i] + x.n;
        const size_t colon = x.text.find(':');                                  // NAME is the region text up to its first ':' (seq_reader.c:443-446)
        nbytes += x.text.substr(0, colon);
        noff[i + 1] = nbytes.size();
    }
    const uint64_t total = soff[n];
    ENSURE(c, F.o_noff, (n + 1) * 8 + 64); ENSURE(c, F.o_soff, (n + 1) * 8 + 64); ENSURE(c, F.o_name, nbytes.size() + 64); ENSURE(c, F.o_seq, total + PAD_BYTES); ENSURE(c, F.rg, n * sizeof(FaRegion) + 64);
    HIPCHK(c, hipMemcpyAsync(F.o_noff.p, noff.data(), (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(F.o_soff.p, soff.data(), (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (!nbytes.empty()) HIPCHK(c, hipMemcpyAsync(F.o_name.p, nbytes.data(), nbytes.size(), hipMemcpyHostToDevice, c->stream));
    if (n) HIPCHK(c, hipMemcpyAsync(F.rg.p, rg.data(), n * sizeof(FaRegion), hipMemcpyHostToDevice, c->stream));
    if (total) hipLaunchKernelGGL(fa_fetch, dim3((unsigned)((total + 4095) / 4096)), dim3(256), 0, c->stream, text, (const FaRegion *)F.rg.p, (uint32_t)n, total, (uint8_t *)F.o_seq.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));                                 // (the host vectors above are the copies' sources)
    out->n_rows = (int64_t)n; out->name_off = (const uint64_t *)F.o_noff.p; out->name_bytes = (const uint8_t *)F.o_name.p; out->name_nbytes = nbytes.size();
    out->seq_off = (const uint64_t *)F.o_soff.p; out->seq_bytes = (const uint8_t *)F.o_seq.p; out->seq_nbytes = total;
    return 0;
}
// read-back in the style of dhts_bam_batch_fetch: the columns of `dev` into `arena` (offsets first, 8-byte aligned), `host` points into it
static uint64_t fasta_up8(uint64_t x) { return (x + 7) & ~7ull; }
extern "C" uint64_t dhts_fasta_batch_host_bytes(const dhts_fasta_batch *b) {
    if (!b) return 0;
    return 2 * (uint64_t)(b->n_rows + 1) * 8 + fasta_up8(b->name_nbytes) + fasta_up8(b->seq_nbytes) + 8;
}
extern "C" int dhts_fasta_batch_fetch(dhts_ctx *c, const dhts_fasta_batch *dev, void *arena, uint64_t cap, dhts_fasta_batch *host) {
    if (!c || !dev || !host) return -1;
    if (!arena || cap < dhts_fasta_batch_host_bytes(dev)) return fail(c, "dhts_fasta_batch_fetch: the arena is too small");
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t no = (uint64_t)(dev->n_rows + 1) * 8;
    uint8_t *a = (uint8_t *)arena;
    uint64_t *h_noff = (uint64_t *)a, *h_soff = (uint64_t *)(a + no); uint8_t *h_name = a + 2 * no, *h_seq = h_name + fasta_up8(dev->name_nbytes);
    HIPCHK(c, hipMemcpyAsync(h_noff, dev->name_off, no, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_soff, dev->seq_off, no, hipMemcpyDeviceToHost, c->stream));
    if (dev->name_nbytes) HIPCHK(c, hipMemcpyAsync(h_name, dev->name_bytes, dev->name_nbytes, hipMemcpyDeviceToHost, c->stream));
    if (dev->seq_nbytes) HIPCHK(c, hipMemcpyAsync(h_seq, dev->seq_bytes, dev->seq_nbytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *host = *dev; host->name_off = h_noff; host->seq_off = h_soff; host->name_bytes = h_name; host->seq_bytes = h_seq;
    return 0;
}
