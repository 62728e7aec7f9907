// dhts_bam_open.inc -- part of dhts_api.hip (included there, inside its extern "C" block; not a translation unit of its own):
// BAM header + @RG dictionary on the host, block-range shards, one file over several GPUs.
// ---- BAM header (host mirror of bam_hdr_read + the @RG dictionary) ---------------------------
static inline uint32_t hle32(const uint8_t *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
static bool is_alpha(char ch) { return (ch >= 'a' && ch <= 'z') || (ch >= 'A' && ch <= 'Z'); }

#define SAM_SEQ_ONLY "SAM text is read as one sequential scan"
#define FASTQ_SEQ_ONLY "FASTQ/FASTA text is read as one sequential scan"
// htslib/header.c:995-1075 + 830-893 + 271-318: any malformed line voids the dictionary
static void parse_rg_dict(dhts_ctx *c) {
    c->rg_id.clear(); c->rg_sm.clear(); c->rg_has_sm.clear();
    const char *text = c->text.data(); size_t len = c->text.size();
    bool ok = true;
    if (len < 3) { return; }
    size_t i = 0;
    while (ok && i < len - 3 && text[i] != '\0') {
        const char *h = text + i; size_t rem = len - i;
        if (h[0] != '@' || !is_alpha(h[1]) || !is_alpha(h[2]) || rem < 3 || h[3] == '\n') { ok = false; break; }
        bool is_rg = h[1] == 'R' && h[2] == 'G', is_co = h[1] == 'C' && h[2] == 'O';
        size_t j = 3; std::string id, sm; bool has_id = false, sm_seen = false;
        if (is_co) {
            if (rem == 3 || h[3] != '\t') { ok = false; break; }
            for (j = 4; j < rem && h[j] != '\0' && h[j] != '\n'; j++) {}
        } else {
            do {
                if (j == rem || h[j] != '\t') { ok = false; break; }
                size_t k = ++j;
                while (k < rem && h[k] != '\0' && h[k] != '\n' && h[k] != '\t') k++;
                if (k - j < 3 || h[j + 2] != ':') { ok = false; break; }
                if (is_rg && h[j] == 'I' && h[j + 1] == 'D' && !has_id) { id.assign(h + j + 3, k - j - 3); has_id = true; }
                if (is_rg && h[j] == 'S' && h[j + 1] == 'M' && !sm_seen) { sm.assign(h + j + 3, k - j - 3); sm_seen = true; }
                j = k;
            } while (j < rem && h[j] != '\0' && h[j] != '\n');
            if (!ok) break;
        }
        if (is_rg) {
            if (!has_id) { ok = false; break; }
            bool dup = false; for (auto &e : c->rg_id) if (e == id) dup = true;
            if (!dup) { c->rg_id.push_back(id); c->rg_sm.push_back(sm); c->rg_has_sm.push_back(sm_seen && !sm.empty()); }
        }
        i += j + 1;
    }
    if (!ok) { c->rg_id.clear(); c->rg_sm.clear(); c->rg_has_sm.clear(); }
}

// ---- SAM text header (sam_hdr_build_from_sam_file, htslib header.c:1353+): the leading lines that start with '@' --------------------------
// Every line needs '@' + a two-letter type of HD / SQ / RG / PG / CO (a bare "@CO" is read as "@CO\t"); a line other than @CO is
// tab-separated KEY:value fields.  sam_hrecs_update_hashes (header.c:141-300): @SQ needs SN and LN (the last SN / AN / LN tag of the line
// counts; LN is strtoll's value, and two LN tags with different values are an error); an SN that names an earlier @SQ is an error, an SN that
// an earlier AN took is a warning and the name moves to the new reference; AN:alt,names resolve to the tid unless the name is taken
// (header.c:90-112); @RG needs ID.  target_len is LN clamped to UINT32_MAX (sam_hdr_update_target_arrays, header.c:1110-1121).
// -> 0 parsed (ref_name / ref_len / text / first_rec_uoff / the name dictionary on the device), 1 the header runs beyond `good` and more
// bytes can be had, -1 malformed.
static int sam_header_parse(dhts_ctx *c, const uint8_t *h, uint64_t good, bool more) {
    c->ref_name.clear(); c->ref_len.clear(); c->text.clear();
    std::unordered_map<std::string, int32_t> names;                  // SN and AN names -> tid
    uint64_t p = 0;
    for (;;) {
        if (p >= good) { if (more) return 1; break; }
        if (h[p] != '@') break;
        const uint8_t *nl = (const uint8_t *)memchr(h + p, '\n', good - p);
        if (!nl && more) return 1;
        const uint64_t e = nl ? (uint64_t)(nl - h) : good;
        uint64_t l = e - p;
        if (l && h[p + l - 1] == '\r') l--;
        { uint64_t z = 0; while (z < l && h[p + z]) z++; l = z; }                 // (a C string)
        std::string line((const char *)h + p, l);
        p = nl ? e + 1 : good;
        if (l < 3 || !is_alpha(line[1]) || !is_alpha(line[2])) return -1;
        if (line == "@CO") line += '\t';                                           // (htslib's original reader took an untabbed @CO)
        const std::string ty = line.substr(1, 2);
        if (ty != "HD" && ty != "SQ" && ty != "RG" && ty != "PG" && ty != "CO") return -1;
        c->text += line; c->text += '\n';
        if (line.size() == 3 || line[3] != '\t') return -1;
        if (ty == "CO") continue;
        std::string sn, an; long long len = -1; bool has_sn = false, has_an = false, has_id = false, inv_ln = false;
        size_t j = 4;
        for (;;) {
            size_t k = line.find('\t', j); if (k == std::string::npos) k = line.size();
            if (k - j < 3 || line[j + 2] != ':') return -1;
            const std::string key = line.substr(j, 2), val = line.substr(j + 3, k - j - 3);
            if (key == "SN") { sn = val; has_sn = true; }
            else if (key == "LN") { const long long t = strtoll(val.c_str(), nullptr, 10); if (len != -1 && len != t) inv_ln = true; len = t; }
            else if (key == "AN") { an = val; has_an = true; }
            if (key == "ID") has_id = true;
            if (k == line.size()) break;
            j = k + 1;
        }
        if (ty == "RG" && !has_id) return -1;                                      // "Header includes @RG line with no ID: tag"
        if (ty != "SQ") continue;
        if (!has_sn || len == -1 || inv_ln) return -1;
        const int32_t tid = (int32_t)c->ref_name.size();
        for (auto &r : c->ref_name) if (r == sn) return -1;                        // "Duplicate entry in sam header"
        names[sn] = tid;                                                           // (a name an earlier AN took moves here)
        c->ref_name.push_back(sn); c->ref_len.push_back(len < 0xffffffffll ? (uint32_t)len : 0xffffffffu);
        for (size_t a0 = 0; has_an && a0 <= an.size();) {
            size_t a1 = an.find(',', a0); if (a1 == std::string::npos) a1 = an.size();
            const std::string alt = an.substr(a0, a1 - a0);
            if (!alt.empty() && !names.count(alt)) names[alt] = tid;
            a0 = a1 + 1;
        }
    }
    c->first_rec_uoff = p; c->scan_first_uoff = p;
    // the names on the device: offsets, bytes, tids and an open-addressing table over FNV-1a (vcf_dict_find)
    std::vector<uint32_t> off(1, 0), ids; std::string bytes; std::vector<std::string> nv;
    for (auto &e : names) { bytes += e.first; off.push_back((uint32_t)bytes.size()); ids.push_back(e.second); nv.push_back(e.first); }
    uint32_t hsz = 16; while (hsz < 2 * names.size() + 16) hsz <<= 1;
    std::vector<uint32_t> hash(hsz, 0);
    for (size_t i = 0; i < nv.size(); i++) {
        uint32_t hh = vcf_name_hash((const uint8_t *)nv[i].data(), (uint32_t)nv[i].size()) & (hsz - 1);
        while (hash[hh]) hh = (hh + 1) & (hsz - 1);
        hash[hh] = (uint32_t)i + 1;
    }
    ENSURE(c, c->s_name_off, off.size() * 4 + 64); ENSURE(c, c->s_name_bytes, bytes.size() + 64); ENSURE(c, c->s_name_id, ids.size() * 4 + 64); ENSURE(c, c->s_name_hash, (size_t)hsz * 4 + 64);
    HIPCHK(c, hipMemcpy(c->s_name_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice));
    if (!bytes.empty()) HIPCHK(c, hipMemcpy(c->s_name_bytes.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
    if (!ids.empty()) HIPCHK(c, hipMemcpy(c->s_name_id.p, ids.data(), ids.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->s_name_hash.p, hash.data(), (size_t)hsz * 4, hipMemcpyHostToDevice));
    c->s_name_hmask = hsz - 1; c->s_n_names = (int32_t)names.size();
    return 0;
}

int dhts_bam_open(dhts_ctx *c) {
    if (!c) return -1;
    c->sam_text = false; c->fastq = 0;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n_blocks <= 0) return fail(c, "Failed to read SAM/BAM/CRAM header");
    // inflate leading blocks until the header is complete
    int64_t k = c->n_blocks < 4 ? c->n_blocks : 4;
    std::vector<uint8_t> h; std::vector<int32_t> bs;
    for (;;) {
        if (huff_ensure(c, 0, k, k)) return -1;              // (phase A first: the block table may be corrected from the decoded lengths)
        uint64_t total = c->h_uoff[k];
        h.resize(total + 16); bs.resize(k);
        if (dhts_bgzf_inflate_to_host(c, 0, k, h.data(), total, bs.data()) < 0) {
            if (c->h_uoff[k] != total) continue;             // a scratch retry inside moved the block table: size the buffer from it again
            return -1;
        }
        total = c->h_uoff[k];                                // (an overstated ISIZE behind a scratch retry: the stream is shorter than the buffer)
        uint64_t good = total;
        for (int64_t b = 0; b < k; b++) if (bs[b] != 0) { good = c->h_uoff[b]; break; }
        // try to parse
        bool need_more = false, bad = false; uint64_t p = 0;
        auto need = [&](uint64_t nbytes) { if (p + nbytes > good) { if (good == total && k < c->n_blocks) need_more = true; else bad = true; return false; } return true; };
        c->ref_name.clear(); c->ref_len.clear();
        const int fq = (good >= 4 && memcmp(h.data(), "BAM\1", 4) == 0) || good == 0 ? 0 : fastq_text_detect(h.data(), (size_t)good);
        if (fq) {
            // FASTQ / FASTA (sam_hdr_read, sam.c:1941-1943): an empty header.  A first record fastq_parse1 refuses keeps the header error
            // (the reference returns zero rows for such a file: INTEGRATION.md)
            const int r = fastq_first_record(h.data(), good, good == total && k < c->n_blocks, fq == 2);
            if (r > 0) { k = (k * 4 < c->n_blocks) ? k * 4 : c->n_blocks; continue; }
            if (r < 0) return fail(c, "Failed to read SAM/BAM/CRAM header");
            c->text.clear(); c->first_rec_uoff = 0; c->scan_first_uoff = 0; c->s_n_names = 0;
            c->sam_text = true; c->fastq = fq;
            break;
        }
        if (!(good >= 4 && memcmp(h.data(), "BAM\1", 4) == 0) && good > 0 && sam_text_detect(h.data(), (size_t)good)) {
            const int r = sam_header_parse(c, h.data(), good, good == total && k < c->n_blocks);
            if (r > 0) { k = (k * 4 < c->n_blocks) ? k * 4 : c->n_blocks; continue; }
            if (r < 0) { c->ref_name.clear(); c->ref_len.clear(); return fail(c, "Failed to read SAM/BAM/CRAM header"); }
            c->sam_text = true;
            break;
        }
        do {
            if (!need(8)) break;
            if (memcmp(h.data(), "BAM\1", 4) != 0) { bad = true; break; }
            uint32_t l_text = hle32(h.data() + 4); p = 8;
            if (!need(l_text)) break;
            c->text.assign((const char *)h.data() + p, l_text); p += l_text;
            if (!need(4)) break;
            int32_t n_ref = (int32_t)hle32(h.data() + p); p += 4;
            if (n_ref < 0) { bad = true; break; }
            for (int32_t i = 0; i < n_ref; i++) {
                if (!need(4)) break;
                int32_t l_name = (int32_t)hle32(h.data() + p); p += 4;
                if (l_name <= 0) { bad = true; break; }
                if (!need((uint64_t)l_name + 4)) break;
                size_t nl = strnlen((const char *)h.data() + p, (size_t)l_name);
                c->ref_name.emplace_back((const char *)h.data() + p, nl); p += (uint64_t)l_name;
                c->ref_len.push_back(hle32(h.data() + p)); p += 4;
            }
        } while (0);
        if (bad) return fail(c, "Failed to read SAM/BAM/CRAM header");
        if (need_more) { k = (k * 4 < c->n_blocks) ? k * 4 : c->n_blocks; continue; }
        c->first_rec_uoff = p; c->scan_first_uoff = p;
        break;
    }
    c->ref_name_p.clear(); for (auto &s : c->ref_name) c->ref_name_p.push_back(s.c_str());
    parse_rg_dict(c);
    c->rg_id_p.clear(); c->rg_sm_p.clear();
    std::vector<uint32_t> off; std::string bytes; off.push_back(0);
    for (size_t i = 0; i < c->rg_id.size(); i++) {
        c->rg_id_p.push_back(c->rg_id[i].c_str()); c->rg_sm_p.push_back(c->rg_has_sm[i] ? c->rg_sm[i].c_str() : nullptr);
        bytes += c->rg_id[i]; off.push_back((uint32_t)bytes.size());
    }
    ENSURE(c, c->d_rg_off, off.size() * 4 + 16); ENSURE(c, c->d_rg_bytes, bytes.size() + 16);
    HIPCHK(c, hipMemcpy(c->d_rg_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice));
    if (!bytes.empty()) HIPCHK(c, hipMemcpy(c->d_rg_bytes.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
    c->bam_open = true;
    return dhts_bam_rewind(c);
}

int dhts_bam_header_get(const dhts_ctx *c, dhts_bam_header *out) {
    if (!c || !c->bam_open) return -1;
    out->n_ref = (int32_t)c->ref_name.size(); out->ref_name = c->ref_name_p.data(); out->ref_len = c->ref_len.data();
    out->text = c->text.data(); out->l_text = (uint32_t)c->text.size();
    out->n_rg = (int32_t)c->rg_id.size(); out->rg_id = c->rg_id_p.data(); out->rg_sm = c->rg_sm_p.data();
    out->first_rec_uoff = c->first_rec_uoff;
    return 0;
}

// contiguous block ranges balanced by compressed bytes (SURVEY.md 8(e)); pure host arithmetic, no device needed
int dhts_shard_cut(const uint64_t *coff, int64_t n_blocks, uint64_t comp_len, int rank, int world, int64_t *b0, int64_t *b1) {
    if (!coff || world < 1 || rank < 0 || rank >= world || !b0 || !b1) return -1;
    auto cut = [&](int r) -> int64_t {
        if (r <= 0) return 0;
        if (r >= world) return n_blocks;
        uint64_t target = (uint64_t)((__uint128_t)comp_len * (unsigned)r / (unsigned)world);
        int64_t lo = 0, hi = n_blocks;
        while (lo < hi) { int64_t mid = (lo + hi) / 2; if (coff[mid] < target) lo = mid + 1; else hi = mid; }
        return lo;
    };
    *b0 = cut(rank); *b1 = cut(rank + 1);
    return 0;
}

int dhts_bam_set_block_range(dhts_ctx *c, int64_t b0, int64_t b1, int speculative_start) {
    BED_REFUSE(c, "a block range");
    if (!c || b0 < 0 || b1 < b0 || b1 > c->n_blocks) return -1;
    if (c->fastq && (b0 != 0 || b1 != c->n_blocks || speculative_start)) return fail(c, "read_bam: shards of FASTQ/FASTA text are not supported (%s)", FASTQ_SEQ_ONLY);
    if (c->sam_text && (b0 != 0 || b1 != c->n_blocks || speculative_start)) return fail(c, "read_bam: shards of SAM text are not supported (%s)", SAM_SEQ_ONLY);
    c->wins.clear(); c->scan_end_uoff = ~0ull;
    c->shard_b0 = b0; c->shard_b1 = b1; c->shard_rank = speculative_start ? 1 : 0; c->shard_world = (b1 < c->n_blocks || speculative_start) ? 2 : 1;
    c->range_cut = b0 != 0 || c->shard_world != 1;
    c->scan_first_uoff = c->first_rec_uoff;
    return dhts_bam_rewind(c);
}

// ---- one file, several GPUs: every rank stages only its own byte window --------------------------------------------------------------
// Cut points: t_0 = 0, t_r = H + (size - H) * r / world for r >= 1 (H = bytes of the header blocks), so rank 0 always owns the header
// and the first records; a block belongs to the rank whose [t_r, t_r+1) holds its first byte -- the rule of dhts_shard_cut applied to
// file offsets.  Rank r > 0 finds the first block start at or behind t_r on the host (BGZF signature + three chained hops), and its
// resident bytes become  file[0, H) ++ file[start_r, t_r+1 + halo) : the header blocks (every rank needs the dictionaries) followed
// by its window and a halo in which the last record of the window completes.
#define DHTS_SHARD_HALO (4u << 20)
static uint64_t shard_target(uint64_t fsize, uint64_t hdr, int r, int world) {
    if (r <= 0) return 0;
    if (r >= world) return fsize;
    if (hdr > fsize) hdr = fsize;
    return hdr + (uint64_t)((__uint128_t)(fsize - hdr) * (unsigned)r / (unsigned)world);
}
static bool host_is_bgzf_header(const uint8_t *p) {
    return p[0] == 31 && p[1] == 139 && p[2] == 8 && (p[3] & 4) && p[10] == 6 && p[11] == 0 && p[12] == 'B' && p[13] == 'C' && p[14] == 2 && p[15] == 0;
}
// the byte window [wbeg, wend) of rank `rank` (host only: signature probe on the open file); t1 = where the rank's ownership ends
static void shard_window_fd(int fd, uint64_t fsize, uint64_t header_bytes, int rank, int world, uint64_t *wbeg_o, uint64_t *wend_o, uint64_t *t1_o) {
    if (header_bytes > fsize) header_bytes = fsize;
    const uint64_t t0 = shard_target(fsize, header_bytes, rank, world), t1 = shard_target(fsize, header_bytes, rank + 1, world);
    uint64_t wend = t1 + DHTS_SHARD_HALO; if (wend > fsize || rank == world - 1) wend = fsize;
    uint64_t wbeg = 0;
    if (rank > 0) {
        // first block start in [t0, ...): probe on the host
        wbeg = fsize;
        const size_t PROBE = 1u << 20;
        std::vector<uint8_t> buf(PROBE + 32);
        for (uint64_t base = t0; base < fsize && wbeg == fsize; base += PROBE - 65536 - 18) {
            const size_t want = (size_t)(fsize - base < PROBE ? fsize - base : PROBE);
            size_t got = 0;
            while (got < want) { ssize_t r = pread(fd, buf.data() + got, want - got, (off_t)(base + got)); if (r <= 0) break; got += (size_t)r; }
            if (got < 18) break;
            for (size_t q = 0; q + 18 <= got && q < PROBE - 65536 - 18; q++) {
                if (!host_is_bgzf_header(buf.data() + q)) continue;
                // three hops must land on headers (or exactly on the end of the file)
                size_t o = q; int hops = 0; bool ok = true;
                while (hops < 3) {
                    const size_t bl = ((size_t)buf[o + 16] | ((size_t)buf[o + 17] << 8)) + 1;
                    if (bl < 26) { ok = false; break; }
                    o += bl;
                    if (base + o == fsize) break;
                    if (o + 18 > got) { ok = (base + o < fsize) && hops >= 1; break; }      // ran out of probe bytes: accept after at least one verified hop
                    if (!host_is_bgzf_header(buf.data() + o)) { ok = false; break; }
                    hops++;
                }
                if (ok) { wbeg = base + q; break; }
            }
            if (got < want) break;
        }
        if (wbeg >= wend) wbeg = wend = fsize > 0 ? fsize : 0;          // no block starts in this rank's range: it scans nothing
    }
    *wbeg_o = wbeg; *wend_o = wend; *t1_o = t1;
}
// host-only view of the cut (no device needed): rank r stages file[win_begin, win_end) behind the header blocks and owns the blocks
// that start in [win_begin, own_end)
extern "C" int dhts_shard_window(const char *path, int rank, int world, uint64_t header_bytes, uint64_t *win_begin, uint64_t *win_end, uint64_t *own_end) {
    if (!path || world < 1 || rank < 0 || rank >= world) return -1;
    int fd = open(path, O_RDONLY);
    if (fd < 0) return -1;
    struct stat sb; if (fstat(fd, &sb) != 0) { close(fd); return -1; }
    uint64_t a = 0, b = 0, t1 = 0;
    shard_window_fd(fd, (uint64_t)sb.st_size, header_bytes, rank, world, &a, &b, &t1);
    close(fd);
    if (win_begin) *win_begin = a;
    if (win_end) *win_end = b;
    if (own_end) *own_end = t1;
    return 0;
}
int dhts_open_path_shard(dhts_ctx *c, const char *path, int rank, int world, uint64_t header_bytes) {
    if (!c || world < 1 || rank < 0 || rank >= world) return -1;
    discard_prefetch(c);
    int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(c, "cannot open %s", path);
    struct stat sb; if (fstat(fd, &sb) != 0) { close(fd); return fail(c, "cannot stat %s", path); }
    const uint64_t fsize = (uint64_t)sb.st_size;
    if (header_bytes > fsize) header_bytes = fsize;
    uint64_t wbeg = 0, wend = 0, t1_ = 0;
    shard_window_fd(fd, fsize, header_bytes, rank, world, &wbeg, &wend, &t1_);
    if (hipSetDevice(c->device) != hipSuccess) { close(fd); return fail(c, "hipSetDevice failed"); }
    reset_file_state(c);
    const uint64_t n_hdr = rank > 0 ? header_bytes : 0, n_win = wend > wbeg ? wend - wbeg : 0, n = n_hdr + n_win;
    if (c->comp.ensure(n + PAD_BYTES) != 0) { close(fd); return fail(c, "hipMalloc of %llu bytes failed", (unsigned long long)(n + PAD_BYTES)); }
    int rc = 0;
    if (n_hdr) rc = stage_file_range(c, fd, 0, n_hdr, (uint8_t *)c->comp.p);
    if (rc == 0 && n_win) rc = stage_file_range(c, fd, wbeg, n_win, (uint8_t *)c->comp.p + n_hdr);
    close(fd);
    if (rc) return fail(c, rc == -3 ? "read error on %s" : "staging %s failed", path);
    HIPCHK(c, hipMemsetAsync((uint8_t *)c->comp.p + n, 0, PAD_BYTES, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->comp_len = n; c->file_off = 0; c->file_size = fsize;
    c->seg_split = n_hdr; c->seg_file_off = rank > 0 ? wbeg : 0; c->partial_tail = wend < fsize; c->hdr_bytes_known = header_bytes;
    return 0;
}
// file offset of resident block i (the two-segment layout of dhts_open_path_shard; identity otherwise)
static uint64_t block_file_off(const dhts_ctx *c, int64_t i) {
    const uint64_t o = i < c->n_blocks ? c->h_coff[i] : c->comp_len;
    if (!c->segs.empty()) {
        size_t lo = 0, hi = c->segs.size();                   // last segment with res_off <= o
        while (hi - lo > 1) { const size_t mid = (lo + hi) / 2; if (c->segs[mid].res_off <= o) lo = mid; else hi = mid; }
        return o - c->segs[lo].res_off + c->segs[lo].file_off;
    }
    return (c->seg_split && o >= c->seg_split) ? o - c->seg_split + c->seg_file_off : o + c->file_off;
}
int dhts_bam_set_file_shard(dhts_ctx *c, int rank, int world) {
    if (!c || !c->bam_open || world < 1 || rank < 0 || rank >= world) return -1;
    if (c->fastq && world > 1) return fail(c, "read_bam: shards of FASTQ/FASTA text are not supported (%s)", FASTQ_SEQ_ONLY);
    if (c->sam_text && world > 1) return fail(c, "read_bam: shards of SAM text are not supported (%s)", SAM_SEQ_ONLY);
    const uint64_t t1 = shard_target(c->file_size, c->hdr_bytes_known, rank + 1, world);
    int64_t b0 = 0;
    if (rank > 0) { while (b0 < c->n_blocks && c->h_coff[b0] < c->seg_split) b0++; }      // behind the header blocks
    int64_t lo = b0, hi = c->n_blocks;
    if (rank == world - 1) lo = c->n_blocks;
    else while (lo < hi) { const int64_t mid = (lo + hi) / 2; if (block_file_off(c, mid) < t1) lo = mid + 1; else hi = mid; }
    return dhts_bam_set_block_range(c, b0, lo, rank > 0);
}
// compressed bytes of the blocks that hold the header: what every rank of a multi-GPU scan stages in front of its window
uint64_t dhts_bam_header_bytes(const dhts_ctx *c) {
    if (!c || !c->bam_open || c->n_blocks <= 0) return 0;
    if (c->fastq) { fail(const_cast<dhts_ctx *>(c), "read_bam: FASTQ/FASTA text has no header blocks to hand out (%s)", FASTQ_SEQ_ONLY); return 0; }
    if (c->sam_text) { fail(const_cast<dhts_ctx *>(c), "read_bam: the header blocks of SAM text are not handed out (%s)", SAM_SEQ_ONLY); return 0; }
    int64_t k = 0;
    while (k + 1 < c->n_blocks && c->h_uoff[k + 1] < c->first_rec_uoff) k++;
    return c->h_coff[k] + c->h_clen[k];
}
// BGZF virtual offset (file offset of the block << 16 | offset inside its inflated payload; htslib bgzf.h bgzf_tell) of a position of
// the inflated stream as this context numbers it: what adjacent ranks compare at a shard boundary (their uoff numbering differs)
uint64_t dhts_voffset(const dhts_ctx *c, uint64_t uoff) {
    if (!c || c->n_blocks <= 0) return 0;
    int64_t lo = 0, hi = c->n_blocks;                       // smallest i with h_uoff[i + 1] > uoff
    while (lo < hi) { const int64_t mid = (lo + hi) / 2; if (c->h_uoff[mid + 1] > uoff) hi = mid; else lo = mid + 1; }
    if (lo >= c->n_blocks) return block_file_off(c, c->n_blocks) << 16;
    return (block_file_off(c, lo) << 16) | (uoff - c->h_uoff[lo]);
}

int dhts_bam_set_shard(dhts_ctx *c, int rank, int world) {
    if (!c) return -1;
    BED_REFUSE(c, "a shard");
    if (c->fastq && world > 1) return fail(c, "read_bam: shards of FASTQ/FASTA text are not supported (%s)", FASTQ_SEQ_ONLY);
    if (c->sam_text && world > 1) return fail(c, "read_bam: shards of SAM text are not supported (%s)", SAM_SEQ_ONLY);
    int64_t b0, b1;
    if (dhts_shard_cut(c->h_coff.data(), c->n_blocks, c->comp_len, rank, world, &b0, &b1)) return -1;
    return dhts_bam_set_block_range(c, b0, b1, rank > 0);
}

// a scan that starts at the top of the file begins with the block that holds the first record (headers may span many blocks)
static void skip_header_blocks(dhts_ctx *c) {
    if (c->shard_rank != 0 || c->n_blocks <= 0) return;
    {   // a scan that starts at an index chunk starts in the chunk's block: the table may misplace the offset while that block's ISIZE is
        // unchecked (a block that understates its length would be passed over, and never decoded)
        int64_t anchor = -1;
        if (!c->wins.empty() && c->win_cur < c->wins.size() && c->wins[c->win_cur].first_uoff == c->scan_first_uoff) anchor = c->wins[c->win_cur].first_blk;
        else if (c->wins.empty() && c->scan_first_blk >= 0 && c->scan_first_uoff == c->scan_first_anchor) anchor = c->scan_first_blk;
        if (anchor >= c->shard_b0 && anchor < c->shard_b1) { c->next_block = anchor; return; }
    }
    // the first block that ends behind scan_first_uoff; blocks that declare no bytes (ISIZE 0) at that position are not skipped: a damaged
    // ISIZE of 0 on the block that holds the first record has to be seen by the inflate stage (round-2 soak, seed 2001161)
    int64_t lo = 0, hi = c->n_blocks;
    while (lo < hi) { int64_t mid = (lo + hi) / 2; if (c->h_uoff[mid + 1] > c->scan_first_uoff) hi = mid; else lo = mid + 1; }
    while (lo > 0 && c->h_uoff[lo - 1] >= c->scan_first_uoff && c->h_isize[lo - 1] == 0) lo--;
    if (lo >= c->n_blocks) { lo = c->n_blocks - 1; while (lo > 0 && c->h_uoff[lo] >= c->scan_first_uoff && c->h_uoff[lo - 1] >= c->scan_first_uoff) lo--; }
    if (lo >= c->shard_b0 && lo < c->shard_b1) c->next_block = lo;
}
