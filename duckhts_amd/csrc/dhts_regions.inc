// dhts_regions.inc -- part of dhts_api.hip (included there, inside its extern "C" block; not a translation unit of its own):
// region strings -> merged intervals; BAI / CSI / TBI readers -> disjoint scan windows and staging segments.
// ---- region queries (SURVEY row A11): host side = region strings -> merged intervals, BAI -> scan window -------------------
// hts_parse_decimal with HTS_PARSE_THOUSANDS_SEP (htslib hts.c:3884-3940)
static long long parse_decimal_sep(const char *str, const char **strend) {
    unsigned long long n = 0; int digits = 0, decimals = 0, e = 0; char sign = '+', esign = '+';
    const char *s = str;
    while (*s == ' ' || (*s >= '\t' && *s <= '\r')) s++;
    if (*s == '+' || *s == '-') sign = *s++;
    while (*s) { if (*s >= '0' && *s <= '9') { digits++; n = n * 10 + (unsigned)(*s++ - '0'); } else if (*s == ',') s++; else break; }
    if (*s == '.') { s++; while (*s >= '0' && *s <= '9') { decimals++; digits++; n = n * 10 + (unsigned)(*s++ - '0'); } }
    switch (*s) {
    case 'e': case 'E': s++; if (*s == '+' || *s == '-') esign = *s++; while (*s >= '0' && *s <= '9') e = e * 10 + (*s++ - '0'); if (esign == '-') e = -e; break;
    case 'k': case 'K': e += 3; s++; break;
    case 'm': case 'M': e += 6; s++; break;
    case 'g': case 'G': e += 9; s++; break;
    }
    e -= decimals;
    while (e > 0) { n *= 10; e--; }
    while (e < 0) { n /= 10; e++; }
    *strend = digits > 0 ? s : str;
    return sign == '+' ? (long long)n : -(long long)n;
}

// hts_parse_region (hts.c:3995-4150) for one region token; name lookup through `names`.  Returns false when the token does not
// name a known reference / is malformed (hts_reglist_create then skips it with a warning, region.c:203-215).
static bool parse_region_token_fn(const std::function<int(const std::string &)> &getid, const std::string &tok, int &tid, int64_t &beg, int64_t &end);
static bool parse_region_token(const std::vector<std::string> &names, const std::string &tok, int &tid, int64_t &beg, int64_t &end) {
    return parse_region_token_fn([&](const std::string &nm) -> int { for (size_t i = 0; i < names.size(); i++) if (names[i] == nm) return (int)i; return -1; }, tok, tid, beg, end);
}
// the same with the name lookup handed in (the .fai of read_fasta keeps a map: dhts_fasta_index.inc)
static bool parse_region_token_fn(const std::function<int(const std::string &)> &getid, const std::string &tok, int &tid, int64_t &beg, int64_t &end) {
    const int64_t POS_MAX = ((((int64_t)INT32_MAX) << 32) | 0xffffffffll);       // HTS_POS_MAX = INT64_MAX in htslib >= 1.10
    (void)POS_MAX;
    const int64_t PMAX = INT64_MAX;
    std::string s = tok; bool quoted = false; size_t colon = std::string::npos;
    if (!s.empty() && s[0] == '{') {
        size_t close = s.find('}');
        if (close == std::string::npos) return false;
        std::string name = s.substr(1, close - 1);
        quoted = true;
        if (close + 1 < s.size() && s[close + 1] == ':') colon = close + 1;
        if (colon == std::string::npos) { beg = 0; end = PMAX; tid = getid(name); return tid >= 0; }
        tid = getid(name);
        if (tid < 0) return false;
    } else {
        colon = s.rfind(':');
        if (colon == std::string::npos) { beg = 0; end = PMAX; tid = getid(s); return tid >= 0; }
        beg = 0; end = PMAX;
        if ((tid = getid(s)) >= 0) return getid(s.substr(0, colon)) < 0;       // whole string is a name; ambiguous if the prefix is one too
        tid = getid(s.substr(0, colon));
        if (tid < 0) return false;
    }
    (void)quoted;
    const char *c1 = s.c_str() + colon + 1, *hy = nullptr;
    beg = parse_decimal_sep(c1, &hy) - 1;
    if (beg < 0) {
        if (beg != -1 && *hy == '-' && *c1 != '\0') return false;               // "Coordinates must be > 0"
        if ((*hy >= '0' && *hy <= '9') || *hy == '\0' || *hy == ',') { end = beg == -1 ? PMAX : -(beg + 1); beg = 0; return true; }   // chr:-100 = chr:1-100
        else if (beg < -1) return false;
    }
    if (*hy == '\0') end = PMAX;
    else if (*hy == '-') { const char *h2; end = parse_decimal_sep(hy + 1, &h2); if (*h2 != '\0' && *h2 != ',') return false; }
    else return false;
    if (end == 0) end = PMAX;
    if (beg >= end) return false;
    return true;
}

// read_bam(region := ...): comma split as src/bam_reader.c:318-348 (strtok: empty tokens vanish), then hts_reglist_create
// (region.c:177-260: "." = everything, "*" = unplaced reads, unknown names skipped, intervals sorted and merged per tid).
// Returns 0, or 1 when no usable region remains (the reference reports "No reads found for region(s): ...").
int dhts_bam_set_regions(dhts_ctx *c, const char *regions) {
    if (!c || !c->bam_open) return -1;
    if (c->fastq && regions && regions[0]) return fail(c, "read_bam: region queries on FASTQ/FASTA text are not supported (%s)", FASTQ_SEQ_ONLY);
    if (c->sam_text && regions && regions[0]) return fail(c, "read_bam: region queries on SAM text are not supported (%s; the reference needs a .tbi / .csi index for them)", SAM_SEQ_ONLY);
    HIPCHK(c, hipSetDevice(c->device));
    c->rg_active = false; c->rg_all = false; c->rg_nocoor = false; c->rg_empty_window = false; c->rg_beg.clear(); c->rg_end.clear(); c->rg_tid_first.clear(); c->rg_given.clear();
    c->wins.clear(); c->win_cur = 0; c->scan_end_uoff = ~0ull;
    c->scan_first_uoff = c->first_rec_uoff; c->shard_b0 = 0; c->shard_b1 = c->n_blocks; c->shard_rank = 0; c->shard_world = 1; c->range_cut = false;
    if (!regions || !*regions) return dhts_bam_rewind(c);
    const size_t n_ref = c->ref_name.size();
    std::vector<std::vector<std::pair<int64_t, int64_t>>> per(n_ref);
    int usable = 0, ntok = 0;
    std::string all(regions); size_t p = 0;
    while (p <= all.size()) {
        size_t q = all.find(',', p); if (q == std::string::npos) q = all.size();
        std::string tok = all.substr(p, q - p); p = q + 1;
        if (tok.empty()) continue;
        ntok++;
        if (tok == ".") { c->rg_all = true; usable++; continue; }
        if (tok == "*") { c->rg_nocoor = true; usable++; continue; }
        int tid; int64_t b, e;
        if (!parse_region_token(c->ref_name, tok, tid, b, e)) continue;
        per[tid].push_back({b, e}); usable++;
        c->rg_given.push_back({(int32_t)tid, b, e, tok});
    }
    if (ntok == 0) return dhts_bam_rewind(c);               // a string of commas only: the reference's strtok split yields no region at all (bam_reader.c:319-345) => plain scan
    if (!usable) return 1;
    c->rg_tid_first.assign(n_ref + 1, 0);
    for (size_t t = 0; t < n_ref; t++) {
        auto &v = per[t];
        std::sort(v.begin(), v.end());
        c->rg_tid_first[t] = (uint32_t)c->rg_beg.size();
        for (size_t j = 0; j < v.size(); j++) {
            if (!c->rg_beg.empty() && c->rg_beg.size() > c->rg_tid_first[t] && !(c->rg_end.back() < v[j].first)) { if (c->rg_end.back() < v[j].second) c->rg_end.back() = v[j].second; }
            else { c->rg_beg.push_back(v[j].first); c->rg_end.push_back(v[j].second); }
        }
    }
    c->rg_tid_first[n_ref] = (uint32_t)c->rg_beg.size();
    ENSURE(c, c->d_rg_beg, c->rg_beg.size() * 8 + 16); ENSURE(c, c->d_rg_end, c->rg_end.size() * 8 + 16); ENSURE(c, c->d_rg_first, (n_ref + 1) * 4 + 16);
    if (!c->rg_beg.empty()) { HIPCHK(c, hipMemcpy(c->d_rg_beg.p, c->rg_beg.data(), c->rg_beg.size() * 8, hipMemcpyHostToDevice)); HIPCHK(c, hipMemcpy(c->d_rg_end.p, c->rg_end.data(), c->rg_end.size() * 8, hipMemcpyHostToDevice)); }
    HIPCHK(c, hipMemcpy(c->d_rg_first.p, c->rg_tid_first.data(), (n_ref + 1) * 4, hipMemcpyHostToDevice));
    c->rg_active = true;
    return dhts_bam_rewind(c);
}

// ---- index -> scan window ----------------------------------------------------------------------------------------------------
// BAI (SAM spec 5.2) and CSI (CSIv1; BGZF-compressed, inflated here on the GPU through a scratch context) as loaded by
// hts_idx_load (htslib hts.c:2920-3055).  For a set of query intervals the window is [smallest chunk start, largest chunk end] over
// the bins the intervals touch (reg2bins hts.c:3142-3213, generalised to min_shift / depth), pruned by the BAI linear index
// (hts.c:3556-3563).  It is a superset of the iterator's chunk list; the device predicate decides the rows, so results are exact.
struct QIv { int32_t tid; int64_t beg, end; };
struct IdxWindow { bool any = false; uint64_t vmin = ~0ull, vmax = 0, last_end = 0; std::vector<std::pair<uint64_t, uint64_t>> chunks; };   // chunks: (begin, end) virtual offsets of every bin chunk the query touches

// the index bytes as stored in memory: a BGZF file (.csi, .tbi) is inflated on the device through a scratch context
static int index_plain(dhts_ctx *c, const uint8_t *&d, uint64_t &n, std::vector<uint8_t> &inflated) {
    if (n >= 18 && d[0] == 0x1f && d[1] == 0x8b) {
        // the same index comes back for every region of a query (and twice per region on text: names, then windows): inflate it once per
        // context.  Identity = address, length and the bytes at both ends.
        uint8_t key[128]; const uint64_t kn = n < 64 ? n : 64;
        memset(key, 0, sizeof(key)); memcpy(key, d, kn); memcpy(key + 64, d + n - kn, kn);
        if (c->idx_cache_src == d && c->idx_cache_n == n && memcmp(c->idx_cache_key, key, 128) == 0 && !c->idx_cache.empty()) { d = c->idx_cache.data(); n = c->idx_cache_len; return 0; }
        const uint8_t *src0 = d; const uint64_t n0 = n;
        dhts_ctx *t = dhts_create(c->device);
        if (!t) return fail(c, "cannot create a scratch context for the index");
        int64_t nb = -1;
        if (dhts_open_host(t, d, n) == 0) nb = dhts_bgzf_index(t);
        if (nb <= 0) { dhts_destroy(t); return fail(c, "index is not readable BGZF"); }
        if (huff_ensure(t, 0, nb, nb)) { dhts_destroy(t); return fail(c, "index inflate failed"); }
        uint64_t tot = t->h_uoff[nb];
        inflated.resize(tot + 16);
        std::vector<int32_t> bs(nb);
        int64_t got = dhts_bgzf_inflate_to_host(t, 0, nb, inflated.data(), tot, bs.data());
        if (got < 0 && t->h_uoff[nb] != tot) {                // a scratch retry inside moved the block table: once more with its sizes
            tot = t->h_uoff[nb]; inflated.resize(tot + 16);
            got = dhts_bgzf_inflate_to_host(t, 0, nb, inflated.data(), tot, bs.data());
        }
        dhts_destroy(t);
        HIPCHK(c, hipSetDevice(c->device));
        if (got < 0) return fail(c, "index inflate failed");
        tot = (uint64_t)got;                                  // (the table may have shrunk behind a scratch retry)
        for (int64_t k = 0; k < nb; k++) if (bs[k] != 0) return fail(c, "index inflate failed (block %lld)", (long long)k);
        c->idx_cache.swap(inflated); c->idx_cache_len = tot; c->idx_cache_src = src0; c->idx_cache_n = n0; memcpy(c->idx_cache_key, key, 128);
        d = c->idx_cache.data(); n = tot;
    }
    return 0;
}
// the tabix header of an index (TBI: behind n_ref; CSI: the aux block), tbx.c:552-597: preset + the sequence names in index order.
// Returns 0, 1 when the index carries no tabix header, <0 on a malformed one.
static int tabix_header(dhts_ctx *c, const uint8_t *d, uint64_t n, int32_t &preset, std::vector<std::string> &names) {
    const uint8_t *m = nullptr; uint64_t lm = 0;
    if (n >= 8 && memcmp(d, "TBI\1", 4) == 0) { m = d + 8; lm = n - 8; }
    else if (n >= 16 && memcmp(d, "CSI\1", 4) == 0) { lm = hle32(d + 12); if (lm > n - 16) return fail(c, "bad CSI header"); m = d + 16; }
    else return 1;
    if (lm < 28) return 1;
    preset = (int32_t)hle32(m);
    const uint32_t l_nm = hle32(m + 24);
    if (l_nm > lm - 28) return fail(c, "Invalid index header");
    names.clear();
    for (uint32_t p = 0; p < l_nm;) { uint32_t e = p; while (e < l_nm && m[28 + e]) e++; names.emplace_back((const char *)m + 28 + p, e - p); p = e + 1; }
    return 0;
}

static int index_window(dhts_ctx *c, const uint8_t *d, uint64_t n, const std::vector<QIv> &q, bool whole, IdxWindow &w) {
    std::vector<uint8_t> inflated;
    if (index_plain(c, d, n, inflated)) return -1;
    uint64_t p = 0;
    auto need = [&](uint64_t k) { return p + k <= n; };
    auto hle64 = [&](const uint8_t *x) { return (uint64_t)hle32(x) | ((uint64_t)hle32(x + 4) << 32); };
    int min_shift = 14, depth = 5; bool csi = false; bool tbi = false;
    if (need(8) && memcmp(d, "BAI\1", 4) == 0) p = 4;
    else if (need(36) && memcmp(d, "TBI\1", 4) == 0) { p = 4; tbi = true; }         // BAI's body behind n_ref + the tabix header
    else if (need(16) && memcmp(d, "CSI\1", 4) == 0) {
        csi = true; min_shift = (int32_t)hle32(d + 4); depth = (int32_t)hle32(d + 8); const uint32_t l_aux = hle32(d + 12); p = 16;
        if (min_shift < 0 || depth < 0 || depth > 10 || !need(l_aux)) return fail(c, "bad CSI header");
        p += l_aux;
    } else return fail(c, "index is neither BAI nor CSI");
    if (!need(4)) return fail(c, "truncated index");
    const int32_t n_ref = (int32_t)hle32(d + p); p += 4;
    if (tbi) { const uint64_t l_nm = hle32(d + p + 24); if (!need(28 + l_nm)) return fail(c, "truncated index"); p += 28 + l_nm; }
    const uint32_t meta_bin = (uint32_t)(((1ull << (depth * 3 + 3)) - 1) / 7 + 1);
    const int maxs = min_shift + 3 * depth;
    for (int32_t t = 0; t < n_ref; t++) {
        if (!need(4)) return fail(c, "truncated index");
        const int32_t n_bin = (int32_t)hle32(d + p); p += 4;
        std::vector<std::pair<uint32_t, uint32_t>> binr; int64_t first_beg = -1;
        for (auto &iv : q) if (iv.tid == t) {
            int64_t b = iv.beg < 0 ? 0 : iv.beg, e = iv.end; if (e > (1ll << maxs)) e = 1ll << maxs; if (b >= e) continue; --e;
            if (first_beg < 0 || b < first_beg) first_beg = b;
            uint32_t tt = 0;
            for (int l = 0, sft = maxs; l <= depth; l++, sft -= 3) { binr.push_back({(uint32_t)(tt + (b >> sft)), (uint32_t)(tt + (e >> sft))}); tt += 1u << (l * 3); }
        }
        struct Ch { uint64_t u, v; };
        std::vector<Ch> chunks;
        for (int32_t bi = 0; bi < n_bin; bi++) {
            if (!need(csi ? 16 : 8)) return fail(c, "truncated index");
            const uint32_t bin = hle32(d + p); p += 4;
            if (csi) p += 8;                                             // loffset: not needed for a superset window
            const int32_t n_chunk = (int32_t)hle32(d + p); p += 4;
            if (n_chunk < 0 || !need((uint64_t)n_chunk * 16)) return fail(c, "truncated index");
            for (int32_t k = 0; k < n_chunk; k++) {
                const uint64_t u = hle64(d + p), v = hle64(d + p + 8); p += 16;
                if (bin == meta_bin) { if (k == 0 && v > w.last_end) w.last_end = v; continue; }   // pseudo-bin: (ref_beg, ref_end), (n_mapped, n_unmapped)
                if (v > w.last_end) w.last_end = v;
                bool hit = whole;
                for (auto &r : binr) if (bin >= r.first && bin <= r.second) { hit = true; break; }
                if (hit) chunks.push_back({u, v});
            }
        }
        uint64_t min_off = 0;
        if (!csi) {
            if (!need(4)) return fail(c, "truncated index");
            const int32_t n_intv = (int32_t)hle32(d + p); p += 4;
            if (n_intv < 0 || !need((uint64_t)n_intv * 8)) return fail(c, "truncated index");
            if (first_beg >= 0 && n_intv > 0) { int64_t wdw = first_beg >> 14; if (wdw >= n_intv) wdw = n_intv - 1; min_off = hle64(d + p + (uint64_t)wdw * 8); }
            p += (uint64_t)n_intv * 8;
        }
        for (auto &ch : chunks) {
            if (ch.v <= min_off) continue;
            w.any = true;
            if (ch.u < w.vmin) w.vmin = ch.u;
            if (ch.v > w.vmax) w.vmax = ch.v;
            w.chunks.push_back({ch.u > min_off ? ch.u : min_off, ch.v});      // (the linear index: nothing below min_off can overlap, hts.c:3540-3560)
        }
    }
    return 0;
}

// Disjoint windows of a query: the chunks sorted by their start, neighbours merged while the gap between them is cheaper to scan than a
// window is to start (a window costs a batch: ~1.5 ms of launches and hand-shakes, i.e. tens of MB at scan speed).  Rows are decided by
// the overlap predicate, so merging never changes the result; the windows only bound what is staged and inflated.  !multi: one
// covering window [vmin, vmax].
static std::vector<std::pair<uint64_t, uint64_t>> merged_windows(const IdxWindow &w, bool multi) {
    std::vector<std::pair<uint64_t, uint64_t>> mg;
    if (!w.any) return mg;
    if (!multi || w.chunks.size() <= 1) { mg.push_back({w.vmin, w.vmax}); return mg; }
    const uint64_t gap_bytes = (uint64_t)(getenv("DHTS_WINDOW_GAP_MB") ? atof(getenv("DHTS_WINDOW_GAP_MB")) : 32.0) * (1u << 20);
    std::vector<std::pair<uint64_t, uint64_t>> ch = w.chunks;
    std::sort(ch.begin(), ch.end());
    for (auto &x : ch) {
        if (!mg.empty() && (x.first >> 16) <= (mg.back().second >> 16) + gap_bytes) { if (x.second > mg.back().second) mg.back().second = x.second; }
        else mg.push_back(x);
    }
    if (mg.size() == 1) { mg[0] = {w.vmin, w.vmax}; }
    return mg;
}

// The byte ranges of the file a region query needs, from a context that holds only the header (bam_open done) with the regions set:
// beg[k] = file offset of the window's first BGZF block, end[k] = file offset of its LAST block (the opener adds that block's length),
// ~0 = up to the end of the file (the "*" region).  *count = -1: the query needs the whole file.  Same windows as dhts_bam_load_index
// builds afterwards on the context that holds the staged ranges.
extern "C" int dhts_bam_region_segments(dhts_ctx *c, const void *index_bytes, uint64_t n, uint64_t *beg, uint64_t *end, int64_t cap, int64_t *count) {
    if (!c || !c->bam_open || !count) return -1;
    if (c->fastq) return fail(c, "read_bam: region segments of FASTQ/FASTA text are not supported (%s)", FASTQ_SEQ_ONLY);
    if (c->sam_text) return fail(c, "read_bam: region segments of SAM text are not supported (%s)", SAM_SEQ_ONLY);
    std::vector<QIv> q;
    if (c->rg_active) for (size_t t = 0; t + 1 < c->rg_tid_first.size(); t++) for (uint32_t k = c->rg_tid_first[t]; k < c->rg_tid_first[t + 1]; k++) q.push_back({(int32_t)t, c->rg_beg[k], c->rg_end[k]});
    const bool whole = !c->rg_active || c->rg_all;
    if (whole) { *count = -1; return 0; }
    IdxWindow w;
    if (index_window(c, (const uint8_t *)index_bytes, n, q, whole, w)) return -1;
    std::vector<std::pair<uint64_t, uint64_t>> sg;
    if (c->rg_nocoor) { const uint64_t s0 = w.any ? w.vmin : w.last_end; sg.push_back({s0 >> 16, ~0ull}); }
    else for (auto &x : merged_windows(w, true)) sg.push_back({x.first >> 16, x.second >> 16});
    *count = (int64_t)sg.size();
    if ((int64_t)sg.size() > cap) return fail(c, "room for %lld segments, the query has %lld", (long long)cap, (long long)sg.size());
    for (size_t k = 0; k < sg.size(); k++) { beg[k] = sg[k].first; end[k] = sg[k].second; }
    return 0;
}

// turns a window into the context's scan range; nocoor = also everything after the last mapped chunk ("*")
static int apply_window(dhts_ctx *c, const IdxWindow &w, bool whole, bool nocoor, bool multi = false) {
    int64_t b0 = 0, b1 = c->n_blocks; uint64_t first_uoff = c->first_rec_uoff;
    auto block_of = [&](uint64_t coffset) -> int64_t {          // first resident block at or behind FILE offset coffset
        int64_t lo = 0, hi = c->n_blocks;
        while (lo < hi) { int64_t mid = (lo + hi) / 2; if (block_file_off(c, mid) < coffset) lo = mid + 1; else hi = mid; }
        return lo;
    };
    const bool sparse = !c->segs.empty();                       // only the windows are resident: every window is cut exactly at its end
    c->rg_empty_window = false;
    c->wins.clear(); c->win_cur = 0; c->scan_end_uoff = ~0ull;
    if (!whole && !nocoor) {
        if (!w.any) { c->rg_empty_window = true; return 0; }
        const bool windows = (multi && w.chunks.size() > 1) || sparse;
        if (!windows || merged_windows(w, multi).size() <= 1) {      // (the covering window starts at the smallest chunk start, which the linear index may have pruned from a list of windows)
            b0 = block_of(w.vmin >> 16); b1 = block_of(w.vmax >> 16) + 1; if (b1 > c->n_blocks) b1 = c->n_blocks;
            if (b0 >= c->n_blocks || block_file_off(c, b0) != (w.vmin >> 16)) return fail(c, "index does not match the file (chunk offset %llu)", (unsigned long long)(w.vmin >> 16));
            first_uoff = c->h_uoff[b0] + (w.vmin & 0xffff);
            if (first_uoff < c->first_rec_uoff) first_uoff = c->first_rec_uoff;
        }
        if (windows) {
            // Disjoint windows: the chunks sorted by their start, neighbours merged while the gap between them is cheaper to scan than a
            // window is to start (a window costs a batch: ~1.5 ms of launches and hand-shakes, i.e. tens of MB at scan speed).  Rows are
            // decided by the overlap predicate, so merging never changes the result; the windows only bound what is inflated.
            std::vector<std::pair<uint64_t, uint64_t>> mg = merged_windows(w, multi);
            if (mg.size() > 1 || sparse) {
                for (auto &x : mg) {
                    dhts_ctx::ScanWin sw;
                    sw.b0 = block_of(x.first >> 16);
                    if (sw.b0 >= c->n_blocks || block_file_off(c, sw.b0) != (x.first >> 16)) return fail(c, "index does not match the file (chunk offset %llu)", (unsigned long long)(x.first >> 16));
                    int64_t be = block_of(x.second >> 16); if (be >= c->n_blocks) be = c->n_blocks - 1;
                    sw.b1 = be + 1;
                    sw.first_uoff = c->h_uoff[sw.b0] + (x.first & 0xffff); sw.first_blk = sw.b0;
                    if (sw.first_uoff < c->first_rec_uoff) { sw.first_uoff = c->first_rec_uoff; sw.first_blk = -1; }
                    const bool in_be = block_file_off(c, be) == (x.second >> 16);
                    sw.end_uoff = in_be ? c->h_uoff[be] + (x.second & 0xffff) : c->h_uoff[be + 1];
                    sw.end_blk = in_be ? be : be + 1;
                    c->wins.push_back(sw);
                }
                b0 = c->wins[0].b0; b1 = c->wins[0].b1; first_uoff = c->wins[0].first_uoff; c->scan_end_uoff = c->wins[0].end_uoff;
            }
        }
    } else if (!whole && nocoor) {
        const uint64_t s0 = w.any ? w.vmin : w.last_end;
        b0 = block_of(s0 >> 16); if (b0 >= c->n_blocks) b0 = c->n_blocks > 0 ? c->n_blocks - 1 : 0;
        if (c->n_blocks > 0 && block_file_off(c, b0) == (s0 >> 16)) first_uoff = c->h_uoff[b0] + (s0 & 0xffff);
        else if (sparse) return fail(c, "index does not match the file (chunk offset %llu)", (unsigned long long)(s0 >> 16));
        else { b0 = 0; first_uoff = c->first_rec_uoff; }
        if (first_uoff < c->first_rec_uoff) first_uoff = c->first_rec_uoff;
    }
    c->shard_b0 = b0; c->shard_b1 = b1; c->shard_rank = 0; c->shard_world = (b1 < c->n_blocks) ? 2 : 1; c->scan_first_uoff = first_uoff;
    // (an index chunk start is an offset inside block b0 -- unless it lay in the header and the first record took its place)
    c->scan_first_blk = (whole || first_uoff == c->first_rec_uoff || first_uoff < c->h_uoff[b0]) ? -1 : b0; c->scan_first_anchor = first_uoff;
    return 0;
}

// how much of the file the current scan range covers: windows (1 without an index) and BGZF blocks
int dhts_scan_window_stats(const dhts_ctx *c, int64_t *n_windows, int64_t *n_blocks) {
    if (!c) return -1;
    int64_t w = 1, b = c->shard_b1 - c->shard_b0;
    if (!c->wins.empty()) { w = (int64_t)c->wins.size(); b = 0; for (auto &x : c->wins) b += x.b1 - x.b0; }
    if (c->rg_empty_window) { w = 0; b = 0; }
    if (n_windows) *n_windows = w;
    if (n_blocks) *n_blocks = b;
    return 0;
}
int dhts_bam_load_index(dhts_ctx *c, const void *bytes, uint64_t n) {
    if (!c || !c->bam_open) return -1;
    if (c->fastq) return fail(c, "read_bam: an index on FASTQ/FASTA text is not supported (%s)", FASTQ_SEQ_ONLY);
    if (c->sam_text) return fail(c, "read_bam: an index on SAM text is not supported (%s)", SAM_SEQ_ONLY);
    std::vector<QIv> q;
    if (c->rg_active) for (size_t t = 0; t + 1 < c->rg_tid_first.size(); t++) for (uint32_t k = c->rg_tid_first[t]; k < c->rg_tid_first[t + 1]; k++) q.push_back({(int32_t)t, c->rg_beg[k], c->rg_end[k]});
    const bool whole = !c->rg_active || c->rg_all;
    IdxWindow w;
    if (index_window(c, (const uint8_t *)bytes, n, q, whole, w)) return -1;
    if (apply_window(c, w, whole, c->rg_nocoor, true)) return -1;
    return dhts_bam_rewind(c);
}

static int bcf_upload_dicts(dhts_ctx *c);
// VCF text (tbx_index_load3 + vcf_hdr_read's "add the missing contigs", vcf.c:2649-2668; tbx_itr_querys): the index names its sequences
// itself.  Returns 1 when the pending region names none of them (no iterator: the reference skips the region).
static int bcf_text_index(dhts_ctx *c, const uint8_t *d, uint64_t n) {
    std::vector<uint8_t> inflated;
    if (index_plain(c, d, n, inflated)) return -1;
    int32_t preset = 0; std::vector<std::string> names;
    const int rc = tabix_header(c, d, n, preset, names);
    if (rc < 0) return -1;
    if (rc == 1) return fail(c, "read_bcf: the index of a VCF text file has no tabix header");
    if ((preset & 0xffff) != 2) return fail(c, "read_bcf: the tabix index was not built with the VCF preset");
    bool added = false;
    for (auto &nm : names) {
        bool have = false;
        for (size_t i = 0; i < c->bh.ctg.size() && !have; i++) have = c->bh.ctg_present[i] && c->bh.ctg[i] == nm;
        if (have) continue;
        if (nm.find('\n') != std::string::npos || !dhts::bcf_header_add_line(c->bh, ("##contig=<ID=" + nm + ">").c_str())) return fail(c, "read_bcf: cannot add contig '%s' of the index to the header", nm.c_str());
        added = true;
    }
    if (added && bcf_upload_dicts(c)) return -1;
    c->tbx_names = names;
    if (c->bcf_rg_pending) {
        int tid; int64_t b, e;
        if (!parse_region_token(names, c->bcf_rg_tok, tid, b, e)) { c->bcf_rg_pending = false; c->bcf_rg_active = false; c->rg_empty_window = true; (void)dhts_bcf_rewind(c); return 1; }
        int32_t rid = -1;
        for (size_t i = 0; i < c->bh.ctg.size(); i++) if (c->bh.ctg_present[i] && c->bh.ctg[i] == names[tid]) { rid = (int32_t)i; break; }
        if (rid < 0) return fail(c, "internal: index sequence without a header id");
        c->bcf_rg_pending = false; c->bcf_rg_itid = tid; c->bcf_rg_tid = rid; c->bcf_rg_beg = b; c->bcf_rg_end = e;
    }
    return 0;
}

int dhts_bcf_load_index(dhts_ctx *c, const void *bytes, uint64_t n) {
    if (!c || !c->bcf_open) return -1;
    if (c->vcf_text) {
        if (c->plain_text) return fail(c, "read_bcf: an uncompressed VCF has no index");
        const int rc = bcf_text_index(c, (const uint8_t *)bytes, n);
        if (rc) return rc;
    }
    std::vector<QIv> q;
    const bool whole = !c->bcf_rg_active || c->bcf_rg_all;
    if (!whole) q.push_back({c->vcf_text ? c->bcf_rg_itid : c->bcf_rg_tid, c->bcf_rg_beg, c->bcf_rg_end});
    IdxWindow w;
    if (index_window(c, (const uint8_t *)bytes, n, q, whole, w)) return -1;
    if (apply_window(c, w, whole, false, true)) return -1;         // disjoint windows, each cut exactly at its end (as for read_bam)
    return dhts_bcf_rewind(c);
}

// compressed bytes of the blocks that hold the header of the open BCF / VCF: what a region query stages in front of its index windows
extern "C" uint64_t dhts_bcf_header_bytes(const dhts_ctx *c) {
    if (!c || !c->bcf_open || c->n_blocks <= 0 || c->plain_text) return 0;
    int64_t k = 0;
    while (k + 1 < c->n_blocks && c->h_uoff[k + 1] < c->first_rec_uoff) k++;
    return c->h_coff[k] + c->h_clen[k];
}
// The byte ranges of the file the regions of read_bcf(region := 'a,b,...') need, from a context that holds the header (dhts_bcf_open done;
// the bind context of the table function): the union of every region's index windows, as dhts_bam_region_segments returns them.
// *count = -1: the query needs the whole file (a "." region, or no usable index).  Regions the index does not know contribute nothing.
extern "C" int dhts_bcf_region_segments(dhts_ctx *c, const char *regions, const void *index_bytes, uint64_t n, uint64_t *beg, uint64_t *end, int64_t cap, int64_t *count) {
    if (!c || !c->bcf_open || !count || !regions) return -1;
    *count = -1;
    if (c->plain_text) return 0;
    IdxWindow all; bool whole = false;
    std::string csv(regions); size_t p = 0;
    while (p <= csv.size() && !whole) {
        size_t q = csv.find(',', p); if (q == std::string::npos) q = csv.size();
        const std::string tok = csv.substr(p, q - p); p = q + 1;
        if (tok.empty()) continue;
        if (dhts_bcf_set_region(c, tok.c_str()) != 0) continue;                 // unknown contig: skipped by the scan as well
        if (c->bcf_rg_all) { whole = true; break; }
        if (c->vcf_text) { const int rc = bcf_text_index(c, (const uint8_t *)index_bytes, n); if (rc == 1) continue; if (rc < 0) return -1; }
        std::vector<QIv> qv; qv.push_back({c->vcf_text ? c->bcf_rg_itid : c->bcf_rg_tid, c->bcf_rg_beg, c->bcf_rg_end});
        IdxWindow w;
        if (index_window(c, (const uint8_t *)index_bytes, n, qv, false, w)) return -1;
        if (!w.any) continue;
        all.any = true;
        for (auto &x : merged_windows(w, true)) all.chunks.push_back(x);         // exactly the windows dhts_bcf_load_index will ask for
    }
    (void)dhts_bcf_set_region(c, nullptr);
    if (whole) return 0;
    std::vector<std::pair<uint64_t, uint64_t>> sg;
    if (all.any) {
        // (the union of the regions' windows: they may overlap; sorted and merged like one region's chunks)
        std::sort(all.chunks.begin(), all.chunks.end());
        std::vector<std::pair<uint64_t, uint64_t>> mg;
        const uint64_t gap_bytes = (uint64_t)(getenv("DHTS_WINDOW_GAP_MB") ? atof(getenv("DHTS_WINDOW_GAP_MB")) : 32.0) * (1u << 20);
        for (auto &x : all.chunks) {
            if (!mg.empty() && (x.first >> 16) <= (mg.back().second >> 16) + gap_bytes) { if (x.second > mg.back().second) mg.back().second = x.second; }
            else mg.push_back(x);
        }
        for (auto &x : mg) sg.push_back({x.first >> 16, x.second >> 16});
    }
    *count = (int64_t)sg.size();
    if ((int64_t)sg.size() > cap) { *count = -1; return 0; }                     // too many ranges for the caller's room: the whole file
    for (size_t k = 0; k < sg.size(); k++) { beg[k] = sg[k].first; end[k] = sg[k].second; }
    return 0;
}

// the scan range becomes window k of a multi-window region query
static void enter_window(dhts_ctx *c, size_t k) {
    const dhts_ctx::ScanWin &w = c->wins[k];
    c->win_cur = k; c->shard_b0 = w.b0; c->shard_b1 = w.b1; c->shard_rank = 0; c->shard_world = (w.b1 < c->n_blocks) ? 2 : 1;
    c->scan_first_uoff = w.first_uoff; c->scan_end_uoff = w.end_uoff;
}
// a batch ended its index window (status 1) and another window follows: the scan moves on to it and goes on (status 0).  The caller asks
// for the next batch at once when this one had no rows.
static bool next_window(dhts_ctx *c, int32_t &status) {
    if (status != 1 || c->win_cur + 1 >= c->wins.size()) return false;
    enter_window(c, c->win_cur + 1);
    discard_prefetch(c);
    c->next_block = c->shard_b0; c->carry_len = 0; c->stream_done = false; c->first_batch = true; c->ucur = 0;
    status = 0;
    return true;
}
int dhts_bam_rewind(dhts_ctx *c) {
    if (!c) return -1;
    discard_prefetch(c);
    if (!c->wins.empty()) enter_window(c, 0);
    c->next_block = c->shard_b0; c->carry_len = 0; c->stream_done = c->rg_empty_window; c->first_batch = true; c->ucur = 0;
    c->huff_b0 = c->huff_nb = 0;            // a new pass redoes phase A (nothing is cached across scans)
    c->last_stream = BamStream{};           // no batch of the new pass has been read yet
    memset(c->tile_stats, 0, sizeof(c->tile_stats));
    skip_header_blocks(c);
    return 0;
}
