// dhts_fasta_nuc.inc -- part of dhts_api.hip (included there, inside its extern "C" block; not a translation unit of its own):
// fasta_nuc.  The loaded .fai goes to the device once (entries, names, a hash table of the names); a batch of intervals -- bins from a
// closed form, BED lines from the delimiter table of a BED context, or host arrays -- becomes an interval table (fasta_nuc.hip), the bases
// are counted by nuc_count and nuc_finalize writes the columns.  The seq column is fa_fetch's output for the same clamped intervals.
static int nuc_col_is_str(int col) { return col == NUC_COL_CHROM || col == NUC_COL_SEQ; }

// ---- staging -----------------------------------------------------------------------------------------------------------------------
// What a query with `region` reads of the FASTA at `path`, by the loaded .fai: of an uncompressed file the byte window of the region's bases
// (whole_sequence: of all bases of the region's sequence -- BED rows that overlap the region may reach past it), of a BGZF file
// everything, as dhts_fasta_open_regions.  The region is ONE region (commas are thousands separators); one that does not parse stages
// nothing and is dhts_nuc_set_region's to report.  dhts_nuc_open follows.
int dhts_nuc_open_region(dhts_ctx *c, const char *path, const char *region, int whole_sequence) {
    if (!c || !path || !region) return -1;
    FastaState &F = c->fa;
    if (!F.loaded) return fail(c, "fasta_nuc: no FASTA index is loaded (dhts_fasta_load_index comes first)");
    uint8_t h[2] = {0, 0};
    { int fd = open(path, O_RDONLY); if (fd < 0) return fail(c, "cannot open %s", path); const ssize_t r = pread(fd, h, 2, 0); close(fd); if (r < 0) return fail(c, "read error on %s", path); }
    if (h[0] == 0x1f && h[1] == 0x8b) { if (dhts_open_path(c, path) != 0 || dhts_bgzf_index(c) < 0) return -1; return 0; }
    uint64_t b = 0, e = 0; int64_t n = 0;
    int tid = -1; int64_t beg = 0, end = 0;
    auto getid = [&](const std::string &nm) { auto it = F.by_name.find(nm); return it == F.by_name.end() ? -1 : it->second; };
    if (parse_region_token_fn(getid, region, tid, beg, end)) {
        const FastaState::Ent &v = F.ents[(size_t)tid];
        if (whole_sequence) { beg = 0; end = (int64_t)v.len; }
        if (beg < 0) beg = 0;
        if ((uint64_t)end > v.len) end = (int64_t)v.len;
        if (v.blen && end > beg) {
            const uint64_t last = (uint64_t)end - 1;
            b = v.off + (uint64_t)beg / v.blen * v.llen + (uint64_t)beg % v.blen; e = v.off + last / v.blen * v.llen + last % v.blen + 1; n = 1;
        }
    }
    return open_path_ranges(c, path, 0, &b, &e, n, true);
}

// ---- open: the index on the device ------------------------------------------------------------------------------------------------
int dhts_nuc_open(dhts_ctx *c, int include_seq) {
    if (!c) return -1;
    FastaState &F = c->fa; NucState &N = c->nuc;
    N.open = false;
    if (!F.loaded) return fail(c, "fasta_nuc: no FASTA index is loaded (dhts_fasta_load_index comes first)");
    HIPCHK(c, hipSetDevice(c->device));
    const uint8_t *text = nullptr; uint64_t text_len = 0;
    if (fasta_text(c, text, text_len)) return -1;
    const size_t n = F.ents.size();
    std::vector<NucEnt> ents(n); std::string names;
    for (size_t i = 0; i < n; i++) {
        const FastaState::Ent &v = F.ents[i]; NucEnt &E = ents[i];
        E.len = v.len; E.blen = v.blen; E.llen = v.llen; E.name_off = (uint32_t)names.size(); E.name_len = (uint32_t)F.idx_names[i].size();
        names += F.idx_names[i];
        // the bases the text holds: fai_retrieve's last read ends with the last base it returns, so a row is readable when that base is there
        E.avail = 0;
        if (v.off < text_len && v.llen > 0) { const uint64_t rel = text_len - v.off, rem = rel % v.llen; E.avail = rel / v.llen * v.blen + (rem < v.blen ? rem : v.blen); }
        E.src = (int64_t)v.off; E.lo = 0; E.hi = text_len;
        if (!c->segs.empty()) {                                                 // staged windows: the one that holds bytes of this sequence
            E.lo = E.hi = 0;
            const uint64_t s0 = v.off, s1 = v.off + (v.blen ? (v.len + v.blen - 1) / v.blen * v.llen : 0);
            for (auto &s : c->segs) if (s.file_off < s1 && s.file_off + s.len > s0) { E.src = (int64_t)v.off + (int64_t)s.res_off - (int64_t)s.file_off; E.lo = s.res_off; E.hi = s.res_off + s.len; break; }
        }
    }
    uint32_t hsize = 16; while (hsize < 2 * n + 2) hsize <<= 1;
    std::vector<uint32_t> table(hsize, 0);
    for (size_t i = 0; i < n; i++) {
        uint32_t h = nuc_hash((const uint8_t *)F.idx_names[i].data(), (uint32_t)F.idx_names[i].size()) & (hsize - 1);
        while (table[h]) h = (h + 1) & (hsize - 1);
        table[h] = (uint32_t)i + 1;
    }
    ENSURE(c, N.ents, n * sizeof(NucEnt) + 64); ENSURE(c, N.names, names.size() + 64); ENSURE(c, N.table, (size_t)hsize * 4); ENSURE(c, N.err, 64);
    if (n) HIPCHK(c, hipMemcpyAsync(N.ents.p, ents.data(), n * sizeof(NucEnt), hipMemcpyHostToDevice, c->stream));
    if (!names.empty()) HIPCHK(c, hipMemcpyAsync(N.names.p, names.data(), names.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(N.table.p, table.data(), (size_t)hsize * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    N.text = text; N.text_len = text_len; N.nseq = (uint32_t)n; N.hmask = hsize - 1; N.include_seq = include_seq != 0;
    N.has_region = false; N.rg_tid = -1; N.bins_bw = 0; N.bins_next = N.bins_total = 0;
    N.proj.clear(); for (int i = 0; i < NUC_N_COLS - (N.include_seq ? 0 : 1); i++) N.proj.push_back(i);
    N.open = true;
    return 0;
}

// init_fasta_region (interval_udf.c:558-571): fai_parse_region with flags 0, then fai_adjust_region, whose every non-zero result counts
// as invalid there -- a start it had to move, or an explicit end behind the sequence's.  Returns 1 for such a region.
int dhts_nuc_set_region(dhts_ctx *c, const char *region) {
    if (!c || !c->nuc.open) return c ? fail(c, "fasta_nuc: dhts_nuc_open not called") : -1;
    FastaState &F = c->fa; NucState &N = c->nuc;
    N.has_region = false; N.rg_tid = -1; N.bins_bw = 0; N.bins_next = N.bins_total = 0;
    if (!region || !*region) return 0;
    int tid = -1; int64_t beg = 0, end = 0;
    auto getid = [&](const std::string &nm) { auto it = F.by_name.find(nm); return it == F.by_name.end() ? -1 : it->second; };
    if (!parse_region_token_fn(getid, region, tid, beg, end)) return 1;
    const int64_t len = (int64_t)F.ents[(size_t)tid].len, ob = beg, oe = end;   // faidx_adjust_position with end_adjust 0
    if (end < beg) beg = end;
    if (beg < 0) beg = 0; else if (len <= beg) beg = len;
    if (end < 0) end = 0; else if (len <= end) end = len;
    if (ob != beg || (oe != end && oe < INT64_MAX)) return 1;
    N.has_region = true; N.rg_tid = tid; N.rg_beg = beg; N.rg_end = end;
    return 0;
}

int dhts_nuc_set_projection(dhts_ctx *c, const int32_t *col_ids, int32_t n) {
    if (!c || !c->nuc.open) return c ? fail(c, "fasta_nuc: dhts_nuc_open not called") : -1;
    if (n < 0 || (n > 0 && !col_ids)) return fail(c, "fasta_nuc: bad projection");
    std::vector<int32_t> p; uint32_t seen = 0;
    for (int32_t i = 0; i < n; i++) {
        const int32_t id = col_ids[i];
        if (id < 0 || id >= NUC_N_COLS || (id == NUC_COL_SEQ && !c->nuc.include_seq) || ((seen >> id) & 1u)) return fail(c, "fasta_nuc: bad projection (column %d)", (int)id);
        seen |= 1u << id; p.push_back(id);
    }
    c->nuc.proj.swap(p);
    return 0;
}

// ---- a batch: N.rows[nrows] -> the projected columns -------------------------------------------------------------------------------
// bed_text: the text the names of NUC_F_NAME_BED rows lie in (the BED context's batch buffer)
static int nuc_emit(dhts_ctx *c, int64_t nrows, const uint8_t *bed_text, dhts_nuc_batch *out) {
    NucState &N = c->nuc;
    const int ncols = (int)N.proj.size();
    N.out.assign((size_t)ncols, dhts_col());
    for (int i = 0; i < ncols; i++) { memset(&N.out[(size_t)i], 0, sizeof(dhts_col)); N.out[(size_t)i].col = N.proj[(size_t)i]; }
    out->n_rows = nrows; out->n_cols = ncols; out->cols = N.out.data();
    if (nrows <= 0 || ncols == 0) return 0;
    bool want_counts = false, want_name = false, want_seq = false;
    for (int id : N.proj) { if (id >= NUC_COL_PCT_AT && id <= NUC_COL_NUM_OTHER) want_counts = true; if (id == NUC_COL_CHROM) want_name = true; if (id == NUC_COL_SEQ) want_seq = true; }
    const uint32_t nr = (uint32_t)nrows; const unsigned rgrid = (unsigned)((nrows + 255) / 256);
    const size_t w4 = (size_t)(nrows + 2) * 4 + 64;
    ENSURE(c, N.npieces, w4); ENSURE(c, N.name_len, w4); ENSURE(c, N.seq_len, w4); ENSURE(c, N.ones, (size_t)nrows + 64);
    HIPCHK(c, hipMemsetAsync(N.err.p, 0, 8, c->stream));
    hipLaunchKernelGGL(nuc_measure, dim3(rgrid), dim3(256), 0, c->stream, (const NucRow *)N.rows.p, nr, (uint32_t *)N.npieces.p, (uint32_t *)N.name_len.p, (uint32_t *)N.seq_len.p, (uint32_t *)N.err.p + 1);
    const unsigned long long *counts = nullptr;
    if (want_counts) {
        ENSURE(c, N.piece_off, (size_t)(nrows + 2) * 8 + 64); ENSURE(c, N.counts, (size_t)nrows * 40 + 64);
        const uint32_t *kin[1] = {(const uint32_t *)N.npieces.p}; uint64_t *kout[1] = {(uint64_t *)N.piece_off.p}; uint64_t total = 0;
        if (run_scan(c, 1, kin, nullptr, kout, nrows, &total)) return -1;
        HIPCHK(c, hipMemsetAsync(N.counts.p, 0, (size_t)nrows * 40, c->stream));
        if (total) {
            KTimer tm(c, DHTS_K_CORE);
            hipLaunchKernelGGL(nuc_count, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, N.text, (const NucRow *)N.rows.p, (const uint64_t *)N.piece_off.p, nr, total, (unsigned long long *)N.counts.p);
        }
        counts = (const unsigned long long *)N.counts.p;
    }
    NucOut o; memset(&o, 0, sizeof(o));
    o.ones = (uint8_t *)N.ones.p;
    for (int id : N.proj) if (!nuc_col_is_str(id)) { ENSURE(c, N.fixed[id], (size_t)nrows * 8 + 64); o.fixed[id] = N.fixed[id].p; }
    if (want_name) { ENSURE(c, N.name_valid, (size_t)nrows + 64); o.name_valid = (uint8_t *)N.name_valid.p; }
    if (want_seq) { ENSURE(c, N.seq_valid, (size_t)nrows + 64); o.seq_valid = (uint8_t *)N.seq_valid.p; }
    hipLaunchKernelGGL(nuc_finalize, dim3(rgrid), dim3(256), 0, c->stream, (const NucRow *)N.rows.p, nr, counts, o);
    uint64_t name_total = 0, seq_total = 0;
    if (want_name) {
        ENSURE(c, N.name_off, w4);
        const uint32_t *kin[1] = {(const uint32_t *)N.name_len.p}; uint32_t *kout[1] = {(uint32_t *)N.name_off.p};
        if (run_scan(c, 1, kin, kout, nullptr, nrows, &name_total)) return -1;
        ENSURE(c, N.name_bytes, (size_t)name_total + 64);
        hipLaunchKernelGGL(nuc_names, dim3(rgrid), dim3(256), 0, c->stream, (const NucRow *)N.rows.p, nr, (const uint8_t *)N.names.p, bed_text, (const uint32_t *)N.name_off.p, (uint8_t *)N.name_bytes.p);
    }
    if (want_seq) {
        ENSURE(c, N.seq_off32, w4); ENSURE(c, N.seq_off64, (size_t)(nrows + 2) * 8 + 64); ENSURE(c, c->fa.rg, (size_t)nrows * sizeof(FaRegion) + 64);
        const uint32_t *kin[1] = {(const uint32_t *)N.seq_len.p}; uint32_t *k32[1] = {(uint32_t *)N.seq_off32.p}; uint64_t *k64[1] = {(uint64_t *)N.seq_off64.p};
        if (run_scan(c, 1, kin, k32, k64, nrows, &seq_total)) return -1;
        if (seq_total >> 32) return fail(c, "fasta_nuc: the seq column of one batch is %llu bytes; a VARCHAR arena holds less than 4 GiB (smaller batches, or no include_seq)", (unsigned long long)seq_total);
        ENSURE(c, c->fa.o_seq, (size_t)seq_total + PAD_BYTES);
        hipLaunchKernelGGL(nuc_fetch_regions, dim3(rgrid), dim3(256), 0, c->stream, (const NucRow *)N.rows.p, nr, (const uint64_t *)N.seq_off64.p, (FaRegion *)c->fa.rg.p);
        if (seq_total) hipLaunchKernelGGL(fa_fetch, dim3((unsigned)((seq_total + 4095) / 4096)), dim3(256), 0, c->stream, N.text, (const FaRegion *)c->fa.rg.p, nr, seq_total, (uint8_t *)c->fa.o_seq.p);
    }
    uint32_t err[2] = {0, 0};
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(err, N.err.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (err[1] && want_seq) return fail(c, "fasta_nuc: an interval of 4 GiB or more cannot be a VARCHAR (no include_seq for it)");
    for (int i = 0; i < ncols; i++) {
        dhts_col &d = N.out[(size_t)i];
        if (d.col == NUC_COL_CHROM) { d.off = (const uint32_t *)N.name_off.p; d.bytes = (const uint8_t *)N.name_bytes.p; d.nbytes = name_total; d.valid = (const uint8_t *)N.name_valid.p; }
        else if (d.col == NUC_COL_SEQ) { d.off = (const uint32_t *)N.seq_off32.p; d.bytes = (const uint8_t *)c->fa.o_seq.p; d.nbytes = seq_total; d.valid = (const uint8_t *)N.seq_valid.p; }
        else { d.fixed = N.fixed[d.col].p; d.valid = (const uint8_t *)N.ones.p; }
    }
    return 0;
}
// keep[n] / tmp[n] -> N.rows (scan, fq_compact, gather); *nrows = the rows kept.  Fails when a row's bases are not resident.
static int nuc_compact(dhts_ctx *c, int64_t n, int64_t *nrows) {
    NucState &N = c->nuc;
    ENSURE(c, N.rank, (size_t)(n + 2) * 4 + 64);
    const uint32_t *kin[1] = {(const uint32_t *)N.keep.p}; uint32_t *kout[1] = {(uint32_t *)N.rank.p}; uint64_t nr = 0;
    if (run_scan(c, 1, kin, kout, nullptr, n, &nr)) return -1;
    uint32_t err = 0;
    HIPCHK(c, hipMemcpy(&err, N.err.p, 4, hipMemcpyDeviceToHost));
    if (err) return fail(c, "fasta_nuc: an interval's bases were not staged (the staged window has to cover every interval)");
    *nrows = (int64_t)nr;
    if (nr == 0) return 0;
    ENSURE(c, N.src, (size_t)nr * 4 + 64); ENSURE(c, N.rows, (size_t)nr * sizeof(NucRow) + 64);
    hipLaunchKernelGGL(fq_compact, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const uint32_t *)N.keep.p, (const uint32_t *)N.rank.p, (uint32_t)n, (uint32_t *)N.src.p);
    hipLaunchKernelGGL(nuc_gather_rows, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, c->stream, (const NucRow *)N.tmp.p, (const uint32_t *)N.src.p, (uint32_t)nr, (NucRow *)N.rows.p);
    return 0;
}

// ---- intervals from host arrays ---------------------------------------------------------------------------------------------------
int dhts_nuc_intervals(dhts_ctx *c, const int32_t *tid, const int64_t *start, const int64_t *end, int64_t n, dhts_nuc_batch *out) {
    if (!c || !out) return -1;
    memset(out, 0, sizeof(*out));
    NucState &N = c->nuc;
    if (!N.open) return fail(c, "fasta_nuc: dhts_nuc_open not called");
    if (n < 0 || n > 0x7fffff00ll || (n > 0 && (!tid || !start || !end))) return fail(c, "fasta_nuc: bad interval arrays");
    HIPCHK(c, hipSetDevice(c->device));
    int64_t nrows = 0;
    if (n > 0) {
        ENSURE(c, N.in_tid, (size_t)n * 4 + 64); ENSURE(c, N.in_start, (size_t)n * 8 + 64); ENSURE(c, N.in_end, (size_t)n * 8 + 64);
        ENSURE(c, N.tmp, (size_t)n * sizeof(NucRow) + 64); ENSURE(c, N.keep, (size_t)(n + 2) * 4 + 64);
        HIPCHK(c, hipMemcpyAsync(N.in_tid.p, tid, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(N.in_start.p, start, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(N.in_end.p, end, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(N.err.p, 0, 8, c->stream));
        hipLaunchKernelGGL(nuc_iv_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const NucEnt *)N.ents.p, N.nseq, (const int32_t *)N.in_tid.p, (const long long *)N.in_start.p, (const long long *)N.in_end.p,
                           (uint32_t)n, (NucRow *)N.tmp.p, (uint32_t *)N.keep.p, (uint32_t *)N.err.p);
        if (nuc_compact(c, n, &nrows)) return -1;
    }
    out->status = 1;
    return nuc_emit(c, nrows, nullptr, out);
}

// ---- bins -------------------------------------------------------------------------------------------------------------------------
// the rows of [beg0, end0) of a sequence at bin width bw: the bins whose last base the text holds (those a file that ends early lacks
// are the last ones of the sequence)
static uint64_t nuc_bins_of(const FastaState::Ent &v, uint64_t avail, uint64_t beg0, uint64_t end0, uint64_t bw) {
    if (v.blen == 0 || end0 <= beg0) return 0;
    if (avail >= end0) return (end0 - beg0 + bw - 1) / bw;
    return avail > beg0 ? (avail - beg0) / bw : 0;
}
int dhts_nuc_next_bins(dhts_ctx *c, int64_t bin_width, int64_t max_rows, dhts_nuc_batch *out) {
    if (!c || !out) return -1;
    memset(out, 0, sizeof(*out));
    NucState &N = c->nuc; FastaState &F = c->fa;
    if (!N.open) return fail(c, "fasta_nuc: dhts_nuc_open not called");
    if (bin_width <= 0) return fail(c, "fasta_nuc bin_width must be > 0");
    HIPCHK(c, hipSetDevice(c->device));
    if (max_rows <= 0) max_rows = 1 << 20;
    if (max_rows > 0x7fffff00ll) max_rows = 0x7fffff00ll;
    const uint64_t bw = (uint64_t)bin_width;
    if (N.bins_bw != bin_width) {                                               // a new scan: the rows in front of every sequence
        std::vector<NucEnt> ents(N.nseq);
        if (N.nseq) HIPCHK(c, hipMemcpy(ents.data(), N.ents.p, (size_t)N.nseq * sizeof(NucEnt), hipMemcpyDeviceToHost));
        std::vector<uint64_t> cum;
        if (N.has_region) { cum.push_back(0); cum.push_back(nuc_bins_of(F.ents[(size_t)N.rg_tid], ents[(size_t)N.rg_tid].avail, (uint64_t)N.rg_beg, (uint64_t)N.rg_end, bw)); }
        else { cum.assign((size_t)N.nseq + 1, 0); for (uint32_t s = 0; s < N.nseq; s++) cum[s + 1] = cum[s] + nuc_bins_of(F.ents[s], ents[s].avail, 0, F.ents[s].len, bw); }
        ENSURE(c, N.cum, cum.size() * 8 + 64);
        HIPCHK(c, hipMemcpy(N.cum.p, cum.data(), cum.size() * 8, hipMemcpyHostToDevice));
        N.bins_bw = bin_width; N.bins_next = 0; N.bins_total = cum.back();
    }
    const uint64_t left = N.bins_total - N.bins_next;
    const int64_t nrows = left < (uint64_t)max_rows ? (int64_t)left : max_rows;
    if (nrows > 0) {
        ENSURE(c, N.rows, (size_t)nrows * sizeof(NucRow) + 64);
        HIPCHK(c, hipMemsetAsync(N.err.p, 0, 8, c->stream));
        hipLaunchKernelGGL(nuc_bin_rows, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, c->stream, (const NucEnt *)N.ents.p, (const uint64_t *)N.cum.p, N.has_region ? 1u : N.nseq, N.has_region ? N.rg_tid : -1,
                           (uint64_t)N.rg_beg, (uint64_t)N.rg_end, bw, N.bins_next, (uint32_t)nrows, (NucRow *)N.rows.p, (uint32_t *)N.err.p);
        uint32_t err = 0;
        HIPCHK(c, hipMemcpyAsync(&err, N.err.p, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (err) return fail(c, "fasta_nuc: a bin's bases were not staged (dhts_fasta_open_regions takes the same region)");
    }
    N.bins_next += (uint64_t)nrows;
    out->status = N.bins_next >= N.bins_total ? 1 : 0;
    return nuc_emit(c, nrows, nullptr, out);
}

// ---- BED --------------------------------------------------------------------------------------------------------------------------
// One batch of the BED context `b` (dhts_bed_open done; with a region and a tabix index: dhts_bed_set_region + dhts_bed_load_index), read
// by fasta_nuc's rules (next_fasta_nuc_bed_interval, interval_udf.c:651-682), not read_bed's: nothing of `b`'s read_bed state changes but
// its scan position.  The lines' chrom, start and end stay on the device.
static int nuc_next_bed_one(dhts_ctx *c, dhts_ctx *b, int64_t max_blocks, dhts_nuc_batch *out) {
    memset(out, 0, sizeof(*out));
    NucState &N = c->nuc; BedState &S = b->bed;
    if (b->stream_done || b->n_blocks <= 0) { out->status = 1; return nuc_emit(c, 0, nullptr, out); }
    if (S.rg_pending) return fail(c, "fasta_nuc: the BED region needs its tabix index (dhts_bed_load_index) before the scan");
    Batch B;
    if (batch_begin(b, max_blocks, B)) return fail(c, "%s", b->err.c_str());
    const uint8_t *u = B.u; const uint64_t ulen = B.ulen;
    LineTab T;
    if (text_line_table(b, B, T)) return fail(c, "%s", b->err.c_str());
    const int64_t nlines = T.nlines; int64_t nrows = 0;
    if (nlines > 0) {
        const size_t ln = (size_t)(nlines + 2) * 4 + 64;
        if (S.lend.ensure(ln) || S.ntab.ensure(ln) || S.is_row.ensure(ln) || S.ctr.ensure(64)) return fail(c, "hipMalloc failed");
        const bool by_region = S.rg_active && !S.rg_all;
        BedLines a; memset(&a, 0, sizeof(a));
        a.u = u; a.line_off = (const uint32_t *)S.lines.line_off.p; a.tab_off = (const uint32_t *)S.tabs.tab_off.p; a.tab0 = (const uint32_t *)S.tabs.tab0.p; a.has_nul = (const uint32_t *)S.tabs.has_nul.p;
        a.nlines = (uint32_t)nlines; a.text_end = (uint32_t)ulen; a.last_open = T.last_open; a.report_bad = 0;
        a.lend = (uint32_t *)S.lend.p; a.ntab = (uint32_t *)S.ntab.p; a.is_row = (uint32_t *)S.is_row.p; a.first_bad = (unsigned long long *)S.ctr.p;
        const unsigned lgrid = (unsigned)((nlines + 255) / 256);
        HIPCHK(c, hipMemsetAsync(S.ctr.p, 0xff, 8, b->stream));
        hipLaunchKernelGGL(bed_classify, dim3(lgrid), dim3(256), 0, b->stream, a);
        if (by_region) {                                                       // tbx_itr_next's test, as read_bed's region query makes it
            if (S.tbx.ensure((size_t)nlines * sizeof(TbxLine) + 64)) return fail(c, "hipMalloc failed");
            hipLaunchKernelGGL(tabix_intervals, dim3(lgrid), dim3(256), 0, b->stream, u, (const uint32_t *)S.lines.line_off.p, nlines, ulen, (int32_t)T.last_open, S.conf, (TbxLine *)S.tbx.p);
            hipLaunchKernelGGL(bed_region_keep, dim3(lgrid), dim3(256), 0, b->stream, u, (const TbxLine *)S.tbx.p, (uint32_t)nlines, (const uint8_t *)S.rg_name_dev.p, (uint32_t)S.rg_name.size(),
                               (long long)S.rg_beg, (long long)S.rg_end, (uint32_t *)S.is_row.p, (unsigned long long *)S.ctr.p);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(b->stream));                             // the rest runs on the FASTA context's stream
        ENSURE(c, N.tmp, (size_t)nlines * sizeof(NucRow) + 64); ENSURE(c, N.keep, ln);
        NucBedArgs g; memset(&g, 0, sizeof(g));
        g.L.u = u; g.L.line_off = a.line_off; g.L.tab_off = a.tab_off; g.L.tab0 = a.tab0; g.L.lend = a.lend; g.L.ntab = a.ntab; g.is_row = a.is_row; g.nlines = (uint32_t)nlines;
        g.ents = (const NucEnt *)N.ents.p; g.names = (const uint8_t *)N.names.p; g.table = (const uint32_t *)N.table.p; g.mask = N.hmask;
        g.region_tid = N.has_region ? N.rg_tid : -1; g.region_beg = N.rg_beg; g.region_end = N.rg_end;
        g.tmp = (NucRow *)N.tmp.p; g.keep = (uint32_t *)N.keep.p; g.err = (uint32_t *)N.err.p;
        HIPCHK(c, hipMemsetAsync(N.err.p, 0, 8, c->stream));
        hipLaunchKernelGGL(nuc_bed_rows, dim3(lgrid), dim3(256), 0, c->stream, g);
        if (nuc_compact(c, nlines, &nrows)) return -1;
    }
    if (nuc_emit(c, nrows, u, out)) return -1;                                  // (synchronises c->stream: the chrom bytes have left the BED batch)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (batch_end(b, B, T.carry_start, false, T.finished, &out->status)) return fail(c, "%s", b->err.c_str());
    if (out->status < 0) return fail(c, "fasta_nuc: the BED stream ended on an error (%s)", b->err.c_str());
    return 0;
}
int dhts_nuc_next_bed(dhts_ctx *c, dhts_ctx *b, int64_t max_blocks, dhts_nuc_batch *out) {
    if (!c || !b || !out) return -1;
    if (!c->nuc.open) return fail(c, "fasta_nuc: dhts_nuc_open not called");
    if (!b->bed.open) return fail(c, "fasta_nuc: the BED context is not open (dhts_bed_open comes first)");
    if (b == c || b->device != c->device) return fail(c, "fasta_nuc: the BED context has to be a second context on the FASTA context's device");
    HIPCHK(c, hipSetDevice(c->device));
    for (;;) {
        if (nuc_next_bed_one(c, b, max_blocks, out)) return -1;
        if (next_window(b, out->status) && out->n_rows == 0) continue;      // several index windows, as in dhts_bed_next_batch
        return 0;
    }
}

// ---- read-back in the style of dhts_bed_batch_fetch (cols_fetch, dhts_bam_accum.inc) -------------------------------------------------
static int nuc_col_kind(int col) { return nuc_col_is_str(col) ? COL_STRING : COL_INT64; }
uint64_t dhts_nuc_batch_host_bytes(const dhts_nuc_batch *b) { return b ? cols_host_bytes(b->n_rows, b->n_cols, b->cols, nuc_col_kind) : 0; }
int dhts_nuc_batch_fetch(dhts_ctx *c, const dhts_nuc_batch *b, void *dst, uint64_t cap, dhts_col *out_cols) {
    return b ? cols_fetch(c, "fasta_nuc", b->n_rows, b->n_cols, b->cols, nuc_col_kind, dst, cap, out_cols) : -1;
}
