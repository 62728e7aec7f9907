// dhts_index_write.inc -- part of dhts_api.hip (included there, inside its extern "C" block; not a translation unit of its own):
// BAI / CSI / TBI writers over hts_index.hip.
// ---- BAI writer (SURVEY 8(f) item 4) ----------------------------------------------------------------------------------------
// Restates samtools-style index building: sam_index (htslib sam.c:989-1027) = hts_idx_init + hts_idx_push per record +
// hts_idx_finish (hts.c:2400-2690: insert_to_b / insert_to_l 2315-2363, update_loff 2426-2455, compress_binning 2457-2508) and
// idx_save_core (hts.c:2754-2818).  The scan supplies (tid, pos, bam_endpos, mapped) per record; virtual offsets follow
// bgzf_tell's rule (bgzf.c bgzf_read: a read that ends exactly at a block end reports the NEXT block's address with offset 0).
// Bins are written in ascending order (the reference writes them in khash order; readers do not depend on it).
// Builds a BAI for the open BAM with one full scan (the scan state is rewound before and after).  Returns the index size.
static int64_t bam_build_index_impl(dhts_ctx *c, int min_shift);
int64_t dhts_bam_build_index(dhts_ctx *c) { if (c && c->fastq) return fail(c, "bam_index: FASTQ/FASTA text cannot be indexed (%s)", FASTQ_SEQ_ONLY); if (c && c->sam_text) return fail(c, "bam_index: SAM text cannot be indexed here (%s)", SAM_SEQ_ONLY); return bam_build_index_impl(c, 0); }
// min_shift > 0: CSI with that min_shift, the depth from the longest reference (sam_index, htslib sam.c:989-1007: hts_adjust_csi_settings
// from n_lvls = 0); min_shift <= 0: BAI
extern "C" int64_t dhts_bam_build_index_csi(dhts_ctx *c, int min_shift) { if (c && c->fastq) return fail(c, "bam_index: FASTQ/FASTA text cannot be indexed (%s)", FASTQ_SEQ_ONLY); if (c && c->sam_text) return fail(c, "bam_index: SAM text cannot be indexed here (%s)", SAM_SEQ_ONLY); return bam_build_index_impl(c, min_shift); }
static int64_t bam_build_index_impl(dhts_ctx *c, int min_shift) {
    if (!c) return -1;
    BED_REFUSE(c, "bam_index");
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->bam_open) return fail(c, "dhts_bam_open not called");
    if (c->rg_active || c->shard_b0 != 0 || c->shard_b1 != c->n_blocks || c->ov_active) return fail(c, "index build needs a whole-file scan (no region, shard or join)");
    if (dhts_bam_rewind(c)) return -1;
    struct Rewind {                                                                  // every way out leaves the scan rewound (the caller's position is not kept mid-scan)
        dhts_ctx *c;
        ~Rewind() { const std::string keep = c->err; (void)dhts_bam_rewind(c); if (!keep.empty()) c->err = keep; }
    } rewind_guard{c};
    const int64_t nb = c->n_blocks;
    auto tell = [&](uint64_t u) -> uint64_t {                                        // bgzf_tell after having read up to inflated offset u
        const uint64_t *uo = c->h_uoff.data();
        int64_t lo = 0, hi = nb + 1;
        while (lo < hi) { const int64_t mid = (lo + hi) / 2; if (uo[mid] < u) lo = mid + 1; else hi = mid; }
        if (lo <= nb && uo[lo] == u) return (lo < nb ? c->h_coff[lo] : c->comp_len) << 16;
        return (c->h_coff[lo - 1] << 16) | (u - uo[lo - 1]);
    };
    IndexAcc ib;
    if (min_shift > 0) {
        int64_t max_len = 0; for (uint32_t l : c->ref_len) if ((int64_t)l > max_len) max_len = l;
        int n_lvls = 0;                                                              // hts_adjust_csi_settings (hts.c:2367-2400) from n_lvls = 0
        const int64_t need = max_len + 256;
        if (need <= (1ll << (min_shift + 27))) { int64_t maxpos = 1ll << min_shift; while (need > maxpos) { ++n_lvls; maxpos *= 8; } }
        else { n_lvls = 9; int64_t maxpos = 1ll << (min_shift + 27); while (need > maxpos) { ++min_shift; maxpos *= 2; } }
        ib.set_csi(min_shift, n_lvls);
    }
    const int n_ref = (int)c->ref_name.size();
    // device state of the passes (hts_index.hip): the windows of every sequence (its length plus 1 Mb of room for reads that hang over its end),
    // counts, violation flags, the last row of the previous batch.  htslib grows a sequence's linear index on demand (insert_to_l, hts.c:2345-2363)
    // and so indexes a file whose header understates a sequence's length: when a record reaches beyond the room (IDX_ERR_LINCAP) the
    // passes have still recorded how many windows every sequence needs, and the build runs once more with that room.
    const bool timing = getenv("DHTS_IDX_TIMING") != nullptr;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t_scan = 0, t_pass = 0; const double t_begin = now();
    std::vector<IdxRun> hruns; int slot = 0;
    std::vector<uint64_t> need_win((size_t)n_ref, 0);
    for (int t = 0; t < n_ref; t++) need_win[(size_t)t] = (((uint64_t)c->ref_len[(size_t)t] + (1u << 20)) >> ib.g.min_shift) + 2;
  for (int attempt = 0; ; attempt++) {
    if (attempt > 0) { if (dhts_bam_rewind(c)) return -1; ib.reset_rows(); }
    ib.begin(n_ref, tell(c->first_rec_uoff));
    std::vector<uint64_t> lin_base((size_t)n_ref + 1, 0);
    for (int t = 0; t < n_ref; t++) lin_base[(size_t)t + 1] = lin_base[(size_t)t] + need_win[(size_t)t];
    const uint64_t n_win = lin_base[(size_t)n_ref];
    DevBuf d_lin, d_base, d_cnt, d_misc;
    ENSURE(c, d_lin, n_win * 8 + 64); ENSURE(c, d_base, ((size_t)n_ref + 1) * 8 + 64); ENSURE(c, d_cnt, (size_t)n_ref * 24 + 64); ENSURE(c, d_misc, 256);
    HIPCHK(c, hipMemsetAsync(d_lin.p, 0xff, n_win * 8 + 64, c->stream));
    HIPCHK(c, hipMemsetAsync(d_cnt.p, 0, (size_t)n_ref * 24 + 64, c->stream));
    HIPCHK(c, hipMemsetAsync(d_misc.p, 0, 256, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_base.p, lin_base.data(), ((size_t)n_ref + 1) * 8, hipMemcpyHostToDevice, c->stream));
    {   // the carry of "batch -1": no row yet, the reader stands in front of the first record
        IdxCarry k{}; k.v = ib.v0;
        HIPCHK(c, hipMemcpyAsync((uint8_t *)d_misc.p + 64, &k, sizeof(k), hipMemcpyHostToDevice, c->stream));
    }
    IdxDev dv; dv.g = ib.g; dv.n_ref = n_ref; dv.lin_base = (const uint64_t *)d_base.p; dv.lin = (unsigned long long *)d_lin.p;
    dv.nmap = (unsigned long long *)d_cnt.p; dv.nunmap = dv.nmap + n_ref; dv.tid_runs = (uint32_t *)(dv.nunmap + n_ref); dv.max_win = dv.tid_runs + n_ref;
    dv.n_nocoor = (unsigned long long *)d_misc.p; dv.err = (uint32_t *)((uint8_t *)d_misc.p + 8);
    IdxCarry *carry2 = (IdxCarry *)((uint8_t *)d_misc.p + 64);
    dhts_bam_batch b; int rc = 0;
    for (;;) {
        const uint32_t mask = (1u << DHTS_BAM_FLAG) | (1u << DHTS_BAM_RNAME) | (1u << DHTS_BAM_POS);
        const double t0 = now();
        if (dhts_bam_next_batch(c, 0, mask, &b)) return -1;
        const double t1 = now(); t_scan += t1 - t0;
        const int64_t n = b.n_rows;
        if (n > 0) {
            ENSURE(c, c->ix_end, (size_t)n * sizeof(IdxRun) * 2 + 64); ENSURE(c, c->c_keep, (size_t)n * 4 + 16); ENSURE(c, c->c_rowmap, ((size_t)n + 1) * 4 + 16);
            BamCols bc; memset(&bc, 0, sizeof(bc));
            bc.flag = (uint16_t *)c->c_flag.p; bc.pos = (int64_t *)c->c_pos.p; bc.cig_rel = (uint32_t *)c->cig_rel.p; bc.ncig_eff = (uint32_t *)c->ncig_eff.p;
            uint32_t r0 = 0; HIPCHK(c, hipMemcpyAsync(&r0, c->rec_off.p, 4, hipMemcpyDeviceToHost, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream));
            const uint64_t out_base = b.first_rec_uoff - r0;
            dv.carry_in = carry2 + slot; dv.carry_out = carry2 + (slot ^ 1); slot ^= 1;
            IdxRun *row_run = (IdxRun *)c->ix_end.p, *runs_dev = row_run + n;
            hipLaunchKernelGGL(bam_index_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->last_stream, (const uint32_t *)c->rec_off.p, bc, (const int32_t *)b.tid, n,
                               out_base, b.end_uoff, (const uint64_t *)c->uoff.p, (const uint64_t *)c->coff.p, nb, c->comp_len, dv, (uint32_t *)c->c_keep.p, row_run);
            const uint32_t *kin[1] = {(const uint32_t *)c->c_keep.p}; uint32_t *kout[1] = {(uint32_t *)c->c_rowmap.p}; uint64_t nruns = 0;
            if (run_scan(c, 1, kin, kout, nullptr, n, &nruns)) return -1;
            hipLaunchKernelGGL(idx_runs_write, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const uint32_t *)c->c_keep.p, (const uint32_t *)c->c_rowmap.p, (const IdxRun *)row_run, n, runs_dev);
            HIPCHK(c, hipGetLastError());
            const size_t at = hruns.size(); hruns.resize(at + (size_t)nruns);
            if (nruns) HIPCHK(c, hipMemcpyAsync(hruns.data() + at, runs_dev, (size_t)nruns * sizeof(IdxRun), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        t_pass += now() - t1;
        if (b.status != 0) { if (b.status < 0) return fail(c, "index build: the scan ended on an error (status %d)", b.status); break; }
    }
    const double t_loop = now();
    {   // the passes' results: violation flags, counts, the linear index up to the last window touched
        uint32_t err = 0; std::vector<uint64_t> cnt((size_t)n_ref * 3 + 8, 0);
        HIPCHK(c, hipMemcpy(&err, dv.err, 4, hipMemcpyDeviceToHost));
        if (n_ref) HIPCHK(c, hipMemcpy(cnt.data(), d_cnt.p, (size_t)n_ref * 24, hipMemcpyDeviceToHost));
        const uint32_t *tr = (const uint32_t *)(cnt.data() + 2 * (size_t)n_ref), *mw = tr + n_ref;
        if (err == IDX_ERR_LINCAP && attempt == 0) {
            for (int t = 0; t < n_ref; t++) if ((uint64_t)mw[t] + 2 > need_win[(size_t)t]) need_win[(size_t)t] = (uint64_t)mw[t] + 2;
            hruns.clear(); slot = 0;
            continue;
        }
        if (err) return fail(c, "index build: %s", ib.err_text(err));
        HIPCHK(c, hipMemcpy(&ib.n_nocoor, dv.n_nocoor, 8, hipMemcpyDeviceToHost));
        for (int t = 0; t < n_ref; t++) {
            ib.nmap[(size_t)t] = cnt[(size_t)t]; ib.nunmap[(size_t)t] = cnt[(size_t)n_ref + (size_t)t]; ib.tid_runs[(size_t)t] = tr[t];
            ib.lin[(size_t)t].resize(mw[t]);
            if (mw[t]) HIPCHK(c, hipMemcpy(ib.lin[(size_t)t].data(), (const uint64_t *)d_lin.p + lin_base[(size_t)t], (size_t)mw[t] * 8, hipMemcpyDeviceToHost));
        }
        ib.runs.swap(hruns);
    }
    (void)rc; (void)t_loop;
    break;
  }
    // where the reader stands after the failing read at EOF: behind the last block that holds data -- the address of the FIRST trailing
    // empty block, else the file size (bgzf_read leaves block_address there, bgzf.c:1282-1285; bgzf_read_block skips the empty blocks
    // with a local address and returns at the end of the file without storing it, 1145-1155)
    uint64_t fin = c->comp_len;
    for (int64_t k = nb; k > 0 && c->h_isize[k - 1] == 0; k--) fin = c->h_coff[k - 1];
    const double t_dl = now();
    if (!ib.finish(fin << 16)) return fail(c, "index build: %s", ib.err.c_str());
    ib.save(c->built_index);
    if (timing) fprintf(stderr, "index build: scan %.2f ms, passes %.2f ms, finish+save %.2f ms (%zu runs)\n", t_scan, t_pass, now() - t_dl, ib.runs.size());
    (void)t_begin;
    return (int64_t)c->built_index.size();
}
int dhts_bam_index_bytes(dhts_ctx *c, uint8_t *out, uint64_t cap) {
    if (!c || !out) return -1;
    if (cap < c->built_index.size()) return fail(c, "index buffer too small");
    memcpy(out, c->built_index.data(), c->built_index.size());
    return 0;
}

// CSI for the open BCF (bcf_index, htslib vcf.c:4657-4688: hts_idx_push(rid, pos, pos + rlen, bgzf_tell) per record; min_shift 14 by
// default, the number of levels from the longest contig of the header, idx_calc_n_lvls_ids + hts_adjust_csi_settings hts.c:2367-2400).
// One scan of the file: the device delivers every record's contig id, position and rlen (the core of the BCF2 record).  The bytes are the
// UNCOMPRESSED index; dhts_bgzf_wrap makes the .csi file of them.
int64_t dhts_bcf_build_index(dhts_ctx *c, int min_shift) {
    if (!c) return -1;
    BED_REFUSE(c, "bcf_index");
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->bcf_open) return fail(c, "dhts_bcf_open not called");
    if (c->vcf_text && c->plain_text) return fail(c, "index build: an uncompressed VCF cannot be indexed (tabix needs BGZF)");
    if (c->bcf_rg_active || c->shard_b0 != 0 || c->shard_b1 != c->n_blocks) return fail(c, "index build needs a whole-file scan (no region or shard)");
    const bool text = c->vcf_text, tbi = text && min_shift <= 0;
    if (min_shift <= 0) min_shift = 14;
    int64_t max_len = 0; int nids = 0;
    for (size_t i = 0; i < c->bh.ctg.size(); i++) if (c->bh.ctg_present[i]) { nids++; if (i < c->bh.ctg_len.size() && c->bh.ctg_len[i] > max_len) max_len = c->bh.ctg_len[i]; }
    int n_lvls = 0;
    auto adjust = [&](int64_t len) {                                                 // hts_adjust_csi_settings (hts.c:2367-2400)
        const int64_t need = len + 256;
        if (need <= (1ll << (min_shift + 27))) { int64_t maxpos = 1ll << (min_shift + 3 * n_lvls); while (need > maxpos) { ++n_lvls; maxpos *= 8; } }
        else { n_lvls = 9; int64_t maxpos = 1ll << (min_shift + 27); while (need > maxpos) { ++min_shift; maxpos *= 2; } }
    };
    if (!text) { if (!max_len) max_len = (1ll << 31) - 1; adjust(max_len); }        // idx_calc_n_lvls_ids
    else if (tbi) n_lvls = 5;
    else {                                                                           // tbx_index (tbx.c:451-484): TBX_MAX_SHIFT 31; the ##contig lengths, or a generous default
        n_lvls = (31 - min_shift + 2) / 3;
        if (max_len) adjust(max_len);
        else n_lvls = min_shift < 10 ? 9 : min_shift < 25 ? 9 - (min_shift - 10) / 3 : 4;
    }
    const std::vector<int32_t> saved_proj = c->bcf_proj;
    const int32_t none = 0;
    if (dhts_bcf_set_projection(c, &none, 0) || dhts_bcf_rewind(c)) return -1;
    const int64_t nb = c->n_blocks;
    auto tell = [&](uint64_t u) -> uint64_t {
        const uint64_t *uo = c->h_uoff.data();
        int64_t lo = 0, hi = nb + 1;
        while (lo < hi) { const int64_t mid = (lo + hi) / 2; if (uo[mid] < u) lo = mid + 1; else hi = mid; }
        if (lo <= nb && uo[lo] == u) return (lo < nb ? c->h_coff[lo] : c->comp_len) << 16;
        return (c->h_coff[lo - 1] << 16) | (u - uo[lo - 1]);
    };
    IndexAcc ib;
    if (tbi) ib.tbi = true; else ib.set_csi(min_shift, n_lvls);
    ib.grow = true;                                                                  // (sequences are numbered as they are met / as the header numbers them: the table grows)
    ib.begin(text ? 0 : nids, tell(c->first_rec_uoff));
    std::vector<int32_t> tid_of; std::vector<std::string> tnames;                    // text: sequence ids in the order of first appearance (get_tid, tbx.c:82-107)
    bool ok = true; int rc = 0;
    std::vector<uint32_t> ro; std::vector<uint8_t> core; int64_t tell_lo = 0;
    const bool timing2 = getenv("DHTS_IDX_TIMING") != nullptr;
    auto now2 = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t2_scan = 0, t2_copy = 0, t2_rows = 0, t2_mark = timing2 ? now2() : 0;
    auto lap = [&](double &acc) { if (timing2) { const double t = now2(); acc += t - t2_mark; t2_mark = t; } };
    struct Restore {                                                                 // every way out puts the caller's projection back and rewinds the scan
        dhts_ctx *c; const std::vector<int32_t> &proj;
        ~Restore() { const std::string keep = c->err; (void)dhts_bcf_set_projection(c, proj.data(), (int32_t)proj.size()); (void)dhts_bcf_rewind(c); if (!keep.empty()) c->err = keep; }
    } restore{c, saved_proj};
    for (;;) {
        dhts_bcf_batch b;
        if (dhts_bcf_next_batch(c, 0, &b)) { rc = -1; break; }
        const int64_t n = b.n_rows / (c->bsch.tidy && c->bsch.n_samples > 0 ? c->bsch.n_samples : 1);
        if (n > 0) {
            // rid / pos / rlen sit in the 32-byte head of every record: offsets from the batch, the heads gathered by one strided copy
            lap(t2_scan);
            ro.resize(n); core.resize((size_t)n * 16);
            HIPCHK(c, hipMemcpyAsync(ro.data(), text ? c->lines.line_off.p : c->b_rec_off.p, n * 4, hipMemcpyDeviceToHost, c->stream));   // (text: a line ends where the next one starts)
            HIPCHK(c, hipStreamSynchronize(c->stream));
            ENSURE(c, c->ix_end, (size_t)n * 16 + 64);
            hipLaunchKernelGGL(bcf_index_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->last_bcf_u, (const uint32_t *)c->b_rec_off.p, n, text ? (const int32_t *)c->v_pos_hi.p : (const int32_t *)nullptr, (uint32_t *)c->ix_end.p);
            HIPCHK(c, hipMemcpyAsync(core.data(), c->ix_end.p, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            lap(t2_copy);
            const uint64_t base = b.first_rec_uoff - ro[0];
            // row by row into the host passes (IndexAcc::push_row): sequence, interval, the virtual offset behind the record.
            // bgzf_tell behind a record: the records' ends only grow, so the block is found by a cursor that moves forward.
            const uint64_t *uo = c->h_uoff.data(); const uint64_t *co = c->h_coff.data();
            const int64_t mp = ib.maxpos(); const int32_t nctg = (int32_t)c->bh.ctg.size();
            if (text && (int32_t)tid_of.size() < nctg) tid_of.resize((size_t)nctg, -1);
            IndexAcc::BatchErr be;
            const uint8_t *cp = core.data();
            for (int64_t i = 0; i < n; i++, cp += 16) {
                int32_t rid, rlen, phi; uint32_t plo; memcpy(&rid, cp, 4); memcpy(&plo, cp + 4, 4); memcpy(&rlen, cp + 8, 4); memcpy(&phi, cp + 12, 4);
                const uint64_t u_end = (i + 1 < n) ? base + ro[i + 1] : b.end_uoff;
                const int64_t p64 = (int64_t)(((uint64_t)(uint32_t)phi << 32) | plo);                   // (BCF: the kernel extends 0xffffffff to -1)
                while (tell_lo <= nb && uo[tell_lo] < u_end) tell_lo++;                  // smallest index with uo[index] >= u_end
                const uint64_t v = (tell_lo <= nb && uo[tell_lo] == u_end) ? ((tell_lo < nb ? co[tell_lo] : c->comp_len) << 16) : ((co[tell_lo - 1] << 16) | (u_end - uo[tell_lo - 1]));
                uint32_t e;
                if (text) {
                    if (rid < 0 || rid >= nctg) { ok = false; ib.err = "record without a sequence name"; break; }
                    int32_t t = tid_of[(size_t)rid];
                    if (t < 0) { t = tid_of[(size_t)rid] = (int32_t)tnames.size(); tnames.push_back(c->bh.ctg[(size_t)rid]); }
                    e = ib.push_row(t, p64 < 0 ? 0 : p64, p64 + rlen, v, true, mp);      // the interval of tbx_parse1: rlen of a text record is its tabix END - pos
                } else e = ib.push_row(rid, p64, p64 + rlen, v, true, mp);
                if (e) { ib.note(be, e); if (e & IndexAcc::IDX_ROW_ERRS) break; }
            }
            if (ok && be.row) {                                                          // (the whole batch's interval violations decide the message, as the device passes report them)
                cp = core.data();
                for (int64_t i = 0; i < n; i++, cp += 16) {
                    int32_t rid, rlen, phi; uint32_t plo; memcpy(&rid, cp, 4); memcpy(&plo, cp + 4, 4); memcpy(&rlen, cp + 8, 4); memcpy(&phi, cp + 12, 4);
                    const int64_t p64 = (int64_t)(((uint64_t)(uint32_t)phi << 32) | plo);
                    int64_t bg = text ? (p64 < 0 ? 0 : p64) : p64, en = p64 + rlen;
                    if (rid < 0) { bg = -1; en = 0; }
                    if (rid >= 0 && !(bg <= mp && en <= mp)) be.row |= IDX_ERR_MAXPOS;
                    if (en < bg) be.row |= IDX_ERR_ENDBEG;
                    if (!text && rid >= ib.n_ref && !ib.grow) be.row |= IDX_ERR_TIDRANGE;
                }
            }
            lap(t2_rows);
            if (ok) ok = ib.batch_ok(be);
            if (!ok) break;
        }
        if (b.status != 0) { if (b.status < 0) { rc = fail(c, "index build: the scan ended on an error (status %d)", b.status); } break; }
    }
    if (rc) return -1;
    if (!ok) return fail(c, "index build: %s", ib.err.c_str());
    uint64_t fin = c->comp_len;
    for (int64_t k = nb; k > 0 && c->h_isize[k - 1] == 0; k--) fin = c->h_coff[k - 1];
    lap(t2_scan);
    if (!ib.finish(fin << 16)) return fail(c, "index build: %s", ib.err.c_str());
    if (text) {                                                                      // tbx_set_meta: the VCF preset {TBX_VCF, 1, 2, 0, '#', 0}, l_nm, names
        const uint32_t conf[6] = {2, 1, 2, 0, '#', 0}; uint32_t l_nm = 0;
        for (auto &nm : tnames) l_nm += (uint32_t)nm.size() + 1;
        auto w32 = [&](uint32_t x) { for (int k = 0; k < 4; k++) ib.aux.push_back((uint8_t)(x >> (8 * k))); };
        for (uint32_t x : conf) w32(x);
        w32(l_nm);
        for (auto &nm : tnames) { ib.aux.insert(ib.aux.end(), nm.begin(), nm.end()); ib.aux.push_back(0); }
    }
    ib.save(c->built_index);
    if (timing2) { fprintf(stderr, "index build (bcf/text): scan %.2f ms, copies %.2f ms, host rows %.2f ms (%zu runs)\n", t2_scan, t2_copy, t2_rows, ib.runs.size()); }
    return (int64_t)c->built_index.size();
}
