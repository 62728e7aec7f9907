// dhts_bam_scan.inc -- part of dhts_api.hip (included there, inside its extern "C" block; not a translation unit of its own):
// the batch driver shared by read_bam and read_bcf, the tabix index build over lines, dhts_bam_next_batch.
// ---- one batch of inflated bytes: carry + blocks [b0, b0+nb), shared by the read_bam and read_bcf drivers ---------------
struct Batch {
    int64_t b0 = 0, nb = 0; bool in_halo = false, last_of_stream = false, sharded_tail = false, final_batch = false;
    uint64_t carry = 0, ulen = 0, out_base = 0; uint8_t *u = nullptr; int blk_err = 0;
    bool status_pending = false;      // the blocks' status words have not been looked at yet (batch_status_resolve)
};
static const uint32_t NONE32 = 0xffffffffu;
// the end of the batch is the end of an undamaged file: what lies behind its last newline is the file's last line (set by batch_begin)
static bool batch_clean_end(const dhts_ctx *c, const Batch &B) { return B.final_batch && !c->gz_error && !B.blk_err; }
// where the batch lies: the carry in front, then blocks [B.b0, B.b0 + B.nb) as the block table places them NOW.  Sets B.carry / ulen / out_base / u
// and grows the stream buffer (the carry bytes at its front are kept).  Called again when the table moved under a batch (a scratch retry).
static int batch_place(dhts_ctx *c, Batch &B) {
    const uint64_t carry = c->carry_len;
    const uint64_t inflated = c->h_uoff[B.b0 + B.nb] - c->h_uoff[B.b0];
    const uint64_t ulen = carry + inflated;
    if (ulen + PAD_BYTES >= (1ull << 32)) return fail(c, "batch too large");
    DevBuf &ub = c->ubuf[c->ucur];
    if (ub.cap < ulen + PAD_BYTES) {
        discard_prefetch(c);
        // grow while preserving the carry bytes at the front
        DevBuf nbuf; if (nbuf.ensure(ulen + PAD_BYTES)) return fail(c, "hipMalloc failed");
        if (carry) HIPCHK(c, hipMemcpyAsync(nbuf.p, ub.p, carry, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        ub.swap(nbuf);                                          // nbuf's destructor frees the old buffer
    }
    B.carry = carry; B.ulen = ulen; B.u = (uint8_t *)ub.p;
    B.out_base = c->h_uoff[B.b0] - carry;                     // absolute stream offset of u[0]
    return 0;
}
// `defer`: do not wait for the inflate here.  The first damaged block is found on the device (bgzf_first_bad_block -> c->d_bstat) and the
// caller reads those four words together with its own first results, then calls batch_status_resolve: the record stage is queued behind
// the inflate without a host round trip, and is queued again on the shortened stream in the rare case that a block was bad.
static int batch_begin(dhts_ctx *c, int64_t max_blocks, Batch &B, bool defer = false) {
    if (max_blocks <= 0) max_blocks = 16384;
    if (max_blocks > 24576) max_blocks = 24576;               // keep every in-batch offset below 2^32
    B.sharded_tail = (c->shard_b1 < c->n_blocks);              // later shards exist: our last record may need halo blocks
    int64_t b0 = c->next_block;
    int64_t limit = c->shard_b1;
    bool in_halo = b0 >= c->shard_b1;
    if (in_halo) limit = c->n_blocks;
    int64_t nb = limit - b0; if (nb > max_blocks) nb = max_blocks;
    if (in_halo && nb > 4) nb = 4;
    if (nb < 0) nb = 0;
    if (c->first_batch && c->shard_rank != 0 && !in_halo) {
        // a shard that starts mid-stream finds its first record by speculation (candidates validated three records deep): give the
        // search at least 1 MiB of inflated bytes to validate against, whatever batch size the caller asked for
        while (b0 + nb < limit && c->h_uoff[b0 + nb] - c->h_uoff[b0] < (1u << 20) && nb < 24576) nb++;
    }
    B.b0 = b0; B.nb = nb; B.in_halo = in_halo;
    B.last_of_stream = (b0 + nb >= c->n_blocks) && !c->growing;        // (more blocks may still arrive: dhts_open_path_async)
    {   // phase A over the range (unless the scratch holds it) BEFORE the batch's sizes are read: the block table may be corrected there
        const int64_t ahead0 = c->shard_b1 + 8 < c->n_blocks ? c->shard_b1 + 8 : c->n_blocks;
        if (!(c->pf.valid && c->pf.b0 == b0 && c->pf.nb == nb) && huff_ensure(c, b0, nb, ahead0)) return -1;
    }
    if (batch_place(c, B)) return -1;
    const uint64_t carry = B.carry;
    uint64_t ulen = B.ulen; uint8_t *u = B.u; uint64_t out_base = B.out_base;
    if (c->pf.valid && c->pf.b0 == b0 && c->pf.nb == nb && c->pf.carry == carry && c->pf.ucur == c->ucur) {
        // this batch's phase B was started during the previous batch's record stage: just order the streams
        c->pf.valid = false;
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->pf_done, 0));
    } else {
        // phase A may run ahead of this batch, but not beyond what the scan can reach: the shard (or index window) plus its halo
        const int64_t ahead = c->shard_b1 + 8 < c->n_blocks ? c->shard_b1 + 8 : c->n_blocks;
        if (inflate_blocks(c, b0, nb, u, out_base, ahead)) return -1;
        HIPCHK(c, hipMemsetAsync(u + ulen, 0, PAD_BYTES, c->stream));
    }
    // first bad block (if any) ends the byte stream there (bgzf.c:1241-1291: the read fails)
    int blk_err = 0;
    if (nb > 0 && defer) {
        ENSURE(c, c->d_bstat, 64);
        hipLaunchKernelGGL(bgzf_first_bad_block, dim3(1), dim3(1024), 0, c->stream, (const int32_t *)c->blk_status.p, b0, (int32_t)nb, (uint32_t *)c->d_bstat.p);
        B.status_pending = true;
    } else if (nb > 0) {
        std::vector<int32_t> bs(nb);
        for (int attempt = 0; ; attempt++) {
            HIPCHK(c, hipMemcpyAsync(bs.data(), (int32_t *)c->blk_status.p + b0, nb * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            bool scratch = false;
            for (int64_t k = 0; k < nb; k++) if (bs[k] == DHTS_BLK_ERR_SCRATCH) { scratch = true; break; }
            if (!scratch) break;
            // the packed phase-A scratch was too small for some block (data that expands into far more tokens than a BAM or BCF does):
            // decode this range again with the full 152 KiB per block
            if (attempt > 0) return fail(c, "internal: phase-A scratch exhausted twice");
            const int64_t ahead = c->shard_b1 + 8 < c->n_blocks ? c->shard_b1 + 8 : c->n_blocks;
            // phase A first: it may move the block table (the blocks that failed are decoded now, isize_repair sees them); the batch is
            // placed again from the table as it stands, then phase B writes into a buffer of that size
            if (scratch_retry_phase_a(c, b0, nb, ahead) || batch_place(c, B)) return -1;
            ulen = B.ulen; u = B.u; out_base = B.out_base;
            if (inflate_blocks(c, b0, nb, u, out_base, ahead)) return -1;
            HIPCHK(c, hipMemsetAsync(u + ulen, 0, PAD_BYTES, c->stream));
        }
        for (int64_t k = 0; k < nb; k++) if (bs[k] != 0) { blk_err = bs[k]; ulen = carry + (c->h_uoff[b0 + k] - c->h_uoff[b0]); break; }
    }
    // (where only index windows are resident, the last resident block is not the end of the FILE: the record that runs out of it is cut by
    // the staging, not truncated)
    B.final_batch = (B.last_of_stream && !(c->partial_tail && !c->segs.empty())) || blk_err != 0;
    B.carry = carry; B.ulen = ulen; B.out_base = out_base; B.u = u; B.blk_err = blk_err;
    return 0;
}
// The four words of bgzf_first_bad_block have reached the host (`bst`).  Returns 0 when every block of the batch is good, 1 when the batch
// changed and the caller has to queue its record stage again (a damaged block cut the stream: B.ulen / B.final_batch / B.blk_err are
// updated; or the packed phase-A scratch was too small: the range has been inflated again with full-size room and the status is pending
// again), -1 on failure.
static int batch_status_resolve(dhts_ctx *c, Batch &B, const uint32_t bst[4], int attempt) {
    B.status_pending = false;
    if (bst[2] != NONE32) {
        if (attempt > 0) return fail(c, "internal: phase-A scratch exhausted twice");
        const int64_t ahead = c->shard_b1 + 8 < c->n_blocks ? c->shard_b1 + 8 : c->n_blocks;
        // (as in batch_begin: phase A, then the batch placed again from the table, then phase B; the caller takes B.u / ulen / out_base anew)
        if (scratch_retry_phase_a(c, B.b0, B.nb, ahead) || batch_place(c, B)) return -1;
        if (inflate_blocks(c, B.b0, B.nb, B.u, B.out_base, ahead)) return -1;
        HIPCHK(c, hipMemsetAsync(B.u + B.ulen, 0, PAD_BYTES, c->stream));
        hipLaunchKernelGGL(bgzf_first_bad_block, dim3(1), dim3(1024), 0, c->stream, (const int32_t *)c->blk_status.p, B.b0, (int32_t)B.nb, (uint32_t *)c->d_bstat.p);
        B.status_pending = true;
        return 1;
    }
    if (bst[0] != NONE32) {
        B.blk_err = (int)(int32_t)bst[1];
        B.ulen = B.carry + (c->h_uoff[B.b0 + bst[0]] - c->h_uoff[B.b0]);
        B.final_batch = true;
        return 1;
    }
    return 0;
}
// advance the scan position; *status as documented for dhts_bam_batch.status
// `synced`: the caller has already waited for the batch's results; the copy of the tail queued here is ordered in front of the next batch's
// work on the same stream, so the batch ends without another host round trip.
static int batch_end(dhts_ctx *c, const Batch &B, uint64_t carry_start, bool rec_err, bool shard_finished, int32_t *status, bool synced = false) {
    c->first_batch = false;
    c->next_block = B.b0 + B.nb;
    if (rec_err || B.blk_err || shard_finished || B.last_of_stream) discard_prefetch(c);
    // a damaged block in the HALO (the successor's blocks, read only until this shard's last record completes) is the successor's to report:
    // when everything in front of it was consumed by complete records, or the first record of the next shard has been seen, this shard ends well
    const bool halo_done = B.in_halo && B.blk_err && !rec_err && (shard_finished || carry_start == B.ulen);
    if ((rec_err || B.blk_err) && !halo_done) { c->stream_done = true; *status = B.blk_err ? B.blk_err * 100 : -4; }
    else if (shard_finished || halo_done) { c->stream_done = true; *status = 1; }
    else if (B.last_of_stream) { c->stream_done = true; *status = (c->bgzf_status != 0) ? c->bgzf_status : 1; if (carry_start < B.ulen && *status == 1 && !(c->partial_tail && !c->segs.empty())) *status = -4; }
    else {
        // move the incomplete tail to the front of the other buffer
        uint64_t tail = B.ulen - carry_start;
        DevBuf &nx = c->ubuf[c->ucur ^ 1];
        if (c->pf.valid && !(c->pf.carry == tail && c->pf.b0 == B.b0 + B.nb && c->pf.ucur == (c->ucur ^ 1))) discard_prefetch(c);
        if (!c->pf.valid) {                                   // (a live prefetch has already copied the tail there)
            ENSURE(c, nx, tail + PAD_BYTES);
            if (tail) HIPCHK(c, hipMemcpyAsync(nx.p, B.u + carry_start, tail, hipMemcpyDeviceToDevice, c->stream));
        }
        c->carry_len = tail; c->ucur ^= 1;
        if (B.in_halo && tail == 0) { c->stream_done = true; *status = 1; }
        if (B.b0 + B.nb >= c->shard_b1 && B.sharded_tail && tail == 0) { c->stream_done = true; *status = 1; }
    }
    if (!synced) HIPCHK(c, hipStreamSynchronize(c->stream));
    timing_collect(c);
    return 0;
}

// ---- tabix index of a bgzipped line format other than VCF (tbx_index_build3 / tbx_index, tbx.c:437-541, with tbx_conf_bed / _gff / _sam or
// custom columns): the device finds the lines and their intervals (tabix_intervals), the host numbers the sequence names in order of first
// appearance and feeds hts_idx_push.  min_shift <= 0: TBI.  The context needs dhts_open_path + dhts_bgzf_index only.
extern "C" int64_t dhts_tabix_build_index(dhts_ctx *c, int preset, int sc, int bc, int ec, int meta_char, int line_skip, int min_shift) {
    if (!c) return -1;
    BED_REFUSE(c, "tabix_index");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n_blocks <= 0 || c->plain_text) return fail(c, "tabix_index: the file is not BGZF");
    if ((preset & 0xffff) == 2) return fail(c, "tabix_index: the vcf preset goes through dhts_bcf_build_index");
    if ((preset & 0xffff) > 2) return fail(c, "tabix_index: preset not supported");
    discard_prefetch(c);
    c->shard_b0 = 0; c->shard_b1 = c->n_blocks; c->shard_rank = 0; c->shard_world = 1; c->wins.clear(); c->win_cur = 0; c->scan_end_uoff = ~0ull; c->rg_empty_window = false;
    c->next_block = 0; c->carry_len = 0; c->stream_done = false; c->first_batch = true; c->ucur = 0; c->huff_b0 = c->huff_nb = 0; c->scan_first_uoff = 0;
    const bool tbi = min_shift <= 0;
    if (tbi) min_shift = 14;
    const int64_t nb = c->n_blocks;
    auto tell = [&](uint64_t u) -> uint64_t {
        const uint64_t *uo = c->h_uoff.data();
        int64_t lo = 0, hi = nb + 1;
        while (lo < hi) { const int64_t mid = (lo + hi) / 2; if (uo[mid] < u) lo = mid + 1; else hi = mid; }
        if (lo <= nb && uo[lo] == u) return (lo < nb ? c->h_coff[lo] : c->comp_len) << 16;
        return (c->h_coff[lo - 1] << 16) | (u - uo[lo - 1]);
    };
    IndexAcc ib; ib.grow = true; bool inited = false; uint64_t last_off = tell(0); int64_t lineno = 0, max_ref_len = 0;
    std::vector<int32_t> a_tid; std::vector<int64_t> a_beg, a_end; std::vector<uint64_t> a_v; std::vector<uint8_t> a_map;     // the data lines of a batch as arrays
    auto init_index = [&]() {
        if (tbi) ib.tbi = true;
        else {
            int n_lvls = (31 - min_shift + 2) / 3;
            if (max_ref_len) {
                const int64_t need = max_ref_len + 256;
                if (need <= (1ll << (min_shift + 27))) { int64_t maxpos = 1ll << (min_shift + 3 * n_lvls); while (need > maxpos) { ++n_lvls; maxpos *= 8; } }
                else { n_lvls = 9; int64_t maxpos = 1ll << (min_shift + 27); while (need > maxpos) { ++min_shift; maxpos *= 2; } }
            } else n_lvls = min_shift < 10 ? 9 : min_shift < 25 ? 9 - (min_shift - 10) / 3 : 4;
            ib.set_csi(min_shift, n_lvls);
        }
        ib.begin(0, last_off); inited = true;
    };
    std::vector<std::string> names; std::map<std::string, int32_t> tid_of; int32_t last_tid = -1;
    std::vector<TbxLine> rows; std::vector<uint32_t> lo; std::string nm;
    TbxConf cf = {preset, sc, bc, ec, meta_char, line_skip};
    int rc = 0; std::string err;
    for (;;) {
        Batch B;
        if (batch_begin(c, 0, B)) return -1;
        const uint8_t *u = B.u; const uint64_t ulen = B.ulen, out_base = B.out_base;
        // (its own rule for the open last line: B.final_batch alone.  It differs from batch_clean_end in B.blk_err only -- gz_error cannot be set
        // on a BGZF file -- and a damaged block fails the build behind this batch either way; the cut line in front of it is parsed first)
        LineTab T;
        if (line_table(c, c->lines, nullptr, u, 0, ulen, B.final_batch, ~0ull, -1, T)) return -1;
        const uint64_t carry_start = T.carry_start; const int64_t nlines = T.nlines; const int last_open = T.last_open;
        if (nlines > 0 && line_starts_fetch(c, c->lines, T.nl + 1, lo)) return -1;
        if (nlines > 0) {
            ENSURE(c, c->v_undef, (size_t)nlines * sizeof(TbxLine) + 64);
            hipLaunchKernelGGL(tabix_intervals, dim3((unsigned)((nlines + 255) / 256)), dim3(256), 0, c->stream, u, (const uint32_t *)c->lines.line_off.p, nlines, ulen, last_open, cf, (TbxLine *)c->v_undef.p);
            rows.resize((size_t)nlines);
            HIPCHK(c, hipMemcpyAsync(rows.data(), c->v_undef.p, (size_t)nlines * sizeof(TbxLine), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            a_tid.clear(); a_beg.clear(); a_end.clear(); a_v.clear();
            for (int64_t i = 0; i < nlines && rc == 0; i++) {
                const TbxLine &r = rows[(size_t)i];
                ++lineno;
                const uint64_t after = tell(out_base + ((last_open && i + 1 == nlines) ? ulen : (uint64_t)lo[(size_t)i + 1]));
                if (lineno <= line_skip || r.flag == 1) {
                    if (r.flag == 1 && !tbi && (preset & 0xffff) == 1) {                   // adjust_max_ref_len_sam (tbx.c:425-435): @SQ ... LN:
                        const uint32_t l0 = lo[(size_t)i], l1 = (last_open && i + 1 == nlines) ? (uint32_t)ulen : lo[(size_t)i + 1] - 1u;
                        std::string line(l1 - l0, '\0');
                        if (l1 > l0) HIPCHK(c, hipMemcpy(&line[0], u + l0, l1 - l0, hipMemcpyDeviceToHost));
                        if (line.compare(0, 3, "@SQ") == 0) { const size_t q = line.find("\tLN:", 3); if (q != std::string::npos) { const long long len = strtoll(line.c_str() + q + 4, nullptr, 10); if (len > max_ref_len) max_ref_len = len; } }
                    }
                    last_off = after; continue;
                }
                if (!inited) init_index();
                if (r.flag == 2) { rc = -1; err = "Failed to parse the line (was the wrong preset used?)"; break; }
                int32_t tid = last_tid;
                if (!r.same || last_tid < 0) {
                    nm.assign(r.name_len, '\0');
                    if (r.name_len) HIPCHK(c, hipMemcpy(&nm[0], u + r.name_off, r.name_len, hipMemcpyDeviceToHost));
                    auto it = tid_of.find(nm);
                    if (it == tid_of.end()) { tid = (int32_t)names.size(); tid_of[nm] = tid; names.push_back(nm); } else tid = it->second;
                    last_tid = tid;
                }
                a_tid.push_back(tid); a_beg.push_back(r.beg); a_end.push_back(r.end); a_v.push_back(after);
            }
            if (rc == 0 && !a_tid.empty()) {
                a_map.assign(a_tid.size(), 1);
                if (!ib.add_rows(a_tid.data(), a_beg.data(), a_end.data(), a_v.data(), a_map.data(), (int64_t)a_tid.size())) { rc = -1; err = ib.err; }
            }
        }
        if (rc) break;
        int32_t status = 0;
        if (batch_end(c, B, carry_start, false, false, &status)) return -1;
        if (status == 1) break;
        if (status < 0) { rc = -1; err = "the BGZF stream ended on an error"; break; }
    }
    discard_prefetch(c);
    c->next_block = 0; c->carry_len = 0; c->stream_done = false; c->first_batch = true; c->ucur = 0;
    if (rc) return fail(c, "tabix_index: %s", err.c_str());
    if (!inited) init_index();
    uint64_t fin = c->comp_len;
    for (int64_t k = nb; k > 0 && c->h_isize[k - 1] == 0; k--) fin = c->h_coff[k - 1];
    if (!ib.finish(fin << 16)) return fail(c, "tabix_index: %s", ib.err.c_str());
    {
        const uint32_t conf[6] = {(uint32_t)preset, (uint32_t)sc, (uint32_t)bc, (uint32_t)ec, (uint32_t)meta_char, (uint32_t)line_skip}; uint32_t l_nm = 0;
        for (auto &x : names) l_nm += (uint32_t)x.size() + 1;
        auto w32 = [&](uint32_t x) { for (int k = 0; k < 4; k++) ib.aux.push_back((uint8_t)(x >> (8 * k))); };
        for (uint32_t x : conf) w32(x);
        w32(l_nm);
        for (auto &x : names) { ib.aux.insert(ib.aux.end(), x.begin(), x.end()); ib.aux.push_back(0); }
    }
    ib.save(c->built_index);
    return (int64_t)c->built_index.size();
}

// tests: what the repair and retry paths of the record stage (read_bam and read_bcf alike) did since the context was opened or rewound.
// Host-side counters, bumped where the driver reads the repair rounds' counts and decides about a speculated shard start.
extern "C" int dhts_debug_tile_stats(dhts_ctx *c, uint64_t out[8]) {
    if (!c || !out) return -1;
    memcpy(out, c->tile_stats, sizeof(c->tile_stats));
    return 0;
}

// ---- the fused row pass (bam_tile_rows.hip) ------------------------------------------------------------------------------------------
// OPT-IN (DHTS_ROWS=fused): measured slower than the three passes (profiles/r04/rows_fused_*.txt: 2.3-4.0 ms against 1.87 ms per 19,813-block
// batch).  The record stage is bound by instruction issue, not by HBM bytes (a tile costs ~7.5 k SIMD-cycles in the unpack part and ~10 k in the
// string part whichever kernel they run in), so saving a read of the inflated stream buys nothing, the fused kernel's 232 VGPRs leave two
// waves per SIMD, and a look-back over 8 KiB tiles (14 ns of device time each) needs 6.5 windows and 20 polls per tile.  Kept because it is
// exact (the GPU suite passes with it) and is the one-host-round-trip form of the batch.
// DHTS_ROWS=sync: the rows of a batch wait for the host after the tile pass and after the string scans (three round trips per batch, rounds 1-3)
static bool rows_deferred_on() { static const bool on = !(getenv("DHTS_ROWS") && !strcmp(getenv("DHTS_ROWS"), "sync")); return on; }
static bool rows_fused_on() { static const bool on = getenv("DHTS_ROWS") && !strcmp(getenv("DHTS_ROWS"), "fused"); return on; }
static int rows_exp() { static const int e = getenv("DHTS_ROWS_EXP") ? (atoi(getenv("DHTS_ROWS_EXP")) & 2) : 0; return e; }   // timing experiments (tools/dbg/time_rows.py)
// DHTS_TILE_SCAN=wave|lanes|auto: which kernel speculates and walks tiles t >= 1 (tile 0 is always bam_tile_scan's: it carries start0, spec_from
// and a search that may run through the whole batch).  lanes = bam_tile_scan_lanes, one lane per tile straight from HBM; wave = one wave per
// tile out of LDS.  auto (the default) takes the lane kernel from TILE_SCAN_LANES_MIN tiles on: a lane's tile is a chain of ~30 dependent
// HBM reads, which only a grid with many waves per CU hides.  Measured at 256 / 1,024 / 4,096 / 19,813 blocks per batch
// (tools/dbg/time_tile_scan.py, DESIGN §5h): the tile pass takes 0.030 / 0.051 / 0.139 / 0.606 ms with the wave kernel and 0.060 / 0.063 /
// 0.090 / 0.303 ms with the lane kernel; 4,096 full blocks (32,640 tiles) is the smallest size measured from which the lane kernel wins.
// Read per batch, so that one process can run both (the kernels are each other's cross-check).
#define TILE_SCAN_LANES_MIN 32640
static int tile_scan_mode() {                                 // 0 auto, 1 wave, 2 lanes; a value that is none of the three is reported once and read as auto
    const char *e = getenv("DHTS_TILE_SCAN");
    if (!e || !strcmp(e, "auto")) return 0;
    if (!strcmp(e, "wave")) return 1;
    if (!strcmp(e, "lanes")) return 2;
    static std::atomic<bool> warned{false};
    if (!warned.exchange(true)) fprintf(stderr, "[dhts] DHTS_TILE_SCAN=%s is not wave, lanes or auto: using auto\n", e);
    return 0;
}
static bool tile_scan_lanes_on(int64_t ntiles) { const int m = tile_scan_mode(); return m == 2 || (m == 0 && ntiles >= TILE_SCAN_LANES_MIN); }
// the tile pass's first kernel: every tile's speculated first record, chain exit, count, error flag and record list
static void tile_scan_launch(dhts_ctx *c, bool lanes, const BamStream &st, uint64_t start0, int64_t ntiles, const TileOut &to, uint16_t *recs, uint64_t *recs_first, uint64_t spec_from) {
    if (lanes && ntiles > 1) {
        hipLaunchKernelGGL(bam_tile_scan, dim3(1), dim3(64), 0, c->stream, st, start0, ntiles, to, recs, recs_first, spec_from);
        hipLaunchKernelGGL(bam_tile_scan_lanes, dim3((unsigned)((ntiles - 1 + 63) / 64)), dim3(64), 0, c->stream, st, ntiles, to, recs, recs_first);
    } else
        hipLaunchKernelGGL(bam_tile_scan, dim3((unsigned)ntiles), dim3(64), 0, c->stream, st, start0, ntiles, to, recs, recs_first, spec_from);
}
// One scan kernel alone over the inflated batch the context holds (c->last_stream), its six tables copied to the host before any repair
// round: kernel 0 = bam_tile_scan on every tile, 1 = bam_tile_scan_lanes (tile 0 by bam_tile_scan).  Tile 0 starts at offset 0 where that
// is a record boundary, so compare tiles t >= 1.  recs holds TL_RECS entries per tile.  Returns the number of tiles, or -1.
extern "C" int64_t dhts_debug_tile_scan(dhts_ctx *c, int kernel, uint64_t *first, uint64_t *end_next, uint32_t *count, int32_t *err, uint64_t *recs_first,
                                        uint16_t *recs, int64_t ntiles_cap) {
    if (!c) return -1;
    if (kernel != 0 && kernel != 1) return fail(c, "dhts_debug_tile_scan: kernel is 0 (wave) or 1 (lanes)");
    const BamStream st = c->last_stream;
    if (!st.u) return fail(c, "dhts_debug_tile_scan: no batch has been read");
    HIPCHK(c, hipSetDevice(c->device));
    int64_t ntiles = (int64_t)((st.ulen + TILE_BYTES - 1) / TILE_BYTES); if (ntiles < 1) ntiles = 1;
    if (ntiles > ntiles_cap) return fail(c, "dhts_debug_tile_scan: the tables are too small");
    DevBuf d_first, d_end, d_count, d_err, d_rf, d_recs;
    ENSURE(c, d_first, ntiles * 8); ENSURE(c, d_end, ntiles * 8); ENSURE(c, d_count, ntiles * 4); ENSURE(c, d_err, ntiles * 4);
    ENSURE(c, d_rf, ntiles * 8 + 64); ENSURE(c, d_recs, (size_t)ntiles * TL_RECS * 2 + 64);
    HIPCHK(c, hipMemsetAsync(d_first.p, 0xee, ntiles * 8, c->stream)); HIPCHK(c, hipMemsetAsync(d_end.p, 0xee, ntiles * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(d_count.p, 0xee, ntiles * 4, c->stream)); HIPCHK(c, hipMemsetAsync(d_err.p, 0xee, ntiles * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(d_rf.p, 0xee, ntiles * 8, c->stream)); HIPCHK(c, hipMemsetAsync(d_recs.p, 0xee, (size_t)ntiles * TL_RECS * 2, c->stream));
    TileOut to; to.first = (uint64_t *)d_first.p; to.end_next = (uint64_t *)d_end.p; to.count = (uint32_t *)d_count.p; to.err = (int32_t *)d_err.p;
    tile_scan_launch(c, kernel == 1, st, 0, ntiles, to, (uint16_t *)d_recs.p, (uint64_t *)d_rf.p, 0);
    HIPCHK(c, hipGetLastError());
    if (first) HIPCHK(c, hipMemcpyAsync(first, d_first.p, ntiles * 8, hipMemcpyDeviceToHost, c->stream));
    if (end_next) HIPCHK(c, hipMemcpyAsync(end_next, d_end.p, ntiles * 8, hipMemcpyDeviceToHost, c->stream));
    if (count) HIPCHK(c, hipMemcpyAsync(count, d_count.p, ntiles * 4, hipMemcpyDeviceToHost, c->stream));
    if (err) HIPCHK(c, hipMemcpyAsync(err, d_err.p, ntiles * 4, hipMemcpyDeviceToHost, c->stream));
    if (recs_first) HIPCHK(c, hipMemcpyAsync(recs_first, d_rf.p, ntiles * 8, hipMemcpyDeviceToHost, c->stream));
    if (recs) HIPCHK(c, hipMemcpyAsync(recs, d_recs.p, (size_t)ntiles * TL_RECS * 2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ntiles;
}
struct RowsQueued { BamCols bc; RowsStr so; };
// Queues the row pass of the batch behind its tile pass: row arrays and string arenas are sized from the hints the previous batches left
// (or from the batch's inflated size) and guarded on the device; the pass reports what it needed in res[8..14].
static int rows_queue(dhts_ctx *c, const BamStream &st, int64_t ntiles, const TileOut &to, uint32_t colmask, RowsQueued &rq) {
    const uint64_t ulen = st.ulen;
    int64_t rcap = (int64_t)(ulen / 160) + 4096; if (c->rows_hint > rcap) rcap = c->rows_hint;
    // typical shares of a 30x BAM's inflated bytes, generous: a batch that needs more says so and is repeated once
    const uint64_t guess[5] = {ulen / 8 + 65536, ulen / 16 + 65536, ulen / 2 + 65536, ulen / 2 + 65536, ulen / 16 + 65536};
    const uint32_t str_cols = (1u << DHTS_BAM_QNAME) | (1u << DHTS_BAM_CIGAR) | (1u << DHTS_BAM_SEQ) | (1u << DHTS_BAM_QUAL) | (1u << DHTS_BAM_READ_GROUP_ID);
    const bool strings = (colmask & str_cols) != 0;
    const uint32_t hbit[5] = {1u << DHTS_BAM_QNAME, 1u << DHTS_BAM_CIGAR, 1u << DHTS_BAM_SEQ, 1u << DHTS_BAM_QUAL, 1u << DHTS_BAM_READ_GROUP_ID};
    RowsCaps caps; caps.rows = rcap;
    DevBuf *arena[5] = {&c->a_qname, &c->a_cigar, &c->a_seq, &c->a_qual, &c->a_rg};
    for (int k = 0; k < 5; k++) {
        uint64_t want = 0;
        if (colmask & hbit[k]) { want = guess[k]; if (c->heap_hint[k] > want) want = c->heap_hint[k]; }
        if (want) { ENSURE(c, *arena[k], want + PAD_BYTES); caps.heap[k] = arena[k]->cap - PAD_BYTES; } else caps.heap[k] = 0;
    }
    const size_t n = (size_t)rcap;
    ENSURE(c, c->rec_off, n * 4 + 16); ENSURE(c, c->c_rgflag, n + 64);
    ENSURE(c, c->c_flag, n * 2 + 16); ENSURE(c, c->c_pos, n * 8); ENSURE(c, c->c_mapq, n * 4); ENSURE(c, c->c_pnext, n * 8); ENSURE(c, c->c_tlen, n * 8);
    ENSURE(c, c->c_tid, n * 4); ENSURE(c, c->c_mtid, n * 4); ENSURE(c, c->c_rgidx, n * 4); ENSURE(c, c->c_rgvalid, (n / 64 + 2) * 8);
    ENSURE(c, c->l_qname, n * 4 + 16); ENSURE(c, c->l_cigar, n * 4 + 16); ENSURE(c, c->l_seq, n * 4 + 16); ENSURE(c, c->l_qual, n * 4 + 16); ENSURE(c, c->l_rg, n * 4 + 16);
    ENSURE(c, c->cig_rel, n * 4); ENSURE(c, c->ncig_eff, n * 4); ENSURE(c, c->rg_rel, n * 4); ENSURE(c, c->alen_qual, n * 4);
    ENSURE(c, c->o_qname, (n + 1) * 4 + 16); ENSURE(c, c->o_cigar, (n + 1) * 4 + 16); ENSURE(c, c->o_seq, (n + 1) * 4 + 16); ENSURE(c, c->o_qual, (n + 1) * 4 + 16); ENSURE(c, c->o_rg, (n + 1) * 4 + 16);
    BamDict dict; dict.n_rg = (int32_t)c->rg_id.size(); dict.rg_off = (const uint32_t *)c->d_rg_off.p; dict.rg_bytes = (const uint8_t *)c->d_rg_bytes.p; { size_t tb_ = 0; for (auto &id_ : c->rg_id) tb_ += id_.size(); dict.n_bytes = (int32_t)tb_; }
    BamCols &bc = rq.bc; memset(&bc, 0, sizeof(bc));
    bc.flag = (uint16_t *)c->c_flag.p; bc.pos = (int64_t *)c->c_pos.p; bc.mapq = (int32_t *)c->c_mapq.p; bc.pnext = (int64_t *)c->c_pnext.p;
    bc.tlen = (int64_t *)c->c_tlen.p; bc.tid = (int32_t *)c->c_tid.p; bc.mtid = (int32_t *)c->c_mtid.p; bc.rg_idx = (int32_t *)c->c_rgidx.p;
    bc.rg_valid = (uint64_t *)c->c_rgvalid.p; bc.len_qname = (uint32_t *)c->l_qname.p; bc.len_cigar = (uint32_t *)c->l_cigar.p; bc.len_seq = (uint32_t *)c->l_seq.p;
    bc.len_qual = (uint32_t *)c->l_qual.p; bc.len_rg = (uint32_t *)c->l_rg.p; bc.cig_rel = (uint32_t *)c->cig_rel.p; bc.ncig_eff = (uint32_t *)c->ncig_eff.p; bc.rg_rel = (uint32_t *)c->rg_rel.p;
    RowsStr &so = rq.so; memset(&so, 0, sizeof(so));
    so.off[0] = (uint32_t *)c->o_qname.p; so.off[1] = (uint32_t *)c->o_cigar.p; so.off[2] = (uint32_t *)c->o_seq.p; so.off[3] = (uint32_t *)c->o_qual.p; so.off[4] = (uint32_t *)c->o_rg.p;
    for (int k = 0; k < 5; k++) so.heap[k] = (uint8_t *)arena[k]->p;
    so.alen_qual = (uint32_t *)c->alen_qual.p;
    if (c->seq_packed && (colmask & (1u << DHTS_BAM_SEQ))) { ENSURE(c, c->seq_chars, n * 4 + 64); so.seq_chars = (uint32_t *)c->seq_chars.p; }
    const size_t look_bytes = ((size_t)TR_LOOK_HDR + (size_t)ntiles * TR_LOOK_STRIDE) * 8;
    ENSURE(c, c->t_look, look_bytes + 64);
    HIPCHK(c, hipMemsetAsync((uint64_t *)c->d_res.p + 4, 0xff, 8, c->stream));     // first invalid row (none)
    HIPCHK(c, hipMemsetAsync((uint64_t *)c->d_res.p + 8, 0, 64, c->stream));       // heap totals, first record, flags
    if (!rows_fused_on()) {
        // the three passes of bam_tiles_lds.hip, queued without the host in between: the row count stays on the device (nrows < 0 = "read res[0],
        // the arrays hold -nrows - 1 rows"), the string scans run over the arrays' capacity and stop at the device's count, bam_rows_guard compares
        // the heap totals with the arenas' room before the string writer starts
        const int64_t neg = -rcap - 1;
        {
            KTimer tm(c, DHTS_K_CORE);
            hipLaunchKernelGGL(bam_tile_unpack, dim3((unsigned)ntiles), dim3(64), 0, c->stream, st, dict, ntiles, to, (const uint32_t *)c->t_rowbase.p,
                               (const uint64_t *)c->d_res.p, neg, (uint32_t *)c->rec_off.p, (uint8_t *)c->c_rgflag.p, bc, (unsigned long long *)((uint64_t *)c->d_res.p + 4), (const uint32_t *)nullptr,
                               (const uint16_t *)c->t_recs.p, (const uint64_t *)c->t_recs_first.p);
            hipLaunchKernelGGL(bam_pack_validity_dev, dim3((unsigned)((rcap + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t *)c->c_rgflag.p, (const unsigned long long *)c->d_res.p, rcap, (uint64_t *)c->c_rgvalid.p);
        }
        if (strings) {
            const uint32_t *in[5] = {bc.len_qname, bc.len_cigar, bc.len_seq, bc.len_qual, bc.len_rg};
            KTimer tm(c, DHTS_K_SCAN);
            if (run_scan(c, 5, in, so.off, nullptr, rcap, nullptr, (const unsigned long long *)c->d_res.p)) return -1;
        }
        HeapCaps hc; for (int k = 0; k < 5; k++) hc.cap[k] = (colmask & hbit[k]) ? caps.heap[k] : ~0ull;
        ENSURE(c, c->scan_total, 8 * 8);
        hipLaunchKernelGGL(bam_rows_guard, dim3(1), dim3(64), 0, c->stream, (unsigned long long *)c->d_res.p, (const uint64_t *)c->scan_total.p, hc, (const uint32_t *)c->rec_off.p, strings ? 1 : 0);
        if (strings) {
            BamStrOut bs; memset(&bs, 0, sizeof(bs));
            bs.off_qname = so.off[0]; bs.off_cigar = so.off[1]; bs.off_seq = so.off[2]; bs.off_qual = so.off[3]; bs.off_rg = so.off[4];
            bs.qname = so.heap[0]; bs.cigar = so.heap[1]; bs.seq = so.heap[2]; bs.qual = so.heap[3]; bs.rg = so.heap[4]; bs.alen_qual = so.alen_qual; bs.seq_chars = so.seq_chars;
            KTimer tm(c, DHTS_K_STRINGS);
            hipLaunchKernelGGL(bam_tile_strings, dim3((unsigned)ntiles), dim3(TS_THREADS), 0, c->stream, st, ntiles, to, (const uint32_t *)c->t_rowbase.p, (const uint64_t *)c->d_res.p,
                               (int64_t)-1, (int64_t)-1, (const uint32_t *)c->rec_off.p, (const uint32_t *)nullptr, bc, bs, colmask);
        }
        HIPCHK(c, hipGetLastError());
        return 0;
    }
    HIPCHK(c, hipMemsetAsync(c->t_look.p, 0, strings ? look_bytes : (size_t)TR_LOOK_HDR * 8, c->stream));     // ticket counter; every tile's look-back record EMPTY
    {
        KTimer tm(c, DHTS_K_CORE);
        // persistent: as many one-wave workgroups as the device holds (tiles are taken by ticket, so any grid size is correct)
        if (c->rows_slots == 0) {
            int per_cu = 0, cus = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)bam_tile_rows, 64, 0) != hipSuccess || per_cu <= 0) per_cu = 8;
            if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || cus <= 0) cus = 256;
            static const int env_wg = getenv("DHTS_ROWS_WG_PER_CU") ? atoi(getenv("DHTS_ROWS_WG_PER_CU")) : 0;
            c->rows_slots = (int64_t)(env_wg > 0 ? env_wg : per_cu) * cus;
        }
        const int64_t grid = ntiles < c->rows_slots ? ntiles : c->rows_slots;
        hipLaunchKernelGGL(bam_tile_rows, dim3((unsigned)grid), dim3(64), 0, c->stream, st, dict, ntiles, to, (const uint32_t *)c->t_rowbase.p, (unsigned long long *)c->d_res.p, caps,
                           (uint32_t *)c->rec_off.p, (uint8_t *)c->c_rgflag.p, bc, so, colmask, strings ? (1 | rows_exp()) : 0, (const uint16_t *)c->t_recs.p, (const uint64_t *)c->t_recs_first.p,
                           (unsigned long long *)c->t_look.p);
        hipLaunchKernelGGL(bam_pack_validity_dev, dim3((unsigned)((rcap + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t *)c->c_rgflag.p, (const unsigned long long *)c->d_res.p, rcap, (uint64_t *)c->c_rgvalid.p);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

static int bam_next_batch_one(dhts_ctx *c, int64_t max_blocks, uint32_t colmask, dhts_bam_batch *out);
static int sam_text_records(dhts_ctx *c, const Batch &B, const uint8_t *&enc, uint64_t &enc_len, int64_t &nrec, uint64_t &carry_start, bool &rejected, uint64_t &t0);
static int fastq_text_records(dhts_ctx *c, const Batch &B, const uint8_t *&enc, uint64_t &enc_len, int64_t &nrec, uint64_t &carry_start, bool &rejected, uint64_t &t0);
static int fastq_record_start(dhts_ctx *c, int64_t i, uint64_t &off);
int dhts_bam_next_batch(dhts_ctx *c, int64_t max_blocks, uint32_t colmask, dhts_bam_batch *out) {
    if (!c || !out) return -1;
    for (;;) {
        c->last_batch_rows = -1;
        if (bam_next_batch_one(c, max_blocks, colmask, out)) return -1;
        c->last_batch_rows = out->n_rows; c->last_batch_first = out->first_rec_uoff;
        // a region query with several index windows: the end of one window is the start of the next, not the end of the scan
        if (next_window(c, out->status) && out->n_rows == 0) continue;
        return 0;
    }
}
static int bam_next_batch_one(dhts_ctx *c, int64_t max_blocks, uint32_t colmask, dhts_bam_batch *out) {
    if (!c || !out) return -1;
    memset(out, 0, sizeof(*out));
    if (!c->bam_open) return fail(c, "dhts_bam_open not called");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->stream_done) { out->status = 1; return 0; }
    // Host round trips of one batch (the plain case: no region filter, no shard cut inside the batch): (1) behind the tile pass -- rows,
    // carry position, the repair rounds' verdict and the inflate's block status in ONE copy; (2) behind the string scan -- heap sizes,
    // first invalid row, first record offset; (3) the end of the batch.  The inflate, the tile scan, two repair rounds and the finalize
    // pass are queued back to back; so are unpack, validity packing and the scans.
    Batch B;
    if (batch_begin(c, max_blocks, B, !c->sam_text)) return -1;
    const bool sharded_tail = B.sharded_tail;
    bool final_batch = B.final_batch;
    uint8_t *u = B.u; uint64_t ulen = B.ulen; uint64_t out_base = B.out_base;
    // SAM text (dhts_sam_scan.inc): the batch's complete lines become BAM records; the record stage below runs over them, every one complete
    const uint8_t *sam_enc = nullptr; int64_t sam_nrec = 0; uint64_t sam_carry = 0, sam_t0 = 0; bool sam_rej = false;
    if (c->sam_text) {
        if (c->fastq ? fastq_text_records(c, B, sam_enc, ulen, sam_nrec, sam_carry, sam_rej, sam_t0) : sam_text_records(c, B, sam_enc, ulen, sam_nrec, sam_carry, sam_rej, sam_t0)) return -1;
        if (sam_nrec == 0) { out->end_uoff = out_base + sam_carry; out->first_rec_uoff = NONE64; return batch_end(c, B, sam_carry, sam_rej, false, &out->status); }
        u = (uint8_t *)sam_enc; final_batch = true;
    }
    BamStream st; st.u = u; st.ulen = ulen; st.n_ref = (int32_t)c->ref_name.size(); st.final_batch = final_batch ? 1 : 0; st.seq_packed = c->seq_packed ? 1 : 0;
    st.want_rg = (colmask & ((1u << DHTS_BAM_READ_GROUP_ID) | (1u << DHTS_BAM_SAMPLE_ID))) ? 1 : 0;
    c->last_stream = st;

    // ---- tiles ----
    int64_t ntiles = (int64_t)((ulen + TILE_BYTES - 1) / TILE_BYTES); if (ntiles < 1) ntiles = 1;
    ENSURE(c, c->t_first, ntiles * 8); ENSURE(c, c->t_end, ntiles * 8); ENSURE(c, c->t_count, ntiles * 4); ENSURE(c, c->t_err, ntiles * 4);
    ENSURE(c, c->t_rowbase, ntiles * 4 + 16); ENSURE(c, c->d_res, 256); ENSURE(c, c->d_nfixed, 64);
    ENSURE(c, c->t_recs, (size_t)ntiles * TL_RECS * 2 + 64); ENSURE(c, c->t_recs_first, ntiles * 8 + 64);
    ENSURE(c, c->t2_first, ntiles * 8); ENSURE(c, c->t2_end, ntiles * 8); ENSURE(c, c->t2_count, ntiles * 4); ENSURE(c, c->t2_err, ntiles * 4);
    TileOut to; to.first = (uint64_t *)c->t_first.p; to.end_next = (uint64_t *)c->t_end.p; to.count = (uint32_t *)c->t_count.p; to.err = (int32_t *)c->t_err.p;
    TileOut to2; to2.first = (uint64_t *)c->t2_first.p; to2.end_next = (uint64_t *)c->t2_end.p; to2.count = (uint32_t *)c->t2_count.p; to2.err = (int32_t *)c->t2_err.p;
    uint64_t start0;
    if (c->sam_text) start0 = 0;                               // (the encoded records of a SAM batch)
    else if (c->first_batch) start0 = (c->shard_rank == 0) ? c->scan_first_uoff - out_base : NONE64;   // later shards speculate their first record
    else start0 = 0;                                           // the carry begins on a record boundary
    if (!c->sam_text && c->first_batch && c->shard_rank == 0 && c->scan_first_uoff < out_base) return fail(c, "internal: header beyond first batch");
    uint64_t res[4] = {0, 0, 0, 0};
    uint64_t first0 = NONE64;
    // A shard that starts mid-stream speculates its first record.  If the chain that grows from the candidate breaks inside this
    // batch, the candidate was a false start (or the file is damaged): resume the search behind it.  The true first record always
    // survives.  Every record start on a failed candidate's chain would, taken as a candidate, walk the same hops to the same break: the
    // retries pass over them (bam_spec_next with the chains' record starts as skip lists), so a failed chain costs ONE tile pass however long
    // it is -- a chain of decoys in a valid file, or the true chain of a damaged shard.  The search ends when a candidate stands or none is
    // left; then the damage is real and the first attempt's result stands.  It does not end at a count of retries, which a valid file with
    // enough decoys in front of the record would reach.
    const bool speculative = (start0 == NONE64);
    // The rows are queued behind the tile pass WITHOUT a host round trip where nothing in between needs the host: no speculated shard
    // start, no region filter (its row map comes from a scan over all rows), no shard end inside the batch (rows are cut on the host).
    // Row arrays and string arenas are sized from what the previous batches needed and guarded on the device; one copy brings back the tile
    // pass's verdicts, the inflate's block status, the first invalid row, the heap sizes and the overflow flags: one round trip per batch.
    const bool fused = !speculative && !(c->rg_active && !c->rg_all) && !(sharded_tail && out_base + ulen > c->h_uoff[c->shard_b1]) && rows_deferred_on();
    unsigned long long hres[16] = {0}; RowsQueued rq;
    uint64_t spec_from = 0, en0 = NONE64; int spec_tries = 0; bool restoring = false;
    SpecSkip sk; memset(&sk, 0, sizeof(sk));
    int status_attempt = 0;
    for (;;) {
        uint64_t start_eff = start0;
        if (speculative && !restoring && spec_tries > 0) {
            // a retry: the next candidate behind the failed one that is no member of a failed chain
            uint64_t *d_cand = (uint64_t *)c->d_nfixed.p + 2, cand = NONE64;
            hipLaunchKernelGGL(bam_spec_next, dim3(1), dim3(64), 0, c->stream, st, spec_from, sk, d_cand);
            HIPCHK(c, hipMemcpyAsync(&cand, d_cand, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (cand == NONE64) { spec_from = 0; restoring = true; c->tile_stats[DHTS_TS_GAVE_UP]++; }      // none left: the first attempt is made again and stands
            else { start_eff = cand; c->tile_stats[DHTS_TS_RETRIES]++; }
        }
        to.first = (uint64_t *)c->t_first.p; to.end_next = (uint64_t *)c->t_end.p; to.count = (uint32_t *)c->t_count.p; to.err = (int32_t *)c->t_err.p;
        to2.first = (uint64_t *)c->t2_first.p; to2.end_next = (uint64_t *)c->t2_end.p; to2.count = (uint32_t *)c->t2_count.p; to2.err = (int32_t *)c->t2_err.p;
        uint32_t nfh[2] = {0, 0}, bst[4] = {NONE32, 0, NONE32, 0};
        {
            KTimer tm(c, DHTS_K_TILES);
            tile_scan_launch(c, tile_scan_lanes_on(ntiles), st, start_eff, ntiles, to, (uint16_t *)c->t_recs.p, (uint64_t *)c->t_recs_first.p, spec_from);
            // two repair rounds are queued unconditionally (a 30x BAM converges in two; a round that finds nothing to repair copies the table)
            uint32_t *nf = (uint32_t *)c->d_nfixed.p;
            (void)hipMemsetAsync(nf, 0, 8, c->stream);
            for (int r = 0; r < 2; r++) {
                hipLaunchKernelGGL(bam_tile_fix, dim3((unsigned)((ntiles + 255) / 256)), dim3(256), 0, c->stream, st, TILE_BYTES, ntiles, to, to2, nf + r);
                TileOut tmp = to; to = to2; to2 = tmp;             // the round's output is the current table
            }
            hipLaunchKernelGGL(bam_tile_finalize, dim3(1), dim3(1024), 0, c->stream, ntiles, to, (uint32_t *)c->t_rowbase.p, (uint64_t *)c->d_res.p);
        }
        // the plain case goes on without the host: the row pass is queued behind the tile pass and ONE copy brings everything back
        if (fused) { if (rows_queue(c, st, ntiles, to, colmask, rq)) return -1; HIPCHK(c, hipMemcpyAsync(hres, c->d_res.p, 128, hipMemcpyDeviceToHost, c->stream)); }
        HIPCHK(c, hipMemcpyAsync(res, c->d_res.p, 32, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&first0, to.first, 8, hipMemcpyDeviceToHost, c->stream));
        if (speculative) HIPCHK(c, hipMemcpyAsync(&en0, to.end_next, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(nfh, c->d_nfixed.p, 8, hipMemcpyDeviceToHost, c->stream));
        if (B.status_pending) HIPCHK(c, hipMemcpyAsync(bst, c->d_bstat.p, 16, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (B.status_pending) {
            const int rs = batch_status_resolve(c, B, bst, status_attempt++);
            if (rs < 0) return -1;
            if (rs > 0) {           // the stream is shorter than assumed (or was inflated again): the tile pass starts over
                ulen = B.ulen; final_batch = B.final_batch;
                // (a scratch retry may have moved the block table: the batch can be longer than first assumed and lie elsewhere)
                u = B.u; out_base = B.out_base; st.u = u;
                if (c->first_batch && c->shard_rank == 0) start0 = c->scan_first_uoff - out_base;
                st.ulen = ulen; st.final_batch = final_batch ? 1 : 0; c->last_stream = st;
                ntiles = (int64_t)((ulen + TILE_BYTES - 1) / TILE_BYTES); if (ntiles < 1) ntiles = 1;
                ENSURE(c, c->t_first, ntiles * 8); ENSURE(c, c->t_end, ntiles * 8); ENSURE(c, c->t_count, ntiles * 4); ENSURE(c, c->t_err, ntiles * 4);
                ENSURE(c, c->t_rowbase, ntiles * 4 + 16);
                ENSURE(c, c->t_recs, (size_t)ntiles * TL_RECS * 2 + 64); ENSURE(c, c->t_recs_first, ntiles * 8 + 64);
                ENSURE(c, c->t2_first, ntiles * 8); ENSURE(c, c->t2_end, ntiles * 8); ENSURE(c, c->t2_count, ntiles * 4); ENSURE(c, c->t2_err, ntiles * 4);
                spec_from = 0; spec_tries = 0; restoring = false; sk.lists = 0;
                continue;
            }
        }
        if (g_debug) fprintf(stderr, "[dhts] tiles=%lld nfixed=%u,%u\n", (long long)ntiles, nfh[0], nfh[1]);
        c->tile_stats[DHTS_TS_REPAIRED] += (uint64_t)nfh[0] + nfh[1]; c->tile_stats[DHTS_TS_ROUNDS] += (nfh[0] != 0) + (nfh[1] != 0);
        if (nfh[1] != 0) {
            // the second round still repaired tiles: go on round by round, then finalize again
            KTimer tm(c, DHTS_K_TILES);
            int rounds = 2; bool seq_fallback = false;
            for (;;) {
                (void)hipMemsetAsync(c->d_nfixed.p, 0, 4, c->stream);
                hipLaunchKernelGGL(bam_tile_fix, dim3((unsigned)((ntiles + 255) / 256)), dim3(256), 0, c->stream, st, TILE_BYTES, ntiles, to, to2, (uint32_t *)c->d_nfixed.p);
                { TileOut tmp = to; to = to2; to2 = tmp; }
                uint32_t nfixed = 0;
                HIPCHK(c, hipMemcpyAsync(&nfixed, c->d_nfixed.p, 4, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                if (g_debug) fprintf(stderr, "[dhts] tiles=%lld round=%d nfixed=%u\n", (long long)ntiles, rounds, nfixed);
                if (nfixed == 0) break;
                c->tile_stats[DHTS_TS_REPAIRED] += nfixed; c->tile_stats[DHTS_TS_ROUNDS]++;
                if (++rounds > 256) {
                    (void)hipMemsetAsync(c->d_nfixed.p, 0, 4, c->stream);
                    hipLaunchKernelGGL(bam_tile_fix_seq, dim3(1), dim3(1), 0, c->stream, st, TILE_BYTES, ntiles, to, (uint32_t *)c->d_nfixed.p);
                    seq_fallback = true; break;
                }
            }
            hipLaunchKernelGGL(bam_tile_finalize, dim3(1), dim3(1024), 0, c->stream, ntiles, to, (uint32_t *)c->t_rowbase.p, (uint64_t *)c->d_res.p);
            uint32_t nseq = 0;
            if (seq_fallback) HIPCHK(c, hipMemcpyAsync(&nseq, c->d_nfixed.p, 4, hipMemcpyDeviceToHost, c->stream));
            if (speculative) HIPCHK(c, hipMemcpyAsync(&en0, to.end_next, 8, hipMemcpyDeviceToHost, c->stream));
            if (fused) { if (rows_queue(c, st, ntiles, to, colmask, rq)) return -1; HIPCHK(c, hipMemcpyAsync(hres, c->d_res.p, 128, hipMemcpyDeviceToHost, c->stream)); }
            HIPCHK(c, hipMemcpyAsync(res, c->d_res.p, 32, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(&first0, to.first, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (seq_fallback) { c->tile_stats[DHTS_TS_REPAIRED] += nseq; c->tile_stats[DHTS_TS_SEQ]++; }
        }
        if (!speculative || restoring) break;
        // the candidate: tile 0 looks for it through the whole batch, so it may lie behind tile 0 (a long record runs across the shard's
        // first tiles); tile 0 then holds no record and its chain exit IS the candidate
        if (first0 == NONE64) first0 = en0;
        if (start_eff != NONE64) first0 = start_eff;
        bool false_start = res[2] != 0 && first0 != NONE64;
        int64_t nskip = (int64_t)res[0];                        // the chain broke: every record on it leads to the same break
        if (false_start && nskip > 0) {
            ENSURE(c, c->rec_off, (size_t)nskip * 4 + 16);
            hipLaunchKernelGGL(bam_tile_offsets, dim3((unsigned)((ntiles + 255) / 256)), dim3(256), 0, c->stream, st, TILE_BYTES, ntiles, to, (const uint32_t *)c->t_rowbase.p,
                               (const uint64_t *)c->d_res.p, (uint32_t *)c->rec_off.p);
        }
        if (!false_start && first0 != NONE64 && (int64_t)res[0] > 0) {
            // the chain holds: do its "records" also pass bam_read1's full validation?  (only speculated shard starts pay for this pass)
            const int64_t nr = (int64_t)res[0];
            unsigned long long bad0 = ~0ull;
            ENSURE(c, c->rec_off, (size_t)nr * 4 + 16);
            HIPCHK(c, hipMemsetAsync((uint64_t *)c->d_res.p + 4, 0xff, 8, c->stream));
            hipLaunchKernelGGL(bam_tile_offsets, dim3((unsigned)((ntiles + 255) / 256)), dim3(256), 0, c->stream, st, TILE_BYTES, ntiles, to, (const uint32_t *)c->t_rowbase.p,
                               (const uint64_t *)c->d_res.p, (uint32_t *)c->rec_off.p);
            hipLaunchKernelGGL(bam_validate_rows, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, c->stream, st, (const uint32_t *)c->rec_off.p, nr, (unsigned long long *)((uint64_t *)c->d_res.p + 4));
            HIPCHK(c, hipMemcpyAsync(&bad0, (uint64_t *)c->d_res.p + 4, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            false_start = bad0 < (unsigned long long)nr;
            if (false_start) { nskip = (int64_t)bad0 + 1; c->tile_stats[DHTS_TS_VALIDATE]++; }      // the chain holds up to a record that is refused: the records up to it lead there
        }
        if (!false_start) break;
        if (nskip > 0 && sk.lists < SPEC_LISTS) {            // (with every list in use the later chains' members cost a tile pass each; nothing else changes)
            DevBuf &sb = c->spec_skip[sk.lists];
            ENSURE(c, sb, (size_t)nskip * 4 + 16);
            HIPCHK(c, hipMemcpyAsync(sb.p, c->rec_off.p, (size_t)nskip * 4, hipMemcpyDeviceToDevice, c->stream));
            sk.off[sk.lists] = (const uint32_t *)sb.p; sk.n[sk.lists] = (uint32_t)nskip; sk.lists++;
        }
        spec_from = first0 + 1; spec_tries++;
    }
    int64_t nrows = (int64_t)res[0]; uint64_t carry_start = res[1]; bool rec_err = res[2] != 0;
    if (carry_start == NONE64) carry_start = ulen;             // nothing recognisable in this batch

    // sharding: rows belong to this shard iff their record STARTS before the shard's end in the inflated stream
    uint64_t shard_end_u = sharded_tail ? c->h_uoff[c->shard_b1] : ~0ull;
    // ---- phase B of the NEXT batch, concurrent with the rest of this one (DHTS_PREFETCH=1; off by default since round 3) ----
    // The carry (where this batch's last complete record ends) is known now, so the next batch's destination is too.  Only the
    // plain case is prefetched: the stream goes on inside this shard, phase A already covers the blocks, nothing can cut this
    // batch short from here on except a bad row (then batch_end discards the prefetch).
    // Measured on the 92 M-record bench file: with the prefetch 173.0-174.5 ms per step, without 176.2 ms -- phase B and the record stage
    // are both bound by instruction issue, so running them side by side only stretches both (bgzf_lz_resolve 4.8 ms per launch beside
    // the record stage, 2.8 ms alone; bam_tile_unpack 1.35 / 0.88 ms), and the 1 % it gains is not worth a second stream, a second set of
    // buffers in flight and per-kernel times that no longer say what a kernel costs.
    {
        const bool no_pf = !(getenv("DHTS_PREFETCH") && atoi(getenv("DHTS_PREFETCH")) != 0) || getenv("DHTS_NO_PREFETCH") != nullptr;
        int64_t mb = max_blocks <= 0 ? 16384 : (max_blocks > 24576 ? 24576 : max_blocks);
        const int64_t nb0 = B.b0 + B.nb;
        int64_t nbn = c->shard_b1 - nb0; if (nbn > mb) nbn = mb;
        const bool plain = !no_pf && !c->sam_text && !rec_err && !B.blk_err && !B.last_of_stream && !B.in_halo && nbn > 0 && !(sharded_tail && out_base + ulen > shard_end_u) &&
                           (!inflate_split() || (nb0 >= c->huff_b0 && nb0 + nbn <= c->huff_b0 + c->huff_nb)) && !c->pf.valid;
        if (plain) {
            const uint64_t tail = ulen - carry_start, ulen_n = tail + (c->h_uoff[nb0 + nbn] - c->h_uoff[nb0]);
            bool ok = ulen_n + PAD_BYTES < (1ull << 32);
            DevBuf &nx = c->ubuf[c->ucur ^ 1];
            if (ok && nx.cap < ulen_n + PAD_BYTES && nx.ensure(ulen_n + PAD_BYTES)) ok = false;
            if (ok) {
                uint8_t *un = (uint8_t *)nx.p;
                if (tail) HIPCHK(c, hipMemcpyAsync(un, u + carry_start, tail, hipMemcpyDeviceToDevice, c->stream_b));
                if (inflate_split() ? launch_lz(c, nb0, nbn, un, c->h_uoff[nb0] - tail, c->stream_b) : launch_fused(c, nb0, nbn, un, c->h_uoff[nb0] - tail, c->stream_b, 1)) return -1;
                HIPCHK(c, hipMemsetAsync(un + ulen_n, 0, PAD_BYTES, c->stream_b));
                HIPCHK(c, hipEventRecord(c->pf_done, c->stream_b));
                c->pf.valid = true; c->pf.b0 = nb0; c->pf.nb = nbn; c->pf.carry = tail; c->pf.ucur = c->ucur ^ 1;
            }
        }
    }
    bool shard_finished = false;

    // ---- rows ----
    BamCols bc; memset(&bc, 0, sizeof(bc));
    const int64_t nrows_scan = nrows;                          // rows the tile pass counted (before the region filter / a bad row / the shard cut)
    const uint32_t *row_map_s = nullptr;
    uint32_t first_rec_rel = 0; bool have_first_rec = false;   // offset of the batch's first row (read with the heap sizes when there are any)
    if (fused) {
        // the row pass ran behind the tile pass: its verdicts arrived with the tile pass's
        for (int attempt = 0; ; attempt++) {
            if (hres[14] & TR_F_TIMEOUT) return fail(c, "internal: look-back wait expired in bam_tile_rows");
            if (!(hres[14] & (TR_F_ROWS | TR_F_HEAP))) break;
            if (attempt > 1) return fail(c, "internal: row pass overflow after regrowth");
            // the arenas sized from the previous batch were too small: the pass has told how much it needs; grow and repeat it
            c->rows_hint = nrows + nrows / 8 + 1024;
            for (int k = 0; k < 5; k++) if (hres[8 + k] + hres[8 + k] / 8 > c->heap_hint[k]) c->heap_hint[k] = hres[8 + k] + hres[8 + k] / 8 + 4096;
            if (g_debug) fprintf(stderr, "[dhts] row pass repeated: rows %lld flags %llu\n", (long long)nrows, hres[14]);
            if (rows_queue(c, st, ntiles, to, colmask, rq)) return -1;
            HIPCHK(c, hipMemcpyAsync(hres, c->d_res.p, 128, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        bc = rq.bc;
        const uint32_t str_cols = (1u << DHTS_BAM_QNAME) | (1u << DHTS_BAM_CIGAR) | (1u << DHTS_BAM_SEQ) | (1u << DHTS_BAM_QUAL) | (1u << DHTS_BAM_READ_GROUP_ID);
        const bool strings = (colmask & str_cols) != 0;
        uint64_t tot[5] = {0, 0, 0, 0, 0};
        if (strings) for (int k = 0; k < 5; k++) tot[k] = hres[8 + k];
        first_rec_rel = (uint32_t)hres[13]; have_first_rec = true;
        if (nrows > 0) {
            // hints for the next batch: what this one needed plus an eighth
            if (nrows + nrows / 8 > c->rows_hint) c->rows_hint = nrows + nrows / 8 + 1024;
            for (int k = 0; k < 5; k++) if (tot[k] + tot[k] / 8 > c->heap_hint[k]) c->heap_hint[k] = tot[k] + tot[k] / 8 + 4096;
        }
        const unsigned long long bad = hres[4];
        if (bad < (unsigned long long)nrows) {
            // rare: a row failed bam_read1's full validation: the scan ends in front of it.  The offsets of the rows before it stand (exclusive
            // sums); the heap sizes and the validity words are made again for the shorter table
            rec_err = true; nrows = (int64_t)bad;
            { uint32_t ro_bad = 0; HIPCHK(c, hipMemcpy(&ro_bad, (const uint32_t *)c->rec_off.p + bad, 4, hipMemcpyDeviceToHost)); carry_start = ro_bad; }      // the stream ends in front of the invalid record
            if (nrows > 0) {
                hipLaunchKernelGGL(bam_pack_validity, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t *)c->c_rgflag.p, nrows, (uint64_t *)c->c_rgvalid.p);
                if (strings) {
                    uint32_t t32[5] = {0, 0, 0, 0, 0};
                    for (int k = 0; k < 5; k++) HIPCHK(c, hipMemcpyAsync(&t32[k], rq.so.off[k] + nrows, 4, hipMemcpyDeviceToHost, c->stream));
                    HIPCHK(c, hipStreamSynchronize(c->stream));
                    for (int k = 0; k < 5; k++) tot[k] = t32[k];
                } else HIPCHK(c, hipStreamSynchronize(c->stream));
            }
        }
        if (nrows > 0) {
            const RowsStr &so = rq.so;
            out->flag = bc.flag; out->pos = bc.pos; out->mapq = bc.mapq; out->pnext = bc.pnext; out->tlen = bc.tlen; out->tid = bc.tid; out->mtid = bc.mtid;
            out->rg_idx = bc.rg_idx; out->rg_valid = bc.rg_valid;
            out->qname = {so.off[0], bc.len_qname, strings ? so.heap[0] : nullptr, tot[0]};
            out->cigar = {so.off[1], bc.len_cigar, strings ? so.heap[1] : nullptr, tot[1]};
            out->seq = {so.off[2], so.seq_chars ? so.seq_chars : bc.len_seq, strings ? so.heap[2] : nullptr, tot[2]};
            out->seq_packed = so.seq_chars ? 1 : 0;
            out->qual = {so.off[3], so.alen_qual, strings ? so.heap[3] : nullptr, tot[3]};
            out->rg = {so.off[4], bc.len_rg, strings ? so.heap[4] : nullptr, tot[4]};
        }
    } else if (nrows > 0) {
        size_t n = (size_t)nrows;
        ENSURE(c, c->rec_off, n * 4 + 16); ENSURE(c, c->c_rgflag, n + 64);
        ENSURE(c, c->c_flag, n * 2 + 16); ENSURE(c, c->c_pos, n * 8); ENSURE(c, c->c_mapq, n * 4); ENSURE(c, c->c_pnext, n * 8); ENSURE(c, c->c_tlen, n * 8);
        ENSURE(c, c->c_tid, n * 4); ENSURE(c, c->c_mtid, n * 4); ENSURE(c, c->c_rgidx, n * 4); ENSURE(c, c->c_rgvalid, (n / 64 + 2) * 8);
        ENSURE(c, c->l_qname, n * 4 + 16); ENSURE(c, c->l_cigar, n * 4 + 16); ENSURE(c, c->l_seq, n * 4 + 16); ENSURE(c, c->l_qual, n * 4 + 16); ENSURE(c, c->l_rg, n * 4 + 16);
        ENSURE(c, c->cig_rel, n * 4); ENSURE(c, c->ncig_eff, n * 4); ENSURE(c, c->rg_rel, n * 4); ENSURE(c, c->alen_qual, n * 4);
        ENSURE(c, c->o_qname, (n + 1) * 4 + 16); ENSURE(c, c->o_cigar, (n + 1) * 4 + 16); ENSURE(c, c->o_seq, (n + 1) * 4 + 16); ENSURE(c, c->o_qual, (n + 1) * 4 + 16); ENSURE(c, c->o_rg, (n + 1) * 4 + 16);
        BamDict dict; dict.n_rg = (int32_t)c->rg_id.size(); dict.rg_off = (const uint32_t *)c->d_rg_off.p; dict.rg_bytes = (const uint8_t *)c->d_rg_bytes.p; { size_t tb_ = 0; for (auto &id_ : c->rg_id) tb_ += id_.size(); dict.n_bytes = (int32_t)tb_; }
        bc.flag = (uint16_t *)c->c_flag.p; bc.pos = (int64_t *)c->c_pos.p; bc.mapq = (int32_t *)c->c_mapq.p; bc.pnext = (int64_t *)c->c_pnext.p;
        bc.tlen = (int64_t *)c->c_tlen.p; bc.tid = (int32_t *)c->c_tid.p; bc.mtid = (int32_t *)c->c_mtid.p; bc.rg_idx = (int32_t *)c->c_rgidx.p;
        bc.rg_valid = (uint64_t *)c->c_rgvalid.p; bc.len_qname = (uint32_t *)c->l_qname.p; bc.len_cigar = (uint32_t *)c->l_cigar.p; bc.len_seq = (uint32_t *)c->l_seq.p;
        bc.len_qual = (uint32_t *)c->l_qual.p; bc.len_rg = (uint32_t *)c->l_rg.p; bc.cig_rel = (uint32_t *)c->cig_rel.p; bc.ncig_eff = (uint32_t *)c->ncig_eff.p; bc.rg_rel = (uint32_t *)c->rg_rel.p;
        HIPCHK(c, hipMemsetAsync((uint64_t *)c->d_res.p + 4, 0xff, 8, c->stream));     // first invalid row (none)
        const bool filtered = c->rg_active && !c->rg_all;
        const uint32_t *row_map = nullptr;
        uint64_t kept_total = (uint64_t)nrows;
        if (filtered) {
            // region predicate per record, then a scan turns the keep flags into compacted row ids
            ENSURE(c, c->c_keep, n * 4 + 16); ENSURE(c, c->c_rowmap, (n + 1) * 4 + 16);
            RegionDev rg; rg.beg = (const int64_t *)c->d_rg_beg.p; rg.end = (const int64_t *)c->d_rg_end.p; rg.tid_first = (const uint32_t *)c->d_rg_first.p;
            rg.n_ref = (int32_t)c->ref_name.size(); rg.all = 0; rg.nocoor = c->rg_nocoor ? 1 : 0; rg.pad = 0;
            {
                KTimer tm(c, DHTS_K_CORE);
                hipLaunchKernelGGL(bam_tile_offsets, dim3((unsigned)((ntiles + 255) / 256)), dim3(256), 0, c->stream, st, TILE_BYTES, ntiles, to, (const uint32_t *)c->t_rowbase.p,
                                   (const uint64_t *)c->d_res.p, (uint32_t *)c->rec_off.p);
                const uint64_t end_rel = c->scan_end_uoff == ~0ull ? ~0ull : (c->scan_end_uoff > out_base ? c->scan_end_uoff - out_base : 0ull);
                hipLaunchKernelGGL(bam_region_keep, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, c->stream, st, rg, (const uint32_t *)c->rec_off.p, nrows, (uint32_t *)c->c_keep.p, end_rel);
            }
            const uint32_t *kin[1] = {(const uint32_t *)c->c_keep.p}; uint32_t *kout[1] = {(uint32_t *)c->c_rowmap.p};
            { KTimer tm(c, DHTS_K_SCAN); if (run_scan(c, 1, kin, kout, nullptr, nrows, &kept_total)) return -1; }
            row_map = (const uint32_t *)c->c_rowmap.p; row_map_s = row_map;
        }
        {
            KTimer tm(c, DHTS_K_CORE);
            hipLaunchKernelGGL(bam_tile_unpack, dim3((unsigned)ntiles), dim3(64), 0, c->stream, st, dict, ntiles, to, (const uint32_t *)c->t_rowbase.p,
                               (const uint64_t *)c->d_res.p, nrows, (uint32_t *)c->rec_off.p, (uint8_t *)c->c_rgflag.p, bc, (unsigned long long *)((uint64_t *)c->d_res.p + 4), row_map,
                               (const uint16_t *)c->t_recs.p, (const uint64_t *)c->t_recs_first.p);
        }
        // the first row that fails bam_read1's validation ends the scan there (rows before it are kept).  In the plain case the verdict is
        // read together with the heap sizes below; a region filter or a shard cut inside the batch need it now.
        bool bad_pending = true;
        unsigned long long bad = ~0ull;
        const bool shard_cut = !filtered && sharded_tail && out_base + ulen > shard_end_u;
        auto apply_bad = [&]() -> int {
            if (bad < (unsigned long long)nrows) {
                rec_err = true;
                if (filtered) { uint32_t kb = 0; HIPCHK(c, hipMemcpy(&kb, (const uint32_t *)c->c_rowmap.p + bad, 4, hipMemcpyDeviceToHost)); kept_total = kb; }
                // the stream ends IN FRONT of the invalid record (the tile scan's walk hops over it: it tests block_size only)
                { uint32_t ro_bad = 0; HIPCHK(c, hipMemcpy(&ro_bad, (const uint32_t *)c->rec_off.p + bad, 4, hipMemcpyDeviceToHost)); carry_start = ro_bad; }
                nrows = (int64_t)bad;
            }
            return 0;
        };
        if (filtered || shard_cut) {
            HIPCHK(c, hipMemcpyAsync(&bad, (uint64_t *)c->d_res.p + 4, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            bad_pending = false;
            if (!shard_cut && apply_bad()) return -1;          // (a shard cut decides below whose row the invalid one is)
        }
        if (filtered) {
            if (sharded_tail && out_base + ulen > shard_end_u && carry_start >= shard_end_u - out_base) shard_finished = true;   // rows past the index window never match
            // the window's exact end lies inside this batch: the window is done, whatever follows it (with only the windows resident the
            // last one ends in the last resident block, and the records behind the cut are not a truncated tail)
            if (c->scan_end_uoff != ~0ull && out_base + ulen >= c->scan_end_uoff && !rec_err) shard_finished = true;
            nrows = (int64_t)kept_total;
        } else if (nrows > 0 && shard_cut) {
            // drop rows whose record starts at/after the shard end (they belong to the next shard): binary search on rec_off.  An invalid
            // row or a broken chain BEHIND the shard end is the next shard's to report (its blocks are read here only as a halo: a damaged
            // block there cuts the stream and makes the record that runs into it look truncated): this shard then ends well.
            std::vector<uint32_t> ro(nrows);
            HIPCHK(c, hipMemcpyAsync(ro.data(), c->rec_off.p, nrows * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            uint64_t lim = shard_end_u - out_base;
            int64_t lo = 0, hi = nrows;
            while (lo < hi) { int64_t mid = (lo + hi) / 2; if (ro[mid] < lim) lo = mid + 1; else hi = mid; }
            const int64_t nvalid = bad < (unsigned long long)nrows ? (int64_t)bad : nrows;      // rows in front of the first invalid one
            if (nvalid < lo) { rec_err = true; nrows = nvalid; carry_start = ro[nvalid]; }        // a row of THIS shard is invalid: the scan ends in front of it
            else if (lo < nrows) { carry_start = ro[lo]; nrows = lo; shard_finished = true; rec_err = false; }
            else if (carry_start >= lim) { shard_finished = true; rec_err = false; }
        }
        if (nrows > 0) {
            {
                KTimer tm(c, DHTS_K_CORE);
                hipLaunchKernelGGL(bam_pack_validity, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t *)c->c_rgflag.p, nrows, (uint64_t *)c->c_rgvalid.p);
            }
            uint32_t *o32[5] = {(uint32_t *)c->o_qname.p, (uint32_t *)c->o_cigar.p, (uint32_t *)c->o_seq.p, (uint32_t *)c->o_qual.p, (uint32_t *)c->o_rg.p};
            uint64_t tot[5] = {0, 0, 0, 0, 0};
            BamStrOut so; memset(&so, 0, sizeof(so));
            so.off_qname = o32[0]; so.off_cigar = o32[1]; so.off_seq = o32[2]; so.off_qual = o32[3]; so.off_rg = o32[4]; so.alen_qual = (uint32_t *)c->alen_qual.p;
            if (c->seq_packed && (colmask & (1u << DHTS_BAM_SEQ))) { ENSURE(c, c->seq_chars, (size_t)nrows * 4 + 64); so.seq_chars = (uint32_t *)c->seq_chars.p; }
            const uint32_t str_cols = (1u << DHTS_BAM_QNAME) | (1u << DHTS_BAM_CIGAR) | (1u << DHTS_BAM_SEQ) | (1u << DHTS_BAM_QUAL) | (1u << DHTS_BAM_READ_GROUP_ID);
            const bool strings = (colmask & str_cols) != 0;     // projection pushdown: with no string column projected the whole string pass is skipped
            if (strings) {
                const uint32_t *in[5] = {bc.len_qname, bc.len_cigar, bc.len_seq, bc.len_qual, bc.len_rg};
                KTimer tm(c, DHTS_K_SCAN);
                if (run_scan(c, 5, in, o32, nullptr, nrows, nullptr)) return -1;
                HIPCHK(c, hipMemcpyAsync(tot, c->scan_total.p, 40, hipMemcpyDeviceToHost, c->stream));
            }
            if (strings || bad_pending) {
                // ONE round trip: heap sizes, the first invalid row and the first record's offset
                if (bad_pending) HIPCHK(c, hipMemcpyAsync(&bad, (uint64_t *)c->d_res.p + 4, 8, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipMemcpyAsync(&first_rec_rel, c->rec_off.p, 4, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                have_first_rec = true;
                if (bad_pending) {
                    bad_pending = false;
                    const int64_t before = nrows;
                    if (apply_bad()) return -1;
                    if (nrows != before && nrows > 0) {
                        // rare: a row failed validation.  The offsets of the rows in front of it stand (exclusive sums); the heap sizes and the
                        // validity words are made again for the shorter table
                        hipLaunchKernelGGL(bam_pack_validity, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t *)c->c_rgflag.p, nrows, (uint64_t *)c->c_rgvalid.p);
                        if (strings) {
                            uint32_t t32[5] = {0, 0, 0, 0, 0};
                            for (int k = 0; k < 5; k++) HIPCHK(c, hipMemcpyAsync(&t32[k], o32[k] + nrows, 4, hipMemcpyDeviceToHost, c->stream));
                            HIPCHK(c, hipStreamSynchronize(c->stream));
                            for (int k = 0; k < 5; k++) tot[k] = t32[k];
                        }
                    }
                }
            }
            if (strings && nrows > 0) {
                ENSURE(c, c->a_qname, tot[0] + PAD_BYTES); ENSURE(c, c->a_cigar, tot[1] + PAD_BYTES); ENSURE(c, c->a_seq, tot[2] + PAD_BYTES);
                ENSURE(c, c->a_qual, tot[3] + PAD_BYTES); ENSURE(c, c->a_rg, tot[4] + PAD_BYTES);
                so.qname = (uint8_t *)c->a_qname.p; so.cigar = (uint8_t *)c->a_cigar.p; so.seq = (uint8_t *)c->a_seq.p; so.qual = (uint8_t *)c->a_qual.p; so.rg = (uint8_t *)c->a_rg.p;
                KTimer tm(c, DHTS_K_STRINGS);
                hipLaunchKernelGGL(bam_tile_strings, dim3((unsigned)ntiles), dim3(TS_THREADS), 0, c->stream, st, ntiles, to, (const uint32_t *)c->t_rowbase.p, (const uint64_t *)c->d_res.p,
                                   nrows_scan, nrows, (const uint32_t *)c->rec_off.p, row_map_s, bc, so, colmask);
            }
            HIPCHK(c, hipGetLastError());
            if (nrows > 0) {
                out->flag = bc.flag; out->pos = bc.pos; out->mapq = bc.mapq; out->pnext = bc.pnext; out->tlen = bc.tlen; out->tid = bc.tid; out->mtid = bc.mtid;
                out->rg_idx = bc.rg_idx; out->rg_valid = bc.rg_valid;
                out->qname = {o32[0], bc.len_qname, so.qname, tot[0]};
                out->cigar = {o32[1], bc.len_cigar, so.cigar, tot[1]};
                out->seq = {o32[2], so.seq_chars ? so.seq_chars : bc.len_seq, so.seq, tot[2]};
                out->seq_packed = so.seq_chars ? 1 : 0;
                out->qual = {o32[3], so.alen_qual, so.qual, tot[3]};
                out->rg = {o32[4], bc.len_rg, so.rg, tot[4]};
            }
        }
    }
    if (bam_tag_columns(c, st, nrows, out)) return -1;
    if (bam_aux_map(c, st, nrows, out)) return -1;
    if (bam_overlap_join(c, st, bc, nrows, out)) return -1;
    if (c->sam_text) {
        // back to text offsets: the carry starts at the first line that was not encoded, or at the line of a record bam_read1's checks refuse
        if (rec_err || nrows < sam_nrec) { rec_err = true; if (c->fastq ? fastq_record_start(c, nrows, carry_start) : line_start(c, c->lines, nrows, carry_start)) return -1; }
        else { carry_start = sam_carry; rec_err = sam_rej; }
        have_first_rec = true; first_rec_rel = (uint32_t)sam_t0;
    }
    out->n_rows = nrows;
    out->end_uoff = out_base + carry_start;
    {
        uint64_t f = NONE64;
        if (nrows > 0 && !have_first_rec) { HIPCHK(c, hipMemcpyAsync(&first_rec_rel, c->rec_off.p, 4, hipMemcpyDeviceToHost, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream)); }
        if (nrows > 0) f = out_base + first_rec_rel;
        out->first_rec_uoff = f;
    }
    // ---- advance ----
    return batch_end(c, B, carry_start, rec_err, shard_finished, &out->status, fused);
}
