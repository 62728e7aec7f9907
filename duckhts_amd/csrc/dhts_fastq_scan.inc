// dhts_fastq_scan.inc -- part of dhts_api.hip (included there, inside its extern "C" block; not a translation unit of its own):
// read_bam on FASTQ / FASTA text.  As for SAM text (dhts_sam_scan.inc) a batch of text is cut into lines; fastq_text.hip finds the lines that
// start a record and encodes the records that lie wholly inside the batch into s_out; bam_next_batch_one runs its unchanged record stage
// over them.  The carry is the text from the first record that is not whole.
//
// out: as sam_text_records.  nrec counts the records in front of the first one fastq_parse1 / bam_set1 refuse; `rejected` ends the scan
// there (a record the end of the file cuts short is refused as well).
// a record has to fit into one batch with the blocks behind it: batch offsets are 32-bit and a batch takes up to 1.5 GiB of new text
#define FASTQ_MAX_RECORD_TEXT (2ull << 30)
static int fastq_text_records(dhts_ctx *c, const Batch &B, const uint8_t *&enc, uint64_t &enc_len, int64_t &nrec, uint64_t &carry_start, bool &rejected, uint64_t &t0) {
    const uint8_t *u = B.u; const uint64_t ulen = B.ulen, out_base = B.out_base;
    if (!first_line_t0(c, out_base, t0)) return fail(c, "internal: header beyond first batch");
    nrec = 0; enc = nullptr; enc_len = 0; rejected = false;
    c->s_last_nrec = 0; c->s_last_len = 0;
    const bool clean_end = batch_clean_end(c, B);
    LineTab T;
    if (line_table(c, c->lines, nullptr, u, t0, ulen, clean_end, ~0ull, -1, T)) return -1;
    if (T.nl + 2 >= (uint64_t)FQ_IDX) return fail(c, "batch too large");         // (line numbers share their word with the chain's flags)
    const int64_t nlines = T.nlines;
    const uint64_t lines_end = T.carry_start;                                  // text offset behind the batch's complete lines
    if (t0 >= ulen) { carry_start = ulen; return 0; }
    carry_start = t0;
    if (nlines == 0) return 0;
    const size_t ln = (size_t)(nlines + 2) * 4 + 64; const int64_t ntiles = (nlines + FQ_TILE - 1) / FQ_TILE;
    ENSURE(c, c->f_len, ln); ENSURE(c, c->f_flag, ln); ENSURE(c, c->f_psum, ln); ENSURE(c, c->f_rank, ln); ENSURE(c, c->f_mark, ln); ENSURE(c, c->f_next, ln);
    ENSURE(c, c->f_plus, ln); ENSURE(c, c->f_exit, ln); ENSURE(c, c->f_isstart, ln); ENSURE(c, c->f_recrank, ln); ENSURE(c, c->f_recline, ln);
    ENSURE(c, c->f_entry, (size_t)ntiles * 4 + 64); ENSURE(c, c->f_stop, 64); ENSURE(c, c->s_ctr, 64);
    FqArgs a; memset(&a, 0, sizeof(a));
    a.u = u; a.line_off = (const uint32_t *)c->lines.line_off.p; a.nlines = (uint32_t)nlines; a.fasta = c->fastq == 2 ? 1 : 0; a.final_batch = clean_end ? 1 : 0;
    a.len = (uint32_t *)c->f_len.p; a.flag = (uint32_t *)c->f_flag.p; a.psum = (const uint32_t *)c->f_psum.p; a.rank = (const uint32_t *)c->f_rank.p; a.mark_idx = (uint32_t *)c->f_mark.p;
    a.next = (uint32_t *)c->f_next.p; a.plus = (uint32_t *)c->f_plus.p; a.exit_ = (uint32_t *)c->f_exit.p; a.entry = (uint32_t *)c->f_entry.p; a.stop = (uint32_t *)c->f_stop.p;
    a.is_start = (uint32_t *)c->f_isstart.p; a.rec_rank = (const uint32_t *)c->f_recrank.p; a.rec_line = (uint32_t *)c->f_recline.p;
    a.first_bad = (unsigned long long *)c->s_ctr.p;
    const unsigned lgrid = (unsigned)((nlines + 255) / 256);
    uint32_t stop[2] = {0, 0}; uint64_t nstart = 0;
    {   // (a read_bam scan runs no BCF kernels: record discovery and the measure pass are timed in the text encoder's measure slot)
        KTimer tm(c, DHTS_K_BCF_MEASURE);
        hipLaunchKernelGGL(fq_line_props, dim3(lgrid), dim3(256), 0, c->stream, a);
        const uint32_t *in2[2] = {a.len, a.flag}; uint32_t *out2[2] = {(uint32_t *)c->f_psum.p, (uint32_t *)c->f_rank.p}; uint64_t tot2[2] = {0, 0};
        if (run_scan(c, 2, in2, out2, nullptr, nlines, tot2)) return -1;
        a.nmark = (uint32_t)tot2[1];
        hipLaunchKernelGGL(fq_compact, dim3(lgrid), dim3(256), 0, c->stream, (const uint32_t *)a.flag, a.rank, a.nlines, a.mark_idx);
        hipLaunchKernelGGL(fq_next, dim3(lgrid), dim3(256), 0, c->stream, a);
        HIPCHK(c, hipMemsetAsync(c->f_entry.p, 0xff, (size_t)ntiles * 4, c->stream));
        hipLaunchKernelGGL(fq_tile<false>, dim3((unsigned)ntiles), dim3(256), 0, c->stream, a);
        hipLaunchKernelGGL(fq_chain, dim3(1), dim3(64), 0, c->stream, a);
        hipLaunchKernelGGL(fq_tile<true>, dim3((unsigned)ntiles), dim3(256), 0, c->stream, a);
        HIPCHK(c, hipMemcpyAsync(stop, c->f_stop.p, 8, hipMemcpyDeviceToHost, c->stream));
        const uint32_t *in1[1] = {a.is_start}; uint32_t *out1[1] = {(uint32_t *)c->f_recrank.p};
        if (run_scan(c, 1, in1, out1, nullptr, nlines, &nstart)) return -1;        // (waits for the stream: `stop` has arrived)
    }
    // where the chain ended: behind the lines (the partial line is the carry), at a refused line, or at a record the batch cuts short
    if (stop[1] == 0) carry_start = lines_end;
    else { if (line_start(c, c->lines, stop[0], carry_start)) return -1; rejected = stop[1] == 1 || B.final_batch; }
    if (!rejected && !B.final_batch && nstart == 0 && ulen - carry_start >= FASTQ_MAX_RECORD_TEXT)
        return fail(c, "read_bam: a FASTQ/FASTA record of more than 2 GiB of text does not fit into one batch");
    if (nstart == 0) return 0;
    a.nrec = (uint32_t)nstart;
    hipLaunchKernelGGL(fq_compact, dim3(lgrid), dim3(256), 0, c->stream, (const uint32_t *)a.is_start, a.rec_rank, a.nlines, a.rec_line);
    ENSURE(c, c->v_rec_len, (size_t)(nstart + 1) * 4 + 64); ENSURE(c, c->b_rec_off, (size_t)(nstart + 1) * 4 + 64);
    a.rec_len = (uint32_t *)c->v_rec_len.p; a.rec_off = (const uint32_t *)c->b_rec_off.p;
    const int64_t waves = FQ_ENC_THREADS / 64;
    const unsigned grid = (unsigned)(((int64_t)nstart + waves - 1) / waves < (1 << 20) ? ((int64_t)nstart + waves - 1) / waves : (1 << 20));
    uint64_t total = 0;
    {
        KTimer tm(c, DHTS_K_BCF_MEASURE);
        HIPCHK(c, hipMemsetAsync(c->s_ctr.p, 0xff, 8, c->stream));
        hipLaunchKernelGGL(fq_encode<false>, dim3(grid), dim3(FQ_ENC_THREADS), 0, c->stream, a);
        const uint32_t *in1[1] = {a.rec_len}; uint32_t *out1[1] = {(uint32_t *)c->b_rec_off.p};
        if (run_scan(c, 1, in1, out1, nullptr, (int64_t)nstart, &total)) return -1;
    }
    if (total + PAD_BYTES >= (1ull << 32)) return fail(c, "read_bam: a FASTQ/FASTA batch encodes to more than 4 GiB: use a smaller max_blocks");
    ENSURE(c, c->s_out, total + PAD_BYTES);
    a.out = (uint8_t *)c->s_out.p;
    unsigned long long first_bad = ~0ull;
    {
        KTimer tm(c, DHTS_K_BCF_WRITE);
        hipLaunchKernelGGL(fq_encode<true>, dim3(grid), dim3(FQ_ENC_THREADS), 0, c->stream, a);
        HIPCHK(c, hipMemsetAsync((uint8_t *)c->s_out.p + total, 0, PAD_BYTES, c->stream));
        HIPCHK(c, hipMemcpyAsync(&first_bad, c->s_ctr.p, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    nrec = (int64_t)nstart; enc_len = total;
    if (first_bad < nstart) {                                                  // bam_set1 refused a record: the scan ends in front of it
        nrec = (int64_t)first_bad; rejected = true;
        uint32_t w = 0; HIPCHK(c, hipMemcpy(&w, (const uint32_t *)c->b_rec_off.p + nrec, 4, hipMemcpyDeviceToHost)); enc_len = w;
        if (fastq_record_start(c, nrec, carry_start)) return -1;
    }
    enc = (const uint8_t *)c->s_out.p;
    c->s_last_nrec = nrec; c->s_last_len = enc_len;
    return 0;
}
// text offset of record `i` of the last FASTQ / FASTA batch
static int fastq_record_start(dhts_ctx *c, int64_t i, uint64_t &off) {
    uint32_t l = 0;
    HIPCHK(c, hipMemcpy(&l, (const uint32_t *)c->f_recline.p + i, 4, hipMemcpyDeviceToHost));
    return line_start(c, c->lines, l, off);
}
// debugging aid (include/duckhts_amd_debug.h): the BAM records the encoder made of the last FASTQ / FASTA batch
extern "C" int64_t dhts_debug_fastq_records(dhts_ctx *c, uint8_t *dst, uint64_t cap, int64_t *nrec) {
    if (!c || !c->fastq) return -1;
    if (nrec) *nrec = c->s_last_nrec;
    const uint64_t n = cap < c->s_last_len ? cap : c->s_last_len;
    if (n && dst) HIPCHK(c, hipMemcpy(dst, c->s_out.p, n, hipMemcpyDeviceToHost));
    return (int64_t)c->s_last_len;
}
