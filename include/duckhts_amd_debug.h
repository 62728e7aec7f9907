/* duckhts_amd_debug.h -- test and measurement hooks of libduckhts_amd.so.
 *
 * NOT part of the drop-in boundary (that is include/duckhts_extension.h) nor of the scan ABI (include/duckhts_amd.h): nothing in the
 * reference corresponds to these.  They exist so that the tests can look at intermediate results of the device path (the phase-A
 * scratch of a BGZF block, the encoder's BCF2 records of a VCF text batch, a block table built over a prefix) and so that tools/dbg/
 * can time one kernel alone.  They are declared here because the library exports exactly what include/ declares (tests/test_abi.py).
 */
#ifndef DUCKHTS_AMD_DEBUG_H
#define DUCKHTS_AMD_DEBUG_H
#include "duckhts_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* hipMalloc calls the device pool could not serve since the process started (DHTS_TRACE reports them) */
void dhts_debug_malloc_stats(uint64_t *calls, uint64_t *bytes, double *seconds);
/* tests: pretend only the first nbytes of the resident file have arrived (a file that is still being staged); returns the block count */
int64_t dhts_debug_index_prefix(dhts_ctx *, uint64_t nbytes);
/* tests: the BCF2 records the device encoder made of the last VCF text batch (bytes and record offsets) */
int64_t dhts_debug_vcf_records(dhts_ctx *, uint8_t *dst, uint64_t cap, uint32_t *rec_off, int64_t nrec);
/* tests: the BAM records (block_size prefixes included) the device encoder made of the last SAM text batch; returns their byte count, *nrec = records */
int64_t dhts_debug_sam_records(dhts_ctx *, uint8_t *dst, uint64_t cap, int64_t *nrec);
/* tests: the same for the last FASTQ / FASTA batch (the encoders share the buffer); -1 when the context is not reading FASTQ / FASTA */
int64_t dhts_debug_fastq_records(dhts_ctx *, uint8_t *dst, uint64_t cap, int64_t *nrec);
/* tools/bench_bed.py: the lane-per-line walk read_bed's delimiter table is measured against, over the whole text of a BED context: device
 * milliseconds of the line table (vcf_line_count / vcf_line_fill) and of bed_intervals (chrom / start / end by walking every line);
 * returns the number of lines */
int64_t dhts_debug_bed_walk(dhts_ctx *, double *ms_line_table, double *ms_walk);
/* tests: the most BED rows dhts_bam_bedcov_open takes, for the whole process (0: the contract's 2^27) */
void dhts_debug_bedcov_max_rows(uint64_t n);
/* tests: the most bytes the depth table of dhts_bam_coverage_open or dhts_bam_depth_open, or the count table of dhts_bam_pileup_open, may take,
 * for the whole process (0: the contract's 16 GiB) */
void dhts_debug_coverage_max_table_bytes(uint64_t n);
/* tests: the most bytes the histogram table of dhts_bam_depth_hist_open may take, for the whole process (0: the contract's 1 GiB) */
void dhts_debug_hist_max_table_bytes(uint64_t n);
/* tests, tools/bench_depth_hist.py: the device time in ms per launch of one pass over the depth table of the context's open bam_depth_hist, `reps`
 * launches between two events: which 0 = dep_tile_reduce (bam_coverage's read of the table), 1 = dhi_hist (the histogram pass).  The next
 * dhts_bam_depth_hist_next makes its result anew.  < 0 with dhts_error set when a call failed. */
double dhts_debug_hist_pass_ms(dhts_ctx *, int which, int reps);
/* tests, tools/bench_pileup.py: the form of bam_pileup's add kernel on this context from the next accumulate on: 0 the default (the window form), 1 direct (one
 * atomic add per counted base into the table), 2 window (the workgroup counts 512 positions of one row in LDS and adds the non-zero words to
 * the table when the window moves).  Any other value fails with a dhts_error. */
int dhts_debug_pileup_add_form(dhts_ctx *, int form);
/* tools/dbg: phase A (kernel 0: lane per block, 1: wave per block) / phase B alone over blocks [b0, b0 + nb); ms per launch */
double dhts_debug_time_huff(dhts_ctx *, int64_t b0, int64_t nb, int reps);
double dhts_debug_time_lz(dhts_ctx *, int64_t b0, int64_t nb, int reps);
int dhts_debug_huff_run(dhts_ctx *, int64_t b0, int64_t nb, int kernel);
/* tests: metadata, literal bytes and tokens phase A left for scratch slot s (the wave and the lane kernel must agree word for word) */
int dhts_debug_scratch_get(dhts_ctx *, int64_t s, uint32_t *meta4, uint8_t *lit, uint32_t *tok);
int dhts_debug_meta(dhts_ctx *, int64_t s, uint32_t *out4);
/* tests: the DEFLATE encoder's code builder alone (bgzf_deflate.hip: dfl_build_lengths + dfl_assign_codes) on ncases count vectors of nsym
 * symbols (host arrays, case after case); lens_out: ncases * nsym code lengths, codes_out: the table words (bit-reversed code | length << 16).
 * Only for count vectors the builder's loops are known to end on (tests/deflate_code_ref.py). */
int dhts_debug_deflate_codes(dhts_ctx *, const uint32_t *counts, uint32_t nsym, uint32_t maxbits, int64_t ncases, uint8_t *lens_out, uint32_t *codes_out);
/* tests: the carry in two levels alone (dev_scan.hip), through the launcher the bam_* count functions call.  kind 0: uint32_t sum, 1: uint64
 * sum, 2: uint64 suffix minimum (host_v[i] = the least element behind i, seed where there is none), 3: sum of elements of four uint64 words
 * added word by word, four elements per thread.  host_v holds n >= 1 elements on entry and the scanned n on return; the sums are exclusive,
 * start at 0 (seed is unused) and return n + 1 elements, the total last.  host_v has room for n + 1 elements of every kind; element n is
 * uploaded as it is and must not change an answer. */
int dhts_debug_carry(dhts_ctx *, int kind, void *host_v, uint64_t n, uint64_t seed);
/* tests: the line table the text readers share, alone (csrc/dhts_text_lines.inc: line_table), on a host text of n bytes that is staged with
 * the 64 zero bytes a batch has behind it.  t0: where the first line starts; open_last_ok: a last line without a newline counts; lim: lines
 * that start at or behind it are cut (~0: no cut); with_tabs: the tab part (bed_delim_count / bed_delim_fill instead of vcf_line_count /
 * vcf_line_fill).  out takes the function's result: nl, ntabs, nlines, last_start, carry_start, last_open, finished.  When t0 < n, line_off takes the nlines + 1 starts line_off[0 .. nlines] (behind an open last
 * line that is n + 1) and, with the tab part, tab0 as many words, has_nul nlines words and tab_off ntabs words; the arrays have room for n + 2
 * words each.  When t0 >= n no table is made and no array is written. */
int dhts_debug_line_table(dhts_ctx *, const uint8_t *text, uint64_t n, uint64_t t0, int open_last_ok, uint64_t lim, int with_tabs, uint64_t out[7],
                          uint32_t *line_off, uint32_t *tab_off, uint32_t *tab0, uint32_t *has_nul);
/* tests: the row-text encoder alone (csrc/rows_text.hip) on host arrays: a table of n_names names (names: the byte arena, name_offs:
 * n_names + 1 offsets into it) and n_rows rows of tid (int32; outside the table: an empty name), start, end (int64) and depth (int32) -> the
 * bytes `name \t start \t end \t depth \n` per row in out.  The text lies 5 bytes into the device buffer, so the write pass meets a span that
 * is not 16-byte aligned.  Returns the bytes of the text (nothing is copied when cap is smaller), or -1 with dhts_error set. */
int64_t dhts_debug_rows_text(dhts_ctx *, const uint8_t *names, const uint32_t *name_offs, int32_t n_names, const int32_t *tid, const int64_t *start, const int64_t *end,
                             const int32_t *depth, int64_t n_rows, uint8_t *out, uint64_t cap);
/* tests: the workgroups of the encoder's write pass that staged their rows in LDS (out2[0]) and that took the fallback for a span over the
 * LDS budget (out2[1]) in the last dhts_debug_rows_text (an export does not count them) */
int dhts_debug_rows_text_paths(dhts_ctx *, uint64_t out2[2]);
/* tests, tools/bench_bedgraph_export.py: the form of the encoder's write pass on this context from the next call on: 0 the default (a workgroup
 * stages its rows in LDS and stores aligned 16-byte pieces), 1 one lane per row storing byte by byte, the form the default is measured against
 * (DESIGN.md 4r).  Any other value fails with a dhts_error. */
int dhts_debug_rows_text_form(dhts_ctx *, int form);
/* tests: the rows of a page and the blocks of a compressor launch dhts_bedgraph_export uses on this context (0: the defaults, 1,048,576
 * rows and 4,096 blocks), so that a small file crosses pages and chunks */
int dhts_debug_export_limits(dhts_ctx *, int64_t page_rows, int64_t chunk_blocks);
/* tests: what the record stage's repair and retry paths did since the context was opened or rewound (host-side counters, read_bam and
 * read_bcf alike).  out[0] tiles changed by the repair rounds and by the sequential fallback, summed over rounds and batches;
 * out[1] repair rounds that changed a tile (the two rounds read_bam always queues count only when they repaired something, so a file that
 * speculates correctly shows 0; the sequential fallback is no round); out[2] batches that went on to the sequential fallback (more than 256 rounds);
 * out[3] retries of a speculated shard start (candidates tried after the first one failed; record starts on a failed chain are passed over
 * without a retry); out[4] candidates whose chain held but whose
 * records the full validation refused (bam_validate_rows / bcf_rec_check); out[5] batches where no candidate was left and the first
 * attempt's result was restored; out[6], out[7] zero. */
int dhts_debug_tile_stats(dhts_ctx *, uint64_t out[8]);
/* tests, tools/dbg: one tile-scan kernel alone over the inflated batch the context holds (the latest dhts_bam_next_batch), before any repair
 * round: kernel 0 = bam_tile_scan (one wave per tile), 1 = bam_tile_scan_lanes (one lane per tile; tile 0 by bam_tile_scan).  Tile 0 is
 * started at offset 0.  Host tables of ntiles_cap entries each, recs of ntiles_cap * 256 (entries k < min(count, 256) of a tile are
 * written; the rest keep 0xeeee).  Any table may be NULL.  Returns the number of tiles, or -1. */
int64_t dhts_debug_tile_scan(dhts_ctx *, int kernel, uint64_t *first, uint64_t *end_next, uint32_t *count, int32_t *err, uint64_t *recs_first,
                             uint16_t *recs, int64_t ntiles_cap);
/* (diagnostic builds only: -DDHTS_DIAG dhts_debug_diag, -DHW_DIAG dhts_debug_hw_diag, -DTR_DIAG dhts_debug_tr_diag: per-phase cycle counters) */
int dhts_debug_diag(dhts_ctx *, unsigned long long *out8);
int dhts_debug_hw_diag(dhts_ctx *, unsigned long long *out16, int reset);
int dhts_debug_tr_diag(dhts_ctx *, unsigned long long *out16, int reset);
/* tests, tools/bench_intervals.py: the interval functions' sort alone (csrc/interval_sort.hip) on host arrays.  keys_u64[n] are compared
 * unsigned, rank_u32[n] is row i's rank (the more significant part of the order); rows_out_u32[n] receives the row numbers 0 .. n - 1 in
 * the order of (rank, key), rows of equal (rank, key) in input order.  *passes: the radix passes that were run (a pass whose digit is equal
 * in all pairs is skipped). */
int dhts_debug_ivl_sort(dhts_ctx *, const uint64_t *keys_u64, const uint32_t *rank_u32, uint64_t n, uint32_t *rows_out_u32, int32_t *passes);
/* tools/bench_intervals.py: device time in milliseconds of the parts of the last dhts_ivl_load (0 load, 1 sort, 2 index), dhts_ivl_merge_open
 * (3), dhts_ivl_overlap_open (4: the count pass and its carry) and of the write passes of the pages taken since (5), and of sort pass p (16 + p);
 * of the last dhts_ivl_nearest_open on the left context: 6 the end sort and gather of the right context (0 when it had its end order already;
 * the right context keeps the figure under 6 as well), 7 the selection pass and its carry, 8 the write passes of the pages taken since */
double dhts_debug_ivl_ms(dhts_ctx *, int what);

#ifdef __cplusplus
}
#endif
#endif
