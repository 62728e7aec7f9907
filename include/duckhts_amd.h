/*
 * duckhts_amd.h -- thin C ABI between host code and the MI355X (gfx950) HIP scan path.
 *
 * This is the "inner" boundary named by the north star ("host C code calls hand-written HIP
 * kernels through a thin C-ABI").  The reference has no such seam of its own: its scan
 * callbacks call htslib directly.  Each entry point below names the reference interface whose
 * work it takes over (paths relative to the reference tree; htslib/ = third_party/htslib/):
 *
 *   dhts_open_* / dhts_bgzf_index   <- hts_open/bgzf_open + the BSIZE chain walk inside
 *                                      bgzf_read_block              htslib/bgzf.c:1155-1236
 *   dhts_bgzf_inflate_to_host       <- inflate_block/bgzf_uncompress + CRC-32 compare
 *                                                                    htslib/bgzf.c:762-824
 *   dhts_bam_open / dhts_bam_header <- sam_hdr_read -> bam_hdr_read  htslib/sam.c:229-342
 *                                      (+ @RG ID->SM dictionary: header.c:271-318, 2282-2312)
 *   dhts_bam_next_batch             <- the loop body of bam_read_function
 *                                      src/bam_reader.c:747-1035 over bam_read1 sam.c:779-855,
 *                                      sam_read1_bam sam.c:4124-4134, bam_aux_get sam.c:4834-4855
 *
 * The "outer" drop-in boundary (DuckDB C-API extension entry point duckhts_init_c_api and the
 * read_bam bind/init/local_init/scan callbacks, src/duckhts.c:48-93, src/bam_reader.c:1044-1068)
 * is declared in duckhts_extension.h and implemented on top of this ABI.
 *
 * All pointers are plain; no torch / HIP types cross the boundary.  Every function fails
 * loudly (non-zero return + dhts_error()) when no MI355X device / code object is available:
 * there is no CPU fallback.
 */
#ifndef DUCKHTS_AMD_H
#define DUCKHTS_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DHTS_ABI_VERSION 1

typedef struct dhts_ctx dhts_ctx;

/* read_bam core column ids, same order as src/bam_reader.c:187-202 */
enum {
    DHTS_BAM_QNAME = 0, DHTS_BAM_FLAG, DHTS_BAM_RNAME, DHTS_BAM_POS, DHTS_BAM_MAPQ, DHTS_BAM_CIGAR, DHTS_BAM_RNEXT,
    DHTS_BAM_PNEXT, DHTS_BAM_TLEN, DHTS_BAM_SEQ, DHTS_BAM_QUAL, DHTS_BAM_READ_GROUP_ID, DHTS_BAM_SAMPLE_ID,
    DHTS_BAM_CORE_COUNT
};
#define DHTS_BAM_ALL_COLS ((1u << DHTS_BAM_CORE_COUNT) - 1u)

/* variable-width column in device memory: row i = bytes[off[i] .. off[i]+len[i])            */
typedef struct {
    const uint32_t *off;     /* n+1 offsets (prefix sum of reserved widths)                    */
    const uint32_t *len;     /* n actual lengths (<= reserved)                                 */
    const uint8_t *bytes;
    uint64_t nbytes;         /* off[n]                                                          */
} dhts_strcol;

/* One projected column of a batch; DEVICE pointers, valid until the next call on the context.
 * scalar fixed-width : fixed[n_rows] in the native width of `type` (BOOLEAN 1 byte, INTEGER/FLOAT/ids 4, BIGINT/DOUBLE 8)
 * scalar VARCHAR     : off[n_rows+1] byte offsets into bytes
 * LIST               : off[n_rows+1] child offsets; children in child_fixed[child_n] (4-byte words) or, for
 *                      LIST(VARCHAR) in plain encoding, child_off[child_n+1] byte offsets into bytes                   */
typedef struct dhts_col {
    int32_t col;             /* schema column id                                                            */
    int32_t child_width;     /* bytes per child_fixed word: 0/4 = 4 (read_bcf), 8 = BIGINT children (read_bam tag lists)     */
    const uint8_t *valid;    /* n_rows bytes, 1 = valid                                                     */
    const void *fixed;
    const uint32_t *off;
    const uint8_t *bytes; uint64_t nbytes;
    const uint32_t *child_fixed; const uint32_t *child_off; uint64_t child_n;
    const uint8_t *child_valid; /* child_n bytes, 0 = NULL element; NULL pointer = every element valid (only VEP_* columns have NULL elements) */
} dhts_col;
typedef dhts_col dhts_bcf_col;

/* auxiliary_tags := true (src/bam_reader.c:967-1027): per row the tags that are not standard-tag columns, in record order, as TYPED
 * entries; the caller renders the value text (bam_aux_to_string bam_reader.c:140-183: %lld / %g / "subtype,v,v..."), because %g is
 * floating-point formatting.  kind: 0 int64, 1 f64 bits, 2 string bytes, 3 one char, 4 int64 array, 5 f64-bits array, 6 corrupt value
 * (the reference reads past the field there; rendered empty).  Device pointers.                                                  */
typedef struct {
    const uint8_t *valid;        /* n_rows: 0 = no entries (the MAP cell is NULL)                          */
    const uint32_t *off;         /* n_rows+1 entry offsets                                                 */
    uint64_t n_ent;
    const uint16_t *key;         /* two raw tag bytes, low byte first                                      */
    const uint8_t *kind, *sub;   /* sub = B-array subtype character                                        */
    const uint32_t *pay_off;     /* n_ent+1 payload offsets                                                */
    const uint8_t *payload; uint64_t payload_bytes;
} dhts_aux_map;

/* One decoded batch.  All pointers are DEVICE pointers owned by the context and stay valid
 * until the next dhts_bam_next_batch / dhts_bam_rewind / dhts_destroy on that context.        */
typedef struct {
    int64_t n_rows;
    int32_t status;          /* 0 = more data may follow, 1 = end of stream reached cleanly,
                                <0 = the stream ended on an error after these rows (the
                                reference ends the scan silently: bam_reader.c:754-766)        */
    int32_t seq_packed;      /* 1: seq.bytes holds the file's 4-bit base codes, seq.len the number of bases (dhts_bam_set_seq_packed) */
    const uint16_t *flag;    /* FLAG  USMALLINT */
    const int64_t *pos;      /* POS   BIGINT (1-based) */
    const int32_t *mapq;     /* MAPQ  INTEGER */
    const int64_t *pnext;    /* PNEXT BIGINT */
    const int64_t *tlen;     /* TLEN  BIGINT */
    const int32_t *tid;      /* dictionary id behind RNAME (-1 => "*") */
    const int32_t *mtid;     /* dictionary id behind RNEXT (-1 => "*") */
    const int32_t *rg_idx;   /* dictionary id behind SAMPLE_ID (index into header @RG table, -1 => NULL) */
    const uint64_t *rg_valid;/* validity words of READ_GROUP_ID (bit = 1 valid) */
    dhts_strcol qname, cigar, seq, qual, rg;
    uint64_t first_rec_uoff; /* absolute inflated-stream offset of the first row's record        */
    uint64_t end_uoff;       /* absolute inflated-stream offset just past the last row's record  */
    int32_t n_tag_cols;      /* standard-tag columns selected by dhts_bam_set_tag_columns         */
    int32_t qual_bits;       /* host batches only (dhts_bam_batch_fetch*, after dhts_bam_set_qual_packed): 0 = qual.bytes are the characters; 2 / 4 =
                              * qual.bytes is a 16-byte symbol table followed by the heap's characters as 2- / 4-bit codes, little end first:
                              * character k of the heap = table[(stream[k * bits / 8] >> (k * bits % 8)) & mask]; off / len count characters */
    const dhts_aux_map *aux_map; /* NULL unless dhts_bam_set_aux_map enabled it                       */
    const dhts_col *tag_cols;/* host array; BIGINT scalars in fixed (8 B), VARCHAR in off/bytes, LIST(BIGINT) in off/child_fixed (8 B words) */
    const uint32_t *ov_off;  /* overlap join (dhts_bam_set_overlap_intervals): n_rows+1 offsets into ov_ids, NULL when off */
    const uint32_t *ov_ids;  /* ids (positions in the caller's interval arrays) of the intervals overlapping each row     */
    uint64_t n_ov;
} dhts_bam_batch;

/* Host copy of the BAM header dictionaries (pointers owned by the context).                   */
typedef struct {
    int32_t n_ref;
    const char *const *ref_name;   /* NUL-terminated, as sam_hdr_tid2name would return          */
    const uint32_t *ref_len;
    const char *text; uint32_t l_text;
    int32_t n_rg;                  /* distinct @RG IDs, header order                             */
    const char *const *rg_id;
    const char *const *rg_sm;      /* NULL when the @RG has no (non-empty) SM                    */
    uint64_t first_rec_uoff;       /* inflated offset of the first alignment record              */
} dhts_bam_header;

/* kernel ids for dhts_kernel_time (a read_bam scan of SAM text times its encoder's measure / write passes as DHTS_K_BCF_MEASURE / _WRITE;
 * read_bed: DHTS_K_TILES the delimiter table, _CORE the line classes, _SCAN the scans, _BCF_CHECK the BIGINT columns, _BCF_MEASURE / _WRITE
 * the lengths and the bytes of the VARCHAR columns) */
enum { DHTS_K_SIGSCAN = 0, DHTS_K_HUFF, DHTS_K_LZ, DHTS_K_TILES, DHTS_K_CORE, DHTS_K_SCAN, DHTS_K_STRINGS,
       DHTS_K_BCF_CHECK, DHTS_K_BCF_MEASURE, DHTS_K_BCF_WRITE, DHTS_K_COUNT };

int dhts_abi_version(void);
int dhts_device_count(void);                       /* number of visible HIP devices (0 => nothing will work) */
dhts_ctx *dhts_create(int device_id);              /* NULL if the device / code object is unavailable */
void dhts_destroy(dhts_ctx *);
const char *dhts_error(const dhts_ctx *);          /* last error message ("" if none) */

/* ---- input: compressed bytes become resident in HBM -------------------------------------- */
int dhts_open_path(dhts_ctx *, const char *path);                  /* pread (reader threads) -> pinned -> HBM, whole file */
/* bytes [off, off+len) of the file (len = 0: to its end) become the resident bytes: a rank of a multi-GPU scan stages only its
 * own block range plus a halo; a bind that only needs the header stages the first megabytes (hts_open + the reads under
 * bgzf_read_block, htslib/bgzf.c:1004-1239, restricted to a window of the file) */
int dhts_open_path_range(dhts_ctx *, const char *path, uint64_t off, uint64_t len);
/* Staging that overlaps the scan (the analogue of bgzf_mt_reader running ahead of the consumer, htslib/bgzf.c:1598-1738):
 * dhts_open_path_async starts reader threads and returns; dhts_stage_wait blocks until at least min_bytes contiguous bytes of the file
 * are resident (or staging has finished: *done) and returns that count; dhts_bgzf_index_staged builds -- later extends -- the block table
 * over the resident prefix; dhts_bam_next_batch then serves the blocks known so far and reports status 0 ("more may follow") until the
 * table covers the whole file; dhts_blocks_ahead = blocks in the table that the scan has not consumed yet. */
int dhts_open_path_async(dhts_ctx *, const char *path);
int64_t dhts_stage_wait(dhts_ctx *, uint64_t min_bytes, int *done);
int64_t dhts_bgzf_index_staged(dhts_ctx *);
int64_t dhts_blocks_ahead(const dhts_ctx *);
/* one rank's share of ONE file: resident bytes = the header blocks file[0, header_bytes) followed by the rank's own
 * window of whole BGZF blocks plus a 4 MiB halo; cut points t_r = header_bytes + (size - header_bytes) * r / world.  Follow with
 * dhts_bgzf_index, dhts_bam_open and dhts_bam_set_file_shard(rank, world).  header_bytes: dhts_bam_header_bytes of a context that has
 * opened (the head of) the file.  dhts_voffset turns a position of the inflated stream into a BGZF virtual offset (bgzf_tell,
 * htslib/bgzf.h): adjacent ranks hand off end == first-record as virtual offsets. */
int dhts_open_path_shard(dhts_ctx *, const char *path, int rank, int world, uint64_t header_bytes);
/* A region query stages only what it needs (htslib seeks to each index chunk, hts.c:4320-4607): dhts_bam_region_segments -- on a context
 * that holds the header (dhts_bam_open) and the regions (dhts_bam_set_regions) -- turns the index into file byte ranges: beg[k] = offset
 * of a window's first BGZF block, end[k] = offset of its LAST block (~0 = to the end of the file), *count = -1 when the whole file is
 * needed; dhts_open_path_segments stages the header blocks file[0, header_bytes) and those windows (whole blocks, merged where they
 * touch).  dhts_bgzf_index / dhts_bam_open / dhts_bam_set_regions / dhts_bam_load_index follow as for a whole file; virtual offsets
 * (dhts_voffset, the index) stay those of the FILE. */
int dhts_bam_region_segments(dhts_ctx *, const void *index_bytes, uint64_t n, uint64_t *beg, uint64_t *end, int64_t cap, int64_t *count);
int dhts_open_path_segments(dhts_ctx *, const char *path, uint64_t header_bytes, const uint64_t *beg, const uint64_t *end, int64_t n);
/* the cut itself, host only (no device): rank r stages file[win_begin, win_end) and owns the blocks that start in [win_begin, own_end) */
int dhts_shard_window(const char *path, int rank, int world, uint64_t header_bytes, uint64_t *win_begin, uint64_t *win_end, uint64_t *own_end);
int dhts_bam_set_file_shard(dhts_ctx *, int rank, int world);
uint64_t dhts_bam_header_bytes(const dhts_ctx *);
uint64_t dhts_voffset(const dhts_ctx *, uint64_t uoff);
int dhts_open_host(dhts_ctx *, const void *bytes, uint64_t n);     /* copy host bytes -> HBM */
int dhts_open_tiled(dhts_ctx *, const void *head, uint64_t n_head, const void *body, uint64_t n_body, int reps,
                    const void *tail, uint64_t n_tail);            /* HBM = head + body x reps + tail (benchmark helper) */
uint64_t dhts_resident_bytes(const dhts_ctx *);

/* ---- BGZF -------------------------------------------------------------------------------- */
int64_t dhts_bgzf_index(dhts_ctx *);               /* block discovery on resident bytes; returns n_blocks or <0 */
int dhts_bgzf_table(const dhts_ctx *, uint64_t *coff, uint32_t *clen, uint32_t *isize, int64_t cap);  /* host copies */
/* inflate blocks [blk0, blk0+nblk) and copy the concatenated payload to host (parity tests) */
int64_t dhts_bgzf_inflate_to_host(dhts_ctx *, int64_t blk0, int64_t nblk, uint8_t *out, uint64_t cap, int32_t *blk_status);

/* ---- read_bam ------------------------------------------------------------------------------ */
int dhts_bam_open(dhts_ctx *);                                     /* header + dictionaries; positions the scan at the first record */
int dhts_bam_header_get(const dhts_ctx *, dhts_bam_header *out);
int dhts_bam_set_shard(dhts_ctx *, int rank, int world);           /* scan only this rank's BGZF block range */
int dhts_bam_set_block_range(dhts_ctx *, int64_t b0, int64_t b1, int speculative_start);   /* explicit shard: blocks [b0,b1) */
/* the shard cut itself (host arithmetic only): blocks [*b0,*b1) of rank, balanced by compressed bytes */
int dhts_shard_cut(const uint64_t *coff, int64_t n_blocks, uint64_t comp_len, int rank, int world, int64_t *b0, int64_t *b1);
/* region := 'chr:beg-end,...' (sam_itr_regarray, htslib sam.c:1763-1790 over hts_reglist_create region.c:177-260, hts_parse_region
 * hts.c:3995-4150, the predicate of hts_itr_multi_next hts.c:4575-4592 + bam_endpos sam.c:668-673).  Rows are filtered on the device.
 * Returns 0, 1 when no region names a known reference (reference: "No reads found for region(s): ..."), <0 on error.          */
int dhts_bam_set_regions(dhts_ctx *, const char *regions);
/* BAI or CSI bytes (hts_idx_load: hts.c:2920-3055; a BGZF-compressed CSI is inflated on the device): narrows the scan window to
 * the chunks of the bins the regions touch (reg2bins hts.c:3142-3213 + BAI linear index); optional for exactness, call after
 * dhts_bam_set_regions / dhts_bcf_set_region.                                                                                    */
int dhts_bam_load_index(dhts_ctx *, const void *index_bytes, uint64_t n);
/* the scan range the regions + index produced: number of disjoint windows (the merged chunk list of hts_itr_multi_bam, hts.c:3597-3739;
 * chunks closer than DHTS_WINDOW_GAP_MB, default 32, are scanned as one window) and the BGZF blocks they cover */
int dhts_scan_window_stats(const dhts_ctx *, int64_t *n_windows, int64_t *n_blocks);
/* what the block table's corrections did on this context (htslib never reads a BGZF trailer's ISIZE; the scan places blocks by it and takes
 * the decoded lengths where they differ): out[0] = blocks re-placed in total, out[1] = block ranges decoded again because the packed inflate
 * scratch was too small, out[2] = blocks re-placed during such a repeat.                                                                  */
int dhts_bgzf_repair_stats(const dhts_ctx *, int64_t out[3]);
/* BCF: CSI bytes, narrows the window as above (optional).  bgzipped VCF TEXT: TBI, or CSI with a tabix header (tbx_index_load3, tbx.c:552-597)
 * -- REQUIRED for a region other than ".": the region names a sequence of the INDEX (tbx_itr_querys -> tbx_name2id), so it is resolved here;
 * the index's sequences missing from the header become ##contig lines as in vcf_hdr_read (vcf.c:2649-2668).  Rows are decided on the
 * device by the interval tbx_parse1 gives a line (tbx.c:96-312: REF length, SVLEN of <DEL>/<DUP>/<CNV>/<INV>, FORMAT/LEN, INFO/END).
 * Returns 0, 1 = the index does not know the region's sequence (no iterator: the reference skips the region), <0 on error.            */
int dhts_bcf_load_index(dhts_ctx *, const void *index_bytes, uint64_t n);
/* What a region query of read_bcf has to stage instead of the whole file (the reference seeks to the index chunks): the compressed bytes of
 * the header blocks, and the union of the index windows of every region of 'a,b,...' as file byte ranges for dhts_open_path_segments
 * (same conventions as dhts_bam_region_segments; *count = -1: stage the whole file).  Both on a context that holds the header. */
uint64_t dhts_bcf_header_bytes(const dhts_ctx *);
int dhts_bcf_region_segments(dhts_ctx *, const char *regions, const void *index_bytes, uint64_t n, uint64_t *beg, uint64_t *end, int64_t cap, int64_t *count);
/* standard_tags := true (src/bam_reader.c:54-70, 920-966): the reference's 56-entry tag table, in its order */
int dhts_bam_std_tag_count(void);
int dhts_bam_std_tag_info(int idx, char name[3], char *type, char *subtype);   /* type: 'i' BIGINT, 'Z'/'A' VARCHAR, 'B' LIST(BIGINT) */
int dhts_bam_set_tag_columns(dhts_ctx *, const int32_t *std_tag_ids, int32_t n);  /* tag columns materialised by the next batches (default none) */
int dhts_bam_set_aux_map(dhts_ctx *, int enable, int exclude_standard_tags);        /* AUXILIARY_TAGS entries in the next batches */
int dhts_bam_rewind(dhts_ctx *);
/* BAI writer (the reference: src/hts_index_builder.c over sam_index_build, htslib sam.c:989-1027 +
 * hts_idx_push / hts_idx_finish / idx_save_core hts.c:2315-2818).  One whole-file scan of the open BAM; returns the size of the
 * index (bytes of a .bai file) kept in the context, or <0 (unsorted input, a record beyond 2^29, ... as in hts_idx_push).       */
int64_t dhts_bam_build_index(dhts_ctx *);
int64_t dhts_bam_build_index_csi(dhts_ctx *, int min_shift);   /* sam_index_build3(fn, fnidx, min_shift): > 0 writes a CSI (depth from the longest @SQ), <= 0 the BAI */
int dhts_bam_index_bytes(dhts_ctx *, uint8_t *out, uint64_t cap);
/* Interval overlap join on the scan (SURVEY 8(f) item 1 / BASELINE config 5).  The reference vendors cgranges
 * (third_party/cgranges, cr_add / cr_index / cr_overlap cgranges.c:255-297) as the model for joining read_bam rows with
 * read_bed intervals (src/interval_udf.c:344-426) but registers no SQL function for it yet; this entry point is what such a
 * function would bind.  Intervals are (tid, beg, end) half-open, 0-based, tid = index in the BAM header's reference table
 * (intervals with tid outside it never match).  Every following batch carries, per row, the ids of the intervals i with
 * beg_i < read_end && read_beg < end_i on the read's contig (read interval = [pos, bam_endpos)), i.e. cr_overlap's answer as
 * a set.  n = 0 switches the join off.  Host pointers; copied.                                                              */
int dhts_bam_set_overlap_intervals(dhts_ctx *, const int32_t *tid, const int64_t *beg, const int64_t *end, int64_t n);
/* The intervals from BED text, i.e. the rows read_bed would return for it (src/interval_udf.c:330-426: next_bed_line skips empty lines and
 * those that begin with '#', "track" or "browser", 141-147; a line with fewer than 3 tab-delimited fields is read_bed's error, 358-365;
 * start / end through strtoll over the whole field, else NULL, 127-139).  The device splits the text into lines and parses chrom / start /
 * end of each (bed_intervals, vcf_text.hip); chrom names are mapped to the BAM header's reference ids.  Interval id = row number of
 * read_bed; rows with a NULL start or end, or a chrom the header does not have, never match.  Returns the number of rows, < 0 on error.
 * _path: a plain or BGZF / gzip-compressed BED file (what hts_open + hts_getline accept, 330-337).                                   */
int64_t dhts_bam_set_overlap_bed(dhts_ctx *, const uint8_t *text, uint64_t n);
int64_t dhts_bam_set_overlap_bed_path(dhts_ctx *, const char *path);
/* Next batch of rows (<= max_blocks BGZF blocks of input; 0 = default 16,384, at most 24,576).  colmask = projection pushdown, bit i
 * = read_bam core column i (DHTS_BAM_*): the fixed-width columns are always produced; the string heaps (QNAME, CIGAR, SEQ, QUAL,
 * READ_GROUP_ID) of columns that are not projected are not written, and with none of them projected the string pass is skipped
 * (what the reference does per column in its writer switch, src/bam_reader.c:783-918).                                            */
int dhts_bam_next_batch(dhts_ctx *, int64_t max_blocks, uint32_t colmask, dhts_bam_batch *out);

/* ---- read_bcf ------------------------------------------------------------------------------
 *   dhts_bcf_open                   <- bcf_hdr_read -> bcf_hdr_parse      htslib/vcf.c:1710-1769, 1410-1489, 831-1024
 *                                      + schema construction              src/bcf_reader.c:540-760, src/include/vcf_types.h
 *   dhts_bcf_next_batch             <- the loop body of bcf_read_function src/bcf_reader.c:1155-2049 over bcf_read
 *                                      vcf.c:2255-2265 (bcf_read1_core 1874-1911, bcf_record_check 2040-2212),
 *                                      bcf_unpack 4234-4302 and the bcf_get_info_* / bcf_get_format_* getters 6056-6248
 * VEP_* columns (a CSQ / BCSQ / ANN / VEP / vep INFO tag in the header, src/vep_parser.c:100-182, src/bcf_reader.c:582-603,
 * 1463-1541): LIST columns with one element per transcript and NULL elements (dhts_bcf_col.child_valid) for missing fields. */

/* element types of a read_bcf column (values of DUCKDB_TYPE_* in duckdb.h) */
enum { DHTS_T_BOOLEAN = 1, DHTS_T_INTEGER = 4, DHTS_T_BIGINT = 5, DHTS_T_FLOAT = 10, DHTS_T_DOUBLE = 11, DHTS_T_VARCHAR = 17 };
/* how a column's payload is coded on the device */
enum { DHTS_ENC_PLAIN = 0,      /* payload is the value itself                                              */
       DHTS_ENC_CONTIG = 1,     /* int32 contig id   -> dhts_bcf_info.contig_name[id]   (CHROM)               */
       DHTS_ENC_DICT = 2,       /* int32 dictionary id -> dhts_bcf_info.dict_name[id], -1 = "PASS" (FILTER)    */
       DHTS_ENC_SAMPLE = 3,     /* int32 sample index -> dhts_bcf_info.sample_name[i]   (SAMPLE_ID)           */
       DHTS_ENC_FLOAT_TEXT = 4 };/* LIST(FLOAT) whose elements arrive as their decimal TEXT (child_off / bytes, like a LIST(VARCHAR)):
                                   the consumer converts every non-NULL element with (float)strtod(text, &end), NaN unless the whole
                                   text converts (vep_parse_float src/vep_parser.c:222-235).  Used by the Float fields of VEP_* columns;
                                   host text conversion, like the %g of AUXILIARY_TAGS. */

typedef struct {
    const char *name;        /* result column name, as duckdb_bind_add_result_column receives it           */
    int32_t type;            /* DHTS_T_* of the element                                                     */
    int32_t is_list;         /* LIST(type)                                                                  */
    int32_t encoding;        /* DHTS_ENC_*                                                                  */
    int32_t reserved;
} dhts_bcf_colinfo;

typedef struct {
    int32_t n_cols; const dhts_bcf_colinfo *cols;
    int32_t n_contigs; const char *const *contig_name;      /* NULL entries = holes left by IDX= numbering    */
    int32_t n_dict; const char *const *dict_name;           /* FILTER/INFO/FORMAT dictionary (BCF_DT_ID)      */
    int32_t n_samples; const char *const *sample_name;
    int32_t tidy;                                           /* rows are (record, sample) pairs                 */
    uint64_t first_rec_uoff;                                /* inflated offset of the first record             */
} dhts_bcf_info;


typedef struct {
    int64_t n_rows;
    int32_t status;          /* same convention as dhts_bam_batch.status                                    */
    int32_t n_cols;          /* projected columns, in projection order                                      */
    const dhts_bcf_col *cols;/* host array of n_cols descriptors (device pointers inside)                   */
    uint64_t first_rec_uoff, end_uoff;
} dhts_bcf_batch;

int dhts_bcf_open(dhts_ctx *, int tidy_format);                      /* header + dictionaries + schema; positions the scan at the first record */
int dhts_bcf_info_get(const dhts_ctx *, dhts_bcf_info *out);
/* QUAL over PCIe by the batch's own alphabet: when on, dhts_bam_batch_fetch / _fetch_begin look at which characters the batch's QUAL heap holds
 * (one pass on the device) and ship 2 bits per character when there are at most 4, 4 bits when at most 16 (binned base qualities: current Illumina
 * instruments write 4-8 distinct values), the characters themselves otherwise; dhts_bam_batch.qual_bits says which.  The batch in HBM is unchanged. */
void dhts_bam_set_qual_packed(dhts_ctx *, int on);
void dhts_bam_set_seq_packed(dhts_ctx *, int on);                    /* SEQ stays 4 bits per base in the batch: (l + 1) / 2 bytes per row, high nibble first, "=ACMGRSVTWYHKDBN"; len = bases, 0 = "*" */
void dhts_set_super_blocks(dhts_ctx *, int64_t n_blocks);             /* phase A look-ahead (default 524,288 blocks = 67 GB of scratch for a 10 GB file); the table functions use 196,608 */
int dhts_bcf_is_text(const dhts_ctx *);                              /* after dhts_bcf_open: 0 binary BCF, 1 bgzipped VCF text, 2 plain VCF text (also: VCF text inside plain, non-BGZF gzip -- inflated by the serial device decoder at open, bgzf.c:828-905) */
int dhts_bam_is_text(const dhts_ctx *);                              /* after dhts_bam_open: 0 BAM, 1 bgzipped SAM text, 2 plain SAM text (uncompressed, or inside plain gzip),
                                                                      * 3 bgzipped FASTQ, 4 plain FASTQ, 5 bgzipped FASTA, 6 plain FASTA (empty header; one unmapped record per read).  Text
                                                                      * is one sequential scan: regions, index building, shards and header_bytes / region_segments fail on it */
int dhts_bcf_set_projection(dhts_ctx *, const int32_t *col_ids, int32_t n);   /* default: every schema column */
int dhts_bcf_set_block_range(dhts_ctx *, int64_t b0, int64_t b1, int speculative_start);
/* ONE region of read_bcf(region := 'a,b,...'): the reference chains single-region iterators in the order given (src/bcf_reader.c:
 * 1327-1345; overlapping regions repeat rows).  bcf_itr_querys + the overlap test of hts_itr_next (hts.c:4287-4300) over bcf_readrec
 * (vcf.c:2267-2276).  0 = set, 1 = no iterator for this region (unknown contig: skipped by the reference), NULL/"" clears.
 * On VCF text the name is resolved by dhts_bcf_load_index (see there), which must follow before the scan.                          */
int dhts_bcf_set_region(dhts_ctx *, const char *region);
int dhts_bcf_rewind(dhts_ctx *);
int dhts_bcf_next_batch(dhts_ctx *, int64_t max_blocks, dhts_bcf_batch *out);

/* ---- batches in host memory ---------------------------------------------------------------------
 * dhts_host_alloc: pinned (page-locked, portable) host memory from a process-wide pool; dhts_host_free returns it to the pool.
 * dhts_bam_batch_fetch copies the projected core columns (colmask as in dhts_bam_next_batch) of `b` into `dst` -- every copy
 * queued, one wait -- and fills `out` = `b` with HOST pointers for those columns (NULL for unprojected ones); tag columns, the
 * auxiliary map and the overlap lists keep their device pointers.  dhts_bam_batch_host_bytes = the room `dst` needs.
 * This is the seam a DuckDB scan callback fills DataChunks from (src/bam_reader.c:783-918 reads the same values out of bam1_t). */
/* NUMA placement of the host side of a device (multi-GPU hosts have several sockets): the node a device hangs off (hipDeviceGetPCIBusId ->
 * /sys/bus/pci/devices/<id>/numa_node; -1 unknown), and binding of the CALLING thread -- and of the threads it starts afterwards: a
 * producer's staging readers -- to that node's CPUs.  Pinned buffers (dhts_host_alloc) remember the node of the thread that allocated them
 * and are handed to threads of the same node first.  0 bound, 1 nothing to do (no NUMA information, DHTS_NUMA=0), -1 failed.
 * The reference's reader threads (hts_set_threads, src/bam_reader.c:584, 625) are placed by the OS. */
int dhts_device_numa_node(int device);
int dhts_bind_thread_to_node(int node);
int dhts_bind_thread_near_device(int device);
void *dhts_host_alloc(uint64_t nbytes);
void dhts_host_free(void *p);
/* Device buffers of destroyed contexts and freed pinned buffers are kept in process-wide pools (a context per query would otherwise pay
 * hipMalloc / hipHostMalloc of gigabytes each time); this returns every idle pooled buffer to the driver. */
void dhts_release_pools(void);
/* 1 when the context's file bytes were taken over from an earlier context of this process instead of being read and copied again: a file
 * staged WHOLE stays in HBM (in the device pool, tagged with device / inode / size / mtime / ctime) after its context is destroyed, until
 * the pool needs the room (least recently used first) or dhts_release_pools.  DHTS_FILE_CACHE=0 disables it. */
int dhts_resident_from_cache(const dhts_ctx *);
int dhts_device_mem_info(int device, uint64_t *free_bytes, uint64_t *total_bytes);   /* hipMemGetInfo after a device synchronise */
/* CSI writer (src/hts_index_builder.c -> bcf_index_build3; htslib vcf.c:4657-4688, hts.c hts_idx_push / hts_idx_finish / idx_save_core):
 * one scan of the open BCF; the bytes (dhts_bam_index_bytes) are the UNCOMPRESSED index, dhts_bgzf_wrap (host only) turns raw bytes into
 * a valid BGZF file -- stored DEFLATE blocks + the EOF block -- which is what a .csi on disk is. */
/* tabix index of a bgzipped line format other than VCF (tbx_index_build3 with tbx_conf_bed / _gff / _sam or custom columns, tbx.c:437-541):
 * preset = TBX_GENERIC 0 | TBX_SAM 1 (| TBX_UCSC 0x10000 for 0-based half-open coordinates), sc / bc / ec = 1-based sequence, begin and end
 * columns, meta_char / line_skip = lines the indexer passes over.  The context needs dhts_open_path + dhts_bgzf_index only.  The device finds
 * the lines and their intervals (tbx_parse1), the host numbers the names in order of first appearance.  min_shift <= 0: TBI, else CSI.
 * Returns the size of the (uncompressed) index, fetched with dhts_bam_index_bytes. */
int64_t dhts_tabix_build_index(dhts_ctx *, int preset, int sc, int bc, int ec, int meta_char, int line_skip, int min_shift);
/* bgzip / bgunzip (src/bgzip.c:88-293 -> bgzf_write / bgzf_read, htslib bgzf.c): DEFLATE *compression* on the device, one wave per BGZF block
 * (0xff00 input bytes each; fixed-Huffman code, hash-table match finder; a block that does not shrink is stored), CRC-32 and ISIZE included,
 * EOF block appended.  level 0 stores; -1 and 1..9 all select the one compressing setting.  The bytes are not zlib's bytes (no two DEFLATE
 * implementations agree); every reader returns the input.
 * dhts_bgzf_compress: host buffer -> host buffer; returns the size, or an upper bound when out is NULL / cap is below that bound.
 * dhts_bgzip_file / dhts_bgunzip_file: 0, -2 cannot open input (or gzip without a block to read), -3 cannot open output, -4 read / block error, -5 write error.
 * bgunzip reads what bgzf_read reads: BGZF, plain gzip (any content; serial device decoder), and files that are not gzip at all (handed through). */
int64_t dhts_bgzf_compress(dhts_ctx *, const void *raw, uint64_t n, int level, void *out, uint64_t cap);
int dhts_bgzip_file(dhts_ctx *, const char *in_path, const char *out_path, int level, int64_t *bytes_in, int64_t *bytes_out);
int dhts_bgunzip_file(dhts_ctx *, const char *in_path, const char *out_path, int64_t *bytes_in, int64_t *bytes_out);
int64_t dhts_bcf_build_index(dhts_ctx *, int min_shift);          /* min_shift <= 0: 14, the default of bcf_index_build */
/* On bgzipped VCF text the same call is the tabix writer (tbx_index_build3 with tbx_conf_vcf, tbx.c:437-510): min_shift <= 0 writes a TBI
 * (14 / 5 levels), > 0 a CSI whose depth follows the ##contig lengths (hts_adjust_csi_settings) and whose aux block is the tabix header;
 * sequence ids in the order of first appearance, intervals by the tbx_parse1 rule above. */
int64_t dhts_bgzf_wrap(const void *raw, uint64_t n, void *out, uint64_t cap);   /* returns the size needed / written */
/* read_bcf: the room the LAST batch of the context needs, and its read-back: out_cols[b->n_cols] = b->cols with HOST pointers (four queued
 * copies -- validity, fixed payloads, offsets, children / bytes -- and one wait) */
uint64_t dhts_bcf_batch_host_bytes(const dhts_ctx *);
int dhts_bcf_batch_fetch(dhts_ctx *, const dhts_bcf_batch *b, void *dst, uint64_t cap, dhts_bcf_col *out_cols);
int dhts_bcf_batch_fetch_begin(dhts_ctx *, const dhts_bcf_batch *dev_batch, void *dst, uint64_t cap, dhts_bcf_col *host_cols, int slot);   /* overlapped, as dhts_bam_batch_fetch_begin */
int dhts_bcf_batch_fetch_wait(dhts_ctx *, int slot);
uint64_t dhts_bam_batch_host_bytes(const dhts_bam_batch *b, uint32_t colmask);
int dhts_bam_batch_fetch(dhts_ctx *, const dhts_bam_batch *b, uint32_t colmask, void *dst, uint64_t cap, dhts_bam_batch *out);
/* the same read-back overlapped with the next batch: the columns are gathered into one of two device snapshots (slot 0 / 1) and leave for
 * the host as ONE copy on a separate stream; _begin returns at once (out points into dst), _wait(slot) when the bytes have landed.  Call
 * dhts_bam_next_batch in between: PCIe and the scan of the next batch then run side by side. */
int dhts_bam_batch_fetch_begin(dhts_ctx *, const dhts_bam_batch *dev_batch, uint32_t colmask, void *dst, uint64_t cap, dhts_bam_batch *host_batch, int slot);
int dhts_bam_batch_fetch_wait(dhts_ctx *, int slot);

/* ---- fasta_index / read_fasta(region := ...) ------------------------------------------------- */
/* .fai builder (src/seq_reader.c:676-750 -> fai_build3 -> fai_build_core, htslib faidx.c:132-349, a bgzf_getc loop; fai_save :352-377):
 * the context holds the whole file (dhts_open_path / dhts_open_host + dhts_bgzf_index), uncompressed or BGZF.  The device finds the lines,
 * their lengths, isgraph counts and classes, and reduces them per record; the host carries the open record from batch to batch and keeps
 * the first of equal names.  Returns the number of .fai bytes ("name\tlen\toffset\tline_blen\tline_len\n" per sequence), or < 0 with
 * htslib's wording and line number in dhts_error ("Different line length in sequence 'x' at line 7", "File truncated at line 9", ...).
 * FASTQ (a first record that starts with '@') and plain gzip ("Cannot index files compressed with gzip, please use bgzip") are refused. */
int64_t dhts_fasta_build_index(dhts_ctx *);
int dhts_fasta_index_bytes(dhts_ctx *, void *dst, uint64_t n);
/* the .gzi that goes with the .fai of a BGZF file (bgzf_index_dump_hfile, bgzf.c:2382-2408, as the single-threaded read path records it,
 * :1225-1236): a u64 count, then (compressed, uncompressed) u64 offsets of every non-empty block behind the first.  n = 0 asks for the
 * size; 0 bytes for uncompressed input. */
int64_t dhts_fasta_gzi_bytes(dhts_ctx *, void *dst, uint64_t n);
/* fai_read (faidx.c:380-446): the first of equal names stays; a line without four numbers is an error */
int dhts_fasta_load_index(dhts_ctx *, const void *fai, uint64_t n);
/* stages what the regions 'a:1-10,b' read, by the loaded .fai: of an uncompressed file only the byte windows of the regions (merged where
 * they touch; dhts_resident_bytes says how much), of a BGZF file everything -- it is inflated whole on the first fetch, so no .gzi is needed */
int dhts_fasta_open_regions(dhts_ctx *, const char *path, const char *regions);
/* fai_fetch64 for every region of 'a:1-10,b' in one launch (fai_parse_region with flags 0; fai_get_val's clamping, faidx.c:798-827;
 * fai_retrieve :716-796): regions are split at commas, blanks trimmed, empty pieces dropped (src/seq_reader.c:192-229), one row per region
 * in the order given.  name = the region text up to its first ':' (seq_reader.c:443-446).  Columns are DEVICE pointers: offsets have
 * n_rows + 1 entries.  beg >= len gives an empty string; an unknown name, line_blen 0 in the index and a source byte behind the end of the
 * file are errors.  Works on resident bytes from dhts_fasta_open_regions, dhts_open_path or dhts_open_host. */
typedef struct {
    int64_t n_rows;
    const uint64_t *name_off; const uint8_t *name_bytes; uint64_t name_nbytes;
    const uint64_t *seq_off; const uint8_t *seq_bytes; uint64_t seq_nbytes;
} dhts_fasta_batch;
int dhts_fasta_fetch(dhts_ctx *, const char *regions, dhts_fasta_batch *out);
/* read-back in the style of dhts_bam_batch_fetch: `out` = `b` with HOST pointers into dst */
uint64_t dhts_fasta_batch_host_bytes(const dhts_fasta_batch *b);
int dhts_fasta_batch_fetch(dhts_ctx *, const dhts_fasta_batch *b, void *dst, uint64_t cap, dhts_fasta_batch *out);

/* ---- read_bed --------------------------------------------------------------------------------
 *   dhts_bed_open / dhts_bed_next_batch  <- read_bed_init / read_bed_scan over next_bed_line          src/interval_udf.c:295-426
 *                                           (hts_getline or tbx_itr_next; is_meta_bed_line, count_tab_fields, get_field_span,
 *                                           get_extra_span, parse_int64_span_local :127-195)
 * The 13 columns of src/interval_udf.c:217-235, in that order.  BIGINT: start, end, thick_start, thick_end, block_count (strtoll over the
 * whole field, else NULL); VARCHAR: the others, NULL when the field is absent or empty; extra = everything behind the 12th tab. */
enum { DHTS_BED_CHROM = 0, DHTS_BED_START, DHTS_BED_END, DHTS_BED_NAME, DHTS_BED_SCORE, DHTS_BED_STRAND, DHTS_BED_THICK_START, DHTS_BED_THICK_END,
       DHTS_BED_ITEM_RGB, DHTS_BED_BLOCK_COUNT, DHTS_BED_BLOCK_SIZES, DHTS_BED_BLOCK_STARTS, DHTS_BED_EXTRA, DHTS_BED_COL_COUNT };
typedef struct {
    int64_t n_rows;
    int32_t status;          /* 0 = more data may follow, 1 = end of stream reached cleanly, <0 = the stream ended on an error after these rows
                                (a line with fewer than 3 fields: dhts_error has read_bed's message and the line number)                   */
    int32_t n_cols;          /* projected columns, in projection order                                                                     */
    const dhts_col *cols;    /* host array of n_cols descriptors, DEVICE pointers inside: valid[n_rows]; BIGINT in fixed (8 bytes, 0 where
                                NULL), VARCHAR in off[n_rows + 1] / bytes (one arena per column)                                           */
} dhts_bed_batch;
/* after dhts_open_path* / dhts_open_host and dhts_bgzf_index (whose result does not matter here): BGZF, plain gzip and uncompressed text
 * are read, whatever the text looks like (hts_getline has no format).  Shards and index building fail on such a context. */
int dhts_bed_open(dhts_ctx *);
int dhts_bed_set_projection(dhts_ctx *, const int32_t *col_ids, int32_t n);   /* DHTS_BED_* ids, each once; default all 13; n = 0: only n_rows (count(*)) */
/* ONE region as tbx_itr_querys takes it ("seq", "seq:1,000-2,000": commas are thousands separators, not a list; "." = every record; NULL /
 * "" clears).  The name is one of the INDEX's sequences: dhts_bed_load_index (.tbi, or .csi with the tabix header) resolves it -- 0, 1 = the
 * index does not know it (the reference: "failed to create region iterator"), <0 error -- and narrows the scan to the index windows.  Rows
 * are kept by hts_itr_next's test on the interval tbx_parse1 gives the line under the index's OWN configuration (preset, columns), not by
 * the BED columns.  Fails on uncompressed or plain-gzip text. */
int dhts_bed_set_region(dhts_ctx *, const char *region);
int dhts_bed_load_index(dhts_ctx *, const void *index_bytes, uint64_t n);
/* what a region query stages instead of the file, for dhts_open_path_segments with header_bytes = 0 (BED has no header; conventions of
 * dhts_bam_region_segments, *count = -1: the whole file).  Needs no open file.  Returns 1 when the index does not know the sequence. */
int dhts_bed_region_segments(dhts_ctx *, const char *region, const void *index_bytes, uint64_t n, uint64_t *beg, uint64_t *end, int64_t cap, int64_t *count);
/* next batch of rows (<= max_blocks BGZF blocks, or 65,280-byte pieces of text; 0 = default); lines open at the end are carried over */
int dhts_bed_next_batch(dhts_ctx *, int64_t max_blocks, dhts_bed_batch *out);
/* read-back: out_cols[b->n_cols] = b->cols with HOST pointers into dst */
uint64_t dhts_bed_batch_host_bytes(const dhts_bed_batch *b);
int dhts_bed_batch_fetch(dhts_ctx *, const dhts_bed_batch *b, void *dst, uint64_t cap, dhts_col *out_cols);

/* ---- fasta_nuc -------------------------------------------------------------------------------
 *   dhts_nuc_open / _set_region        <- fasta_nuc_init, init_fasta_region                           src/interval_udf.c:558-627
 *   dhts_nuc_next_bins                 <- next_fasta_nuc_bin_interval                                 :684-726
 *   dhts_nuc_next_bed                  <- next_fasta_nuc_bed_interval, bed_overlap_region             :645-682
 *   every row                          <- fasta_nuc_scan :728-836: faidx_fetch_seq64(start, end - 1) (htslib faidx.c:914-983),
 *                                         count_nucleotides :629-643, pct_at / pct_gc :765-768
 * The 13 columns of add_fasta_nuc_columns (:451-473), in that order.  VARCHAR: chrom, seq; DOUBLE: pct_at, pct_gc; BIGINT: the others.
 * Rows: end - start <= 0 gives a row without any fetch (counts 0, seq_len = end - start, seq NULL, unknown chrom included); otherwise a
 * chrom the .fai does not know, line_blen 0 and bases behind the end of the file drop the row, and seq_len is what
 * faidx_adjust_position(end_adjust = 1) leaves of (start, end - 1).  start and end are always the caller's / the BED's own numbers. */
enum { DHTS_NUC_CHROM = 0, DHTS_NUC_START, DHTS_NUC_END, DHTS_NUC_PCT_AT, DHTS_NUC_PCT_GC, DHTS_NUC_NUM_A, DHTS_NUC_NUM_C, DHTS_NUC_NUM_G, DHTS_NUC_NUM_T,
       DHTS_NUC_NUM_N, DHTS_NUC_NUM_OTHER, DHTS_NUC_SEQ_LEN, DHTS_NUC_SEQ, DHTS_NUC_COL_COUNT };
typedef struct {
    int64_t n_rows;
    int32_t status;          /* 0 = more rows may follow, 1 = the last batch                                                               */
    int32_t n_cols;          /* projected columns, in projection order                                                                     */
    const dhts_col *cols;    /* host array of n_cols descriptors, DEVICE pointers inside: valid[n_rows]; BIGINT and DOUBLE in fixed
                                (8 bytes), VARCHAR in off[n_rows + 1] / bytes                                                              */
} dhts_nuc_batch;
/* stages what a query with `region` reads of the FASTA at `path`, by the loaded .fai (dhts_fasta_load_index first): of an uncompressed file
 * the byte window of the region's bases -- with whole_sequence, for BED mode, of the whole sequence the region names, since a BED row
 * that overlaps the region may reach past it -- of a BGZF file everything.  ONE region: commas are thousands separators, not a list. */
int dhts_nuc_open_region(dhts_ctx *fasta, const char *path, const char *region, int whole_sequence);
/* after the FASTA is resident (dhts_open_path / dhts_open_host / dhts_nuc_open_region) and dhts_fasta_load_index: the index goes to
 * the device.  Fails with a message that names the FASTA index when none is loaded.  include_seq adds the 13th column. */
int dhts_nuc_open(dhts_ctx *fasta, int include_seq);
/* ONE region as init_fasta_region reads it: fai_parse_region with flags 0, then fai_adjust_region.  Returns 1 for a region the reference
 * calls invalid (unknown name, malformed, or one fai_adjust_region had to move: a start behind the sequence, an explicit end behind it).
 * NULL / "" clears.  Bins mode walks the region; BED mode keeps the rows that pass bed_overlap_region. */
int dhts_nuc_set_region(dhts_ctx *fasta, const char *region);
/* DHTS_NUC_* ids, each once (DHTS_NUC_SEQ only with include_seq); default all; n = 0: only n_rows (count(*)).  With none of pct_at ..
 * num_other projected the bases are not read. */
int dhts_nuc_set_projection(dhts_ctx *fasta, const int32_t *col_ids, int32_t n);
/* the next <= max_rows bins (0 = default) of the region or of every sequence, in order; built on the device from the bin number */
int dhts_nuc_next_bins(dhts_ctx *fasta, int64_t bin_width, int64_t max_rows, dhts_nuc_batch *out);
/* the rows of the next batch of `bed`, a second context on the same device prepared as for read_bed (dhts_bed_open; with a region and a
 * tabix index also dhts_bed_set_region + dhts_bed_load_index).  Lines are read by fasta_nuc's rules: fewer than three fields, or a start
 * or end that is not a whole number, skip the line.  chrom is resolved against the .fai on the device. */
int dhts_nuc_next_bed(dhts_ctx *fasta, dhts_ctx *bed, int64_t max_blocks, dhts_nuc_batch *out);
/* rows for n intervals in host arrays, tid = index of the sequence in the .fai (< 0: a chrom it does not know) */
int dhts_nuc_intervals(dhts_ctx *fasta, const int32_t *tid, const int64_t *start, const int64_t *end, int64_t n, dhts_nuc_batch *out);
/* read-back: out_cols[b->n_cols] = b->cols with HOST pointers into dst */
uint64_t dhts_nuc_batch_host_bytes(const dhts_nuc_batch *b);
int dhts_nuc_batch_fetch(dhts_ctx *fasta, const dhts_nuc_batch *b, void *dst, uint64_t cap, dhts_col *out_cols);

/* ---- bam_bin_counts --------------------------------------------------------------------------
 * Read-start counts in fixed-width bins with a strand split, accumulated on the device from the fixed-width columns a read_bam batch
 * leaves in HBM: no row crosses PCIe.  The reference has only a plan for it (.github/PLAN.md, Phase 10, 10.7.2; its SQL equivalent is
 * read_bam + flag functions + GROUP BY), so this is the specification.
 *   Input: the rows of the context's read_bam scan in file order, i.e. what dhts_bam_open reads after the device region filter.  Per row:
 *     flag, tid, pos0 = POS - 1, mapq, pnext.
 *   Each row falls out at exactly one step, and every step has a 64-bit counter:
 *     1. flags -> n_flag_filtered: the row passes iff (flag & require_flags) == require_flags, (flag & exclude_flags) == 0 and
 *        (include_flags == 0 || (flag & include_flags) != 0)            (samtools -f / -F / --rf)
 *     2. placement: tid < 0 or pos0 < 0 -> n_unplaced; pos0 >= ref_len[tid] -> n_out_of_range.  Such rows never touch the table.
 *     3. duplicate, only with dedup = adjacent -> n_duplicate: let p be the previous row, in file order and across batches, that passed
 *        steps 1 and 2.  The row is a duplicate iff p exists, p.tid == tid, p.pos0 == pos0 and ((flag & 1) == 0 or p.pnext == pnext).
 *        Rows that failed step 1 or 2 are invisible to the rule; rows that fall out at step 3 or 4 still become p for the next row.
 *        This is the adjacent-start rule of the plan, "WisecondorX-like"; it is not FLAG & 0x400 and not exact compatibility.
 *     4. MAPQ -> n_low_mapq: mapq < min_mapq (after the duplicate step, as in the plan)
 *     5. counted -> n_counted: bin b = pos0 / bin_width of contig tid, reverse iff flag & 0x10, forward otherwise.
 *     n_rows = the sum of the six counters.
 *   Result rows: contigs in header order, bins ascending; a bin is a row where count_total > 0, or everywhere with emit_zero_bins
 *     (with regions: every bin of every contig a region names).  chrom (here: the contig's id), start = b * bin_width,
 *     end = min(start + bin_width, ref_len) -- the clipping of fasta_nuc's bins, so the two join on (chrom, start, end) -- bin_id = b,
 *     count_total = count_fwd + count_rev, count_fwd, count_rev.  A contig of length 0 has no bins; a header without references gives no rows.
 *   Limits: more than 2^28 bins in total is an error that states the bin count.  A batch with status < 0 has its rows counted and the
 *     result carries that status.  A shard or a block range other than the whole file is refused: the duplicate rule does not cross shards.
 *   Left out of the plan's signature: strand_mode (both strands are always counted) and reference (CRAM is not read; GC columns are a
 *     join with fasta_nuc).
 * Every call on a context in the wrong state fails with a dhts_error that names what is missing.  The kernels are timed as DHTS_K_BCF_CHECK. */
enum { DHTS_BINS_DEDUP_NONE = 0, DHTS_BINS_DEDUP_ADJACENT = 1 };
enum { DHTS_BINS_CHROM = 0, DHTS_BINS_START, DHTS_BINS_END, DHTS_BINS_BIN_ID, DHTS_BINS_COUNT_TOTAL, DHTS_BINS_COUNT_FWD, DHTS_BINS_COUNT_REV, DHTS_BINS_COL_COUNT };
typedef struct {
    int64_t bin_width;       /* > 0 (the table function's default: 5000)                                      */
    int32_t min_mapq;        /* 0..255                                                                        */
    int32_t require_flags, exclude_flags, include_flags;   /* 0..65535                                        */
    int32_t dedup;           /* DHTS_BINS_DEDUP_*                                                             */
    int32_t emit_zero_bins;
} dhts_bins_params;
typedef struct {
    uint64_t n_rows, n_flag_filtered, n_unplaced, n_out_of_range, n_duplicate, n_low_mapq, n_counted;
    uint64_t total_bins;     /* bins of the table: the sum of ceil(ref_len / bin_width)                        */
    int32_t status;          /* the status of the last batch that had one: 0 = the scan has not ended, 1 = clean end, < 0 = the stream
                                ended on an error after the counted rows                                       */
    int32_t reserved;
} dhts_bins_stats;
typedef struct {
    int64_t n_rows;
    int32_t status;          /* 0 = more rows follow, 1 = the last batch                                                                   */
    int32_t n_cols;          /* DHTS_BINS_COL_COUNT, in that order                                                                         */
    const dhts_col *cols;    /* host array of descriptors, DEVICE pointers inside: valid[n_rows] (all 1), fixed = 8-byte integers           */
} dhts_bins_batch;
/* after dhts_bam_open and the optional dhts_bam_set_regions / dhts_bam_load_index: the table and the counters, zeroed */
int dhts_bam_bins_open(dhts_ctx *, const dhts_bins_params *params);
/* any batch of this context's scan (a caller may feed the batches it scans itself; FLAG, tid, POS, MAPQ and PNEXT are always there) */
int dhts_bam_bins_accumulate(dhts_ctx *, const dhts_bam_batch *batch);
/* dhts_bam_next_batch (<= max_blocks blocks each, no string column) + accumulate to the end of the stream.  Returns the status the stream
 * ended on: 1, or its negative status (the rows are counted; dhts_bins_stats.status repeats it); a call that failed returns < 0 with
 * dhts_error set and leaves dhts_bins_stats.status 0. */
int dhts_bam_bins_scan(dhts_ctx *, int64_t max_blocks);
int dhts_bam_bins_stats(dhts_ctx *, dhts_bins_stats *out);
/* the next <= max_rows result rows (0 = default); an accumulate call starts the result over */
int dhts_bam_bins_next(dhts_ctx *, int64_t max_rows, dhts_bins_batch *out);
/* read-back: out_cols[b->n_cols] = b->cols with HOST pointers into dst */
uint64_t dhts_bam_bins_batch_host_bytes(const dhts_bins_batch *b);
int dhts_bam_bins_batch_fetch(dhts_ctx *, const dhts_bins_batch *b, void *dst, uint64_t cap, dhts_col *out_cols);

/* ---- bam_bedcov ------------------------------------------------------------------------------
 * For every interval of a BED file the summed per-base depth and the number of reads that overlap it (what `samtools bedcov [-c] [-j]`
 * prints), accumulated on the device from the fixed-width columns and the binary CIGARs a read_bam batch leaves in HBM: no row crosses
 * PCIe.  The reference has only a plan for it (.github/PLAN.md, Phase 10, 10.6.1 / 10.7.3; its SQL equivalent is a range join of read_bam
 * with read_bed plus CIGAR arithmetic per pair), so this is the specification.
 *   Input: the rows of the context's read_bam scan in file order, i.e. what dhts_bam_open reads after the device region filter, and the rows
 *     of a BED file as read_bed returns them (its line rules; a line with fewer than three fields is its error).  BED row i is
 *     (chrom_i, s_i, e_i), 0-based half-open; chrom_i is resolved against the BAM header (the first @SQ of a name listed twice).
 *   Each read falls out at exactly one step, and every step has a 64-bit counter:
 *     1. flags -> n_flag_filtered: the three-mask rule of bam_bin_counts
 *     2. placement -> n_unplaced: tid < 0, tid >= n_ref or pos0 < 0.  Positions are not compared with ref_len.
 *     3. MAPQ -> n_low_mapq: mapq < min_mapq
 *     4. counted -> n_counted
 *     n_rows = the sum of the four counters.
 *   A counted read has
 *     the read interval [pos0, pos0 + max(1, rlen)): rlen = the reference length of the effective CIGAR (the CG tag's when the record has
 *       one), 0 when FLAG & 4 is set -- bam_endpos, as the region filter computes it;
 *     depth segments: the maximal runs of reference positions its CIGAR covers by M, = and X, by D when count_deletions is on and by N
 *       when count_ref_skips is on.  A read with FLAG & 4, or without such an operation, has none; with both options on there is at most
 *       one, [pos0, pos0 + rlen).
 *   Result: one row per BED row, in BED file order.  chrom, start, end, name, score, strand are read_bed's columns with its types and NULLs;
 *     bases_covered BIGINT = the sum over the segments [a, b) on the row's contig of max(0, min(b, e) - max(a, s));
 *     read_count BIGINT = the counted reads on that contig with pos0 < e and read_end > s.
 *     Both are 0, not NULL, for a row with e <= s, a NULL start or end, or a chrom the header lacks.  Overlapping, nested and repeated
 *     rows are each answered independently.
 *   Parameters: min_mapq 0..255; require_flags, exclude_flags, include_flags 0..65535; count_deletions, count_ref_skips 0 or 1.  This ABI
 *     takes the masks as given; the table function and the Python function default exclude_flags to 0x704 (UNMAP, SECONDARY, QCFAIL, DUP:
 *     samtools' default) and both options to on.
 *   Limits: more than 2^27 BED rows is an error that states the count.  A batch with status < 0 has its rows counted and the result carries
 *     that status.  A shard or a block range other than the whole file is refused.
 *   Not in this contract: depth thresholds (-d), several BAM files, reference / CRAM, a region on the BED side.  A region and an index on
 *     the BAM side work as in bam_bin_counts: they restrict which reads are scanned, and nothing else.
 *   Method: the counters are O(breakpoints) -- the distinct starts and ends of the BED rows per contig -- not O(genome); a segment costs a
 *     constant number of atomics, and the result is a 64-bit prefix sum over the breakpoints (csrc/bam_bedcov.hip).
 * Every call on a context in the wrong state fails with a dhts_error that names what is missing.  The kernels are timed as DHTS_K_BCF_CHECK. */
enum { DHTS_BEDCOV_CHROM = 0, DHTS_BEDCOV_START, DHTS_BEDCOV_END, DHTS_BEDCOV_NAME, DHTS_BEDCOV_SCORE, DHTS_BEDCOV_STRAND, DHTS_BEDCOV_BASES_COVERED,
       DHTS_BEDCOV_READ_COUNT, DHTS_BEDCOV_COL_COUNT };
typedef struct {
    int32_t min_mapq;        /* 0..255                                                                        */
    int32_t require_flags, exclude_flags, include_flags;   /* 0..65535                                        */
    int32_t count_deletions, count_ref_skips;              /* 0 or 1                                          */
} dhts_bedcov_params;
typedef struct {
    uint64_t n_rows, n_flag_filtered, n_unplaced, n_low_mapq, n_counted;
    uint64_t n_bed_rows;     /* rows of the BED file                                                           */
    uint64_t n_breakpoints;  /* distinct (contig, position) pairs among the starts and ends of its valid rows   */
    int32_t status;          /* the status of the last batch that had one: 0 = the scan has not ended, 1 = clean end, < 0 = the stream
                                ended on an error after the counted rows                                       */
    int32_t reserved;
} dhts_bedcov_stats;
typedef struct {
    int64_t n_rows;
    int32_t status;          /* 0 = more rows follow, 1 = the last batch                                                                   */
    int32_t n_cols;          /* DHTS_BEDCOV_COL_COUNT, in that order                                                                       */
    const dhts_col *cols;    /* host array of descriptors, DEVICE pointers inside: valid[n_rows]; BIGINT (start, end, bases_covered,
                                read_count) in fixed (8 bytes, 0 where NULL), VARCHAR in off[n_rows + 1] / bytes                           */
} dhts_bedcov_batch;
/* after dhts_bam_open on `bam` (and the optional dhts_bam_set_regions / dhts_bam_load_index).  `bed` is a second context on the same device,
 * prepared as for read_bed (dhts_bed_open).  One pass over it collects contig, start and end of every row; the breakpoints go to the device
 * and the counters are zeroed.  A second open starts a new count.  The projection of `bed` belongs to bam_bedcov from here on. */
int dhts_bam_bedcov_open(dhts_ctx *bam, dhts_ctx *bed, const dhts_bedcov_params *params);
/* the batch dhts_bam_next_batch returned LAST on this context: the binary CIGARs are read where the scan left them (the inflated stream and the
 * record offsets of a batch stay in HBM until the next one is made), so the scan needs no string column.  Starts a result over. */
int dhts_bam_bedcov_accumulate(dhts_ctx *bam, const dhts_bam_batch *batch);
/* dhts_bam_next_batch (<= max_blocks blocks each, no string column) + accumulate to the end of the stream.  Returns the status the stream
 * ended on: 1, or its negative status (the rows are counted; dhts_bedcov_stats.status repeats it); a call that failed returns < 0 with
 * dhts_error set and leaves dhts_bedcov_stats.status 0. */
int dhts_bam_bedcov_scan(dhts_ctx *bam, int64_t max_blocks);
int dhts_bam_bedcov_stats(dhts_ctx *bam, dhts_bedcov_stats *out);
/* the result for the rows of the next batch of `bed` (<= max_blocks blocks of it, 0 = default): a second pass over the BED context, whose six
 * passthrough columns are followed by the two result columns for the same rows.  The first call after open or accumulate rewinds `bed` and
 * takes the prefix sums. */
int dhts_bam_bedcov_next(dhts_ctx *bam, dhts_ctx *bed, int64_t max_blocks, dhts_bedcov_batch *out);
/* read-back: out_cols[b->n_cols] = b->cols with HOST pointers into dst */
uint64_t dhts_bam_bedcov_batch_host_bytes(const dhts_bedcov_batch *b);
int dhts_bam_bedcov_batch_fetch(dhts_ctx *bam, const dhts_bedcov_batch *b, void *dst, uint64_t cap, dhts_col *out_cols);

/* ---- bam_coverage ----------------------------------------------------------------------------
 * Per contig or region: numreads, covbases, coverage, meandepth, meanbaseq, meanmapq (what `samtools coverage` prints), accumulated on the
 * device from the fixed-width columns, the binary CIGARs and the QUAL bytes a read_bam batch leaves in HBM: nothing but one row per contig
 * leaves the device.  The reference has only a plan for it (.github/PLAN.md, Phase 10, 10.4 / 10.7.3; its SQL equivalent is read_bam with
 * CIGAR and QUAL plus a per-base expansion), so this is the specification.
 *   Input: the rows of the context's read_bam scan in file order, i.e. what dhts_bam_open reads after the device region filter.
 *   Target rows: without regions one row per @SQ in header order, [0, ref_len).  With regions (dhts_bam_set_regions, and an index as in
 *     bam_bin_counts) one row per region that names a contig, in the order given: [beg, end), 0-based half-open, clipped to ref_len ('.' and
 *     '*' name no row; with nothing but them the rows are the @SQ's).  Regions on one contig that overlap each other are refused at open
 *     with an error that names the two; adjacent ones are fine.  A row of length 0 is emitted with all-zero results.
 *   Each read falls out at exactly one step, and every step has a 64-bit counter:
 *     1. flags -> n_flag_filtered: the three-mask rule of bam_bin_counts
 *     2. placement -> n_unplaced: tid < 0, tid >= n_ref or pos0 < 0
 *     3. length -> n_short: l_seq < min_read_len                               (samtools' order: length before MAPQ)
 *     4. MAPQ -> n_low_mapq: mapq < min_mapq
 *     5. overlaps no target row -> n_outside: the read interval is bam_bedcov's, [pos0, pos0 + max(1, rlen)), rlen from the effective CIGAR
 *        (the CG tag's when the record has one), 0 with FLAG & 4
 *     6. counted -> n_counted
 *     n_rows = the sum of the six counters.
 *   A counted read adds 1 to numreads and its MAPQ to sum_mapq of every row its interval overlaps.
 *   Counted bases: a reference position x of the read counts iff it is covered by an M, = or X operation (D, N and P never count), x lies
 *     inside the row, and with q the query index of that base q >= l_seq or qual[q] >= min_baseq.  QUAL bytes are taken as they are (0xff is
 *     255).  Each counted base adds 1 to depth[x] and qual[q] (0 when q >= l_seq) to the row's sum_baseq; q >= l_seq covers SEQ = * and a
 *     CIGAR longer than l_seq.  A read with FLAG & 4 has no counted bases.  There is no mate-overlap handling and no hidden flag mask.
 *   Result per row: chrom (here: the contig's id), start, end, numreads, covbases = # positions with depth >= min_depth (BIGINT);
 *     coverage = 100 * covbases / (end - start), meandepth = sum_depth / (end - start), meanbaseq = sum_baseq / sum_depth,
 *     meanmapq = sum_mapq / numreads (DOUBLE: one IEEE division of the two 64-bit integers converted to double, 0.0 for a zero
 *     denominator); behind these nine the BIGINT sums sum_depth, sum_baseq, sum_mapq.  min_depth affects covbases and coverage only.
 *   Parameters: min_read_len >= 0; min_mapq, min_baseq 0..255; the three masks 0..65535; min_depth >= 1.  This ABI takes them as given; the
 *     table function and the Python function default exclude_flags to 0x704, min_depth to 1 and the rest to 0.
 *   Limits: depth per position is 32-bit.  The depth table takes 4 bytes per position of every target row (each row's span rounded up to
 *     1,024 slots); beyond the cap (16 GiB; a human genome needs 12.4 GB) open fails with an error that states the bytes needed and the cap.
 *     A batch with status < 0 has its rows counted and the result carries that status.  A shard or a block range other than the whole file
 *     is refused.
 *   Not in this contract: bam_list (several files), reference / CRAM and max_depth (htslib's pileup cap depends on the order reads arrive in:
 *     it has no order-free definition).  The depth histogram is bam_depth_hist's (below).
 *   Method: a 32-bit difference table, two atomics per maximal run of counted bases; QUAL is read in aligned 16-byte pieces by eight lanes
 *     per read; the result is a scan of the table reduced per tile and summed per row (csrc/bam_coverage.hip).
 * Every call on a context in the wrong state fails with a dhts_error that names what is missing.  The kernels are timed as DHTS_K_BCF_CHECK. */
enum { DHTS_COVERAGE_CHROM = 0, DHTS_COVERAGE_START, DHTS_COVERAGE_END, DHTS_COVERAGE_NUMREADS, DHTS_COVERAGE_COVBASES, DHTS_COVERAGE_COVERAGE,
       DHTS_COVERAGE_MEANDEPTH, DHTS_COVERAGE_MEANBASEQ, DHTS_COVERAGE_MEANMAPQ, DHTS_COVERAGE_SUM_DEPTH, DHTS_COVERAGE_SUM_BASEQ, DHTS_COVERAGE_SUM_MAPQ,
       DHTS_COVERAGE_COL_COUNT };
typedef struct {
    int64_t min_read_len;    /* >= 0                                                                          */
    int64_t min_depth;       /* >= 1                                                                          */
    int32_t min_mapq;        /* 0..255                                                                        */
    int32_t min_baseq;       /* 0..255                                                                        */
    int32_t require_flags, exclude_flags, include_flags;   /* 0..65535                                        */
    int32_t reserved;
} dhts_coverage_params;
typedef struct {
    uint64_t n_rows, n_flag_filtered, n_unplaced, n_short, n_low_mapq, n_outside, n_counted;
    uint64_t n_target_rows;  /* rows of the result                                                             */
    uint64_t table_bytes;    /* bytes of the depth table                                                       */
    int32_t status;          /* the status of the last batch that had one: 0 = the scan has not ended, 1 = clean end, < 0 = the stream
                                ended on an error after the counted rows                                       */
    int32_t reserved;
} dhts_coverage_stats;
typedef struct {
    int64_t n_rows;
    int32_t status;          /* 0 = more rows follow, 1 = the last batch                                                                   */
    int32_t n_cols;          /* DHTS_COVERAGE_COL_COUNT, in that order                                                                     */
    const dhts_col *cols;    /* host array of descriptors, DEVICE pointers inside: valid[n_rows] (all 1), fixed = 8 bytes per row: BIGINT,
                                or the bits of a DOUBLE (coverage .. meanmapq)                                                             */
} dhts_coverage_batch;
/* after dhts_bam_open and the optional dhts_bam_set_regions / dhts_bam_load_index: the target rows, the depth table and the counters, zeroed.
 * A second open starts a new count. */
int dhts_bam_coverage_open(dhts_ctx *, const dhts_coverage_params *params);
/* the batch dhts_bam_next_batch returned LAST on this context: CIGAR and QUAL are read where the scan left them (the inflated stream and the
 * record offsets of a batch stay in HBM until the next one is made), so the scan needs no string column.  Starts a result over. */
int dhts_bam_coverage_accumulate(dhts_ctx *, const dhts_bam_batch *batch);
/* dhts_bam_next_batch (<= max_blocks blocks each, no string column) + accumulate to the end of the stream.  Returns the status the stream
 * ended on: 1, or its negative status (the rows are counted; dhts_coverage_stats.status repeats it); a call that failed returns < 0 with
 * dhts_error set and leaves dhts_coverage_stats.status 0. */
int dhts_bam_coverage_scan(dhts_ctx *, int64_t max_blocks);
int dhts_bam_coverage_stats(dhts_ctx *, dhts_coverage_stats *out);
/* the next <= max_rows result rows (0 = default).  The first call after open or accumulate takes the result from the table, which stays as
 * it is: a later accumulate adds to intact counters and the result is taken again. */
int dhts_bam_coverage_next(dhts_ctx *, int64_t max_rows, dhts_coverage_batch *out);
/* read-back: out_cols[b->n_cols] = b->cols with HOST pointers into dst */
uint64_t dhts_bam_coverage_batch_host_bytes(const dhts_coverage_batch *b);
int dhts_bam_coverage_batch_fetch(dhts_ctx *, const dhts_coverage_batch *b, void *dst, uint64_t cap, dhts_col *out_cols);

/* ---- bam_depth -------------------------------------------------------------------------------
 * Per position: chrom, pos, depth (what `samtools depth` prints), streamed page by page out of the depth table bam_coverage's add pass fills in
 * HBM: the per-base result is never resident as a whole, on the device or on the host.  The reference has only a plan for it (.github/PLAN.md,
 * Phase 10, 10.4 / 10.7.3), so this is the specification.
 *   Input, the six steps with their 64-bit counters, the read interval, the effective CIGAR (the CG tag's) and the rule that a read with
 *     FLAG & 4 has no counted base: exactly bam_coverage's.
 *   Target rows without a BED: exactly bam_coverage's -- one per @SQ, or one per region in the order given, clipped to ref_len; regions that
 *     overlap are refused with an error that names the two; empty rows are allowed (they emit nothing).
 *   Target rows with a BED (a second context, as in dhts_bam_bedcov_open): the union of the BED's rows -- per contig in header order, sorted by
 *     start, with overlapping, nested, duplicate and adjacent rows merged into maximal intervals, clipped to ref_len, empty ones dropped.  BED
 *     rows that name a contig the header lacks are skipped and counted (n_bed_skipped).  A BED together with regions is refused by name.
 *     Every merged interval costs at least 4 KiB of table: a row's span is padded to 1,024 slots, as in bam_coverage.
 *   Counted bases: as in bam_coverage -- covered by M, = or X, inside a row, and q >= l_seq or qual[q] >= min_baseq.  With include_deletions
 *     every reference position of a D operation inside a row counts as well, whatever min_baseq and the qualities of the bases around it are;
 *     a leading or trailing D counts.  N and P never count.
 *   Result: one row per emitted position: chrom (here: the contig's id, int32), pos (1-based, int64), depth (int32).  Order: the target rows
 *     in result order (the order given for regions, sorted order otherwise), positions ascending inside a row.  all_positions:
 *       0  positions with depth > 0
 *       1  (-a) every position of every target row on a touched contig, positions with depth > 0 elsewhere (there are none, by construction).
 *          A contig is touched iff at least one read reached step 6 (counted) against any of its target rows -- a counted read without a
 *          counted base included.
 *       2  (-aa) every position of every target row
 *   Parameters: min_read_len >= 0; min_mapq, min_baseq 0..255; the three masks 0..65535; include_deletions 0..1; all_positions 0..2.  This ABI
 *     takes them as given; the table function and the Python function default exclude_flags to 0x704 and the rest to 0.
 *   Limits: bam_coverage's -- 32-bit depth, the table cap and its error (dhts_debug_coverage_max_table_bytes applies to both functions), a
 *     shard or block range refused, a stream that ends on an error has its rows counted and its status carried.
 *   Not in this contract: suppress_overlaps (mates are not paired on the device), several input files, reference / CRAM and max_depth.  The
 *     run-length (bedGraph) form of the result is bam_bedgraph's (below).
 *   Method: the add pass without the per-row words, a D joined to the runs around it; a carry in two levels for the depth and the result index
 *     in front of every tile; a page is a window of result indices, emitted by the tiles that hold it (csrc/bam_depth.hip).
 * All errors are prefixed "bam_depth:".  Every call on a context in the wrong state fails with a dhts_error that names what is missing. */
enum { DHTS_DEPTH_CHROM = 0, DHTS_DEPTH_POS, DHTS_DEPTH_DEPTH, DHTS_DEPTH_COL_COUNT };
typedef struct {
    int64_t min_read_len;    /* >= 0                                                                          */
    int32_t min_mapq;        /* 0..255                                                                        */
    int32_t min_baseq;       /* 0..255                                                                        */
    int32_t require_flags, exclude_flags, include_flags;   /* 0..65535                                        */
    int32_t include_deletions;                             /* 0 or 1                                          */
    int32_t all_positions;                                 /* 0, 1 (-a) or 2 (-aa)                            */
    int32_t reserved;
} dhts_depth_params;
typedef struct {
    uint64_t n_rows, n_flag_filtered, n_unplaced, n_short, n_low_mapq, n_outside, n_counted;
    uint64_t n_target_rows;  /* target rows (regions, @SQ lines or merged BED intervals)                       */
    uint64_t n_bed_skipped;  /* BED rows that name a contig the header lacks                                   */
    uint64_t table_bytes;    /* bytes of the depth table                                                       */
    uint64_t n_positions;    /* rows of the whole result: valid once a result was taken (dhts_bam_depth_next), 0 before */
    int32_t status;          /* as in dhts_coverage_stats                                                      */
    int32_t reserved;
} dhts_depth_stats;
typedef struct {
    int64_t n_rows;
    int32_t status;          /* 0 = more rows follow, 1 = the last page                                                                    */
    int32_t n_cols;          /* DHTS_DEPTH_COL_COUNT, in that order                                                                        */
    const dhts_col *cols;    /* host array of descriptors, DEVICE pointers inside: fixed = int32 (chrom, depth) or int64 (pos) per row, a
                                null pointer for a column colmask left out; no row is NULL and valid stays a null pointer                   */
} dhts_depth_batch;
/* after dhts_bam_open and the optional dhts_bam_set_regions / dhts_bam_load_index.  bed: NULL, or a second context on the same device prepared
 * as for read_bed (dhts_bed_open); its projection belongs to bam_depth from here on.  The target rows, the depth table and the counters,
 * zeroed.  A second open starts a new count. */
int dhts_bam_depth_open(dhts_ctx *bam, const dhts_depth_params *params, dhts_ctx *bed);
/* the batch dhts_bam_next_batch returned LAST on this context, as in dhts_bam_coverage_accumulate.  Starts a result over: the table and the
 * counters stay intact, the next dhts_bam_depth_next returns the first page of the new result. */
int dhts_bam_depth_accumulate(dhts_ctx *bam, const dhts_bam_batch *batch);
/* dhts_bam_next_batch + accumulate to the end of the stream; returns as dhts_bam_coverage_scan does */
int dhts_bam_depth_scan(dhts_ctx *bam, int64_t max_blocks);
int dhts_bam_depth_stats(dhts_ctx *bam, dhts_depth_stats *out);
/* the next <= max_rows rows of the result (0 = 1,048,576 rows: 16 MiB with all three columns).  colmask: bit DHTS_DEPTH_* set = the column is
 * written and fetched; a query that reads depth alone moves 4 bytes per row.  The first call after open or accumulate counts the rows of the
 * result from the table, which stays as it is.  The page's columns stay valid until the next call on the context. */
int dhts_bam_depth_next(dhts_ctx *bam, int64_t max_rows, uint32_t colmask, dhts_depth_batch *out);
/* read-back: out_cols[b->n_cols] = b->cols with HOST pointers into dst (null where the batch has none); the columns follow each other,
 * each rounded up to 8 bytes */
uint64_t dhts_bam_depth_batch_host_bytes(const dhts_depth_batch *b);
int dhts_bam_depth_batch_fetch(dhts_ctx *bam, const dhts_depth_batch *b, void *dst, uint64_t cap, dhts_col *out_cols);

/* ---- bam_pileup ------------------------------------------------------------------------------
 * Per position and strand: how many A, C, G, T, N, '=', deletions and insertions lie on it (an Rsamtools-style base-level pileup), counted
 * into a table in HBM from the columns, the binary CIGARs and the SEQ and QUAL bytes a read_bam batch leaves there, and streamed page by
 * page as the compaction of that table.  The reference has only a plan for it (.github/PLAN.md, Phase 10, 10.4 / 10.7.3), so this is the
 * specification.
 *   Input, the six steps with their 64-bit counters, the read interval, the effective CIGAR (the CG tag's) and the rule that a read with
 *     FLAG & 4 contributes nothing: exactly bam_coverage's.
 *   Target rows: exactly bam_coverage's -- one per @SQ, or one per region in the order given, clipped to ref_len; regions that overlap are
 *     refused with an error that names the two; empty rows emit nothing.  There is no BED and no all_positions here.
 *   Symbols, eight, in this order: A C G T N = - +.
 *     A base of an M, = or X operation at reference position x inside a row, with query index q, counts iff q >= l_seq or
 *       qual[q] >= min_baseq (bam_coverage's rule).  Its symbol comes from the 4-bit code of SEQ: 1, 2, 4, 8 give A, C, G, T; 0 gives '=';
 *       every other code (15 and the ambiguity codes) gives N; q >= l_seq (SEQ = *, or a CIGAR longer than l_seq) gives N.
 *     '-' only with include_deletions: every reference position of a D operation inside a row counts, whatever min_baseq and the qualities
 *       of the bases around it are; a leading or trailing D counts.
 *     '+' only with include_insertions: every I operation of non-zero length adds 1 at its anchor, the reference position x - 1 where x is
 *       the reference position the walk stands on at the I.  The last operation before the I that consumed reference must be M, =, X or D,
 *       not N; S, I, P, H and zero-length operations in between are skipped; the anchor must lie inside a row; an I with no reference
 *       consumed before it has no anchor and does not count; qualities play no part.  Two I operations with the same anchor count twice
 *       (htslib's pileup sees one event there).
 *     N and P operations never count.
 *   Strand: with distinguish_strands '-' iff FLAG & 16, else '+'; without it '*'.
 *   Result: one row per (position, strand, symbol) whose count is at least min_nucleotide_depth: chrom (here: the contig's id, int32), pos
 *     (1-based, int64), strand (uint8, ASCII '+', '-' or '*'), nucleotide (uint8, ASCII of the eight symbols), count (int32).  Order: the
 *     target rows in result order, then positions ascending, then '+' before '-', then the symbols in the order above.
 *   Parameters: min_read_len >= 0; min_mapq, min_baseq 0..255; the three masks 0..65535; include_deletions, include_insertions,
 *     distinguish_strands 0..1; min_nucleotide_depth >= 1.  This ABI takes them as given; the table function and the Python function default
 *     exclude_flags to 0x704, include_deletions to 1, include_insertions to 0, distinguish_strands to 1 (Rsamtools' PileupParam),
 *     min_nucleotide_depth to 1 and the rest to 0.
 *   Limits: counts are 32-bit.  The count table takes 4 bytes x 8 symbols x (2 with strands, else 1) per position of every target row, each
 *     row's span laid out as in bam_coverage ((end - beg) + 1 positions rounded up to 1,024 positions).  dhts_debug_coverage_max_table_bytes
 *     and the 16 GiB cap apply; beyond the cap open fails with "bam_pileup: the count table needs N bytes (B per position of every row); at
 *     most C are supported (fewer or shorter regions)".  A whole human genome therefore needs a region per contig: chr1 with strands is
 *     15.9 GB and fits.  A shard or block range is refused; a stream that ends on an error has its rows counted and its status carried.
 *   Not in this contract: mate-overlap handling, max_depth (for the reason given under bam_coverage), reference / CRAM, several files, a
 *     BED, a wide one-row-per-position form, and sweeping a genome in several scans.
 *   Method: one atomic add per counted base, SEQ read as aligned words by the eight lanes that read QUAL; the result is the table's words
 *     compacted tile by tile behind a 64-bit carry (csrc/bam_pileup.hip).
 * All errors are prefixed "bam_pileup:".  Every call on a context in the wrong state fails with a dhts_error that names what is missing. */
enum { DHTS_PILEUP_CHROM = 0, DHTS_PILEUP_POS, DHTS_PILEUP_STRAND, DHTS_PILEUP_NUCLEOTIDE, DHTS_PILEUP_COUNT, DHTS_PILEUP_COL_COUNT };
typedef struct {
    int64_t min_read_len;    /* >= 0                                                                          */
    int32_t min_mapq;        /* 0..255                                                                        */
    int32_t min_baseq;       /* 0..255                                                                        */
    int32_t require_flags, exclude_flags, include_flags;   /* 0..65535                                        */
    int32_t include_deletions;                             /* 0 or 1                                          */
    int32_t include_insertions;                            /* 0 or 1                                          */
    int32_t distinguish_strands;                           /* 0 or 1                                          */
    int32_t min_nucleotide_depth;                          /* >= 1                                            */
    int32_t reserved;
} dhts_pileup_params;
typedef struct {
    uint64_t n_rows, n_flag_filtered, n_unplaced, n_short, n_low_mapq, n_outside, n_counted;
    uint64_t n_target_rows;  /* target rows (regions or @SQ lines)                                             */
    uint64_t table_bytes;    /* bytes of the count table                                                       */
    uint64_t n_result_rows;  /* rows of the whole result: valid once a result was taken (dhts_bam_pileup_next), 0 before */
    int32_t status;          /* as in dhts_coverage_stats                                                      */
    int32_t reserved;
} dhts_pileup_stats;
typedef struct {
    int64_t n_rows;
    int32_t status;          /* 0 = more rows follow, 1 = the last page                                                                    */
    int32_t n_cols;          /* DHTS_PILEUP_COL_COUNT, in that order                                                                       */
    const dhts_col *cols;    /* host array of descriptors, DEVICE pointers inside: fixed = int32 (chrom, count), int64 (pos) or uint8 (strand,
                                nucleotide) per row, a null pointer for a column colmask left out; no row is NULL and valid stays null       */
} dhts_pileup_batch;
/* after dhts_bam_open and the optional dhts_bam_set_regions / dhts_bam_load_index: the target rows, the count table and the counters,
 * zeroed.  A second open starts a new count. */
int dhts_bam_pileup_open(dhts_ctx *bam, const dhts_pileup_params *params);
/* the batch dhts_bam_next_batch returned LAST on this context, as in dhts_bam_coverage_accumulate (SEQ is read where the scan left it, too).
 * Starts a result over: the table and the counters stay intact, the next dhts_bam_pileup_next returns the first page of the new result. */
int dhts_bam_pileup_accumulate(dhts_ctx *bam, const dhts_bam_batch *batch);
/* dhts_bam_next_batch + accumulate to the end of the stream; returns as dhts_bam_coverage_scan does */
int dhts_bam_pileup_scan(dhts_ctx *bam, int64_t max_blocks);
int dhts_bam_pileup_stats(dhts_ctx *bam, dhts_pileup_stats *out);
/* the next <= max_rows rows of the result (0 = 1,048,576 rows: 18 MiB with all five columns).  colmask: bit DHTS_PILEUP_* set = the column
 * is written and fetched.  The first call after open or accumulate counts the rows of the result from the table, which stays as it is.  The
 * page's columns stay valid until the next call on the context. */
int dhts_bam_pileup_next(dhts_ctx *bam, int64_t max_rows, uint32_t colmask, dhts_pileup_batch *out);
/* read-back: out_cols[b->n_cols] = b->cols with HOST pointers into dst (null where the batch has none); the columns follow each other,
 * each rounded up to 8 bytes */
uint64_t dhts_bam_pileup_batch_host_bytes(const dhts_pileup_batch *b);
int dhts_bam_pileup_batch_fetch(dhts_ctx *bam, const dhts_pileup_batch *b, void *dst, uint64_t cap, dhts_col *out_cols);

/* ---- bam_bedgraph ----------------------------------------------------------------------------
 * Per run of equal depth class: chrom, start, end, depth -- bedGraph rows, what `bedtools genomecov -bg / -bga` and `mosdepth --quantize`
 * print -- cut and paged on the device out of the depth table bam_depth's add pass fills in HBM.  The rows join read_bed, fasta_nuc and
 * bam_bin_counts on the same 0-based half-open key.  The reference has only a plan for it (.github/PLAN.md, Phase 10), so this is the
 * specification.
 *   Input, the six steps with their 64-bit counters, the read interval, the effective CIGAR, the counted bases (include_deletions: every
 *     reference position of a D operation inside a row counts, a leading or trailing D too; N and P never count) and the target rows -- one
 *     per @SQ, one per region in the order given, or the merged intervals of a BED (n_bed_skipped; at least 4 KiB of table each, a row's span
 *     is padded to 1,024 slots): exactly bam_depth's.  A BED together with regions is refused by name; regions that overlap are refused.
 *   Classes: breaks is up to 16 strictly increasing integers in 1 .. 2147483647.  class(d) = the number of breaks <= d.  The reported depth of
 *     class 0 is 0, of class j > 0 it is breaks[j - 1] (the class's lower edge; its upper edge is the next break).  Without breaks
 *     class(d) = d and the reported depth is d.
 *   Runs: inside one target row a run is a maximal stretch of positions of equal class.  A run never spans two target rows, not even
 *     adjacent regions of one contig.  A run is emitted iff its class is > 0 or zero_runs is 1; with zero_runs a contig of length L that no
 *     read touches gives the one row (chrom, 0, L, 0).
 *   Result: one row per emitted run: chrom (here: the contig's id, int32), start (0-based, int64), end (exclusive, int64), depth (int32, the
 *     reported depth of the run's class).  No column is ever NULL.  Order: the target rows in the order they are answered in (the order given
 *     for regions, sorted order otherwise), then by start.
 *   The identity that defines correctness: without breaks, every row (chrom, start, end, d) of zero_runs = 1 expanded into the positions
 *     start + 1 .. end is exactly bam_depth with all_positions = 2 on the same input and parameters; zero_runs = 0 gives all_positions = 0.
 *     There is no counterpart of all_positions = 1 (touched contigs).
 *   Parameters: min_read_len >= 0; min_mapq, min_baseq 0..255; the three masks 0..65535; include_deletions, zero_runs 0..1; n_breaks 0..16.
 *     This ABI takes them as given; the table function and the Python function default exclude_flags to 0x704 and the rest to 0.
 *   Limits: bam_depth's -- 32-bit depth, the table cap and its error (dhts_debug_coverage_max_table_bytes applies here as well), a shard or
 *     block range refused, a stream that ends on an error has its rows counted and its status carried.
 *   Not in this contract: a mean depth per class run, suppress_overlaps, several input files, reference / CRAM, max_depth.  The depth
 *     histogram is bam_depth_hist's (below).
 *   Method: bam_depth's add pass; per tile the emitted boundaries and its first boundary of any class, a suffix minimum in two levels for the
 *     next boundary behind every tile and a carry in two levels for the result index in front of it; a page is a window of result indices,
 *     emitted by the tiles that hold it, and a run that leaves its tile ends where the suffix minimum says, clipped to its row
 *     (csrc/bam_bedgraph.hip).
 * All errors are prefixed "bam_bedgraph:".  Every call on a context in the wrong state fails with a dhts_error that names what is missing. */
enum { DHTS_BEDGRAPH_CHROM = 0, DHTS_BEDGRAPH_START, DHTS_BEDGRAPH_END, DHTS_BEDGRAPH_DEPTH, DHTS_BEDGRAPH_COL_COUNT };
typedef struct {
    int64_t min_read_len;    /* >= 0                                                                          */
    int32_t min_mapq;        /* 0..255                                                                        */
    int32_t min_baseq;       /* 0..255                                                                        */
    int32_t require_flags, exclude_flags, include_flags;   /* 0..65535                                        */
    int32_t include_deletions;                             /* 0 or 1                                          */
    int32_t zero_runs;                                     /* 0 or 1: runs of class 0 are emitted             */
    int32_t n_breaks;                                      /* 0..16                                           */
    int32_t breaks[16];                                    /* the first n_breaks: strictly increasing, >= 1   */
    int32_t reserved[2];
} dhts_bedgraph_params;
typedef struct {
    uint64_t n_rows, n_flag_filtered, n_unplaced, n_short, n_low_mapq, n_outside, n_counted;
    uint64_t n_target_rows;  /* target rows (regions, @SQ lines or merged BED intervals)                       */
    uint64_t n_bed_skipped;  /* BED rows that name a contig the header lacks                                   */
    uint64_t table_bytes;    /* bytes of the depth table                                                       */
    uint64_t n_runs;         /* rows of the whole result: valid once a result was taken (dhts_bam_bedgraph_next), 0 before */
    int32_t status;          /* as in dhts_coverage_stats                                                      */
    int32_t reserved;
} dhts_bedgraph_stats;
typedef struct {
    int64_t n_rows;
    int32_t status;          /* 0 = more rows follow, 1 = the last page                                                                    */
    int32_t n_cols;          /* DHTS_BEDGRAPH_COL_COUNT, in that order                                                                     */
    const dhts_col *cols;    /* host array of descriptors, DEVICE pointers inside: fixed = int32 (chrom, depth) or int64 (start, end) per row,
                                a null pointer for a column colmask left out; no row is NULL and valid stays a null pointer                 */
} dhts_bedgraph_batch;
/* after dhts_bam_open and the optional dhts_bam_set_regions / dhts_bam_load_index.  bed: NULL, or a second context on the same device prepared
 * as for read_bed (dhts_bed_open); its projection belongs to bam_bedgraph from here on.  The target rows, the depth table and the counters,
 * zeroed.  A second open starts a new count. */
int dhts_bam_bedgraph_open(dhts_ctx *bam, const dhts_bedgraph_params *params, dhts_ctx *bed);
/* the batch dhts_bam_next_batch returned LAST on this context, as in dhts_bam_depth_accumulate.  Starts a result over: the table and the
 * counters stay intact, the next dhts_bam_bedgraph_next returns the first page of the new result. */
int dhts_bam_bedgraph_accumulate(dhts_ctx *bam, const dhts_bam_batch *batch);
/* dhts_bam_next_batch + accumulate to the end of the stream; returns as dhts_bam_coverage_scan does */
int dhts_bam_bedgraph_scan(dhts_ctx *bam, int64_t max_blocks);
int dhts_bam_bedgraph_stats(dhts_ctx *bam, dhts_bedgraph_stats *out);
/* the next <= max_rows rows of the result (0 = 1,048,576 rows: 24 MiB with all four columns).  colmask: bit DHTS_BEDGRAPH_* set = the column
 * is written and fetched.  The first call after open or accumulate counts the runs of the result from the table, which stays as it is.  The
 * page's columns stay valid until the next call on the context. */
int dhts_bam_bedgraph_next(dhts_ctx *bam, int64_t max_rows, uint32_t colmask, dhts_bedgraph_batch *out);
/* read-back: out_cols[b->n_cols] = b->cols with HOST pointers into dst (null where the batch has none); the columns follow each other,
 * each rounded up to 8 bytes */
uint64_t dhts_bam_bedgraph_batch_host_bytes(const dhts_bedgraph_batch *b);
int dhts_bam_bedgraph_batch_fetch(dhts_ctx *bam, const dhts_bedgraph_batch *b, void *dst, uint64_t cap, dhts_col *out_cols);

/* ---- bam_bedgraph_export ----------------------------------------------------------------------
 * The result of bam_bedgraph written as a bgzipped bedGraph file (`chrom \t start \t end \t depth \n` per row, decimal, the contig by its name)
 * with its tabix index -- mosdepth's per-base.bed.gz + .csi -- without a result row crossing PCIe: the pages of the result are printed on the
 * device (csrc/rows_text.hip), compressed on the device (bgzip's encoder) and only the compressed bytes reach the host and the file.  It is the
 * writer layer the reference plans (.github/PLAN.md, 10.5.4 / 10.7.4) for this one result; the reference has no code for it, so this is the
 * specification.  (The entry is dhts_bedgraph_export: the dhts_bam_bedgraph_* names are the seven of the count function.)
 *   Call it after dhts_bam_bedgraph_open and a scan (or any number of accumulates).  The rows are dhts_bam_bedgraph_next's, in its order.  On
 *     return the paging state is as after an accumulate: the next dhts_bam_bedgraph_next returns page one.
 *   The identity that defines correctness: the file's bytes equal what dhts_bgzip_file makes of the plain text of the same rows at the same
 *     level, whatever the page size and the chunk size: blocks of 0xff00 bytes of the row stream, the last one short, then the EOF block.  This
 *     holds because the encoder compresses every block on its own: a block's bytes depend on its 0xff00 input bytes and the level alone.
 *   Parameters: level as dhts_bgzip_file (0 stores, every other value is the one compressing setting); index 0 none, 1 TBI (out_path + ".tbi"),
 *     2 CSI (out_path + ".csi", min_shift <= 0: 14); overwrite 0 / 1.
 *   Index: after the file is closed the existing tabix writer (dhts_tabix_build_index) reads it back through a scratch context on the same
 *     device with the BED preset (0-based half-open, columns 1 / 2 / 3), and the index is wrapped by dhts_bgzf_wrap.  With an index and regions
 *     the regions must keep each contig's rows together and ascending; without an index any region order is written as answered.
 *   Empty result: the file is the 28-byte EOF block; the index is what dhts_tabix_build_index makes of that file: a valid index without a
 *     sequence name, on which every region query finds no such sequence.
 *   Returns 0, or: -1 a call in the wrong state, a parameter out of range or a device error; -3 an output cannot be opened; -5 write error;
 *     -6 out_path exists and overwrite is 0 (the file is left alone); -7 the regions are not in file order; -8 the index could not be built.
 *     Behind every failure but -6 neither output file is left.  dhts_error names the cause with the prefix "bam_bedgraph_export:".
 *   With dhts_set_timing the count and emit kernels are timed as DHTS_K_SCAN, the encoder's lengths and carry as DHTS_K_BCF_MEASURE, its write
 *     pass as DHTS_K_BCF_WRITE and the compressor as DHTS_K_HUFF.
 *   Not in this contract: building the index from the row arrays without reading the file back; other results than bam_bedgraph's (the
 *     encoder is generic over a name column and up to 8 integer columns; bam_bin_counts is to follow); .tsv.gz; several threads of file I/O. */
typedef struct {
    int32_t level;           /* as dhts_bgzip_file                                                            */
    int32_t index;           /* 0 none, 1 TBI, 2 CSI                                                           */
    int32_t min_shift;       /* CSI: <= 0 is 14                                                                */
    int32_t overwrite;       /* 0 or 1                                                                         */
    int32_t reserved[4];
} dhts_bedgraph_export_params;
typedef struct {
    uint64_t n_rows;         /* rows written                                                                   */
    uint64_t bytes_text;     /* bytes of their text                                                            */
    uint64_t bytes_out;      /* bytes of the file, EOF block included                                          */
    uint64_t bytes_index;    /* bytes of the index file, 0 without one                                         */
    int32_t status;          /* the scan's, as in dhts_bedgraph_stats                                          */
    int32_t reserved;
} dhts_bedgraph_export_stats;
int dhts_bedgraph_export(dhts_ctx *bam, const char *out_path, const dhts_bedgraph_export_params *p, dhts_bedgraph_export_stats *out);

/* ---- bam_depth_hist ---------------------------------------------------------------------------
 * Per group of target rows and per depth: the number of positions on that depth -- mosdepth's *.dist.txt, the COV section of `samtools stats`,
 * "what fraction of the target is covered at >= 20x" -- binned on the device out of the depth table bam_depth's add pass fills in HBM.  The
 * per-base result never leaves the device; the answer is a few thousand rows.  The reference has no counterpart, so this is the specification.
 *   Input, the six steps with their 64-bit counters, the read interval, the effective CIGAR, the counted bases (include_deletions: every
 *     reference position of a D operation inside a row counts; N and P never count) and the target rows -- one per @SQ, one per region in the
 *     order given, or the merged intervals of a BED (n_bed_skipped; a row's span is padded to 1,024 slots): exactly bam_depth's.  A BED
 *     together with regions is refused by name; regions that overlap are refused.
 *   Groups: per = 0 ('row'): a group is one target row, in the order answered.  per = 1 ('contig'): a group is all non-empty target rows of one
 *     contig, with the contigs in header order; a contig without a non-empty target row has no group.  A target row that is empty after
 *     clipping contributes nothing under either value.  Any other value: "bam_depth_hist: per must be 'row' or 'contig'".
 *   Bins: bin(d) = min(d, depth_cap), so the last bin holds every position of depth >= depth_cap (`samtools stats`' [1000<]).  depth_cap is an
 *     integer in 1 .. 1,048,575; otherwise "bam_depth_hist: depth_cap must be between 1 and 1048575".
 *   The identity that defines correctness: for every group g and every d in 0 .. depth_cap, n_positions(g, d) is the number of positions p in
 *     g's rows with bin(depth(p)) == d, where depth(p) is what bam_depth with all_positions = 2 answers for p on the same input and parameters.
 *     Padding slots of a row's span never count.
 *   Result: one row per group and per bin with n_positions > 0, ordered by group and then by depth ascending: chrom (here: the contig's id,
 *     int32), start (0-based, int64; with 'contig' the least start of the group's rows), end (exclusive, int64; with 'contig' the greatest
 *     end), depth (int32, the bin), n_positions (int64), n_at_least (int64: the sum of n_positions over the bins >= this one in the group) and
 *     length (int64: the positions of the group, the sum of its rows' end - start).  No column is ever NULL.  An untouched contig of length L
 *     gives the single row (chrom, 0, L, 0, L, L, L).  The table function adds fraction_at_least = n_at_least / length from the two integers.
 *   The histogram table: groups x (depth_cap + 1) 64-bit words, zeroed at open, at most 1 GiB (dhts_debug_hist_max_table_bytes sets the cap
 *     for tests).  Past the cap open fails with "bam_depth_hist: the histogram needs N bytes (8 per bin of every group); at most C are
 *     supported (per := 'contig' or a smaller depth_cap)": 200,000 exome targets at the default cap exceed it per row and fit per contig.
 *   Reaccumulate: an accumulate after a page was taken starts the result over.  The depth table and the counters stay; the histogram is
 *     zeroed and made again from the depth table, of which it is a pure function.
 *   Parameters: min_read_len >= 0; min_mapq, min_baseq 0..255; the three masks 0..65535; include_deletions 0..1; depth_cap; per 0..1.  This
 *     ABI takes them as given; the table function and the Python function default exclude_flags to 0x704, depth_cap to 1000, per to 'row'.
 *   Limits: bam_depth's -- 32-bit depth, the 16 GiB cap of the depth table and its error (dhts_debug_coverage_max_table_bytes applies here as
 *     well), a shard or block range refused, a stream that ends on an error has its rows counted and its status carried.
 *   Not in this contract: a 'total' group (SQL sums the contigs), dense output of empty bins, mosdepth --thresholds per BED row,
 *     suppress_overlaps, several input files, reference / CRAM, max_depth.
 *   Method: bam_depth's add pass; tile sums and their carry; one read of the table by workgroups that own a span of tiles and count into an
 *     LDS histogram of 4,096 bins, flushed into the table where the group changes; per group the non-empty bins and their carry; a page is a
 *     window of result indices, emitted by the groups that hold it from the top bin down behind a suffix sum (csrc/bam_depth_hist.hip,
 *     DESIGN.md 4p).
 * The entries are dhts_bam_hist_*: the names that begin dhts_bam_depth_ are bam_depth's own.
 * All errors are prefixed "bam_depth_hist:".  Every call on a context in the wrong state fails with a dhts_error that names what is missing. */
enum { DHTS_DEPTH_HIST_CHROM = 0, DHTS_DEPTH_HIST_START, DHTS_DEPTH_HIST_END, DHTS_DEPTH_HIST_DEPTH, DHTS_DEPTH_HIST_N_POSITIONS, DHTS_DEPTH_HIST_N_AT_LEAST,
       DHTS_DEPTH_HIST_LENGTH, DHTS_DEPTH_HIST_COL_COUNT };
typedef struct {
    int64_t min_read_len;    /* >= 0                                                                          */
    int32_t min_mapq;        /* 0..255                                                                        */
    int32_t min_baseq;       /* 0..255                                                                        */
    int32_t require_flags, exclude_flags, include_flags;   /* 0..65535                                        */
    int32_t include_deletions;                             /* 0 or 1                                          */
    int32_t depth_cap;                                     /* 1..1048575: the last bin                        */
    int32_t per;                                           /* 0 = 'row', 1 = 'contig'                         */
    int32_t reserved[2];
} dhts_depth_hist_params;
typedef struct {
    uint64_t n_rows, n_flag_filtered, n_unplaced, n_short, n_low_mapq, n_outside, n_counted;
    uint64_t n_target_rows;  /* target rows (regions, @SQ lines or merged BED intervals)                       */
    uint64_t n_groups;       /* groups: the non-empty target rows, or the contigs that have one                */
    uint64_t n_bed_skipped;  /* BED rows that name a contig the header lacks                                   */
    uint64_t table_bytes;    /* bytes of the depth table                                                       */
    uint64_t hist_bytes;     /* bytes of the histogram table                                                   */
    uint64_t n_result_rows;  /* rows of the whole result: valid once a result was taken (dhts_bam_hist_next), 0 before */
    int32_t status;          /* as in dhts_coverage_stats                                                      */
    int32_t reserved;
} dhts_depth_hist_stats;
typedef struct {
    int64_t n_rows;
    int32_t status;          /* 0 = more rows follow, 1 = the last page                                                                    */
    int32_t n_cols;          /* DHTS_DEPTH_HIST_COL_COUNT, in that order                                                                   */
    const dhts_col *cols;    /* host array of descriptors, DEVICE pointers inside: fixed = int32 (chrom, depth) or int64 (the rest) per row,
                                a null pointer for a column colmask left out; no row is NULL and valid stays a null pointer                 */
} dhts_depth_hist_batch;
/* after dhts_bam_open and the optional dhts_bam_set_regions / dhts_bam_load_index.  bed: NULL, or a second context on the same device prepared
 * as for read_bed (dhts_bed_open); its projection belongs to bam_depth_hist from here on.  The target rows, the groups, the two tables and the
 * counters, zeroed.  A second open starts a new count. */
int dhts_bam_hist_open(dhts_ctx *bam, const dhts_depth_hist_params *params, dhts_ctx *bed);
/* the batch dhts_bam_next_batch returned LAST on this context, as in dhts_bam_depth_accumulate.  Starts a result over: the depth table and the
 * counters stay intact, the next dhts_bam_hist_next makes the histogram anew and returns the first page of the new result. */
int dhts_bam_hist_accumulate(dhts_ctx *bam, const dhts_bam_batch *batch);
/* dhts_bam_next_batch + accumulate to the end of the stream; returns as dhts_bam_coverage_scan does */
int dhts_bam_hist_scan(dhts_ctx *bam, int64_t max_blocks);
int dhts_bam_hist_stats(dhts_ctx *bam, dhts_depth_hist_stats *out);
/* the next <= max_rows rows of the result (0 = 1,048,576 rows: 48 MiB with all seven columns).  colmask: bit DHTS_DEPTH_HIST_* set = the
 * column is written and fetched.  The first call after open or accumulate reads the depth table, which stays as it is, into the histogram.
 * The page's columns stay valid until the next call on the context. */
int dhts_bam_hist_next(dhts_ctx *bam, int64_t max_rows, uint32_t colmask, dhts_depth_hist_batch *out);
/* read-back: out_cols[b->n_cols] = b->cols with HOST pointers into dst (null where the batch has none); the columns follow each other,
 * each rounded up to 8 bytes */
uint64_t dhts_bam_hist_batch_host_bytes(const dhts_depth_hist_batch *b);
int dhts_bam_hist_batch_fetch(dhts_ctx *bam, const dhts_depth_hist_batch *b, void *dst, uint64_t cap, dhts_col *out_cols);

/* ---- read_tabix / read_gtf / read_gff ---------------------------------------------------------
 * src/tabix_reader.c.  The context is prepared as for read_bed (dhts_open_path[_segments] + dhts_bgzf_index): BGZF, plain gzip and
 * uncompressed text are read.  Bind is dhts_tabix_set_conf + dhts_tabix_sniff + dhts_tabix_resolve_schema + dhts_tabix_set_schema;
 * GTF / GFF have the fixed schema of :564-587 and need none of them. */
enum { DHTS_TABIX_GENERIC = 0, DHTS_TABIX_GTF = 1, DHTS_TABIX_GFF = 2 };
enum { DHTS_TABIX_MAX_COLS = 256,       /* TABIX_MAX_GENERIC_COLS                                                    */
       DHTS_GXF_ATTRIBUTES_MAP = 9 };   /* projection id of attributes_map in GTF / GFF mode (ids 0..8: seqname .. attributes) */
/* hts_open + tabix_init :786-846 for `mode`; positions the scan at the first line.  Shards, block ranges other than the whole file and index
 * building fail on such a context. */
int dhts_tabix_open(dhts_ctx *, int mode);
/* what bind takes from the index, tbx->conf :649-656: the meta character (0: none) and line_skip.  '#' / 0 after dhts_tabix_open; GTF / GFF
 * keep '#' / 0 whatever an index says (their bind never loads it) and refuse this call. */
int dhts_tabix_set_conf(dhts_ctx *, int meta_char, int line_skip);
/* the peek of bind :658-679 on the device's line table of the first batch(es); only the bytes of the header candidate are fetched.
 * n_fields = count_fields of the first data line (0: there is none); candidate = the line `header := true` takes its names from when no
 * header_names are given (have_candidate; owned by the context, valid until the next call on it): the last line of the line_skip prefix
 * (candidate_from_skip) or else the first line that is neither empty nor meta.  The scan is rewound afterwards. */
typedef struct { int32_t n_fields, have_candidate, candidate_from_skip, reserved; const char *candidate; uint64_t candidate_len; } dhts_tabix_sniffed;
int dhts_tabix_sniff(dhts_ctx *, int header, int have_header_names, dhts_tabix_sniffed *out);
/* the rest of bind :684-771, host only (no context): names, types (DHTS_T_INTEGER / _BIGINT / _DOUBLE / _VARCHAR, parse_type_name :218-230)
 * and skip_header_line.  header_names / column_types: NULL or n = 0 when the parameter is absent.  auto_detect :709-755 looks at up to 100
 * data rows: cells[r * n_cols + k] / cell_len[...] are the fields of row r under the returned n_cols (NULL = the line has no such field);
 * when it needs them and cells is NULL the call fills `out` with the all-VARCHAR schema and returns 1: scan 100 rows under it (after
 * dhts_tabix_set_schema), rewind, and call again.  names[k] point into memory of the library that stays valid until the calling thread's
 * next dhts_tabix_resolve_schema.  < 0: the message is in err. */
typedef struct {
    int32_t n_cols, skip_header_line;
    int32_t types[DHTS_TABIX_MAX_COLS]; const char *names[DHTS_TABIX_MAX_COLS];
} dhts_tabix_schema;
int dhts_tabix_resolve_schema(const dhts_tabix_sniffed *sniffed, int header, const char *const *header_names, int32_t n_header_names,
                              const char *const *column_types, int32_t n_column_types, int auto_detect,
                              const char *const *cells, const uint32_t *cell_len, int32_t n_cell_rows, dhts_tabix_schema *out, char *err, uint64_t err_cap);
/* generic mode: the schema bind resolved (INTEGER is parsed as BIGINT: the consumer narrows); the projection becomes every column */
int dhts_tabix_set_schema(dhts_ctx *, int32_t n_cols, const int32_t *types, int skip_header_line);
/* column ids, each once (init :834-843); n = 0: only n_rows.  GTF / GFF: 0..8 and DHTS_GXF_ATTRIBUTES_MAP; default 0..8 */
int dhts_tabix_set_projection(dhts_ctx *, const int32_t *col_ids, int32_t n);
/* ONE region at a time, with dhts_bed_set_region / _load_index / _region_segments' conventions (tbx_itr_querys; the caller splits
 * region := 'a,b' by parse_regions :301-344 and chains the scans, tabix_advance_region_iterator :346-360).  Inside a region query line_skip
 * and the header line are not applied (:898, 903 test !id->itr). */
int dhts_tabix_set_region(dhts_ctx *, const char *region);
int dhts_tabix_load_index(dhts_ctx *, const void *index_bytes, uint64_t n);
int dhts_tabix_region_segments(dhts_ctx *, const char *region, const void *index_bytes, uint64_t n, uint64_t *beg, uint64_t *end, int64_t cap, int64_t *count);
/* what an index says for dhts_tabix_set_conf (.tbi, or .csi with the tabix header; BGZF or already inflated): 0, < 0 not a tabix index */
int dhts_tabix_index_conf(dhts_ctx *, const void *index_bytes, uint64_t n, int32_t *meta_char, int32_t *line_skip);
/* attributes_map (fill_attr_map :412-494): row r owns pairs pair_off[r] .. pair_off[r + 1] - 1; pair p has the key key_bytes[key_off[p],
 * key_off[p + 1]) and the value val_bytes[val_off[p], val_off[p + 1]).  valid[r] = 0: NULL map (field 8 missing, empty or "."). */
typedef struct {
    const uint32_t *pair_off; const uint8_t *valid; uint64_t n_pairs;
    const uint32_t *key_off; const uint8_t *key_bytes; uint64_t key_nbytes;
    const uint32_t *val_off; const uint8_t *val_bytes; uint64_t val_nbytes;
} dhts_tabix_map;
typedef struct {
    int64_t n_rows;
    int32_t status;          /* 0 = more data may follow, 1 = end of stream reached cleanly, < 0 = the stream ended on an error            */
    int32_t n_cols;          /* projected columns, in projection order                                                                     */
    const dhts_col *cols;    /* as dhts_bed_batch.cols: BIGINT and DOUBLE in fixed (8 bytes), VARCHAR in off / bytes.  The descriptor of
                                attributes_map is empty: `map` holds it                                                                    */
    const int32_t *col_types;/* host array: DHTS_T_* of every projected column (attributes_map: 0)                                          */
    int32_t has_map, reserved;
    dhts_tabix_map map;
    uint64_t n_double_fast, n_double_patched;   /* DOUBLE tokens of this batch converted on the device / by strtod on the host (the columns
                                                   are complete on the device either way)                                                  */
} dhts_tabix_batch;
int dhts_tabix_next_batch(dhts_ctx *, int64_t max_blocks, dhts_tabix_batch *out);     /* the loop body of tabix_scan :880-1028 */
/* read-back: out_cols[b->n_cols] = b->cols and *out_map = b->map with HOST pointers into dst (out_map may be NULL without a map) */
uint64_t dhts_tabix_batch_host_bytes(const dhts_tabix_batch *b);
int dhts_tabix_batch_fetch(dhts_ctx *, const dhts_tabix_batch *b, void *dst, uint64_t cap, dhts_col *out_cols, dhts_tabix_map *out_map);

/* ---- seq_* / cigar_* / SAM flag functions on device columns --------------------------------------
 * register_kmer_udf_functions (src/kmer_udf.c:1223-1254) evaluated where a batch lives: the arguments are DEVICE columns -- the seq, cigar
 * and flag of a dhts_bam_batch as they are, or host values brought over by dhts_udf_upload -- and so are the results.
 *   DHTS_UDF_SEQ_REVCOMP               <- seq_revcomp_scalar :297-336, dna_complement :88-97
 *   DHTS_UDF_SEQ_CANONICAL             <- seq_canonical_scalar :338-388
 *   DHTS_UDF_SEQ_HASH_2BIT             <- seq_hash_2bit_scalar :390-427, dna_to_2bit :99-107
 *   DHTS_UDF_SEQ_ENCODE_4BIT / _DECODE <- seq_encode_4bit_scalar :429-480, iupac_to_4bit :109-128 / seq_decode_4bit_scalar :482-528, :130-149
 *   DHTS_UDF_SEQ_GC_CONTENT            <- seq_gc_content_scalar :530-581
 *   DHTS_UDF_CIGAR_HAS_SOFT_CLIP .. _REFERENCE_LENGTH <- cigar_metric_scalar :695-742 over parse_cigar_metrics :197-269
 *   DHTS_UDF_CIGAR_HAS_OP              <- cigar_has_op_scalar :744-790 over cigar_has_operator_text :271-295
 *   DHTS_UDF_SAM_FLAG_BITS / _HAS / DHTS_UDF_IS_FORWARD_ALIGNED / DHTS_UDF_IS_PAIRED .. _IS_SUPPLEMENTARY <- :583-693
 *   dhts_udf_seq_kmers                 <- seq_kmers_bind / seq_kmers_function :820-974, over a whole column
 * The ids follow the registration order of :1223-1254 (seq_kmers, a table function, has its own entry). */
enum { DHTS_UDF_SEQ_REVCOMP = 0, DHTS_UDF_SEQ_CANONICAL, DHTS_UDF_SEQ_HASH_2BIT, DHTS_UDF_SEQ_ENCODE_4BIT, DHTS_UDF_SEQ_DECODE_4BIT, DHTS_UDF_SEQ_GC_CONTENT,
       DHTS_UDF_CIGAR_HAS_SOFT_CLIP, DHTS_UDF_CIGAR_HAS_HARD_CLIP, DHTS_UDF_CIGAR_LEFT_SOFT_CLIP, DHTS_UDF_CIGAR_RIGHT_SOFT_CLIP, DHTS_UDF_CIGAR_QUERY_LENGTH,
       DHTS_UDF_CIGAR_ALIGNED_QUERY_LENGTH, DHTS_UDF_CIGAR_REFERENCE_LENGTH, DHTS_UDF_CIGAR_HAS_OP,
       DHTS_UDF_SAM_FLAG_BITS, DHTS_UDF_SAM_FLAG_HAS, DHTS_UDF_IS_FORWARD_ALIGNED,
       DHTS_UDF_IS_PAIRED, DHTS_UDF_IS_PROPER_PAIR, DHTS_UDF_IS_UNMAPPED, DHTS_UDF_IS_NEXT_SEGMENT_UNMAPPED, DHTS_UDF_IS_REVERSE_COMPLEMENTED,
       DHTS_UDF_IS_NEXT_SEGMENT_REVERSE_COMPLEMENTED, DHTS_UDF_IS_FIRST_SEGMENT, DHTS_UDF_IS_LAST_SEGMENT, DHTS_UDF_IS_SECONDARY, DHTS_UDF_IS_QC_FAIL,
       DHTS_UDF_IS_DUPLICATE, DHTS_UDF_IS_SUPPLEMENTARY, DHTS_UDF_OP_COUNT };
enum { DHTS_T_UTINYINT = 6, DHTS_T_UBIGINT = 9 };      /* DUCKDB_TYPE_* values the results add to DHTS_T_* */
/* One argument column.  VARCHAR: the first four members are a dhts_strcol (a batch column is copied in as it is, reserved widths and all;
 * len = NULL: row i is bytes[off[i], off[i + 1])).  LIST(UTINYINT) (seq_decode_4bit): the same shape with one byte per child, child_valid
 * beside bytes.  Integers (FLAG, a mask): fixed[n] of |width| bytes, width < 0 = signed.  is_const: the column has ONE row that stands for
 * every row (the 'S' of cigar_has_op(CIGAR, 'S'), the mask of sam_flag_has). */
typedef struct {
    const uint32_t *off; const uint32_t *len; const uint8_t *bytes; uint64_t nbytes;
    const uint8_t *valid;        /* n bytes, 1 = valid; NULL = every row is valid */
    const uint8_t *child_valid;  /* nbytes bytes; NULL = every child is valid */
    const void *fixed; int32_t width;
    int32_t is_const;
} dhts_udf_arg;
/* A result column: DEVICE pointers owned by the context, valid until the next dhts_udf_* call on it -- which may still take them as an
 * argument (seq_decode_4bit of the list seq_encode_4bit just made).  A dhts_udf_* call leaves the context's current dhts_bam_batch alone.
 *   BOOLEAN                 col.fixed[n_rows] bytes; sam_flag_bits: n_fields = 12 arrays of n_rows bytes behind each other (:21-49's order)
 *   BIGINT, UBIGINT, DOUBLE col.fixed[n_rows] 8-byte values
 *   VARCHAR                 row i = col.bytes[col.off[i], col.off[i] + len[i]); off is the ARGUMENT's (same-length results keep its layout:
 *                           a NULL row keeps its reserved bytes, content unspecified), col.nbytes its arena size
 *   LIST(UTINYINT)          col.off[n_rows + 1] child offsets, the codes in col.bytes[col.child_n]; a NULL row has no children */
typedef struct {
    int32_t op, type;            /* DHTS_T_* of the value (of the child when is_list) */
    int32_t is_list, n_fields;
    int64_t n_rows;
    dhts_col col;
    const uint32_t *len;
} dhts_udf_result;
/* Host values -> device, into one of two argument slots of the context (slot 0 / 1; they live until the same slot is uploaded again):
 * whichever of off (n + 1 entries, or 2 with is_const), len, bytes (nbytes), valid, child_valid and fixed `host` sets is copied, *dev =
 * the same description with device pointers.  Host callers and the tests come in through here. */
int dhts_udf_upload(dhts_ctx *, int slot, const dhts_udf_arg *host, int64_t n_rows, dhts_udf_arg *dev);
/* result = op(a0[, a1]) for n_rows rows (0 is valid); a1 = NULL for the one-argument functions.  A VARCHAR arena is addressed with 32-bit
 * offsets: a result that would reach 4 GiB is an error that says so.  The SEQ column of a batch scanned under dhts_bam_set_seq_packed holds
 * 4-bit codes, not text: it is refused with an error that names packed SEQ.  DHTS_UDF_GROUP = 4 | 16 | 64 forces the lanes per row of the
 * text kernels (default: by the column's mean width). */
int dhts_udf_apply(dhts_ctx *, int op, const dhts_udf_arg *a0, const dhts_udf_arg *a1, int64_t n_rows, dhts_udf_result *out);
/* read-back with one wait: *out = *r with HOST pointers into dst (dhts_udf_result_host_bytes = the room dst needs) */
uint64_t dhts_udf_result_host_bytes(const dhts_udf_result *r);
int dhts_udf_fetch(dhts_ctx *, const dhts_udf_result *r, void *dst, uint64_t cap, dhts_udf_result *out);
/* seq_kmers over a column: k-mer number t (0-based, counted over the whole column in row order) lies in row `row` at the 1-based `pos`.
 * want_text: kmer = the raw bytes (no validation, no upper-casing :944) or, canonical, what seq_canonical makes of them (NULL when the
 * k-mer holds a byte outside ACGTN :948-963).  want_hash: hash = seq_hash_2bit(kmer), 8 bytes instead of k; needs k <= 32.  A sequence
 * shorter than k gives no rows.  At most max_rows (<= 0: 4,194,304; always so few that the text stays below 4 GiB) k-mers from number
 * `resume` on are returned; next = the `resume` of the following call, status = 1 with the last ones.  "seq_kmers: k must be > 0". */
typedef struct {
    int64_t n_rows; int32_t status; int32_t k;
    uint64_t next, total;        /* total: k-mers of the whole column */
    const int64_t *row, *pos;
    dhts_col kmer;               /* valid[n_rows], off[n_rows + 1], bytes; all NULL without want_text */
    const uint64_t *hash; const uint8_t *hash_valid;      /* NULL without want_hash */
} dhts_udf_kmers;
int dhts_udf_seq_kmers(dhts_ctx *, const dhts_udf_arg *seq, int64_t n_rows, int64_t k, int canonical, int want_text, int want_hash,
                       int64_t max_rows, uint64_t resume, dhts_udf_kmers *out);
uint64_t dhts_udf_kmers_host_bytes(const dhts_udf_kmers *b);
int dhts_udf_kmers_fetch(dhts_ctx *, const dhts_udf_kmers *b, void *dst, uint64_t cap, dhts_udf_kmers *out);

/* ---- utilities ------------------------------------------------------------------------------ */
int dhts_memcpy_d2h(dhts_ctx *, void *dst, const void *src_dev, uint64_t n);
int dhts_sync(dhts_ctx *);
/* accumulated device time of one kernel family, measured with HIP events on the context's stream */
double dhts_kernel_time_ms(const dhts_ctx *, int kernel_id, int64_t *launches);
void dhts_kernel_time_reset(dhts_ctx *);
void dhts_set_timing(dhts_ctx *, int enabled);

/* ---- interval algebra: interval_merge, interval_overlap ------------------------------------------
 * BED interval algebra on the device: the rows of a BED file are sorted by (chrom, start) with a radix sort on the device, indexed, and
 * merged into runs (interval_merge) or joined with the rows of a second file (interval_overlap).  The reference has only a plan for these
 * (.github/PLAN.md 10.5.2 / 10.7.1; INTEGRATION.md "Interval overlap join" names cgranges as the model of the join), so this is the
 * specification.
 *   Rows: those read_bed returns -- meta lines (empty, '#', "track", "browser") do not count; a line with fewer than 3 fields raises
 *     read_bed's error with its line number.  A row's number is its 0-based index among read_bed's rows.  A row is invalid if its start or
 *     end is NULL, if end < start, or if start or end lies outside [-2^62, 2^62) (so no sum or difference below can overflow).  Invalid rows
 *     keep their number, take no part in any result and are counted in n_skipped.  Empty rows (start == end) are valid and follow the
 *     predicates literally.
 *   Chrom names are compared byte for byte; chrom order is byte order of the name (memcmp, the shorter name first on a common prefix --
 *     DuckDB's default ORDER BY on VARCHAR).
 *   interval_merge(path, max_gap := 0): chrom, start, end, n_merged.  The valid rows sorted by (chrom order, start); within a chrom a row
 *     joins the current run iff start <= run_end + max_gap, where run_end is the largest end seen in the run -- rows that touch merge at
 *     max_gap = 0 (bedtools merge -d, and the rule of the count functions' BED merge).  One output row per run: its first start, its run_end,
 *     the number of rows in it.  Order: (chrom order, start).  max_gap 0 .. 2^40, else "interval_merge: max_gap must be between 0 and
 *     1099511627776".  No column is ever NULL.
 *   interval_overlap(path, right_path :=, mode := 'any' | 'contain' | 'within'): chrom, start, end, left_row, right_start, right_end,
 *     right_row, overlap.  One row per pair (l, r) of valid rows with the same chrom name that satisfies the mode's predicate; with
 *     l = [s, e) and r = [rs, re):  any: rs < e && s < re (cgranges' cr_overlap);  contain: s <= rs && re <= e && rs < e (cr_contain with l
 *     as the query);  within: rs <= s && e <= re && s < re (the same with the roles swapped).  overlap = max(0, min(e, re) - max(s, rs)).
 *     Order: by left_row; within a left row by (right_start, right_row).  A left chrom the right file lacks gives no rows.  No column is
 *     ever NULL.
 *   Paging: the concatenation of the pages is the result, whatever max_rows is (0 = 1,048,576).  A page of interval_overlap is the longest
 *     run of whole left rows, from where the last page ended, whose pairs fit max_rows; it holds at least one left row, so a single left row
 *     with more pairs than max_rows makes a larger page.
 *   Limits: fewer than 2^32 - 16 rows per file ("<fn>: more than 4294967279 rows"), fewer than 2^63 pairs.
 *   Not in this contract: interval_nearest; strand-aware merge; a region parameter; unmatched left rows (a left join) and counts-only output;
 *     BED columns beyond the first three in the results (rows are identified by left_row / right_row, as the BAM join identifies intervals
 *     by read_bed's row number); table-valued (subquery) arguments; dhts_bam_set_overlap_intervals and the count functions' BED merge stay
 *     on their host sort; two files on different devices.
 *   Method: the batches of the BED context go through the line table and bed_intervals, a compaction appends (name id, start, end, valid)
 *     per row to arrays in HBM and the host sees chrom names only at the heads of name runs; a stable LSD radix sort of (key, row) pairs,
 *     8 bits a pass, passes whose digit is equal in all keys skipped (csrc/interval_sort.hip); one gather for beg / end / id, the running
 *     maximum of (rank, end) through the carry for pmax, bmax per 64 rows; merge: head flags, their scan, a window of runs per page;
 *     overlap: a count pass with one lane per left row (binary search, walk back by pmax and bmax), a 64-bit carry, a write pass per page
 *     (csrc/interval_algebra.hip).
 * Every error is prefixed with the function's name ("interval_merge:", "interval_overlap:"; read_bed's own errors keep "read_bed:").  Every
 * call on a context in the wrong state fails with a dhts_error that names what is missing. */
enum { DHTS_IVL_MERGE_CHROM = 0, DHTS_IVL_MERGE_START, DHTS_IVL_MERGE_END, DHTS_IVL_MERGE_N, DHTS_IVL_MERGE_COL_COUNT };
enum { DHTS_IVL_OV_CHROM = 0, DHTS_IVL_OV_START, DHTS_IVL_OV_END, DHTS_IVL_OV_LEFT_ROW, DHTS_IVL_OV_RIGHT_START, DHTS_IVL_OV_RIGHT_END, DHTS_IVL_OV_RIGHT_ROW,
       DHTS_IVL_OV_OVERLAP, DHTS_IVL_OV_COL_COUNT };
enum { DHTS_IVL_ANY = 0, DHTS_IVL_CONTAIN = 1, DHTS_IVL_WITHIN = 2 };      /* mode */
#define DHTS_IVL_MAX_GAP (1ll << 40)
typedef struct {
    uint64_t n_rows;         /* read_bed's rows                                                                */
    uint64_t n_skipped;      /* invalid rows                                                                   */
    uint64_t n_chroms;       /* distinct chrom names (of all rows)                                             */
    uint64_t n_name_runs;    /* heads of name runs the host looked at: chrom changes, and one per batch       */
    uint64_t n_runs;         /* interval_merge: rows of the result, valid after dhts_ivl_merge_open           */
    uint64_t n_pairs;        /* interval_overlap: rows of the result, valid after dhts_ivl_overlap_open       */
    int32_t sort_passes;     /* radix passes that were run (of 12)                                             */
    int32_t status;          /* 1, or the negative status of a stream that ended on an error; -2: too many rows */
} dhts_ivl_stats;
typedef struct {
    int64_t n_rows;
    int32_t status;          /* 0 = more rows follow, 1 = the last page                                                                    */
    int32_t n_cols;          /* DHTS_IVL_MERGE_COL_COUNT or DHTS_IVL_OV_COL_COUNT, in that order                                           */
    const dhts_col *cols;    /* host array of descriptors, DEVICE pointers inside: fixed = int32 (chrom: the context's name id; for overlap the
                                left context's) or int64 (every other column) per row, a null pointer for a column colmask left out; no row is
                                NULL and valid stays a null pointer                                                                         */
} dhts_ivl_batch;
/* bed: a context prepared as for read_bed (dhts_open_path, dhts_bgzf_index, dhts_bed_open).  Reads it to its end, max_blocks BGZF blocks a
 * batch (0 = the default), and leaves the interval table -- the rows, the sort and the index -- on the context. */
int dhts_ivl_load(dhts_ctx *bed, int64_t max_blocks);
int dhts_ivl_stats_get(dhts_ctx *bed, dhts_ivl_stats *out);
/* the chrom name of a name id (ids are given in order of first appearance); NULL for an id out of range */
const char *dhts_ivl_chrom_name(dhts_ctx *bed, int32_t id, uint64_t *len);
int dhts_ivl_merge_open(dhts_ctx *bed, int64_t max_gap);
int dhts_ivl_merge_next(dhts_ctx *bed, int64_t max_rows, uint32_t colmask, dhts_ivl_batch *out);
/* left and right: two loaded contexts on one device (refused otherwise); right has to stay as it is while the result is paged out.  The
 * pairs are counted here. */
int dhts_ivl_overlap_open(dhts_ctx *left, dhts_ctx *right, int32_t mode);
int dhts_ivl_overlap_next(dhts_ctx *left, int64_t max_rows, uint32_t colmask, dhts_ivl_batch *out);
/* read-back as for dhts_bedgraph_batch */
uint64_t dhts_ivl_batch_host_bytes(const dhts_ivl_batch *b);
int dhts_ivl_batch_fetch(dhts_ctx *bed, const dhts_ivl_batch *b, void *dst, uint64_t cap, dhts_col *out_cols);

/* ---- interval nearest: interval_nearest ----------------------------------------------------------
 * interval_nearest(path, right_path :=, k := 1, max_distance := NULL, ties := 'all' | 'first'): for every row of the left file the k nearest
 * rows of the right file on its chrom.  It completes the plan's Layer 1 (.github/PLAN.md 10.5.2 / 10.7.1); the reference has no code for it and
 * cgranges no model, so the rules below are the specification.  They follow `bedtools closest -k -t all|first` in the coordinates and orders of
 * interval_overlap.
 *   Rows, validity, row numbers and chrom comparison are those of the block above: only valid rows take part, invalid ones keep their number
 *     and are counted in n_skipped (dhts_ivl_stats_get); a left chrom the right file lacks gives no rows.
 *   For a valid left row l = [s, e) and a valid right row r = [rs, re) of the same chrom:
 *     distance = max(0, rs - e, s - re), the gap in bases: 0 for rows that overlap or touch, as touching rows merge at max_gap = 0.
 *       `bedtools closest -d` prints this plus one for rows that do not overlap.  With positions in [-2^62, 2^62) every distance fits an
 *       int64; the largest is 2^63 - 1.
 *     overlap = max(0, min(e, re) - max(s, rs)), as in interval_overlap.
 *   Candidates of l: the right rows of its chrom with distance <= max_distance, all of them when max_distance is absent (-1 in this ABI),
 *     ranked by (distance, right_start, right_row).
 *     ties = 'first' emits the first min(k, candidates) of that ranking.
 *     ties = 'all' (the default): when there are more than k candidates, every candidate whose distance is at most that of the k-th.
 *     A left row with no candidate emits nothing and is counted in n_unmatched.  No column is ever NULL.
 *   Columns: chrom, start, end, left_row, right_start, right_end, right_row, overlap, distance -- interval_overlap's eight in its order, then
 *     distance.  Order: by left_row; within a left row by (right_start, right_row): interval_overlap's order, not distance order.
 *   Paging: whole left rows, as for interval_overlap (0 = 1,048,576 rows; at least one left row a page).
 *   Limits: k 1 .. 1,048,576 ("interval_nearest: k must be between 1 and 1048576"); max_distance >= 0 ("interval_nearest: max_distance must
 *     not be negative"); ties ("interval_nearest: ties must be 'all' or 'first'"); fewer than 2^32 - 16 rows per file.
 *   Not in this contract: strand or direction restriction (bedtools -D, -iu / -id); ignoring overlaps (-io); unmatched left rows (a left
 *     join); distance-ordered output (ORDER BY distance in SQL).
 *   Method: beside the index of the block above the right file gets a second order, its ends sorted by (chrom rank, end) with the same radix
 *     sort, built on the first dhts_ivl_nearest_open that names the context as right and dropped by dhts_ivl_load.  Selection, one lane per
 *     left row with binary searches alone: the rows within D number nb(e + D + 1) - ne(s - D) (starts in front, ends in front); the rows
 *     farther than 0 are two sequences sorted by distance, and the k-th distance is found by the partition search of two sorted sequences in
 *     O(log k).  The count, D and the tie quota are stored per left row; a 64-bit carry gives the offsets; a write pass per page walks the
 *     start order from the first row whose running maximum end admits a hit, 64-row blocks skipped (csrc/interval_nearest.hip).
 * One result is open per context: dhts_ivl_nearest_open closes a merge or overlap result, and their opens close this one.  Every error is
 * prefixed "interval_nearest:". */
enum { DHTS_IVL_NEAR_CHROM = 0, DHTS_IVL_NEAR_START, DHTS_IVL_NEAR_END, DHTS_IVL_NEAR_LEFT_ROW, DHTS_IVL_NEAR_RIGHT_START, DHTS_IVL_NEAR_RIGHT_END,
       DHTS_IVL_NEAR_RIGHT_ROW, DHTS_IVL_NEAR_OVERLAP, DHTS_IVL_NEAR_DISTANCE, DHTS_IVL_NEAR_COL_COUNT };
enum { DHTS_IVL_TIES_ALL = 0, DHTS_IVL_TIES_FIRST = 1 };
#define DHTS_IVL_MAX_K 1048576
typedef struct {
    uint64_t n_pairs;            /* rows of the result                                                          */
    uint64_t n_unmatched;        /* valid left rows without a candidate                                         */
    uint32_t end_sort_passes;    /* radix passes of the right context's end sort (of 12)                        */
    int32_t status;              /* as dhts_ivl_stats.status of the left context                                */
} dhts_ivl_nearest_stats;
/* left and right: two loaded contexts on one device; right has to stay as it is while the result is paged out.  max_distance -1: none.  Every
 * left row's count is taken here.  The batches are dhts_ivl_batch with DHTS_IVL_NEAR_COL_COUNT columns, fetched with dhts_ivl_batch_fetch. */
int dhts_ivl_nearest_open(dhts_ctx *left, dhts_ctx *right, int64_t k, int64_t max_distance, int32_t ties);
int dhts_ivl_nearest_next(dhts_ctx *left, int64_t max_rows, uint32_t colmask, dhts_ivl_batch *out);
int dhts_ivl_nearest_stats_get(dhts_ctx *left, dhts_ivl_nearest_stats *out);

#ifdef __cplusplus
}
#endif
#endif
