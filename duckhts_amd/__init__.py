"""duckhts_amd -- MI355X-native read_bam scan path (host-side Python mirror over the C ABI).

The product is `libduckhts_amd.so` (hand-written HIP for gfx950 behind include/duckhts_amd.h and
the DuckDB C-API extension entry point).  This module only loads it with ctypes and mirrors the
reference's operator surface for tests and benchmarks:

    read_bam(path_or_bytes)  ->  dict of the 13 core columns of src/bam_reader.c:514-526

There is NO CPU fallback: everything raises if the library or an MI355X device is missing.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DHTS_LIB") or os.path.join(_HERE, "libduckhts_amd.so")   # DHTS_LIB: kernel-variant experiments
_LIB = None

BAM_COLUMNS = ["QNAME", "FLAG", "RNAME", "POS", "MAPQ", "CIGAR", "RNEXT", "PNEXT", "TLEN", "SEQ", "QUAL",
               "READ_GROUP_ID", "SAMPLE_ID"]
K_NAMES = ["sigscan", "huff_decode", "lz_resolve", "tiles", "core_unpack", "scan", "string_write", "bcf_check", "bcf_measure", "bcf_write"]


class StrCol(C.Structure):
    _fields_ = [("off", C.c_void_p), ("len", C.c_void_p), ("bytes", C.c_void_p), ("nbytes", C.c_uint64)]


class BamBatch(C.Structure):
    _fields_ = [("n_rows", C.c_int64), ("status", C.c_int32), ("seq_packed", C.c_int32),
                ("flag", C.c_void_p), ("pos", C.c_void_p), ("mapq", C.c_void_p), ("pnext", C.c_void_p),
                ("tlen", C.c_void_p), ("tid", C.c_void_p), ("mtid", C.c_void_p), ("rg_idx", C.c_void_p),
                ("rg_valid", C.c_void_p),
                ("qname", StrCol), ("cigar", StrCol), ("seq", StrCol), ("qual", StrCol), ("rg", StrCol),
                ("first_rec_uoff", C.c_uint64), ("end_uoff", C.c_uint64), ("n_tag_cols", C.c_int32), ("qual_bits", C.c_int32), ("aux_map", C.c_void_p), ("tag_cols", C.c_void_p),
                ("ov_off", C.c_void_p), ("ov_ids", C.c_void_p), ("n_ov", C.c_uint64)]


class AuxMap(C.Structure):
    _fields_ = [("valid", C.c_void_p), ("off", C.c_void_p), ("n_ent", C.c_uint64), ("key", C.c_void_p), ("kind", C.c_void_p), ("sub", C.c_void_p),
                ("pay_off", C.c_void_p), ("payload", C.c_void_p), ("payload_bytes", C.c_uint64)]


class BamHeader(C.Structure):
    _fields_ = [("n_ref", C.c_int32), ("ref_name", C.POINTER(C.c_char_p)), ("ref_len", C.POINTER(C.c_uint32)),
                ("text", C.POINTER(C.c_char)), ("l_text", C.c_uint32), ("n_rg", C.c_int32),
                ("rg_id", C.POINTER(C.c_char_p)), ("rg_sm", C.POINTER(C.c_char_p)), ("first_rec_uoff", C.c_uint64)]


class BcfColInfo(C.Structure):
    _fields_ = [("name", C.c_char_p), ("type", C.c_int32), ("is_list", C.c_int32), ("encoding", C.c_int32), ("reserved", C.c_int32)]


class BcfInfo(C.Structure):
    _fields_ = [("n_cols", C.c_int32), ("cols", C.POINTER(BcfColInfo)), ("n_contigs", C.c_int32), ("contig_name", C.POINTER(C.c_char_p)),
                ("n_dict", C.c_int32), ("dict_name", C.POINTER(C.c_char_p)), ("n_samples", C.c_int32), ("sample_name", C.POINTER(C.c_char_p)),
                ("tidy", C.c_int32), ("first_rec_uoff", C.c_uint64)]


class BcfCol(C.Structure):
    _fields_ = [("col", C.c_int32), ("reserved", C.c_int32), ("valid", C.c_void_p), ("fixed", C.c_void_p), ("off", C.c_void_p),
                ("bytes", C.c_void_p), ("nbytes", C.c_uint64), ("child_fixed", C.c_void_p), ("child_off", C.c_void_p), ("child_n", C.c_uint64), ("child_valid", C.c_void_p)]


class BcfBatch(C.Structure):
    _fields_ = [("n_rows", C.c_int64), ("status", C.c_int32), ("n_cols", C.c_int32), ("cols", C.POINTER(BcfCol)),
                ("first_rec_uoff", C.c_uint64), ("end_uoff", C.c_uint64)]


class FastaBatch(C.Structure):
    _fields_ = [("n_rows", C.c_int64), ("name_off", C.c_void_p), ("name_bytes", C.c_void_p), ("name_nbytes", C.c_uint64),
                ("seq_off", C.c_void_p), ("seq_bytes", C.c_void_p), ("seq_nbytes", C.c_uint64)]


class BedBatch(C.Structure):
    _fields_ = [("n_rows", C.c_int64), ("status", C.c_int32), ("n_cols", C.c_int32), ("cols", C.POINTER(BcfCol))]


class BinsParams(C.Structure):
    _fields_ = [("bin_width", C.c_int64), ("min_mapq", C.c_int32), ("require_flags", C.c_int32), ("exclude_flags", C.c_int32), ("include_flags", C.c_int32),
                ("dedup", C.c_int32), ("emit_zero_bins", C.c_int32)]


class BinsStats(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_flag_filtered", C.c_uint64), ("n_unplaced", C.c_uint64), ("n_out_of_range", C.c_uint64), ("n_duplicate", C.c_uint64),
                ("n_low_mapq", C.c_uint64), ("n_counted", C.c_uint64), ("total_bins", C.c_uint64), ("status", C.c_int32), ("reserved", C.c_int32)]


class BedcovParams(C.Structure):
    _fields_ = [("min_mapq", C.c_int32), ("require_flags", C.c_int32), ("exclude_flags", C.c_int32), ("include_flags", C.c_int32),
                ("count_deletions", C.c_int32), ("count_ref_skips", C.c_int32)]


class BedcovStats(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_flag_filtered", C.c_uint64), ("n_unplaced", C.c_uint64), ("n_low_mapq", C.c_uint64), ("n_counted", C.c_uint64),
                ("n_bed_rows", C.c_uint64), ("n_breakpoints", C.c_uint64), ("status", C.c_int32), ("reserved", C.c_int32)]


class CoverageParams(C.Structure):
    _fields_ = [("min_read_len", C.c_int64), ("min_depth", C.c_int64), ("min_mapq", C.c_int32), ("min_baseq", C.c_int32),
                ("require_flags", C.c_int32), ("exclude_flags", C.c_int32), ("include_flags", C.c_int32), ("reserved", C.c_int32)]


class CoverageStats(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_flag_filtered", C.c_uint64), ("n_unplaced", C.c_uint64), ("n_short", C.c_uint64), ("n_low_mapq", C.c_uint64),
                ("n_outside", C.c_uint64), ("n_counted", C.c_uint64), ("n_target_rows", C.c_uint64), ("table_bytes", C.c_uint64), ("status", C.c_int32), ("reserved", C.c_int32)]


class DepthParams(C.Structure):
    _fields_ = [("min_read_len", C.c_int64), ("min_mapq", C.c_int32), ("min_baseq", C.c_int32), ("require_flags", C.c_int32), ("exclude_flags", C.c_int32),
                ("include_flags", C.c_int32), ("include_deletions", C.c_int32), ("all_positions", C.c_int32), ("reserved", C.c_int32)]


class DepthStats(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_flag_filtered", C.c_uint64), ("n_unplaced", C.c_uint64), ("n_short", C.c_uint64), ("n_low_mapq", C.c_uint64),
                ("n_outside", C.c_uint64), ("n_counted", C.c_uint64), ("n_target_rows", C.c_uint64), ("n_bed_skipped", C.c_uint64), ("table_bytes", C.c_uint64),
                ("n_positions", C.c_uint64), ("status", C.c_int32), ("reserved", C.c_int32)]


class PileupParams(C.Structure):
    _fields_ = [("min_read_len", C.c_int64), ("min_mapq", C.c_int32), ("min_baseq", C.c_int32), ("require_flags", C.c_int32), ("exclude_flags", C.c_int32),
                ("include_flags", C.c_int32), ("include_deletions", C.c_int32), ("include_insertions", C.c_int32), ("distinguish_strands", C.c_int32),
                ("min_nucleotide_depth", C.c_int32), ("reserved", C.c_int32)]


class PileupStats(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_flag_filtered", C.c_uint64), ("n_unplaced", C.c_uint64), ("n_short", C.c_uint64), ("n_low_mapq", C.c_uint64),
                ("n_outside", C.c_uint64), ("n_counted", C.c_uint64), ("n_target_rows", C.c_uint64), ("table_bytes", C.c_uint64), ("n_result_rows", C.c_uint64),
                ("status", C.c_int32), ("reserved", C.c_int32)]


class BedgraphParams(C.Structure):
    _fields_ = [("min_read_len", C.c_int64), ("min_mapq", C.c_int32), ("min_baseq", C.c_int32), ("require_flags", C.c_int32), ("exclude_flags", C.c_int32),
                ("include_flags", C.c_int32), ("include_deletions", C.c_int32), ("zero_runs", C.c_int32), ("n_breaks", C.c_int32), ("breaks", C.c_int32 * 16),
                ("reserved", C.c_int32 * 2)]


class BedgraphStats(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_flag_filtered", C.c_uint64), ("n_unplaced", C.c_uint64), ("n_short", C.c_uint64), ("n_low_mapq", C.c_uint64),
                ("n_outside", C.c_uint64), ("n_counted", C.c_uint64), ("n_target_rows", C.c_uint64), ("n_bed_skipped", C.c_uint64), ("table_bytes", C.c_uint64),
                ("n_runs", C.c_uint64), ("status", C.c_int32), ("reserved", C.c_int32)]


class BedgraphExportParams(C.Structure):
    _fields_ = [("level", C.c_int32), ("index", C.c_int32), ("min_shift", C.c_int32), ("overwrite", C.c_int32), ("reserved", C.c_int32 * 4)]


class BedgraphExportStats(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("bytes_text", C.c_uint64), ("bytes_out", C.c_uint64), ("bytes_index", C.c_uint64), ("status", C.c_int32), ("reserved", C.c_int32)]


class DepthHistParams(C.Structure):
    _fields_ = [("min_read_len", C.c_int64), ("min_mapq", C.c_int32), ("min_baseq", C.c_int32), ("require_flags", C.c_int32), ("exclude_flags", C.c_int32),
                ("include_flags", C.c_int32), ("include_deletions", C.c_int32), ("depth_cap", C.c_int32), ("per", C.c_int32), ("reserved", C.c_int32 * 2)]


class DepthHistStats(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_flag_filtered", C.c_uint64), ("n_unplaced", C.c_uint64), ("n_short", C.c_uint64), ("n_low_mapq", C.c_uint64),
                ("n_outside", C.c_uint64), ("n_counted", C.c_uint64), ("n_target_rows", C.c_uint64), ("n_groups", C.c_uint64), ("n_bed_skipped", C.c_uint64),
                ("table_bytes", C.c_uint64), ("hist_bytes", C.c_uint64), ("n_result_rows", C.c_uint64), ("status", C.c_int32), ("reserved", C.c_int32)]


class IvlStats(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_skipped", C.c_uint64), ("n_chroms", C.c_uint64), ("n_name_runs", C.c_uint64), ("n_runs", C.c_uint64), ("n_pairs", C.c_uint64),
                ("sort_passes", C.c_int32), ("status", C.c_int32)]


class IvlNearestStats(C.Structure):
    _fields_ = [("n_pairs", C.c_uint64), ("n_unmatched", C.c_uint64), ("end_sort_passes", C.c_uint32), ("status", C.c_int32)]


class TabixMap(C.Structure):
    _fields_ = [("pair_off", C.c_void_p), ("valid", C.c_void_p), ("n_pairs", C.c_uint64), ("key_off", C.c_void_p), ("key_bytes", C.c_void_p), ("key_nbytes", C.c_uint64),
                ("val_off", C.c_void_p), ("val_bytes", C.c_void_p), ("val_nbytes", C.c_uint64)]


class TabixBatch(C.Structure):
    _fields_ = [("n_rows", C.c_int64), ("status", C.c_int32), ("n_cols", C.c_int32), ("cols", C.POINTER(BcfCol)), ("col_types", C.POINTER(C.c_int32)),
                ("has_map", C.c_int32), ("reserved", C.c_int32), ("map", TabixMap), ("n_double_fast", C.c_uint64), ("n_double_patched", C.c_uint64)]


class TabixSniffed(C.Structure):
    _fields_ = [("n_fields", C.c_int32), ("have_candidate", C.c_int32), ("candidate_from_skip", C.c_int32), ("reserved", C.c_int32),
                ("candidate", C.c_void_p), ("candidate_len", C.c_uint64)]


TABIX_MAX_COLS = 256


class TabixSchema(C.Structure):
    _fields_ = [("n_cols", C.c_int32), ("skip_header_line", C.c_int32), ("types", C.c_int32 * TABIX_MAX_COLS), ("names", C.c_char_p * TABIX_MAX_COLS)]


class UdfArg(C.Structure):
    _fields_ = [("off", C.c_void_p), ("len", C.c_void_p), ("bytes", C.c_void_p), ("nbytes", C.c_uint64), ("valid", C.c_void_p), ("child_valid", C.c_void_p),
                ("fixed", C.c_void_p), ("width", C.c_int32), ("is_const", C.c_int32)]


class UdfResult(C.Structure):
    _fields_ = [("op", C.c_int32), ("type", C.c_int32), ("is_list", C.c_int32), ("n_fields", C.c_int32), ("n_rows", C.c_int64), ("col", BcfCol), ("len", C.c_void_p)]


class UdfKmers(C.Structure):
    _fields_ = [("n_rows", C.c_int64), ("status", C.c_int32), ("k", C.c_int32), ("next", C.c_uint64), ("total", C.c_uint64), ("row", C.c_void_p), ("pos", C.c_void_p),
                ("kmer", BcfCol), ("hash", C.c_void_p), ("hash_valid", C.c_void_p)]


# the scalar functions of the reference's k-mer family in registration order (src/kmer_udf.c:1223-1254 without the table function): index = DHTS_UDF_* id
UDF_OPS = ["seq_revcomp", "seq_canonical", "seq_hash_2bit", "seq_encode_4bit", "seq_decode_4bit", "seq_gc_content",
           "cigar_has_soft_clip", "cigar_has_hard_clip", "cigar_left_soft_clip", "cigar_right_soft_clip", "cigar_query_length", "cigar_aligned_query_length",
           "cigar_reference_length", "cigar_has_op", "sam_flag_bits", "sam_flag_has", "is_forward_aligned",
           "is_paired", "is_proper_pair", "is_unmapped", "is_next_segment_unmapped", "is_reverse_complemented", "is_next_segment_reverse_complemented",
           "is_first_segment", "is_last_segment", "is_secondary", "is_qc_fail", "is_duplicate", "is_supplementary"]
_UDF_TEXT_OPS = 14           # the ids below take a VARCHAR (or list) first argument, the others an integer column
TABIX_GENERIC, TABIX_GTF, TABIX_GFF = 0, 1, 2
T_INTEGER, T_BIGINT, T_DOUBLE, T_VARCHAR = 4, 5, 11, 17
GXF_COLUMNS = ["seqname", "source", "feature", "start", "end", "score", "strand", "frame", "attributes", "attributes_map"]
GXF_TYPES = [T_VARCHAR, T_VARCHAR, T_VARCHAR, T_BIGINT, T_BIGINT, T_DOUBLE, T_VARCHAR, T_VARCHAR, T_VARCHAR]
BED_COLUMNS = ["chrom", "start", "end", "name", "score", "strand", "thick_start", "thick_end", "item_rgb", "block_count", "block_sizes", "block_starts", "extra"]
BED_INT_COLUMNS = (1, 2, 6, 7, 9)
NUC_COLUMNS = ["chrom", "start", "end", "pct_at", "pct_gc", "num_a", "num_c", "num_g", "num_t", "num_n", "num_other", "seq_len", "seq"]
NUC_DOUBLE_COLUMNS = (3, 4)
NUC_STR_COLUMNS = (0, 12)
BINS_COLUMNS = ["chrom", "start", "end", "bin_id", "count_total", "count_fwd", "count_rev"]
BINS_DEDUP = {"none": 0, "adjacent": 1}
BEDCOV_COLUMNS = ["chrom", "start", "end", "name", "score", "strand", "bases_covered", "read_count"]
BEDCOV_INT_COLUMNS = (1, 2, 6, 7)
COVERAGE_COLUMNS = ["chrom", "start", "end", "numreads", "covbases", "coverage", "meandepth", "meanbaseq", "meanmapq", "sum_depth", "sum_baseq", "sum_mapq"]
COVERAGE_DOUBLE_COLUMNS = (5, 6, 7, 8)
COVERAGE_COLMASK = (1 << 1) | (1 << 2) | (1 << 3) | (1 << 4)              # FLAG, RNAME, POS, MAPQ: no string column (CIGAR and QUAL are read in their binary form)
DEPTH_COLUMNS = ["tid", "pos", "depth"]
DEPTH_DTYPES = (np.int32, np.int64, np.int32)
DEPTH_COLMASK = (1 << 1) | (1 << 2) | (1 << 3) | (1 << 4)                 # FLAG, RNAME, POS, MAPQ: the columns of the scan bam_depth accumulates (no string column)
PILEUP_COLUMNS = ["tid", "pos", "strand", "nucleotide", "count"]
PILEUP_DTYPES = (np.int32, np.int64, np.uint8, np.uint8, np.int32)           # strand and nucleotide: one ASCII byte per row
PILEUP_SYMBOLS = b"ACGTN=-+"                                                # the order of the symbols inside a position and strand
PILEUP_COLMASK = DEPTH_COLMASK                                              # the columns of the scan bam_pileup accumulates (SEQ and QUAL are read in their binary form)
BEDGRAPH_COLUMNS = ["tid", "start", "end", "depth"]
BEDGRAPH_DTYPES = (np.int32, np.int64, np.int64, np.int32)                   # start 0-based, end exclusive
BEDGRAPH_COLMASK = DEPTH_COLMASK                                            # the columns of the scan bam_bedgraph accumulates (no string column)
BEDGRAPH_MAX_BREAKS = 16
BEDGRAPH_EXPORT_INDEX = {"none": 0, "tbi": 1, "csi": 2}                     # the C struct's index
ROWS_TEXT_LDS_BYTES = 16384                                                 # csrc/rows_text.hip: RTX_LDS_BYTES, the longest span of 256 rows the write pass stages in LDS
INTERVAL_MERGE_COLUMNS = ["chrom", "start", "end", "n_merged"]
INTERVAL_OVERLAP_COLUMNS = ["chrom", "start", "end", "left_row", "right_start", "right_end", "right_row", "overlap"]
INTERVAL_NEAREST_COLUMNS = INTERVAL_OVERLAP_COLUMNS + ["distance"]
INTERVAL_TIES = {"all": 0, "first": 1}                                      # the C ABI's ties
INTERVAL_MAX_K = 1 << 20
INTERVAL_DTYPES = (np.int32,) + (np.int64,) * 8                              # chrom: the context's name id; every other column an int64
INTERVAL_MODES = {"any": 0, "contain": 1, "within": 2}                      # the C ABI's mode
INTERVAL_MAX_GAP = 1 << 40
IVL_SORT_TILE = 4096                                                        # csrc/interval_sort.hip: IVL_SORT_TILE, the pairs one workgroup of the sort ranks
IVL_SORT_MAX_PASSES = 12                                                    # ... IVL_SORT_MAX_PASSES: 8 bytes of the start, 4 of the chrom's rank
DEPTH_HIST_COLUMNS = ["tid", "start", "end", "depth", "n_positions", "n_at_least", "length"]
DEPTH_HIST_DTYPES = (np.int32, np.int64, np.int64, np.int32, np.int64, np.int64, np.int64)   # start 0-based, end exclusive
DEPTH_HIST_COLMASK = DEPTH_COLMASK                                          # the columns of the scan bam_depth_hist accumulates (no string column)
DEPTH_HIST_PER = {"row": 0, "contig": 1}                                    # the C struct's per
DEPTH_HIST_LDS_BINS = 4096                                                  # csrc/bam_depth_hist.hip: DHI_LDS_BINS, the bins the histogram pass counts in LDS
DEPTH_HIST_GRID_TARGET = 2048                                               # ... DHI_GRID_TARGET, the workgroups the spans of tiles are cut for
DEPTH_HIST_SPAN_MIN_TILES = 8                                               # ... DHI_SPAN_MIN_TILES, the shortest span


def depth_hist_span_tiles(ntiles):
    """the tiles (of 1,024 slots of the depth table) one workgroup of the histogram pass owns in a table of ntiles tiles"""
    return max(DEPTH_HIST_SPAN_MIN_TILES, -(-int(ntiles) // DEPTH_HIST_GRID_TARGET))


BEDCOV_COLMASK = (1 << 1) | (1 << 2) | (1 << 3) | (1 << 4)                # FLAG, RNAME, POS, MAPQ: no string column (the CIGARs are read in their binary form)
BINS_COLMASK = (1 << 1) | (1 << 2) | (1 << 3) | (1 << 4) | (1 << 7)        # FLAG, RNAME, POS, MAPQ, PNEXT: no string column

# DUCKDB_TYPE_* element codes -> the canonical type tags of the test oracle's column blob
_CANON_TYPE = {17: 1, 5: 2, 11: 3, 1: 4, 4: 5, 10: 6}
ENC_PLAIN, ENC_CONTIG, ENC_DICT, ENC_SAMPLE, ENC_FLOAT_TEXT = 0, 1, 2, 3, 4

EXPORTS = ["dhts_abi_version", "dhts_device_count", "dhts_create", "dhts_destroy", "dhts_error", "dhts_open_path",
           "dhts_open_host", "dhts_open_tiled", "dhts_resident_bytes", "dhts_bgzf_index", "dhts_bgzf_table",
           "dhts_bgzf_inflate_to_host", "dhts_bam_open", "dhts_bam_header_get", "dhts_bam_set_shard", "dhts_bam_set_block_range", "dhts_shard_cut",
           "dhts_bam_set_regions", "dhts_bam_load_index", "dhts_scan_window_stats", "dhts_bgzf_repair_stats", "dhts_bam_std_tag_count", "dhts_bam_std_tag_info", "dhts_bam_set_tag_columns", "dhts_bam_set_aux_map", "dhts_bam_set_overlap_intervals", "dhts_bam_set_overlap_bed", "dhts_bam_set_overlap_bed_path", "dhts_bam_build_index", "dhts_bam_index_bytes", "dhts_bam_rewind", "dhts_bam_next_batch", "dhts_memcpy_d2h", "dhts_sync", "dhts_kernel_time_ms",
           "dhts_kernel_time_reset", "dhts_set_timing", "dhts_bcf_open", "dhts_bcf_info_get", "dhts_bcf_set_projection", "dhts_bcf_set_block_range", "dhts_bcf_set_region", "dhts_bcf_load_index",
           "dhts_bcf_rewind", "dhts_bcf_next_batch",
           "dhts_open_path_range", "dhts_open_path_shard", "dhts_bam_set_file_shard", "dhts_bam_header_bytes", "dhts_voffset",
           "dhts_host_alloc", "dhts_host_free", "dhts_release_pools", "dhts_device_mem_info", "dhts_shard_window", "dhts_bcf_build_index", "dhts_bgzf_wrap", "dhts_bgzf_compress", "dhts_bgzip_file", "dhts_bgunzip_file", "dhts_bcf_is_text", "dhts_bam_is_text", "dhts_bam_set_seq_packed", "dhts_bcf_header_bytes", "dhts_bcf_region_segments", "dhts_set_super_blocks", "dhts_bam_build_index_csi", "dhts_tabix_build_index", "dhts_bcf_batch_host_bytes", "dhts_bcf_batch_fetch", "dhts_resident_from_cache", "dhts_bam_region_segments", "dhts_open_path_segments", "dhts_open_path_async", "dhts_stage_wait", "dhts_bgzf_index_staged", "dhts_blocks_ahead", "dhts_bam_batch_host_bytes", "dhts_bam_batch_fetch", "dhts_bam_batch_fetch_begin", "dhts_bam_batch_fetch_wait", "dhts_bcf_batch_fetch_begin", "dhts_bcf_batch_fetch_wait", "dhts_device_numa_node", "dhts_bind_thread_to_node", "dhts_bind_thread_near_device", "dhts_bam_set_qual_packed",
           "dhts_fasta_build_index", "dhts_fasta_index_bytes", "dhts_fasta_gzi_bytes", "dhts_fasta_load_index", "dhts_fasta_open_regions", "dhts_fasta_fetch", "dhts_fasta_batch_host_bytes", "dhts_fasta_batch_fetch",
           "dhts_bed_open", "dhts_bed_set_projection", "dhts_bed_set_region", "dhts_bed_load_index", "dhts_bed_region_segments", "dhts_bed_next_batch", "dhts_bed_batch_host_bytes", "dhts_bed_batch_fetch",
           "dhts_nuc_open_region", "dhts_nuc_open", "dhts_nuc_set_region", "dhts_nuc_set_projection", "dhts_nuc_next_bins", "dhts_nuc_next_bed", "dhts_nuc_intervals", "dhts_nuc_batch_host_bytes", "dhts_nuc_batch_fetch",
           "dhts_bam_bins_open", "dhts_bam_bins_accumulate", "dhts_bam_bins_scan", "dhts_bam_bins_stats", "dhts_bam_bins_next", "dhts_bam_bins_batch_host_bytes", "dhts_bam_bins_batch_fetch",
           "dhts_bam_bedcov_open", "dhts_bam_bedcov_accumulate", "dhts_bam_bedcov_scan", "dhts_bam_bedcov_stats", "dhts_bam_bedcov_next", "dhts_bam_bedcov_batch_host_bytes", "dhts_bam_bedcov_batch_fetch",
           "dhts_bam_coverage_open", "dhts_bam_coverage_accumulate", "dhts_bam_coverage_scan", "dhts_bam_coverage_stats", "dhts_bam_coverage_next", "dhts_bam_coverage_batch_host_bytes", "dhts_bam_coverage_batch_fetch",
           "dhts_bam_depth_open", "dhts_bam_depth_accumulate", "dhts_bam_depth_scan", "dhts_bam_depth_stats", "dhts_bam_depth_next", "dhts_bam_depth_batch_host_bytes", "dhts_bam_depth_batch_fetch",
           "dhts_bam_pileup_open", "dhts_bam_pileup_accumulate", "dhts_bam_pileup_scan", "dhts_bam_pileup_stats", "dhts_bam_pileup_next", "dhts_bam_pileup_batch_host_bytes", "dhts_bam_pileup_batch_fetch",
           "dhts_bam_bedgraph_open", "dhts_bam_bedgraph_accumulate", "dhts_bam_bedgraph_scan", "dhts_bam_bedgraph_stats", "dhts_bam_bedgraph_next", "dhts_bam_bedgraph_batch_host_bytes", "dhts_bam_bedgraph_batch_fetch",
           "dhts_bedgraph_export",
           "dhts_bam_hist_open", "dhts_bam_hist_accumulate", "dhts_bam_hist_scan", "dhts_bam_hist_stats", "dhts_bam_hist_next", "dhts_bam_hist_batch_host_bytes", "dhts_bam_hist_batch_fetch",
           "dhts_ivl_load", "dhts_ivl_stats_get", "dhts_ivl_chrom_name", "dhts_ivl_merge_open", "dhts_ivl_merge_next", "dhts_ivl_overlap_open", "dhts_ivl_overlap_next",
           "dhts_ivl_batch_host_bytes", "dhts_ivl_batch_fetch", "dhts_ivl_nearest_open", "dhts_ivl_nearest_next", "dhts_ivl_nearest_stats_get",
           "dhts_tabix_open", "dhts_tabix_set_conf", "dhts_tabix_index_conf", "dhts_tabix_sniff", "dhts_tabix_resolve_schema", "dhts_tabix_set_schema", "dhts_tabix_set_projection",
           "dhts_tabix_set_region", "dhts_tabix_load_index", "dhts_tabix_region_segments", "dhts_tabix_next_batch", "dhts_tabix_batch_host_bytes", "dhts_tabix_batch_fetch",
           "dhts_udf_upload", "dhts_udf_apply", "dhts_udf_result_host_bytes", "dhts_udf_fetch", "dhts_udf_seq_kmers", "dhts_udf_kmers_host_bytes", "dhts_udf_kmers_fetch"]


def lib():
    """Loads the HIP library; raises if it has not been built (run __graft_entry__.build())."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() (hipcc, gfx950)")
        L = C.CDLL(LIB_PATH)
        L.dhts_create.restype = C.c_void_p
        L.dhts_create.argtypes = [C.c_int]
        L.dhts_destroy.argtypes = [C.c_void_p]
        L.dhts_error.restype = C.c_char_p
        L.dhts_error.argtypes = [C.c_void_p]
        L.dhts_open_path.argtypes = [C.c_void_p, C.c_char_p]
        L.dhts_open_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.dhts_open_tiled.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p,
                                      C.c_uint64]
        L.dhts_resident_bytes.restype = C.c_uint64
        L.dhts_resident_bytes.argtypes = [C.c_void_p]
        L.dhts_bgzf_index.restype = C.c_int64
        L.dhts_bgzf_index.argtypes = [C.c_void_p]
        L.dhts_bgzf_table.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        L.dhts_bgzf_inflate_to_host.restype = C.c_int64
        L.dhts_bgzf_inflate_to_host.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p]
        L.dhts_bam_open.argtypes = [C.c_void_p]
        L.dhts_bam_header_get.argtypes = [C.c_void_p, C.POINTER(BamHeader)]
        L.dhts_bam_is_text.argtypes = [C.c_void_p]
        L.dhts_debug_sam_records.restype = C.c_int64
        L.dhts_debug_sam_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_int64)]
        L.dhts_debug_fastq_records.restype = C.c_int64
        L.dhts_debug_fastq_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_int64)]
        L.dhts_debug_tile_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        if hasattr(L, "dhts_debug_tile_scan"):            # (absent from a DHTS_LIB variant built from older sources)
            L.dhts_debug_tile_scan.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int64]
            L.dhts_debug_tile_scan.restype = C.c_int64
        L.dhts_bam_set_shard.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.dhts_bam_set_block_range.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int]
        L.dhts_shard_cut.argtypes = [C.c_void_p, C.c_int64, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.dhts_bam_rewind.argtypes = [C.c_void_p]
        L.dhts_bam_set_regions.argtypes = [C.c_void_p, C.c_char_p]
        L.dhts_bam_std_tag_info.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_char_p]
        L.dhts_bam_set_tag_columns.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.dhts_bam_set_aux_map.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.dhts_bam_build_index.restype = C.c_int64
        L.dhts_bam_build_index.argtypes = [C.c_void_p]
        L.dhts_bam_index_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.dhts_bam_set_overlap_intervals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        L.dhts_bam_load_index.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.dhts_bam_next_batch.argtypes = [C.c_void_p, C.c_int64, C.c_uint32, C.POINTER(BamBatch)]
        L.dhts_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.dhts_sync.argtypes = [C.c_void_p]
        L.dhts_kernel_time_ms.restype = C.c_double
        L.dhts_kernel_time_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
        L.dhts_kernel_time_reset.argtypes = [C.c_void_p]
        L.dhts_set_timing.argtypes = [C.c_void_p, C.c_int]
        L.dhts_bcf_open.argtypes = [C.c_void_p, C.c_int]
        L.dhts_bcf_info_get.argtypes = [C.c_void_p, C.POINTER(BcfInfo)]
        L.dhts_bcf_set_projection.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.dhts_bcf_set_block_range.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int]
        L.dhts_bcf_rewind.argtypes = [C.c_void_p]
        L.dhts_bcf_set_region.argtypes = [C.c_void_p, C.c_char_p]
        L.dhts_bcf_load_index.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.dhts_bcf_next_batch.argtypes = [C.c_void_p, C.c_int64, C.POINTER(BcfBatch)]
        L.dhts_fasta_build_index.restype = C.c_int64
        L.dhts_fasta_build_index.argtypes = [C.c_void_p]
        L.dhts_fasta_index_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.dhts_fasta_gzi_bytes.restype = C.c_int64
        L.dhts_fasta_gzi_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.dhts_fasta_load_index.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64]
        L.dhts_fasta_open_regions.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
        L.dhts_fasta_fetch.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(FastaBatch)]
        L.dhts_fasta_batch_host_bytes.restype = C.c_uint64
        L.dhts_fasta_batch_host_bytes.argtypes = [C.POINTER(FastaBatch)]
        L.dhts_fasta_batch_fetch.argtypes = [C.c_void_p, C.POINTER(FastaBatch), C.c_void_p, C.c_uint64, C.POINTER(FastaBatch)]
        L.dhts_bed_open.argtypes = [C.c_void_p]
        L.dhts_bed_set_projection.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.dhts_bed_set_region.argtypes = [C.c_void_p, C.c_char_p]
        L.dhts_bed_load_index.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.dhts_bed_region_segments.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        L.dhts_bed_next_batch.argtypes = [C.c_void_p, C.c_int64, C.POINTER(BedBatch)]
        L.dhts_bed_batch_host_bytes.restype = C.c_uint64
        L.dhts_bed_batch_host_bytes.argtypes = [C.POINTER(BedBatch)]
        L.dhts_bed_batch_fetch.argtypes = [C.c_void_p, C.POINTER(BedBatch), C.c_void_p, C.c_uint64, C.POINTER(BcfCol)]
        L.dhts_nuc_open_region.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int]
        L.dhts_nuc_open.argtypes = [C.c_void_p, C.c_int]
        L.dhts_nuc_set_region.argtypes = [C.c_void_p, C.c_char_p]
        L.dhts_nuc_set_projection.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.dhts_nuc_next_bins.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(BedBatch)]
        L.dhts_nuc_next_bed.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(BedBatch)]
        L.dhts_nuc_intervals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(BedBatch)]
        L.dhts_nuc_batch_host_bytes.restype = C.c_uint64
        L.dhts_nuc_batch_host_bytes.argtypes = [C.POINTER(BedBatch)]
        L.dhts_nuc_batch_fetch.argtypes = [C.c_void_p, C.POINTER(BedBatch), C.c_void_p, C.c_uint64, C.POINTER(BcfCol)]
        # the seven bam_* count functions: the stats structure and the arguments of open and next around the common ones
        for name, stats, open_args, next_args in (("bins", BinsStats, [C.POINTER(BinsParams)], [C.c_int64]),
                                                  ("bedcov", BedcovStats, [C.c_void_p, C.POINTER(BedcovParams)], [C.c_void_p, C.c_int64]),
                                                  ("coverage", CoverageStats, [C.POINTER(CoverageParams)], [C.c_int64]),
                                                  ("depth", DepthStats, [C.POINTER(DepthParams), C.c_void_p], [C.c_int64, C.c_uint32]),
                                                  ("pileup", PileupStats, [C.POINTER(PileupParams)], [C.c_int64, C.c_uint32]),
                                                  ("bedgraph", BedgraphStats, [C.POINTER(BedgraphParams), C.c_void_p], [C.c_int64, C.c_uint32]),
                                                  ("hist", DepthHistStats, [C.POINTER(DepthHistParams), C.c_void_p], [C.c_int64, C.c_uint32])):
            f = {what: getattr(L, "dhts_bam_%s_%s" % (name, what)) for what in ("open", "accumulate", "scan", "stats", "next", "batch_host_bytes", "batch_fetch")}
            f["open"].argtypes = [C.c_void_p] + open_args
            f["accumulate"].argtypes = [C.c_void_p, C.POINTER(BamBatch)]
            f["scan"].argtypes = [C.c_void_p, C.c_int64]
            f["stats"].argtypes = [C.c_void_p, C.POINTER(stats)]
            f["next"].argtypes = [C.c_void_p] + next_args + [C.POINTER(BedBatch)]
            f["batch_host_bytes"].restype = C.c_uint64
            f["batch_host_bytes"].argtypes = [C.POINTER(BedBatch)]
            f["batch_fetch"].argtypes = [C.c_void_p, C.POINTER(BedBatch), C.c_void_p, C.c_uint64, C.POINTER(BcfCol)]
        L.dhts_bedgraph_export.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(BedgraphExportParams), C.POINTER(BedgraphExportStats)]
        L.dhts_ivl_load.argtypes = [C.c_void_p, C.c_int64]
        L.dhts_ivl_stats_get.argtypes = [C.c_void_p, C.POINTER(IvlStats)]
        L.dhts_ivl_chrom_name.restype = C.c_void_p
        L.dhts_ivl_chrom_name.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_uint64)]
        L.dhts_ivl_merge_open.argtypes = [C.c_void_p, C.c_int64]
        L.dhts_ivl_merge_next.argtypes = [C.c_void_p, C.c_int64, C.c_uint32, C.POINTER(BedBatch)]
        L.dhts_ivl_overlap_open.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.dhts_ivl_overlap_next.argtypes = [C.c_void_p, C.c_int64, C.c_uint32, C.POINTER(BedBatch)]
        L.dhts_ivl_batch_host_bytes.restype = C.c_uint64
        L.dhts_ivl_batch_host_bytes.argtypes = [C.POINTER(BedBatch)]
        L.dhts_ivl_batch_fetch.argtypes = [C.c_void_p, C.POINTER(BedBatch), C.c_void_p, C.c_uint64, C.POINTER(BcfCol)]
        L.dhts_ivl_nearest_open.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32]
        L.dhts_ivl_nearest_next.argtypes = [C.c_void_p, C.c_int64, C.c_uint32, C.POINTER(BedBatch)]
        L.dhts_ivl_nearest_stats_get.argtypes = [C.c_void_p, C.POINTER(IvlNearestStats)]
        L.dhts_debug_ivl_sort.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_int32)]
        L.dhts_debug_ivl_ms.restype = C.c_double
        L.dhts_debug_ivl_ms.argtypes = [C.c_void_p, C.c_int]
        L.dhts_debug_rows_text.restype = C.c_int64
        L.dhts_debug_rows_text.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64]
        L.dhts_debug_rows_text_paths.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.dhts_debug_export_limits.argtypes = [C.c_void_p, C.c_int64, C.c_int64]
        L.dhts_debug_rows_text_form.argtypes = [C.c_void_p, C.c_int]
        L.dhts_debug_pileup_add_form.argtypes = [C.c_void_p, C.c_int]
        L.dhts_debug_carry.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_uint64]
        L.dhts_debug_line_table.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, C.c_int] + [C.c_void_p] * 5
        L.dhts_debug_hist_max_table_bytes.argtypes = [C.c_uint64]
        L.dhts_debug_hist_max_table_bytes.restype = None
        L.dhts_debug_hist_pass_ms.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.dhts_debug_hist_pass_ms.restype = C.c_double
        L.dhts_debug_coverage_max_table_bytes.restype = None
        L.dhts_debug_coverage_max_table_bytes.argtypes = [C.c_uint64]
        L.dhts_debug_bedcov_max_rows.restype = None
        L.dhts_debug_bedcov_max_rows.argtypes = [C.c_uint64]
        L.dhts_tabix_open.argtypes = [C.c_void_p, C.c_int]
        L.dhts_tabix_set_conf.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.dhts_tabix_index_conf.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.dhts_tabix_sniff.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(TabixSniffed)]
        L.dhts_tabix_resolve_schema.argtypes = [C.POINTER(TabixSniffed), C.c_int, C.POINTER(C.c_char_p), C.c_int32, C.POINTER(C.c_char_p), C.c_int32, C.c_int,
                                                C.POINTER(C.c_char_p), C.c_void_p, C.c_int32, C.POINTER(TabixSchema), C.c_char_p, C.c_uint64]
        L.dhts_tabix_set_schema.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int]
        L.dhts_tabix_set_projection.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.dhts_tabix_set_region.argtypes = [C.c_void_p, C.c_char_p]
        L.dhts_tabix_load_index.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.dhts_tabix_region_segments.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        L.dhts_tabix_next_batch.argtypes = [C.c_void_p, C.c_int64, C.POINTER(TabixBatch)]
        L.dhts_tabix_batch_host_bytes.restype = C.c_uint64
        L.dhts_tabix_batch_host_bytes.argtypes = [C.POINTER(TabixBatch)]
        L.dhts_tabix_batch_fetch.argtypes = [C.c_void_p, C.POINTER(TabixBatch), C.c_void_p, C.c_uint64, C.POINTER(BcfCol), C.POINTER(TabixMap)]
        L.dhts_udf_upload.argtypes = [C.c_void_p, C.c_int, C.POINTER(UdfArg), C.c_int64, C.POINTER(UdfArg)]
        L.dhts_udf_apply.argtypes = [C.c_void_p, C.c_int, C.POINTER(UdfArg), C.POINTER(UdfArg), C.c_int64, C.POINTER(UdfResult)]
        L.dhts_udf_result_host_bytes.restype = C.c_uint64
        L.dhts_udf_result_host_bytes.argtypes = [C.POINTER(UdfResult)]
        L.dhts_udf_fetch.argtypes = [C.c_void_p, C.POINTER(UdfResult), C.c_void_p, C.c_uint64, C.POINTER(UdfResult)]
        L.dhts_udf_seq_kmers.argtypes = [C.c_void_p, C.POINTER(UdfArg), C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_uint64, C.POINTER(UdfKmers)]
        L.dhts_udf_kmers_host_bytes.restype = C.c_uint64
        L.dhts_udf_kmers_host_bytes.argtypes = [C.POINTER(UdfKmers)]
        L.dhts_udf_kmers_fetch.argtypes = [C.c_void_p, C.POINTER(UdfKmers), C.c_void_p, C.c_uint64, C.POINTER(UdfKmers)]
        _LIB = L
    return _LIB


class DhtsError(RuntimeError):
    pass


def _clip(v, bits):
    """what a signed C field of bits + 1 bits holds of v; the C side checks the ranges"""
    return max(-1, min(int(v), 2 ** bits - 1))


class Context:
    """One scan context = one GPU + one HIP stream (include/duckhts_amd.h)."""

    def __init__(self, device=0):
        self.L = lib()
        self.h = self.L.dhts_create(device)
        if not self.h:
            raise DhtsError("dhts_create failed: no MI355X device / gfx950 code object (there is no CPU fallback)")

    def close(self):
        if self.h:
            self.L.dhts_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc < 0:
            raise DhtsError(self.L.dhts_error(self.h).decode())
        return rc

    # ---- input ----
    def open(self, src):
        if isinstance(src, (bytes, bytearray, memoryview)):
            buf = np.frombuffer(src, dtype=np.uint8)
            self._chk(self.L.dhts_open_host(self.h, buf.ctypes.data, buf.nbytes))
        elif isinstance(src, np.ndarray):
            self._chk(self.L.dhts_open_host(self.h, src.ctypes.data, src.nbytes))
        else:
            self._chk(self.L.dhts_open_path(self.h, os.fsencode(src)))
        return self

    def open_tiled(self, head, body, reps, tail):
        a = [np.ascontiguousarray(np.frombuffer(x, dtype=np.uint8)) if not isinstance(x, np.ndarray) else x
             for x in (head, body, tail)]
        self._chk(self.L.dhts_open_tiled(self.h, a[0].ctypes.data, a[0].nbytes, a[1].ctypes.data, a[1].nbytes, reps,
                                         a[2].ctypes.data, a[2].nbytes))
        return self

    # ---- BGZF ----
    def bgzf_index(self):
        return self._chk(self.L.dhts_bgzf_index(self.h))

    def bgzf_compress(self, raw, level=-1):
        """bgzip on the device: raw bytes -> the bytes of a BGZF file (EOF block included)"""
        buf = np.frombuffer(raw, dtype=np.uint8) if len(raw) else np.zeros(0, np.uint8)
        f = self.L.dhts_bgzf_compress
        f.restype = C.c_int64
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64]
        bound = self._chk(f(self.h, buf.ctypes.data, buf.nbytes, level, None, 0))
        out = np.empty(bound, np.uint8)
        n = self._chk(f(self.h, buf.ctypes.data, buf.nbytes, level, out.ctypes.data, bound))
        return out[:n].tobytes()

    def bgzip_file(self, src, dst, level=-1):
        a, b = C.c_int64(0), C.c_int64(0)
        self.L.dhts_bgzip_file.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        self._chk(self.L.dhts_bgzip_file(self.h, os.fsencode(src), os.fsencode(dst), level, C.byref(a), C.byref(b)))
        return a.value, b.value

    def bgunzip_file(self, src, dst):
        a, b = C.c_int64(0), C.c_int64(0)
        self.L.dhts_bgunzip_file.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        self._chk(self.L.dhts_bgunzip_file(self.h, os.fsencode(src), os.fsencode(dst), C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_seq_packed(self, on=True):
        self.L.dhts_bam_set_seq_packed.argtypes = [C.c_void_p, C.c_int]
        self.L.dhts_bam_set_seq_packed.restype = None
        self.L.dhts_bam_set_seq_packed(self.h, int(on))

    def scan_window_stats(self):
        """(index windows, BGZF blocks) of the current scan range (the whole file without an index)"""
        w, b = C.c_int64(0), C.c_int64(0)
        self.L.dhts_scan_window_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        self._chk(self.L.dhts_scan_window_stats(self.h, C.byref(w), C.byref(b)))
        return w.value, b.value

    REPAIR_STATS = ("replaced", "scratch_retries", "replaced_in_retry")

    def bgzf_repair_stats(self):
        """what the block table's corrections did on this context: {blocks re-placed from their decoded length in total, block ranges
        decoded again after the packed scratch ran out, blocks re-placed during such a repeat} (dhts_bgzf_repair_stats)"""
        out = (C.c_int64 * 3)()
        self.L.dhts_bgzf_repair_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        self._chk(self.L.dhts_bgzf_repair_stats(self.h, out))
        return {k: int(out[i]) for i, k in enumerate(self.REPAIR_STATS)}

    def tell(self, uoff):
        """BGZF virtual offset of the byte at `uoff` of the inflated stream as this context numbers it (dhts_voffset): the block is the one
        that holds the byte, which every context that reached it has decoded, so the value does not depend on ISIZE fields"""
        self.L.dhts_voffset.restype = C.c_uint64
        self.L.dhts_voffset.argtypes = [C.c_void_p, C.c_uint64]
        return int(self.L.dhts_voffset(self.h, int(uoff)))

    def bgzf_table(self, n):
        coff = np.zeros(n, np.uint64)
        clen = np.zeros(n, np.uint32)
        isize = np.zeros(n, np.uint32)
        st = self.L.dhts_bgzf_table(self.h, coff.ctypes.data, clen.ctypes.data, isize.ctypes.data, n)
        return coff, clen, isize, st

    def bgzf_inflate(self, blk0, nblk, cap):
        out = np.zeros(max(cap, 1), np.uint8)
        st = np.zeros(max(nblk, 1), np.int32)
        n = self._chk(self.L.dhts_bgzf_inflate_to_host(self.h, blk0, nblk, out.ctypes.data, cap, st.ctypes.data))
        return out[:n], st[:nblk]

    # ---- read_bam ----
    def bam_open(self):
        self._chk(self.L.dhts_bam_open(self.h))
        return self.header()

    def bam_is_text(self):
        """after bam_open: 0 BAM, 1 bgzipped SAM text, 2 plain SAM text (uncompressed or plain gzip), 3 / 4 FASTQ and 5 / 6 FASTA likewise"""
        return self.L.dhts_bam_is_text(self.h)

    def debug_sam_records(self):
        """the BAM records the device encoder made of the last SAM text batch: (bytes, number of records)"""
        n = C.c_int64(0)
        size = self._chk(self.L.dhts_debug_sam_records(self.h, None, 0, C.byref(n)))
        buf = np.zeros(max(size, 1), np.uint8)
        self._chk(self.L.dhts_debug_sam_records(self.h, buf.ctypes.data, size, C.byref(n)))
        return buf[:size].tobytes(), n.value

    TILE_STATS = ("repaired_tiles", "repair_rounds", "fallback_batches", "spec_retries", "validate_rejections", "gave_up")

    def debug_tile_stats(self):
        """what the record stage's repair and retry paths did since the scan was opened or rewound (read_bam and read_bcf alike):
        {TILE_STATS name: count} (include/duckhts_amd_debug.h: dhts_debug_tile_stats)"""
        out = (C.c_uint64 * 8)()
        self._chk(self.L.dhts_debug_tile_stats(self.h, out))
        return {k: int(out[i]) for i, k in enumerate(self.TILE_STATS)}

    def debug_tile_scan(self, kernel, ulen):
        """one tile-scan kernel alone ("wave" or "lanes") over the inflated batch the context holds (`ulen` bytes or fewer), before any
        repair round: {first, end_next, count, err, recs_first: arrays per tile; recs: [ntiles, 256] record starts relative to the tile,
        entries k >= min(count, 256) masked to 0xeeee} (include/duckhts_amd_debug.h: dhts_debug_tile_scan)"""
        import numpy as np
        cap = max(1, (int(ulen) + 8191) // 8192)
        t = {"first": np.zeros(cap, np.uint64), "end_next": np.zeros(cap, np.uint64), "count": np.zeros(cap, np.uint32), "err": np.zeros(cap, np.int32),
             "recs_first": np.zeros(cap, np.uint64), "recs": np.zeros((cap, 256), np.uint16)}
        n = self._chk(self.L.dhts_debug_tile_scan(self.h, {"wave": 0, "lanes": 1}[kernel], *[t[k].ctypes.data for k in ("first", "end_next", "count", "err", "recs_first", "recs")], cap))
        return {k: v[:n] for k, v in t.items()}

    def debug_fastq_records(self):
        """the BAM records the device encoder made of the last FASTQ / FASTA batch: (bytes, number of records)"""
        n = C.c_int64(0)
        size = self._chk(self.L.dhts_debug_fastq_records(self.h, None, 0, C.byref(n)))
        buf = np.zeros(max(size, 1), np.uint8)
        self._chk(self.L.dhts_debug_fastq_records(self.h, buf.ctypes.data, size, C.byref(n)))
        return buf[:size].tobytes(), n.value

    def debug_deflate_codes(self, counts, maxbits):
        """the DEFLATE encoder's code builder on the device: counts[ncases, nsym] -> (lengths uint8[ncases, nsym], table words
        uint32[ncases, nsym]: bit-reversed code | length << 16).  Only for count vectors the builder is known to end on."""
        cnt = np.ascontiguousarray(counts, dtype=np.uint32)
        assert cnt.ndim == 2
        lens, codes = np.zeros(cnt.shape, np.uint8), np.zeros(cnt.shape, np.uint32)
        f = self.L.dhts_debug_deflate_codes
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int64, C.c_void_p, C.c_void_p]
        self._chk(f(self.h, cnt.ctypes.data, cnt.shape[1], maxbits, cnt.shape[0], lens.ctypes.data, codes.ctypes.data))
        return lens, codes

    def debug_carry(self, kind, v, seed=0):
        """the carry in two levels alone (dhts_debug_carry) on a copy of v: uint32[n] (kind 0), uint64[n] (1, 2) or uint64[n, 4] (3).  Returns
        the scanned array; kinds 0, 1 and 3 return n + 1 elements, the total last.  The element behind the last goes to the device as one
        that would change every answer it took part in (0 for the minimum, all ones for the sums)."""
        a = np.ascontiguousarray(v, dtype=np.uint32 if kind == 0 else np.uint64)
        n = a.shape[0]
        out = np.empty((n + 1,) + a.shape[1:], a.dtype)
        out[:n] = a
        out[n] = 0 if kind == 2 else np.iinfo(a.dtype).max
        self._chk(self.L.dhts_debug_carry(self.h, kind, out.ctypes.data, n, seed))
        return out[:n] if kind == 2 else out

    def debug_line_table(self, text, t0=0, open_last_ok=True, lim=None, tabs=False):
        """the text readers' line table alone (dhts_debug_line_table) on `text`: a dict of the result's fields and the arrays line_off
        (nlines + 1 starts) and, with tabs, tab_off, tab0 and has_nul; the arrays are empty when t0 lies at or behind the text's end"""
        n = len(text)
        src = np.frombuffer(bytes(text) + b"\0", np.uint8)
        w = np.zeros(7, np.uint64)
        a = [np.zeros(n + 2, np.uint32) for _ in range(4)]
        self._chk(self.L.dhts_debug_line_table(self.h, src.ctypes.data, n, t0, int(bool(open_last_ok)), 0xffffffffffffffff if lim is None else lim, int(bool(tabs)),
                                               w.ctypes.data, *[x.ctypes.data for x in a]))
        out = dict(zip(("nl", "ntabs", "nlines", "last_start", "carry_start", "last_open", "finished"), (int(x) for x in w)))
        nlines, made = out["nlines"], t0 < n
        out["line_off"] = a[0][:nlines + 1 if made else 0]
        if tabs:
            out["tab_off"], out["tab0"], out["has_nul"] = a[1][:out["ntabs"]], a[2][:nlines + 1 if made else 0], a[3][:nlines]
        return out

    def header(self):
        h = BamHeader()
        self._chk(self.L.dhts_bam_header_get(self.h, C.byref(h)))
        return {
            "n_ref": h.n_ref,
            "ref_names": [h.ref_name[i] for i in range(h.n_ref)],
            "ref_len": [h.ref_len[i] for i in range(h.n_ref)],
            "text": C.string_at(h.text, h.l_text) if h.l_text else b"",
            "rg_id": [h.rg_id[i] for i in range(h.n_rg)],
            "rg_sm": [h.rg_sm[i] for i in range(h.n_rg)],
            "first_rec_uoff": h.first_rec_uoff,
        }

    def set_shard(self, rank, world):
        self._chk(self.L.dhts_bam_set_shard(self.h, rank, world))

    def set_block_range(self, b0, b1, speculative):
        self._chk(self.L.dhts_bam_set_block_range(self.h, b0, b1, int(speculative)))

    def rewind(self):
        self._chk(self.L.dhts_bam_rewind(self.h))

    def set_tag_columns(self, ids):
        arr = np.array(list(ids), np.int32)
        self._chk(self.L.dhts_bam_set_tag_columns(self.h, arr.ctypes.data, len(arr)))
        self._tag_ids = list(ids)

    def build_index(self, min_shift=0):
        """BAI bytes for the open BAM (one whole-file scan; hts_idx_push / hts_idx_finish restated on the host).  min_shift > 0: a CSI with
        that min_shift and the depth the longest reference asks for (dhts_bam_build_index_csi); those bytes are the UNCOMPRESSED CSI, a
        .csi file on disk is their BGZF wrapping (dhts_bgzf_wrap)."""
        if min_shift > 0:
            self.L.dhts_bam_build_index_csi.restype = C.c_int64
            self.L.dhts_bam_build_index_csi.argtypes = [C.c_void_p, C.c_int]
            n = self._chk(self.L.dhts_bam_build_index_csi(self.h, min_shift))
        else:
            n = self._chk(self.L.dhts_bam_build_index(self.h))
        out = np.empty(n, np.uint8)
        self._chk(self.L.dhts_bam_index_bytes(self.h, out.ctypes.data, n))
        return out.tobytes()

    def set_overlap_intervals(self, tid, beg, end):
        """Interval overlap join (cgranges cr_overlap semantics): intervals (tid, beg, end) half-open 0-based, tid = BAM header index."""
        tid = np.ascontiguousarray(tid, np.int32); beg = np.ascontiguousarray(beg, np.int64); end = np.ascontiguousarray(end, np.int64)
        assert len(tid) == len(beg) == len(end)
        self._chk(self.L.dhts_bam_set_overlap_intervals(self.h, tid.ctypes.data, beg.ctypes.data, end.ctypes.data, len(tid)))

    def set_overlap_bed(self, bed):
        """The join's intervals from a BED: bytes = the text itself, str / PathLike = a plain or bgzipped file.  Returns the number of
        read_bed rows; interval ids are those row numbers."""
        if isinstance(bed, (bytes, bytearray, memoryview)):
            buf = np.frombuffer(bytes(bed), dtype=np.uint8)
            self.L.dhts_bam_set_overlap_bed.restype = C.c_int64; self.L.dhts_bam_set_overlap_bed.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
            n = self.L.dhts_bam_set_overlap_bed(self.h, buf.ctypes.data if buf.nbytes else None, buf.nbytes)
        else:
            self.L.dhts_bam_set_overlap_bed_path.restype = C.c_int64; self.L.dhts_bam_set_overlap_bed_path.argtypes = [C.c_void_p, C.c_char_p]
            n = self.L.dhts_bam_set_overlap_bed_path(self.h, os.fsencode(bed))
        self._chk(-1 if n < 0 else 0)
        return int(n)

    def overlap_lists(self, b):
        """(offsets u32[n_rows+1], ids u32[n_ov]) of one batch; ids are positions in the arrays given to set_overlap_intervals"""
        n = int(b.n_rows)
        if not b.ov_off:                               # join switched off (no intervals): every row has an empty list
            return np.zeros(n + 1, np.uint32), np.zeros(0, np.uint32)
        return self.d2h(b.ov_off, n + 1, np.uint32), self.d2h(b.ov_ids, int(b.n_ov), np.uint32)

    def set_aux_map(self, enable=True, exclude_standard=True):
        self._chk(self.L.dhts_bam_set_aux_map(self.h, int(enable), int(exclude_standard)))

    def aux_table(self, b):
        """AUXILIARY_TAGS of one batch: typed device entries -> keys / rendered value text (bam_aux_to_string, src/bam_reader.c:140-183;
        the %g / %lld text is host-side formatting) as two LIST(VARCHAR) columns in the canonical layout"""
        import math
        import struct as st_
        n = int(b.n_rows)
        am = C.cast(b.aux_map, C.POINTER(AuxMap)).contents
        ne = int(am.n_ent)
        valid = self.d2h(am.valid, n, np.uint8) if n else np.zeros(0, np.uint8)
        off = self.d2h(am.off, n + 1, np.uint32).astype(np.uint64) if n else np.zeros(1, np.uint64)
        key = self.d2h(am.key, ne, np.uint16)
        kind = self.d2h(am.kind, ne, np.uint8)
        sub = self.d2h(am.sub, ne, np.uint8)
        po = self.d2h(am.pay_off, ne + 1, np.uint32) if n else np.zeros(1, np.uint32)
        pay = self.d2h(am.payload, int(am.payload_bytes), np.uint8).tobytes()
        keys, vals = [], []
        g = lambda x: (b"-nan" if math.copysign(1.0, x) < 0 else b"nan") if x != x else b"%g" % x      # printf prints a NaN with its sign, Python's %g without
        for i in range(ne):
            kb = bytes([int(key[i]) & 0xff, int(key[i]) >> 8]).split(b"\0")[0]
            p = pay[int(po[i]):int(po[i + 1])]
            k = int(kind[i])
            if k == 0:
                v = b"%d" % st_.unpack("<q", p)[0]
            elif k == 1:
                v = g(st_.unpack("<d", p)[0])
            elif k in (2, 3):
                v = p
            elif k == 4:
                v = bytes([int(sub[i])]) + b"".join(b",%d" % x for x in st_.unpack("<%dq" % (len(p) // 8), p))
            elif k == 5:
                v = bytes([int(sub[i])]) + b"".join(b"," + g(x) for x in st_.unpack("<%dd" % (len(p) // 8), p))
            else:
                v = b""
            keys.append(kb)
            vals.append(v.split(b"\0")[0])                    # assigned through the NUL-terminated API
        cols = []
        for name, items in (("AUX_KEYS", keys), ("AUX_VALUES", vals)):
            lens = np.array([len(x) for x in items], np.int64)
            cols.append({"name": name, "type": 1, "is_list": 1, "valid": valid, "loff": off[:-1].copy(), "llen": off[1:] - off[:-1], "child_n": ne,
                         "csoff": np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), "csbytes": np.frombuffer(b"".join(items), np.uint8)})
        return {"n_rows": n, "cols": cols}

    def tag_table(self, b):
        """standard-tag columns of one batch -> canonical column table (layout of tests/orc.py decode_bcf_blob)"""
        n = int(b.n_rows)
        cols = []
        arr = C.cast(b.tag_cols, C.POINTER(BcfCol))
        for i in range(b.n_tag_cols):
            dc = arr[i]
            name, ty, _ = std_tags()[dc.col]
            c = {"name": name, "type": 2 if ty in "iB" else 1, "is_list": 1 if ty == "B" else 0}
            c["valid"] = self.d2h(dc.valid, n, np.uint8) if n else np.zeros(0, np.uint8)
            if ty == "i":
                c["fixed"] = self.d2h(dc.fixed, n, np.uint64) if n else np.zeros(0, np.uint64)
            elif ty == "B":
                off = self.d2h(dc.off, n + 1, np.uint32).astype(np.uint64) if n else np.zeros(1, np.uint64)
                c["loff"], c["llen"], c["child_n"] = off[:-1].copy(), off[1:] - off[:-1], int(dc.child_n)
                c["cfixed"] = self.d2h(dc.child_fixed, int(dc.child_n), np.uint64)
            else:
                c["soff"] = self.d2h(dc.off, n + 1, np.uint32).astype(np.uint64) if n else np.zeros(1, np.uint64)
                c["sbytes"] = self.d2h(dc.bytes, int(dc.nbytes), np.uint8)
            cols.append(c)
        return {"n_rows": n, "status": int(b.status), "cols": cols}

    def set_regions(self, regions):
        """region := 'chr:beg-end,...'; returns False when no region names a known reference"""
        return self._chk(self.L.dhts_bam_set_regions(self.h, regions.encode() if isinstance(regions, str) else regions)) == 0

    def load_index(self, bai_bytes):
        buf = np.frombuffer(bai_bytes, dtype=np.uint8)
        self._chk(self.L.dhts_bam_load_index(self.h, buf.ctypes.data, buf.nbytes))

    def region_segments(self, index_bytes, cap=4096):
        """file byte ranges (beg[], end[]) the regions set on this context need, or None for the whole file (dhts_bam_region_segments)"""
        buf = np.frombuffer(index_bytes, dtype=np.uint8)
        beg, end, n = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), C.c_int64(0)
        self.L.dhts_bam_region_segments.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        self._chk(self.L.dhts_bam_region_segments(self.h, buf.ctypes.data, buf.nbytes, beg.ctypes.data, end.ctypes.data, cap, C.byref(n)))
        return None if n.value < 0 else (beg[:n.value].copy(), end[:n.value].copy())

    def bcf_region_segments(self, regions, index_bytes, cap=4096):
        """(header bytes, beg[], end[]) a read_bcf region query stages instead of the whole file, or None (dhts_bcf_region_segments)"""
        buf = np.frombuffer(index_bytes, dtype=np.uint8)
        beg, end, n = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), C.c_int64(0)
        self.L.dhts_bcf_header_bytes.restype = C.c_uint64
        self.L.dhts_bcf_header_bytes.argtypes = [C.c_void_p]
        self.L.dhts_bcf_region_segments.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        self._chk(self.L.dhts_bcf_region_segments(self.h, regions.encode(), buf.ctypes.data, buf.nbytes, beg.ctypes.data, end.ctypes.data, cap, C.byref(n)))
        return None if n.value < 0 else (int(self.L.dhts_bcf_header_bytes(self.h)), beg[:n.value].copy(), end[:n.value].copy())

    def open_segments(self, path, header_bytes, beg, end):
        beg, end = np.ascontiguousarray(beg, np.uint64), np.ascontiguousarray(end, np.uint64)
        self.L.dhts_open_path_segments.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int64]
        self._chk(self.L.dhts_open_path_segments(self.h, os.fsencode(path), int(header_bytes), beg.ctypes.data, end.ctypes.data, len(beg)))
        return self

    # ---- fasta_index / read_fasta regions ----
    def fasta_build_index(self):
        """(.fai bytes, .gzi bytes) of the resident FASTA (open + bgzf_index first); the .gzi is b"" for uncompressed input"""
        n = self._chk(self.L.dhts_fasta_build_index(self.h))
        fai = np.zeros(max(n, 1), np.uint8)
        self._chk(self.L.dhts_fasta_index_bytes(self.h, fai.ctypes.data, n))
        m = self._chk(self.L.dhts_fasta_gzi_bytes(self.h, None, 0))
        gzi = np.zeros(max(m, 1), np.uint8)
        if m:
            self._chk(self.L.dhts_fasta_gzi_bytes(self.h, gzi.ctypes.data, m))
        return fai[:n].tobytes(), gzi[:m].tobytes()

    def fasta_load_index(self, fai):
        self._chk(self.L.dhts_fasta_load_index(self.h, bytes(fai), len(fai)))
        return self

    def fasta_open_regions(self, path, regions):
        self._chk(self.L.dhts_fasta_open_regions(self.h, os.fsencode(path), regions.encode() if isinstance(regions, str) else regions))
        return self

    def resident_bytes(self):
        return int(self.L.dhts_resident_bytes(self.h))

    def fasta_fetch(self, regions):
        """[(name, sequence)] of the regions 'a:1-10,b', through the device batch and the host fetch"""
        b, hb = FastaBatch(), FastaBatch()
        self._chk(self.L.dhts_fasta_fetch(self.h, regions.encode() if isinstance(regions, str) else regions, C.byref(b)))
        need = int(self.L.dhts_fasta_batch_host_bytes(C.byref(b)))
        arena = np.zeros(need, np.uint8)
        self._chk(self.L.dhts_fasta_batch_fetch(self.h, C.byref(b), arena.ctypes.data, need, C.byref(hb)))
        base = arena.ctypes.data
        n = hb.n_rows
        noff = arena[hb.name_off - base: hb.name_off - base + (n + 1) * 8].view(np.uint64)
        soff = arena[hb.seq_off - base: hb.seq_off - base + (n + 1) * 8].view(np.uint64)
        nb = arena[hb.name_bytes - base: hb.name_bytes - base + hb.name_nbytes].tobytes()
        sb = arena[hb.seq_bytes - base: hb.seq_bytes - base + hb.seq_nbytes].tobytes()
        return [(nb[int(noff[i]):int(noff[i + 1])], sb[int(soff[i]):int(soff[i + 1])]) for i in range(n)]

    # ---- fasta_nuc (the batch has dhts_bed_batch's layout) ----
    def nuc_open(self, include_seq=False):
        self._chk(self.L.dhts_nuc_open(self.h, int(bool(include_seq))))
        self.nuc_projection = list(range(len(NUC_COLUMNS) - (0 if include_seq else 1)))
        return self

    def nuc_set_region(self, region):
        """False for a region the reference calls invalid ("fasta_nuc: invalid FASTA region")"""
        r = region.encode() if isinstance(region, str) else region
        return self._chk(self.L.dhts_nuc_set_region(self.h, r)) == 0

    def nuc_set_projection(self, cols):
        ids = [c if isinstance(c, int) else NUC_COLUMNS.index(c) for c in cols]
        arr = np.array(ids, np.int32)
        self._chk(self.L.dhts_nuc_set_projection(self.h, arr.ctypes.data, len(ids)))
        self.nuc_projection = ids

    def nuc_next_bins(self, bin_width, max_rows=0):
        b = BedBatch()
        self._chk(self.L.dhts_nuc_next_bins(self.h, bin_width, max_rows, C.byref(b)))
        return b

    def nuc_next_bed(self, bed_ctx, max_blocks=0):
        b = BedBatch()
        self._chk(self.L.dhts_nuc_next_bed(self.h, bed_ctx.h, max_blocks, C.byref(b)))
        return b

    def nuc_batch_columns(self, b):
        """the projected columns of one batch through dhts_nuc_batch_fetch: {"n_rows", name: python list, None for NULL}; the two
        fractions come back as float64 values whose bits are the device's"""
        n = int(b.n_rows)
        need = int(self.L.dhts_nuc_batch_host_bytes(C.byref(b)))
        arena = np.zeros(max(need, 8), np.uint8)
        host = (BcfCol * max(b.n_cols, 1))()
        self._chk(self.L.dhts_nuc_batch_fetch(self.h, C.byref(b), arena.ctypes.data, need, host))
        base = arena.ctypes.data
        out = {"n_rows": n}
        for i in range(b.n_cols):
            hc = host[i]
            name = NUC_COLUMNS[hc.col]
            if n == 0:
                out[name] = []
                continue
            valid = arena[hc.valid - base: hc.valid - base + n]
            if hc.col in NUC_STR_COLUMNS:
                off = arena[hc.off - base: hc.off - base + 4 * (n + 1)].view(np.uint32)
                data = arena[hc.bytes - base: hc.bytes - base + int(hc.nbytes)].tobytes()
                out[name] = [data[int(off[r]):int(off[r + 1])] if valid[r] else None for r in range(n)]
            else:
                vals = arena[hc.fixed - base: hc.fixed - base + 8 * n].view(np.float64 if hc.col in NUC_DOUBLE_COLUMNS else np.int64)
                out[name] = vals.tolist()
        return out

    def nuc_intervals(self, tid, start, end):
        """fasta_nuc's rows for already-resolved intervals (tid = index of the sequence in the loaded .fai, < 0: unknown); nuc_open first"""
        t, s, e = np.ascontiguousarray(tid, np.int32), np.ascontiguousarray(start, np.int64), np.ascontiguousarray(end, np.int64)
        if not (len(t) == len(s) == len(e)):
            raise ValueError("tid, start and end have to be of one length")
        b = BedBatch()
        self._chk(self.L.dhts_nuc_intervals(self.h, t.ctypes.data, s.ctypes.data, e.ctypes.data, len(t), C.byref(b)))
        return self.nuc_batch_columns(b)

    # ---- what the seven bam_* count functions share (the batches have dhts_bed_batch's layout) ----
    def _accum_scan(self, name, max_blocks, stats=None):
        """name: the C entries' (dhts_bam_<name>_*); stats: the method that reads the stats where it is not bam_<name>_stats"""
        rc = getattr(self.L, "dhts_bam_%s_scan" % name)(self.h, max_blocks)
        if rc < 0:
            msg = self.L.dhts_error(self.h).decode()
            if (stats or getattr(self, "bam_%s_stats" % name))()["status"] == 0:        # a call failed (a stream that ended on an error has set its status)
                raise DhtsError(msg)
        return rc

    def _accum_stats(self, name, cls):
        st = cls()
        self._chk(getattr(self.L, "dhts_bam_%s_stats" % name)(self.h, C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in cls._fields_ if k != "reserved"}

    def _fetch_cols(self, name, b):
        """the columns of the result batch b on the host: (arena, host columns with pointers into it, rows)"""
        need = int(getattr(self.L, "dhts_bam_%s_batch_host_bytes" % name)(C.byref(b)))
        arena = np.zeros(max(need, 8), np.uint8)
        host = (BcfCol * max(b.n_cols, 1))()
        self._chk(getattr(self.L, "dhts_bam_%s_batch_fetch" % name)(self.h, C.byref(b), arena.ctypes.data, need, host))
        return arena, host, int(b.n_rows)

    def _fixed_cols(self, name, b, mask, names, dtypes):
        """a page of bare fixed columns (bam_depth, bam_pileup, bam_bedgraph, bam_depth_hist): None for a column the mask leaves out"""
        arena, host, n = self._fetch_cols(name, b)
        out = {"n_rows": n}
        for i in range(b.n_cols):
            col, dt = names[host[i].col], dtypes[host[i].col]
            if not (mask >> host[i].col) & 1:
                assert not b.cols[i].fixed and not host[i].fixed
                out[col] = None
            elif n == 0:
                out[col] = np.zeros(0, dt)
            else:
                off = host[i].fixed - arena.ctypes.data
                out[col] = arena[off:off + n * np.dtype(dt).itemsize].view(dt).copy()
        return out, int(b.status)

    # ---- bam_bin_counts ----
    def bam_bins_open(self, bin_width=5000, min_mapq=0, include_flags=0, require_flags=0, exclude_flags=0, dedup="none", emit_zero_bins=False):
        """after bam_open and the optional set_regions / load_index: the table of counters, zeroed"""
        if dedup not in BINS_DEDUP:
            raise DhtsError("bam_bin_counts: dedup must be one of: none, adjacent")
        p = BinsParams(_clip(bin_width, 63), _clip(min_mapq, 31), _clip(require_flags, 31), _clip(exclude_flags, 31), _clip(include_flags, 31), BINS_DEDUP[dedup], int(bool(emit_zero_bins)))
        self._chk(self.L.dhts_bam_bins_open(self.h, C.byref(p)))

    def bam_bins_accumulate(self, b):
        self._chk(self.L.dhts_bam_bins_accumulate(self.h, C.byref(b)))

    def bam_bins_scan(self, max_blocks=0):
        """the scan to the end of the stream; the status it ended on (1, or the negative status of a stream that ended on an error)"""
        return self._accum_scan("bins", max_blocks)

    def bam_bins_stats(self):
        return self._accum_stats("bins", BinsStats)

    def bam_bins_next(self, max_rows=0):
        """the next rows of the result: ({"n_rows", column: int64 array; chrom = the contig's id}, status)"""
        b = BedBatch()
        self._chk(self.L.dhts_bam_bins_next(self.h, max_rows, C.byref(b)))
        arena, host, n = self._fetch_cols("bins", b)
        out = {"n_rows": n}
        for i in range(b.n_cols):
            out[BINS_COLUMNS[host[i].col]] = np.ctypeslib.as_array(C.cast(host[i].fixed, C.POINTER(C.c_int64)), (n,)).copy() if n else np.zeros(0, np.int64)
        return out, int(b.status)

    # ---- bam_coverage ----
    def bam_coverage_open(self, min_read_len=0, min_mapq=0, min_baseq=0, include_flags=0, require_flags=0, exclude_flags=0, min_depth=1):
        """after bam_open and the optional set_regions / load_index: the target rows, the depth table and the counters, zeroed.  The
        parameters are taken as given (the C ABI's rule)."""
        p = CoverageParams(_clip(min_read_len, 63), _clip(min_depth, 63), _clip(min_mapq, 31), _clip(min_baseq, 31), _clip(require_flags, 31), _clip(exclude_flags, 31), _clip(include_flags, 31), 0)
        self._chk(self.L.dhts_bam_coverage_open(self.h, C.byref(p)))

    def bam_coverage_accumulate(self, b):
        """b: the batch next_batch returned last on this context"""
        self._chk(self.L.dhts_bam_coverage_accumulate(self.h, C.byref(b)))

    def bam_coverage_scan(self, max_blocks=0):
        """the scan to the end of the stream; the status it ended on (1, or the negative status of a stream that ended on an error)"""
        return self._accum_scan("coverage", max_blocks)

    def bam_coverage_stats(self):
        return self._accum_stats("coverage", CoverageStats)

    def bam_coverage_next(self, max_rows=0):
        """the next rows of the result: ({"n_rows", column: int64 array (chrom = the contig's id), float64 for the four means}, status)"""
        b = BedBatch()
        self._chk(self.L.dhts_bam_coverage_next(self.h, max_rows, C.byref(b)))
        arena, host, n = self._fetch_cols("coverage", b)
        out = {"n_rows": n}
        for i in range(b.n_cols):
            dt = np.float64 if host[i].col in COVERAGE_DOUBLE_COLUMNS else np.int64
            vals = np.ctypeslib.as_array(C.cast(host[i].fixed, C.POINTER(C.c_int64)), (n,)).copy() if n else np.zeros(0, np.int64)
            out[COVERAGE_COLUMNS[host[i].col]] = vals.view(dt)
        return out, int(b.status)

    # ---- bam_depth ----
    def bam_depth_open(self, bed_ctx=None, min_read_len=0, min_mapq=0, min_baseq=0, include_flags=0, require_flags=0, exclude_flags=0, include_deletions=0, all_positions=0):
        """after bam_open and the optional set_regions / load_index; bed_ctx: None, or a second Context on this device after bed_open.  The
        target rows, the depth table and the counters, zeroed.  The parameters are taken as given (the C ABI's rule)."""
        p = DepthParams(_clip(min_read_len, 63), _clip(min_mapq, 31), _clip(min_baseq, 31), _clip(require_flags, 31), _clip(exclude_flags, 31), _clip(include_flags, 31),
                        _clip(include_deletions, 31), _clip(all_positions, 31), 0)
        self._chk(self.L.dhts_bam_depth_open(self.h, C.byref(p), bed_ctx.h if bed_ctx is not None else None))

    def bam_depth_accumulate(self, b):
        """b: the batch next_batch returned last on this context"""
        self._chk(self.L.dhts_bam_depth_accumulate(self.h, C.byref(b)))

    def bam_depth_scan(self, max_blocks=0):
        """the scan to the end of the stream; the status it ended on (1, or the negative status of a stream that ended on an error)"""
        return self._accum_scan("depth", max_blocks)

    def bam_depth_stats(self):
        return self._accum_stats("depth", DepthStats)

    def bam_depth_next(self, max_rows=0, columns=None):
        """the next page of the result: ({"n_rows", "tid": int32, "pos": int64 (1-based), "depth": int32 arrays; None for a column that
        `columns` (names of DEPTH_COLUMNS; None: all) leaves out -- the batch has a null pointer there}, status)"""
        mask = sum(1 << DEPTH_COLUMNS.index(k) for k in set(columns)) if columns is not None else 7
        b = BedBatch()
        self._chk(self.L.dhts_bam_depth_next(self.h, max_rows, mask, C.byref(b)))
        return self._fixed_cols("depth", b, mask, DEPTH_COLUMNS, DEPTH_DTYPES)

    # ---- bam_pileup ----
    def bam_pileup_open(self, min_read_len=0, min_mapq=0, min_baseq=0, include_flags=0, require_flags=0, exclude_flags=0, include_deletions=0, include_insertions=0,
                        distinguish_strands=0, min_nucleotide_depth=1):
        """after bam_open and the optional set_regions / load_index: the target rows, the count table and the counters, zeroed.  The
        parameters are taken as given (the C ABI's rule)."""
        p = PileupParams(_clip(min_read_len, 63), _clip(min_mapq, 31), _clip(min_baseq, 31), _clip(require_flags, 31), _clip(exclude_flags, 31), _clip(include_flags, 31),
                         _clip(include_deletions, 31), _clip(include_insertions, 31), _clip(distinguish_strands, 31), _clip(min_nucleotide_depth, 31), 0)
        self._chk(self.L.dhts_bam_pileup_open(self.h, C.byref(p)))

    def bam_pileup_add_form(self, form):
        """tests and tools/bench_pileup.py: the add kernel's form (dhts_debug_pileup_add_form)"""
        self._chk(self.L.dhts_debug_pileup_add_form(self.h, form))

    def bam_pileup_accumulate(self, b):
        """b: the batch next_batch returned last on this context"""
        self._chk(self.L.dhts_bam_pileup_accumulate(self.h, C.byref(b)))

    def bam_pileup_scan(self, max_blocks=0):
        """the scan to the end of the stream; the status it ended on (1, or the negative status of a stream that ended on an error)"""
        return self._accum_scan("pileup", max_blocks)

    def bam_pileup_stats(self):
        return self._accum_stats("pileup", PileupStats)

    def bam_pileup_next(self, max_rows=0, columns=None):
        """the next page of the result: ({"n_rows", "tid": int32, "pos": int64 (1-based), "strand", "nucleotide": uint8 (ASCII), "count": int32
        arrays; None for a column that `columns` (names of PILEUP_COLUMNS; None: all) leaves out -- the batch has a null pointer there}, status)"""
        mask = sum(1 << PILEUP_COLUMNS.index(k) for k in set(columns)) if columns is not None else 31
        b = BedBatch()
        self._chk(self.L.dhts_bam_pileup_next(self.h, max_rows, mask, C.byref(b)))
        return self._fixed_cols("pileup", b, mask, PILEUP_COLUMNS, PILEUP_DTYPES)

    # ---- bam_bedgraph ----
    def bam_bedgraph_open(self, bed_ctx=None, min_read_len=0, min_mapq=0, min_baseq=0, include_flags=0, require_flags=0, exclude_flags=0, include_deletions=0, zero_runs=0,
                          breaks=None):
        """after bam_open and the optional set_regions / load_index; bed_ctx: None, or a second Context on this device after bed_open.  The
        target rows, the depth table and the counters, zeroed.  breaks: None, or the integers that cut the depths into classes.  The
        parameters are taken as given (the C ABI's rule): the first 16 breaks travel, and n_breaks says how many were given."""
        br = [] if breaks is None else [int(x) for x in breaks]
        p = BedgraphParams(_clip(min_read_len, 63), _clip(min_mapq, 31), _clip(min_baseq, 31), _clip(require_flags, 31), _clip(exclude_flags, 31), _clip(include_flags, 31),
                           _clip(include_deletions, 31), _clip(zero_runs, 31), len(br))
        for j, x in enumerate(br[:BEDGRAPH_MAX_BREAKS]):
            p.breaks[j] = x if 0 < x < 2 ** 31 else 0                       # (what an int32 cannot hold travels as 0, which the C side refuses)
        self._chk(self.L.dhts_bam_bedgraph_open(self.h, C.byref(p), bed_ctx.h if bed_ctx is not None else None))

    def bam_bedgraph_accumulate(self, b):
        """b: the batch next_batch returned last on this context"""
        self._chk(self.L.dhts_bam_bedgraph_accumulate(self.h, C.byref(b)))

    def bam_bedgraph_scan(self, max_blocks=0):
        """the scan to the end of the stream; the status it ended on (1, or the negative status of a stream that ended on an error)"""
        return self._accum_scan("bedgraph", max_blocks)

    def bam_bedgraph_stats(self):
        return self._accum_stats("bedgraph", BedgraphStats)

    def bam_bedgraph_next(self, max_rows=0, columns=None):
        """the next page of the result: ({"n_rows", "tid": int32, "start": int64 (0-based), "end": int64 (exclusive), "depth": int32 arrays; None
        for a column that `columns` (names of BEDGRAPH_COLUMNS; None: all) leaves out -- the batch has a null pointer there}, status)"""
        mask = sum(1 << BEDGRAPH_COLUMNS.index(k) for k in set(columns)) if columns is not None else 15
        b = BedBatch()
        self._chk(self.L.dhts_bam_bedgraph_next(self.h, max_rows, mask, C.byref(b)))
        return self._fixed_cols("bedgraph", b, mask, BEDGRAPH_COLUMNS, BEDGRAPH_DTYPES)

    # ---- interval_merge / interval_overlap ----
    def ivl_load(self, max_blocks=0):
        """after open, bgzf_index and dhts_bed_open: the BED read to its end, its valid rows sorted and indexed on the device"""
        self._chk(self.L.dhts_ivl_load(self.h, max_blocks))

    def ivl_stats(self):
        st = IvlStats()
        self._chk(self.L.dhts_ivl_stats_get(self.h, C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in IvlStats._fields_}

    def ivl_chrom_names(self):
        """the chrom names by name id (order of first appearance), as bytes"""
        out, n = [], C.c_uint64(0)
        while True:
            p = self.L.dhts_ivl_chrom_name(self.h, len(out), C.byref(n))
            if not p:
                return out
            out.append(C.string_at(p, n.value))

    def _ivl_fetch(self, b, mask, names):
        need = int(self.L.dhts_ivl_batch_host_bytes(C.byref(b)))
        arena = np.zeros(max(need, 8), np.uint8)
        host = (BcfCol * max(b.n_cols, 1))()
        self._chk(self.L.dhts_ivl_batch_fetch(self.h, C.byref(b), arena.ctypes.data, need, host))
        n, out = int(b.n_rows), {"n_rows": int(b.n_rows)}
        for i in range(b.n_cols):
            col, dt = names[host[i].col], INTERVAL_DTYPES[host[i].col]
            if not (mask >> host[i].col) & 1:
                out[col] = None
            elif n == 0:
                out[col] = np.zeros(0, dt)
            else:
                off = host[i].fixed - arena.ctypes.data
                out[col] = arena[off:off + n * np.dtype(dt).itemsize].view(dt).copy()
        return out, int(b.status)

    def ivl_merge_open(self, max_gap=0):
        """after ivl_load: the runs of interval_merge flagged and numbered"""
        if not 0 <= int(max_gap) <= INTERVAL_MAX_GAP:
            raise DhtsError("interval_merge: max_gap must be between 0 and 1099511627776")
        self._chk(self.L.dhts_ivl_merge_open(self.h, int(max_gap)))

    def ivl_merge_next(self, max_rows=0, columns=None):
        """the next rows of the result: ({"n_rows", "chrom": int32 name ids, "start", "end", "n_merged": int64 arrays; None for a column
        `columns` leaves out}, status)"""
        mask = sum(1 << INTERVAL_MERGE_COLUMNS.index(k) for k in (INTERVAL_MERGE_COLUMNS if columns is None else columns))
        b = BedBatch()
        self._chk(self.L.dhts_ivl_merge_next(self.h, max_rows, mask, C.byref(b)))
        return self._ivl_fetch(b, mask, INTERVAL_MERGE_COLUMNS)

    def ivl_overlap_open(self, right, mode="any"):
        """after ivl_load on both contexts (one device): every left row's pairs counted against right's index"""
        if mode not in INTERVAL_MODES:
            raise DhtsError("interval_overlap: mode must be 'any', 'contain' or 'within'")
        self._chk(self.L.dhts_ivl_overlap_open(self.h, right.h if right is not None else None, INTERVAL_MODES[mode]))

    def ivl_overlap_next(self, max_rows=0, columns=None):
        """the next page of whole left rows: ({"n_rows", "chrom": the left context's int32 name ids, the other columns int64 arrays; None for
        a column `columns` leaves out}, status)"""
        mask = sum(1 << INTERVAL_OVERLAP_COLUMNS.index(k) for k in (INTERVAL_OVERLAP_COLUMNS if columns is None else columns))
        b = BedBatch()
        self._chk(self.L.dhts_ivl_overlap_next(self.h, max_rows, mask, C.byref(b)))
        return self._ivl_fetch(b, mask, INTERVAL_OVERLAP_COLUMNS)

    def ivl_nearest_open(self, right, k=1, max_distance=None, ties="all"):
        """after ivl_load on both contexts (one device): right's end order built when it has none, every left row's nearest rows selected"""
        if ties not in INTERVAL_TIES:
            raise DhtsError("interval_nearest: ties must be 'all' or 'first'")
        if not 1 <= int(k) <= INTERVAL_MAX_K:
            raise DhtsError("interval_nearest: k must be between 1 and 1048576")
        if max_distance is not None and int(max_distance) < 0:
            raise DhtsError("interval_nearest: max_distance must not be negative")
        self._chk(self.L.dhts_ivl_nearest_open(self.h, right.h if right is not None else None, int(k), -1 if max_distance is None else int(max_distance), INTERVAL_TIES[ties]))

    def ivl_nearest_next(self, max_rows=0, columns=None):
        """the next page of whole left rows: ({"n_rows", "chrom": the left context's int32 name ids, the other columns int64 arrays; None for
        a column `columns` leaves out}, status)"""
        mask = sum(1 << INTERVAL_NEAREST_COLUMNS.index(k) for k in (INTERVAL_NEAREST_COLUMNS if columns is None else columns))
        b = BedBatch()
        self._chk(self.L.dhts_ivl_nearest_next(self.h, max_rows, mask, C.byref(b)))
        return self._ivl_fetch(b, mask, INTERVAL_NEAREST_COLUMNS)

    def ivl_nearest_stats(self):
        st = IvlNearestStats()
        self._chk(self.L.dhts_ivl_nearest_stats_get(self.h, C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in IvlNearestStats._fields_}

    def debug_ivl_sort(self, keys, rank):
        """tests, tools/bench_intervals.py: the sort alone.  keys: uint64, compared unsigned; rank: uint32 per row, the more significant part.
        (the row numbers in sorted order as uint32, the radix passes that were run)"""
        k, r = np.ascontiguousarray(keys, np.uint64), np.ascontiguousarray(rank, np.uint32)
        if len(k) != len(r):
            raise ValueError("keys and rank have to be of one length")
        out, passes = np.zeros(max(len(k), 1), np.uint32), C.c_int32(0)
        self._chk(self.L.dhts_debug_ivl_sort(self.h, k.ctypes.data, r.ctypes.data, len(k), out.ctypes.data, C.byref(passes)))
        return out[:len(k)], int(passes.value)

    def debug_ivl_ms(self, what):
        """tools/bench_intervals.py: device milliseconds of a part (0 load, 1 sort, 2 index, 3 merge, 4 overlap count, 5 overlap write, 6 nearest end
        order, 7 nearest selection, 8 nearest write, 16 + p sort pass p)"""
        return float(self.L.dhts_debug_ivl_ms(self.h, what))

    # ---- bam_bedgraph_export ----
    def bam_bedgraph_export(self, out_path, index="tbi", level=-1, min_shift=0, overwrite=False):
        """after bam_bedgraph_open and a scan: the result as a bgzipped bedGraph file at out_path, printed and compressed on the device, and its
        tabix index (index: 'tbi', 'csi' or 'none'; out_path + '.tbi' / '.csi').  -> {"n_rows", "bytes_text", "bytes_out", "bytes_index",
        "status", "output_path", "index_path" (None without an index)}.  The next bam_bedgraph_next returns page one."""
        if index not in BEDGRAPH_EXPORT_INDEX:
            raise DhtsError("bam_bedgraph_export: index must be one of: tbi, csi, none")
        p = BedgraphExportParams(_clip(level, 31), BEDGRAPH_EXPORT_INDEX[index], _clip(min_shift, 31), int(bool(overwrite)))
        st = BedgraphExportStats()
        self._chk(self.L.dhts_bedgraph_export(self.h, os.fsencode(out_path), C.byref(p), C.byref(st)))
        out = {k: int(getattr(st, k)) for k, _ in BedgraphExportStats._fields_ if k != "reserved"}
        out["output_path"] = os.fspath(out_path)
        out["index_path"] = None if index == "none" else os.fspath(out_path) + "." + index
        return out

    def debug_export_limits(self, page_rows=0, chunk_blocks=0):
        """tests: the rows of a page and the blocks of a compressor launch of bam_bedgraph_export on this context (0: the defaults)"""
        self._chk(self.L.dhts_debug_export_limits(self.h, page_rows, chunk_blocks))

    def debug_rows_text_form(self, form):
        """tests, tools/bench_bedgraph_export.py: the encoder's write pass, "staged" (the default) or "lane" (one lane per row, byte by byte)"""
        self._chk(self.L.dhts_debug_rows_text_form(self.h, {"staged": 0, "lane": 1}.get(form, -1)))

    def debug_rows_text(self, names, tid, start, end, depth):
        """tests: the row-text encoder alone (dhts_debug_rows_text): names: a list of bytes; tid, start, end, depth: arrays of one length ->
        (the text, {"staged", "fallback": the workgroups of the write pass that took either path})"""
        arena = np.frombuffer(b"".join(names), np.uint8) if names else np.zeros(0, np.uint8)
        offs = np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.uint32)
        t, s, e, d = (np.ascontiguousarray(tid, np.int32), np.ascontiguousarray(start, np.int64), np.ascontiguousarray(end, np.int64), np.ascontiguousarray(depth, np.int32))
        if not len(t) == len(s) == len(e) == len(d):
            raise ValueError("tid, start, end and depth have to be of one length")
        args = (arena.ctypes.data, offs.ctypes.data, len(names), t.ctypes.data, s.ctypes.data, e.ctypes.data, d.ctypes.data, len(t))
        need = self._chk(self.L.dhts_debug_rows_text(self.h, *args, None, 0))
        out = np.zeros(max(need, 1), np.uint8)
        got = self._chk(self.L.dhts_debug_rows_text(self.h, *args, out.ctypes.data, need))
        assert got == need
        w = (C.c_uint64 * 2)()
        self._chk(self.L.dhts_debug_rows_text_paths(self.h, w))
        return out[:need].tobytes(), {"staged": int(w[0]), "fallback": int(w[1])}

    # ---- bam_depth_hist (C ABI: dhts_bam_hist_*) ----
    def bam_depth_hist_open(self, bed_ctx=None, min_read_len=0, min_mapq=0, min_baseq=0, include_flags=0, require_flags=0, exclude_flags=0, include_deletions=0, depth_cap=1000,
                            per="row"):
        """after bam_open and the optional set_regions / load_index; bed_ctx: None, or a second Context on this device after bed_open.  The
        target rows, their groups, the depth table, the histogram table and the counters, zeroed.  per: 'row' or 'contig' (or the C struct's
        0 / 1).  The parameters are taken as given (the C ABI's rule): any other per travels as -1, which the C side refuses."""
        per = DEPTH_HIST_PER.get(per, -1) if isinstance(per, (str, bytes)) else _clip(per, 31)
        p = DepthHistParams(_clip(min_read_len, 63), _clip(min_mapq, 31), _clip(min_baseq, 31), _clip(require_flags, 31), _clip(exclude_flags, 31), _clip(include_flags, 31),
                            _clip(include_deletions, 31), _clip(depth_cap, 31), per)
        self._chk(self.L.dhts_bam_hist_open(self.h, C.byref(p), bed_ctx.h if bed_ctx is not None else None))

    def bam_depth_hist_accumulate(self, b):
        """b: the batch next_batch returned last on this context"""
        self._chk(self.L.dhts_bam_hist_accumulate(self.h, C.byref(b)))

    def bam_depth_hist_scan(self, max_blocks=0):
        """the scan to the end of the stream; the status it ended on (1, or the negative status of a stream that ended on an error)"""
        return self._accum_scan("hist", max_blocks, self.bam_depth_hist_stats)

    def bam_depth_hist_stats(self):
        return self._accum_stats("hist", DepthHistStats)

    def bam_depth_hist_next(self, max_rows=0, columns=None):
        """the next page of the result: ({"n_rows", "tid": int32, "start": int64 (0-based), "end": int64 (exclusive), "depth": int32, "n_positions",
        "n_at_least", "length": int64 arrays; None for a column that `columns` (names of DEPTH_HIST_COLUMNS; None: all) leaves out -- the batch
        has a null pointer there}, status)"""
        mask = sum(1 << DEPTH_HIST_COLUMNS.index(k) for k in set(columns)) if columns is not None else 127
        b = BedBatch()
        self._chk(self.L.dhts_bam_hist_next(self.h, max_rows, mask, C.byref(b)))
        return self._fixed_cols("hist", b, mask, DEPTH_HIST_COLUMNS, DEPTH_HIST_DTYPES)

    # ---- bam_bedcov ----
    def bam_bedcov_open(self, bed_ctx, min_mapq=0, require_flags=0, exclude_flags=0, include_flags=0, count_deletions=True, count_ref_skips=True):
        """after bam_open and the optional set_regions / load_index; bed_ctx: a second Context on this device after bed_open.  One pass over
        the BED, the breakpoints to the device, the counters zeroed.  The masks are taken as given (the C ABI's rule)."""
        p = BedcovParams(_clip(min_mapq, 31), _clip(require_flags, 31), _clip(exclude_flags, 31), _clip(include_flags, 31), int(count_deletions), int(count_ref_skips))
        self._chk(self.L.dhts_bam_bedcov_open(self.h, bed_ctx.h if bed_ctx is not None else None, C.byref(p)))

    def bam_bedcov_accumulate(self, b):
        """b: the batch next_batch returned last on this context"""
        self._chk(self.L.dhts_bam_bedcov_accumulate(self.h, C.byref(b)))

    def bam_bedcov_scan(self, max_blocks=0):
        """the scan to the end of the stream; the status it ended on (1, or the negative status of a stream that ended on an error)"""
        return self._accum_scan("bedcov", max_blocks)

    def bam_bedcov_stats(self):
        return self._accum_stats("bedcov", BedcovStats)

    def bam_bedcov_next(self, bed_ctx, max_blocks=0):
        """the result for the next batch of the BED: ({"n_rows", chrom / name / score / strand: lists of bytes or None, start / end: lists of
        int or None, bases_covered / read_count: int64 arrays}, status)"""
        b = BedBatch()
        self._chk(self.L.dhts_bam_bedcov_next(self.h, bed_ctx.h if bed_ctx is not None else None, max_blocks, C.byref(b)))
        arena, host, n = self._fetch_cols("bedcov", b)
        base = arena.ctypes.data
        out = {"n_rows": n}
        for i in range(b.n_cols):
            hc = host[i]
            name = BEDCOV_COLUMNS[hc.col]
            if n == 0:
                out[name] = np.zeros(0, np.int64) if hc.col >= 6 else []
                continue
            valid = arena[hc.valid - base: hc.valid - base + n]
            if hc.col in BEDCOV_INT_COLUMNS:
                vals = arena[hc.fixed - base: hc.fixed - base + 8 * n].view(np.int64)
                out[name] = vals.copy() if hc.col >= 6 else [int(v) if ok else None for v, ok in zip(vals, valid)]
            else:
                off = arena[hc.off - base: hc.off - base + 4 * (n + 1)].view(np.uint32)
                data = arena[hc.bytes - base: hc.bytes - base + int(hc.nbytes)].tobytes()
                out[name] = [data[int(off[r]):int(off[r + 1])] if valid[r] else None for r in range(n)]
        return out, int(b.status)

    # ---- seq_* / cigar_* / SAM flag functions on device columns (dhts_udf_*) ----
    def udf_upload(self, values, slot=0, kind="str", const=False, reserve=0):
        """host values -> a device argument column (UdfArg).  kind "str": bytes / str / None per row (reserve = extra reserved bytes behind
        every row, the layout of a batch column); "list": a list of 4-bit codes per row (None = NULL row, None inside = NULL child); "int":
        integers / None (BIGINT).  const: `values` is ONE value that stands for every row."""
        vals = [values] if const else list(values)
        n = len(vals)
        h = UdfArg()
        h.is_const = int(const)
        valid = np.array([v is not None for v in vals], np.uint8)
        keep = [valid]
        if not valid.all():
            h.valid = valid.ctypes.data
        if kind == "int":
            fixed = np.array([0 if v is None else v for v in vals], np.int64)
            keep.append(fixed)
            h.fixed, h.width = fixed.ctypes.data, -8
        else:
            rows, cvalid = [], []
            for v in vals:
                if kind == "list":
                    v = [] if v is None else list(v)
                    cvalid.append(bytes(x is not None for x in v))
                    rows.append(bytes(0 if x is None else x for x in v))
                else:
                    rows.append(b"" if v is None else (v.encode() if isinstance(v, str) else bytes(v)))
            ln = np.array([len(r) for r in rows], np.uint32)
            off = np.zeros(n + 1, np.uint32)
            off[1:] = np.cumsum(ln.astype(np.uint64) + np.uint64(reserve))
            pad = b"\xee" * reserve
            data = np.frombuffer(b"".join(r + pad for r in rows) + b"\0", np.uint8)
            keep += [ln, off, data]
            h.off, h.bytes, h.nbytes = off.ctypes.data, data.ctypes.data, len(data) - 1
            if reserve:
                h.len = ln.ctypes.data
            if kind == "list" and not all(all(c) for c in cvalid):
                cv = np.frombuffer(b"".join(c + b"\1" * reserve for c in cvalid) + b"\0", np.uint8)
                keep.append(cv)
                h.child_valid = cv.ctypes.data
        d = UdfArg()
        self._chk(self.L.dhts_udf_upload(self.h, slot, C.byref(h), 0 if const else n, C.byref(d)))
        d._n = n
        return d

    def _udf_arg(self, col, slot, width):
        if isinstance(col, UdfArg):
            return col
        a = UdfArg()
        if isinstance(col, StrCol):                       # a batch's own column: the four pointers as they are
            a.off, a.len, a.bytes, a.nbytes = col.off, col.len, col.bytes, col.nbytes
            return a
        if isinstance(col, int) and width:               # a device pointer to integers of |width| bytes (a batch's flag: width = 2)
            a.fixed, a.width = col, width
            return a
        return self.udf_upload(col, slot, kind="int" if isinstance(col, int) else "str", const=True)

    def udf(self, op, col, arg=None, n_rows=None, width=0, fetch=True):
        """op(col[, arg]) on the device.  col: a batch's seq / cigar / qname column (StrCol) or its flag pointer (width = 2), with n_rows =
        the batch's; or an uploaded UdfArg.  arg, for cigar_has_op and sam_flag_has: a UdfArg / batch column, or one str / int for every row.
        Returns python values (None = NULL), or with fetch = False the UdfResult whose device pointers live until the next udf call."""
        opid = UDF_OPS.index(op) if isinstance(op, str) else int(op)
        a0 = self._udf_arg(col, 0, width)
        n = getattr(a0, "_n", None) if n_rows is None else n_rows
        if n is None:
            raise ValueError("udf on a batch column needs n_rows")
        a1 = None if arg is None else self._udf_arg(arg, 1, 0)
        r = UdfResult()
        self._chk(self.L.dhts_udf_apply(self.h, opid, C.byref(a0), None if a1 is None else C.byref(a1), int(n), C.byref(r)))
        return self.udf_fetch(r) if fetch else r

    def udf_as_arg(self, r):
        """a LIST / VARCHAR result as the argument of the next call (seq_decode_4bit(seq_encode_4bit(x)))"""
        a = UdfArg()
        a.off, a.len, a.bytes, a.nbytes, a.valid = r.col.off, r.len, r.col.bytes, r.col.nbytes, r.col.valid
        a._n = int(r.n_rows)
        return a

    def udf_fetch(self, r, raw=False):
        """one result column as python values through dhts_udf_fetch: bytes, int, float (its bits are the device's), bool, a list of codes,
        12 bools for sam_flag_bits; None = NULL.  raw: the dict of numpy arrays instead (valid, off, len, bytes / fixed)."""
        n = int(r.n_rows)
        need = int(self.L.dhts_udf_result_host_bytes(C.byref(r)))
        arena = np.zeros(max(need, 8), np.uint8)
        h = UdfResult()
        self._chk(self.L.dhts_udf_fetch(self.h, C.byref(r), arena.ctypes.data, need, C.byref(h)))
        if n == 0:
            return {"n_rows": 0} if raw else []
        base = arena.ctypes.data
        valid = arena[h.col.valid - base: h.col.valid - base + n]
        if h.is_list or h.type == T_VARCHAR:
            off = arena[h.col.off - base: h.col.off - base + 4 * (n + 1)].view(np.uint32)
            data = arena[h.col.bytes - base: h.col.bytes - base + int(h.col.nbytes)]
            ln = (off[1:] - off[:-1]) if h.is_list else arena[h.len - base: h.len - base + 4 * n].view(np.uint32)
            if raw:
                return {"n_rows": n, "valid": valid, "off": off, "len": ln, "bytes": data}
            blob = data.tobytes()
            if h.is_list:
                return [list(blob[int(off[i]):int(off[i]) + int(ln[i])]) if valid[i] else None for i in range(n)]
            return [blob[int(off[i]):int(off[i]) + int(ln[i])] if valid[i] else None for i in range(n)]
        if h.type == 1:                                   # BOOLEAN
            nf = max(int(h.n_fields), 1)
            b = arena[h.col.fixed - base: h.col.fixed - base + n * nf].reshape(nf, n)
            if raw:
                return {"n_rows": n, "valid": valid, "fixed": b}
            if nf > 1:
                return [[bool(b[k, i]) for k in range(nf)] if valid[i] else None for i in range(n)]
            return [bool(b[0, i]) if valid[i] else None for i in range(n)]
        vals = arena[h.col.fixed - base: h.col.fixed - base + 8 * n].view({5: np.int64, 9: np.uint64, 11: np.float64}[int(h.type)])
        if raw:
            return {"n_rows": n, "valid": valid, "fixed": vals}
        return [v if valid[i] else None for i, v in enumerate(vals.tolist())]

    def udf_seq_kmers(self, col, k, canonical=False, text=True, hash=False, max_rows=0, n_rows=None):
        """every k-mer of the column, max_rows per call of dhts_udf_seq_kmers until the end: {"row", "pos"[, "kmer"][, "hash"]: lists}"""
        a = self._udf_arg(col, 0, 0)
        n = getattr(a, "_n", None) if n_rows is None else n_rows
        out = {"row": [], "pos": []}
        if text:
            out["kmer"] = []
        if hash:
            out["hash"] = []
        nxt = 0
        while True:
            b = UdfKmers()
            self._chk(self.L.dhts_udf_seq_kmers(self.h, C.byref(a), int(n), int(k), int(canonical), int(text), int(hash), int(max_rows), nxt, C.byref(b)))
            m = int(b.n_rows)
            if m:
                need = int(self.L.dhts_udf_kmers_host_bytes(C.byref(b)))
                arena = np.zeros(max(need, 8), np.uint8)
                h = UdfKmers()
                self._chk(self.L.dhts_udf_kmers_fetch(self.h, C.byref(b), arena.ctypes.data, need, C.byref(h)))
                base = arena.ctypes.data
                out["row"] += arena[h.row - base: h.row - base + 8 * m].view(np.int64).tolist()
                out["pos"] += arena[h.pos - base: h.pos - base + 8 * m].view(np.int64).tolist()
                if text:
                    v = arena[h.kmer.valid - base: h.kmer.valid - base + m]
                    off = arena[h.kmer.off - base: h.kmer.off - base + 4 * (m + 1)].view(np.uint32)
                    blob = arena[h.kmer.bytes - base: h.kmer.bytes - base + int(h.kmer.nbytes)].tobytes()
                    out["kmer"] += [blob[int(off[i]):int(off[i + 1])] if v[i] else None for i in range(m)]
                if hash:
                    hv = arena[h.hash_valid - base: h.hash_valid - base + m]
                    hs = arena[h.hash - base: h.hash - base + 8 * m].view(np.uint64).tolist()
                    out["hash"] += [x if hv[i] else None for i, x in enumerate(hs)]
            if b.status != 0 or (m == 0 and b.next == nxt):
                return out
            nxt = int(b.next)

    def next_batch(self, max_blocks=0, colmask=0x1FFF):
        b = BamBatch()
        self._chk(self.L.dhts_bam_next_batch(self.h, max_blocks, colmask, C.byref(b)))
        return b

    def d2h(self, ptr, count, dtype):
        out = np.empty(count, dtype)
        if count:
            self._chk(self.L.dhts_memcpy_d2h(self.h, out.ctypes.data, ptr, out.nbytes))
        return out

    def kernel_times(self):
        res = {}
        for i, name in enumerate(K_NAMES):
            n = C.c_int64(0)
            ms = self.L.dhts_kernel_time_ms(self.h, i, C.byref(n))
            res[name] = (ms, n.value)
        return res

    def set_timing(self, on):
        self.L.dhts_set_timing(self.h, int(on))

    def reset_times(self):
        self.L.dhts_kernel_time_reset(self.h)

    # ---- host mirror of one batch: device columns -> python values ----
    def batch_to_host(self, b, hdr):
        n = b.n_rows

        def strs(col, valid=None):
            off = self.d2h(col.off, n + 1, np.uint32)
            ln = self.d2h(col.len, n, np.uint32)
            data = self.d2h(col.bytes, int(col.nbytes), np.uint8).tobytes()
            return [None if (valid is not None and not valid[i]) else data[off[i]:off[i] + ln[i]] for i in range(n)]

        res = {"n_rows": n, "status": b.status}
        if n == 0:
            for k in BAM_COLUMNS:
                res[k] = [] if k in ("QNAME", "RNAME", "CIGAR", "RNEXT", "SEQ", "QUAL", "READ_GROUP_ID", "SAMPLE_ID") else np.zeros(0)
            res["tid"] = np.zeros(0, np.int32)
            res["mtid"] = np.zeros(0, np.int32)
            return res
        res["FLAG"] = self.d2h(b.flag, n, np.uint16)
        res["POS"] = self.d2h(b.pos, n, np.int64)
        res["MAPQ"] = self.d2h(b.mapq, n, np.int32)
        res["PNEXT"] = self.d2h(b.pnext, n, np.int64)
        res["TLEN"] = self.d2h(b.tlen, n, np.int64)
        tid = self.d2h(b.tid, n, np.int32)
        mtid = self.d2h(b.mtid, n, np.int32)
        res["tid"], res["mtid"] = tid, mtid
        names = hdr["ref_names"]
        res["RNAME"] = [names[t] if t >= 0 else b"*" for t in tid]       # sam_hdr_tid2name, '*' if tid < 0
        res["RNEXT"] = [names[t] if t >= 0 else b"*" for t in mtid]      # the NAME, never '='
        words = self.d2h(b.rg_valid, (n + 63) // 64, np.uint64)
        valid = [(int(words[i >> 6]) >> (i & 63)) & 1 for i in range(n)]
        res["QNAME"] = strs(b.qname)
        res["CIGAR"] = strs(b.cigar)
        if b.seq_packed:                               # dhts_bam_set_seq_packed: 4-bit codes, len = bases (0: "*")
            off = self.d2h(b.seq.off, n + 1, np.uint32); ln = self.d2h(b.seq.len, n, np.uint32)
            data = self.d2h(b.seq.bytes, int(b.seq.nbytes), np.uint8)
            lut = np.frombuffer(b"=ACMGRSVTWYHKDBN", np.uint8)
            both = np.empty(2 * len(data), np.uint8); both[0::2] = lut[data >> 4]; both[1::2] = lut[data & 15]
            txt = both.tobytes()
            res["SEQ"] = [b"*" if ln[i] == 0 else txt[2 * int(off[i]):2 * int(off[i]) + int(ln[i])] for i in range(n)]
        else:
            res["SEQ"] = strs(b.seq)
        res["QUAL"] = strs(b.qual)
        res["READ_GROUP_ID"] = strs(b.rg, valid)
        rgi = self.d2h(b.rg_idx, n, np.int32)
        sm = hdr["rg_sm"]
        res["SAMPLE_ID"] = [sm[k] if (valid[i] and k >= 0 and sm[k] is not None) else None for i, k in enumerate(rgi)]
        return res


def _gather_strings(ids, names):
    """ids (int array, -1 allowed only when names has a trailing default) -> (offsets u64[n+1], bytes u8) by dictionary lookup."""
    lens = np.array([len(x) for x in names], np.int64)
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1]
    flat = np.frombuffer(b"".join(names), np.uint8)
    l = lens[ids]
    off = np.concatenate([[0], np.cumsum(l)]).astype(np.uint64)
    total = int(off[-1])
    if total == 0:
        return off, np.zeros(0, np.uint8)
    idx = np.repeat(starts[ids] - off[:-1].astype(np.int64), l) + np.arange(total)
    return off, flat[idx]


class BcfScan:
    """read_bcf over one context: schema + batches as canonical column tables (same layout tests/orc.py decodes)."""

    def __init__(self, ctx, tidy=False):
        self.ctx = ctx
        ctx._chk(ctx.L.dhts_bcf_open(ctx.h, int(tidy)))
        inf = BcfInfo()
        ctx._chk(ctx.L.dhts_bcf_info_get(ctx.h, C.byref(inf)))
        self.schema = [{"name": inf.cols[i].name.decode(), "type": inf.cols[i].type, "is_list": inf.cols[i].is_list, "encoding": inf.cols[i].encoding}
                       for i in range(inf.n_cols)]
        self._names(inf)
        self.samples = [inf.sample_name[i] for i in range(inf.n_samples)]
        self.tidy = bool(inf.tidy)
        self.first_rec_uoff = inf.first_rec_uoff
        self.projection = list(range(len(self.schema)))

    def _names(self, inf=None):
        """contig / dictionary names; a scan of VCF text adds the names records use without a header definition (ask again after a batch)"""
        if inf is None:
            inf = BcfInfo()
            self.ctx._chk(self.ctx.L.dhts_bcf_info_get(self.ctx.h, C.byref(inf)))
        self.contigs = [inf.contig_name[i] if inf.contig_name[i] is not None else b"" for i in range(inf.n_contigs)]
        self.dict_names = [inf.dict_name[i] if inf.dict_name[i] is not None else b"." for i in range(inf.n_dict)] + [b"PASS"]   # id -1 -> literal PASS

    def set_projection(self, cols):
        ids = [c if isinstance(c, int) else [s["name"] for s in self.schema].index(c) for c in cols]
        arr = np.array(ids, np.int32)
        self.ctx._chk(self.ctx.L.dhts_bcf_set_projection(self.ctx.h, arr.ctypes.data, len(ids)))
        self.projection = ids

    def set_block_range(self, b0, b1, speculative):
        self.ctx._chk(self.ctx.L.dhts_bcf_set_block_range(self.ctx.h, b0, b1, int(speculative)))

    def rewind(self):
        self.ctx._chk(self.ctx.L.dhts_bcf_rewind(self.ctx.h))

    def set_region(self, region):
        """one region (the reference chains them); False when the region yields no iterator (unknown contig)"""
        return self.ctx._chk(self.ctx.L.dhts_bcf_set_region(self.ctx.h, region.encode() if region else None)) == 0

    def load_index(self, index_bytes):
        """CSI / TBI bytes: narrows the scan window of the region set last (call after set_region)"""
        buf = np.frombuffer(index_bytes, dtype=np.uint8)
        # VCF text: the region names a sequence of the tabix index, so it is resolved here; False = the index does not know it (region skipped)
        return self.ctx._chk(self.ctx.L.dhts_bcf_load_index(self.ctx.h, buf.ctypes.data, buf.nbytes)) == 0

    def next_batch(self, max_blocks=0):
        b = BcfBatch()
        self.ctx._chk(self.ctx.L.dhts_bcf_next_batch(self.ctx.h, max_blocks, C.byref(b)))
        return b

    def batch_table(self, b):
        """device columns of one batch -> canonical table (dictionary-coded columns expanded to strings)"""
        n = int(b.n_rows)
        d2h = self.ctx.d2h
        cols = []
        self._names()
        for i in range(b.n_cols):
            dc = b.cols[i]
            sc = self.schema[dc.col]
            c = {"name": sc["name"], "type": _CANON_TYPE[sc["type"]], "is_list": sc["is_list"]}
            c["valid"] = d2h(dc.valid, n, np.uint8) if n else np.zeros(0, np.uint8)
            enc = sc["encoding"]
            names = {ENC_CONTIG: self.contigs, ENC_DICT: self.dict_names, ENC_SAMPLE: self.samples}.get(enc)
            if not sc["is_list"]:
                if enc != ENC_PLAIN:
                    ids = d2h(dc.fixed, n, np.int32).astype(np.int64)
                    c["soff"], c["sbytes"] = _gather_strings(ids, names)
                elif sc["type"] == 17:
                    c["soff"] = d2h(dc.off, n + 1, np.uint32).astype(np.uint64) if n else np.zeros(1, np.uint64)
                    c["sbytes"] = d2h(dc.bytes, int(dc.nbytes), np.uint8)
                else:
                    w = {1: np.uint8, 4: np.uint32, 10: np.uint32, 5: np.uint64, 11: np.uint64}[sc["type"]]
                    c["fixed"] = d2h(dc.fixed, n, w).astype(np.uint64)
            else:
                off = d2h(dc.off, n + 1, np.uint32).astype(np.uint64) if n else np.zeros(1, np.uint64)
                c["loff"], c["llen"] = off[:-1].copy(), off[1:] - off[:-1]
                cn = int(dc.child_n)
                c["child_n"] = cn
                if dc.child_valid:
                    c["cvalid"] = d2h(dc.child_valid, cn, np.uint8)
                if enc == ENC_FLOAT_TEXT:                 # LIST(FLOAT) delivered as text: (float)strtod per element, NaN unless the whole text converts
                    co = d2h(dc.child_off, cn + 1, np.uint32) if n else np.zeros(1, np.uint32)
                    raw = d2h(dc.bytes, int(dc.nbytes), np.uint8).tobytes()
                    cv = c.get("cvalid", np.ones(cn, np.uint8))
                    vals = np.array([c_strtof(raw[int(co[k]):int(co[k + 1])]) if cv[k] else 0.0 for k in range(cn)], np.float32)
                    c["cfixed"] = vals.view(np.uint32).astype(np.uint64)
                elif enc != ENC_PLAIN:
                    ids = d2h(dc.child_fixed, cn, np.int32).astype(np.int64)
                    c["csoff"], c["csbytes"] = _gather_strings(ids, names)
                elif sc["type"] == 17:
                    c["csoff"] = d2h(dc.child_off, cn + 1, np.uint32).astype(np.uint64) if n else np.zeros(1, np.uint64)
                    c["csbytes"] = d2h(dc.bytes, int(dc.nbytes), np.uint8)
                else:
                    c["cfixed"] = d2h(dc.child_fixed, cn, np.uint32).astype(np.uint64)
            cols.append(c)
        return {"n_rows": n, "status": int(b.status), "cols": cols}


class BedIteratorError(DhtsError):
    """the index does not know the region's sequence (the reference: "read_bed: failed to create region iterator")"""


class BedScan:
    """read_bed over one context (open + bgzf_index done): projection, region, batches as python columns."""

    def __init__(self, ctx):
        self.ctx = ctx
        ctx._chk(ctx.L.dhts_bed_open(ctx.h))
        self.projection = list(range(len(BED_COLUMNS)))
        self.error = None

    def set_projection(self, cols):
        ids = [c if isinstance(c, int) else BED_COLUMNS.index(c) for c in cols]
        arr = np.array(ids, np.int32)
        self.ctx._chk(self.ctx.L.dhts_bed_set_projection(self.ctx.h, arr.ctypes.data, len(ids)))
        self.projection = ids

    def set_region(self, region):
        self.ctx._chk(self.ctx.L.dhts_bed_set_region(self.ctx.h, region.encode() if region else None))

    def load_index(self, index_bytes):
        """False when the index does not know the region's sequence"""
        buf = np.frombuffer(index_bytes, dtype=np.uint8)
        return self.ctx._chk(self.ctx.L.dhts_bed_load_index(self.ctx.h, buf.ctypes.data, buf.nbytes)) == 0

    def next_batch(self, max_blocks=0):
        b = BedBatch()
        self.ctx._chk(self.ctx.L.dhts_bed_next_batch(self.ctx.h, max_blocks, C.byref(b)))
        if b.status < 0:
            self.error = self.ctx.L.dhts_error(self.ctx.h).decode()
        return b

    def batch_columns(self, b):
        """the projected columns of one batch through dhts_bed_batch_fetch: {name: int64 array + validity, or list of bytes / None}"""
        n = int(b.n_rows)
        need = int(self.ctx.L.dhts_bed_batch_host_bytes(C.byref(b)))
        arena = np.zeros(max(need, 8), np.uint8)
        host = (BcfCol * max(b.n_cols, 1))()
        self.ctx._chk(self.ctx.L.dhts_bed_batch_fetch(self.ctx.h, C.byref(b), arena.ctypes.data, need, host))
        base = arena.ctypes.data
        out = {}
        for i in range(b.n_cols):
            hc = host[i]
            name = BED_COLUMNS[hc.col]
            if n == 0:
                out[name] = []
                continue
            valid = arena[hc.valid - base: hc.valid - base + n]
            if hc.col in BED_INT_COLUMNS:
                vals = arena[hc.fixed - base: hc.fixed - base + 8 * n].view(np.int64)
                out[name] = [int(vals[r]) if valid[r] else None for r in range(n)]
            else:
                off = arena[hc.off - base: hc.off - base + 4 * (n + 1)].view(np.uint32)
                data = arena[hc.bytes - base: hc.bytes - base + int(hc.nbytes)].tobytes()
                out[name] = [data[int(off[r]):int(off[r + 1])] if valid[r] else None for r in range(n)]
        return out


class NucRegionError(DhtsError):
    """the reference's "fasta_nuc: invalid FASTA region" """


def fasta_nuc(fasta, bed=None, bin_width=None, region=None, fai=None, bed_index=None, include_seq=False, columns=None, device=0, max_rows=0, stats=None):
    """fasta_nuc(fasta, bed_path := / bin_width :=, region :=, index_path :=, bed_index_path :=, include_seq :=): {"n_rows", column: python
    list with None for NULL} for the projected columns (default all of NUC_COLUMNS; seq only with include_seq).  fasta: a path
    (uncompressed or BGZF) or, with fai given as bytes, the file's bytes; fai: the .fai's path (default fasta + ".fai"; it is never built here) or its bytes.  bed: a path (uncompressed,
    BGZF or plain gzip) or the BED's bytes; bed_index: the tabix index of a BGZF BED, used with a region (default bed + ".tbi" / ".csi"; without
    one the whole BED is read and filtered).  max_rows: rows per batch in bins mode, BED blocks per batch in BED mode.  stats (a dict)
    receives resident_bytes (of the FASTA) and n_batches."""
    fasta_is_bytes = isinstance(fasta, (bytes, bytearray, memoryview, np.ndarray))
    if not fasta_is_bytes and not fasta:
        raise DhtsError("fasta_nuc requires a FASTA path")
    if (bed is None) == (bin_width is None):
        raise DhtsError("fasta_nuc requires exactly one of bed_path or bin_width")
    if bin_width is not None and bin_width <= 0:
        raise DhtsError("fasta_nuc bin_width must be > 0")
    if isinstance(fai, (bytes, bytearray)):
        fai_bytes = bytes(fai)
    else:
        fp = fai or (None if fasta_is_bytes else os.fspath(fasta) + ".fai")
        if fp is None or not os.path.exists(fp):
            raise DhtsError("fasta_nuc: failed to open FASTA index")
        fai_bytes = open(fp, "rb").read()
    ctx, bctx = Context(device), None
    try:
        ctx.fasta_load_index(fai_bytes)
        if region and not fasta_is_bytes and not _is_bgzf(fasta):
            # only what the region reads is staged: its own window for bins, the whole sequence for BED rows (they may reach past the region)
            ctx._chk(ctx.L.dhts_nuc_open_region(ctx.h, os.fsencode(fasta), region.encode() if isinstance(region, str) else region, int(bed is not None)))
        else:
            ctx.open(fasta)
            ctx.L.dhts_bgzf_index(ctx.h)
        ctx.nuc_open(include_seq)
        if region and not ctx.nuc_set_region(region):
            raise NucRegionError("fasta_nuc: invalid FASTA region")
        if columns is not None:
            ctx.nuc_set_projection(columns)
        names = [NUC_COLUMNS[i] for i in ctx.nuc_projection]
        out = {"n_rows": 0}
        out.update({k: [] for k in names})
        if bed is not None:
            is_path = not isinstance(bed, (bytes, bytearray, memoryview, np.ndarray))
            if is_path and not os.path.exists(bed):
                raise DhtsError("fasta_nuc: failed to open BED file")
            index = None
            if region and is_path and _is_bgzf(bed):                          # HTS_IDX_SILENT_FAIL: no index, no iterator
                for p in ([bed_index] if bed_index else [os.fspath(bed) + ".tbi", os.fspath(bed) + ".csi"]):
                    if os.path.exists(p):
                        index = open(p, "rb").read()
                        break
            bctx = Context(device)
            sparse = None
            if index is not None:
                ibuf = np.frombuffer(index, dtype=np.uint8)
                beg, end, cnt = np.zeros(4096, np.uint64), np.zeros(4096, np.uint64), C.c_int64(0)
                rb = region.encode() if isinstance(region, str) else region
                rc = bctx._chk(bctx.L.dhts_bed_region_segments(bctx.h, rb, ibuf.ctypes.data, ibuf.nbytes, beg.ctypes.data, end.ctypes.data, 4096, C.byref(cnt)))
                if rc == 1:
                    raise BedIteratorError("fasta_nuc: failed to create BED region iterator")
                if cnt.value >= 0:
                    sparse = (beg[:cnt.value].copy(), end[:cnt.value].copy())
            if sparse is not None:
                bctx.open_segments(bed, 0, *sparse)
            else:
                bctx.open(bed)
            bctx.L.dhts_bgzf_index(bctx.h)
            sc = BedScan(bctx)
            if index is not None:
                sc.set_region(region if isinstance(region, str) else region.decode())
                if not sc.load_index(index):
                    raise BedIteratorError("fasta_nuc: failed to create BED region iterator")
        nb = 0
        while True:
            b = ctx.nuc_next_bed(bctx, max_rows) if bed is not None else ctx.nuc_next_bins(bin_width, max_rows)
            nb += 1
            if b.n_rows:
                out["n_rows"] += int(b.n_rows)
                for k, v in ctx.nuc_batch_columns(b).items():
                    if k != "n_rows":
                        out[k].extend(v)
            if b.status != 0:
                break
        if stats is not None:
            stats["resident_bytes"] = ctx.resident_bytes()
            stats["n_batches"] = nb
        return out
    finally:
        if bctx is not None:
            bctx.close()
        ctx.close()


def _is_bgzf(path):
    with open(path, "rb") as f:
        h = f.read(18)
    return len(h) == 18 and h[:4] == b"\x1f\x8b\x08\x04" and h[10:16] == b"\x06\x00BC\x02\x00"


def read_bed(src, region=None, index_path=None, columns=None, device=0, max_blocks=0, stats=None):
    """read_bed(path, region := ..., index_path := ...): {"n_rows", "status", "error", column: python list with None for NULL} for the
    projected columns (default all 13, BED_COLUMNS).  src: a path (uncompressed, BGZF or plain gzip) or the file's bytes (no region).  A
    region needs the tabix index (index_path, else src + ".tbi" / ".csi") and stages only the index windows; stats (a dict) receives
    resident_bytes and n_batches.  A line with fewer than 3 fields ends the scan: the rows in front of it, status < 0 and the message in "error"."""
    index = None
    if region is not None:
        if isinstance(src, (bytes, bytearray, memoryview, np.ndarray)):
            raise DhtsError("read_bed: region queries require a tabix index")
        cand = [index_path] if index_path else [os.fspath(src) + ".tbi", os.fspath(src) + ".csi"]
        for p in cand:
            if os.path.exists(p):
                index = open(p, "rb").read()
                break
        if index is None:
            raise DhtsError("read_bed: region queries require a tabix index")
    ctx = Context(device)
    try:
        sparse = None
        if index is not None and _is_bgzf(src):
            ibuf = np.frombuffer(index, dtype=np.uint8)
            beg, end, cnt = np.zeros(4096, np.uint64), np.zeros(4096, np.uint64), C.c_int64(0)
            rc = ctx._chk(ctx.L.dhts_bed_region_segments(ctx.h, region.encode(), ibuf.ctypes.data, ibuf.nbytes, beg.ctypes.data, end.ctypes.data, 4096, C.byref(cnt)))
            if rc == 1:
                raise BedIteratorError("read_bed: failed to create region iterator")
            if cnt.value >= 0:
                sparse = (beg[:cnt.value].copy(), end[:cnt.value].copy())
        if sparse is not None:
            ctx.open_segments(src, 0, *sparse)
        else:
            ctx.open(src)
        ctx.L.dhts_bgzf_index(ctx.h)                      # (fails on text that is not BGZF: dhts_bed_open reads that as text)
        sc = BedScan(ctx)
        if columns is not None:
            sc.set_projection(columns)
        if region is not None:
            sc.set_region(region)
            if not sc.load_index(index):
                raise BedIteratorError("read_bed: failed to create region iterator")
        names = [BED_COLUMNS[i] for i in sc.projection]
        out = {"n_rows": 0, "status": 0, "error": None}
        out.update({k: [] for k in names})
        nb = 0
        while True:
            b = sc.next_batch(max_blocks)
            nb += 1
            if b.n_rows:
                out["n_rows"] += int(b.n_rows)
                for k, v in sc.batch_columns(b).items():
                    out[k].extend(v)
            out["status"] = int(b.status)
            if b.status != 0:
                break
        out["error"] = sc.error
        if stats is not None:
            stats["resident_bytes"] = ctx.resident_bytes()
            stats["n_batches"] = nb
        return out
    finally:
        ctx.close()


def tabix_parse_regions(region):
    """parse_regions (src/tabix_reader.c:301-344): comma-separated, trimmed of blanks and tabs, empty tokens dropped"""
    if not region:
        return []
    return [t.strip(" \t") for t in region.split(",") if t.strip(" \t")]


def tabix_resolve_schema(sniffed, header=False, header_names=None, column_types=None, auto_detect=False, rows=None):
    """dhts_tabix_resolve_schema (no device): {"n_cols", "names", "types", "skip_header_line", "need_rows"}.  sniffed: a TabixSniffed, or
    (n_fields, candidate bytes or None, candidate_from_skip).  rows: for auto_detect, lists of n_cols cells (bytes or None)."""
    L = lib()
    if not isinstance(sniffed, TabixSniffed):
        n_fields, cand, from_skip = sniffed
        keep = C.create_string_buffer(cand, len(cand)) if cand is not None else None
        sniffed = TabixSniffed(n_fields, 1 if cand is not None else 0, 1 if from_skip else 0, 0, C.addressof(keep) if keep is not None else None, len(cand) if cand is not None else 0)
        sniffed._keep = keep

    def strs(xs):
        if not xs:
            return None, 0
        return (C.c_char_p * len(xs))(*[x.encode() if isinstance(x, str) else x for x in xs]), len(xs)
    hn, n_hn = strs(header_names)
    ct, n_ct = strs(column_types)
    out, err = TabixSchema(), C.create_string_buffer(256)
    cells = lens = None
    n_rows = 0
    if rows is not None:
        flat = [c for r in rows for c in r]
        bufs = [C.create_string_buffer(c, len(c)) if c is not None else None for c in flat]
        cells = (C.c_char_p * max(len(flat), 1))(*[C.cast(b, C.c_char_p) if b is not None else None for b in bufs])
        lens = np.array([len(c) if c is not None else 0 for c in flat] + [0], np.uint32)
        n_rows = len(rows)
    rc = L.dhts_tabix_resolve_schema(C.byref(sniffed), 1 if header else 0, hn, n_hn, ct, n_ct, 1 if auto_detect else 0,
                                     cells, lens.ctypes.data if lens is not None else None, n_rows, C.byref(out), err, 256)
    if rc < 0:
        raise DhtsError(err.value.decode() or "dhts_tabix_resolve_schema failed")
    n = out.n_cols
    return {"n_cols": n, "names": [out.names[i].decode() for i in range(n)], "types": [int(out.types[i]) for i in range(n)],
            "skip_header_line": bool(out.skip_header_line), "need_rows": rc == 1}


class TabixScan:
    """read_tabix / read_gtf / read_gff over one context (open + bgzf_index done): bind, projection, region, batches as python columns."""

    def __init__(self, ctx, mode=TABIX_GENERIC):
        self.ctx, self.mode = ctx, mode
        ctx._chk(ctx.L.dhts_tabix_open(ctx.h, mode))
        gxf = mode != TABIX_GENERIC
        self.names = GXF_COLUMNS[:9] if gxf else ["column0"]
        self.types = list(GXF_TYPES) if gxf else [T_VARCHAR]
        self.projection = list(range(len(self.names)))
        self.n_double_fast = self.n_double_patched = 0

    def set_conf(self, meta_char, line_skip):
        self.ctx._chk(self.ctx.L.dhts_tabix_set_conf(self.ctx.h, meta_char, line_skip))

    def index_conf(self, index_bytes):
        buf = np.frombuffer(index_bytes, dtype=np.uint8)
        m, s = C.c_int32(0), C.c_int32(0)
        self.ctx._chk(self.ctx.L.dhts_tabix_index_conf(self.ctx.h, buf.ctypes.data, buf.nbytes, C.byref(m), C.byref(s)))
        return m.value, s.value

    def sniff(self, header=False, have_header_names=False):
        sn = TabixSniffed()
        self.ctx._chk(self.ctx.L.dhts_tabix_sniff(self.ctx.h, 1 if header else 0, 1 if have_header_names else 0, C.byref(sn)))
        cand = C.string_at(sn.candidate, sn.candidate_len) if sn.have_candidate else None
        return sn.n_fields, cand, bool(sn.candidate_from_skip)

    def set_schema(self, types, skip_header_line=False, names=None):
        arr = np.array(types, np.int32)
        self.ctx._chk(self.ctx.L.dhts_tabix_set_schema(self.ctx.h, len(types), arr.ctypes.data, 1 if skip_header_line else 0))
        self.types = list(types)
        self.names = list(names) if names else ["column%d" % i for i in range(len(types))]
        self.projection = list(range(len(types)))

    def bind(self, header=False, header_names=None, column_types=None, auto_detect=False, max_blocks=0):
        """generic bind (src/tabix_reader.c:658-771): the peek, the schema rules and, for auto_detect, the first 100 rows; returns the schema"""
        sn = self.sniff(header, bool(header_names))
        sch = tabix_resolve_schema(sn, header, header_names, column_types, auto_detect)
        if sch["need_rows"]:
            self.set_schema(sch["types"], sch["skip_header_line"])
            rows = []
            while len(rows) < 100:
                b = self.next_batch(max_blocks or 64)
                cols = self.batch_columns(b) if b.n_rows else {}
                for r in range(int(b.n_rows)):
                    rows.append([cols["column%d" % i][r] for i in range(sch["n_cols"])])
                if b.status != 0:
                    break
            self.set_region(None)                                            # rewinds
            sch = tabix_resolve_schema(sn, header, header_names, column_types, auto_detect, rows[:100])
        self.set_schema(sch["types"], sch["skip_header_line"], sch["names"])
        return sch

    def set_projection(self, cols):
        allnames = GXF_COLUMNS if self.mode != TABIX_GENERIC else self.names
        ids = [c if isinstance(c, int) else allnames.index(c) for c in cols]
        arr = np.array(ids + [0], np.int32)
        self.ctx._chk(self.ctx.L.dhts_tabix_set_projection(self.ctx.h, arr.ctypes.data, len(ids)))
        self.projection = ids

    def set_region(self, region):
        self.ctx._chk(self.ctx.L.dhts_tabix_set_region(self.ctx.h, region.encode() if region else None))

    def load_index(self, index_bytes):
        """False when the index does not know the region's sequence"""
        buf = np.frombuffer(index_bytes, dtype=np.uint8)
        return self.ctx._chk(self.ctx.L.dhts_tabix_load_index(self.ctx.h, buf.ctypes.data, buf.nbytes)) == 0

    def next_batch(self, max_blocks=0):
        b = TabixBatch()
        self.ctx._chk(self.ctx.L.dhts_tabix_next_batch(self.ctx.h, max_blocks, C.byref(b)))
        self.n_double_fast += int(b.n_double_fast)
        self.n_double_patched += int(b.n_double_patched)
        return b

    def col_name(self, cid):
        return GXF_COLUMNS[cid] if self.mode != TABIX_GENERIC else self.names[cid]

    def batch_columns(self, b):
        """the projected columns of one batch through dhts_tabix_batch_fetch: {name: list of int / float (float64) / bytes / None; the map
        column: list of [(key, value), ...] / None}"""
        n = int(b.n_rows)
        need = int(self.ctx.L.dhts_tabix_batch_host_bytes(C.byref(b)))
        arena = np.zeros(max(need, 8), np.uint8)
        host = (BcfCol * max(b.n_cols, 1))()
        hmap = TabixMap()
        self.ctx._chk(self.ctx.L.dhts_tabix_batch_fetch(self.ctx.h, C.byref(b), arena.ctypes.data, need, host, C.byref(hmap)))
        base = arena.ctypes.data

        def view(ptr, nbytes, dt=np.uint8):
            return arena[ptr - base: ptr - base + nbytes].view(dt) if nbytes else np.zeros(0, dt)
        out = {}
        for i in range(b.n_cols):
            hc, ty = host[i], int(b.col_types[i])
            name = self.col_name(hc.col)
            if n == 0:
                out[name] = []
            elif ty == 0:
                po, valid = view(hmap.pair_off, 4 * (n + 1), np.uint32), view(hmap.valid, n)
                npairs = int(hmap.n_pairs)
                ko, vo = view(hmap.key_off, 4 * (npairs + 1), np.uint32), view(hmap.val_off, 4 * (npairs + 1), np.uint32)
                kb, vb = view(hmap.key_bytes, int(hmap.key_nbytes)).tobytes(), view(hmap.val_bytes, int(hmap.val_nbytes)).tobytes()
                out[name] = [[(kb[int(ko[p]):int(ko[p + 1])], vb[int(vo[p]):int(vo[p + 1])]) for p in range(int(po[r]), int(po[r + 1]))] if valid[r] else None for r in range(n)]
            else:
                valid = view(hc.valid, n)
                if ty == T_VARCHAR:
                    off = view(hc.off, 4 * (n + 1), np.uint32)
                    data = view(hc.bytes, int(hc.nbytes)).tobytes()
                    out[name] = [data[int(off[r]):int(off[r + 1])] if valid[r] else None for r in range(n)]
                elif ty == T_DOUBLE:
                    vals = view(hc.fixed, 8 * n, np.float64)
                    out[name] = [vals[r] if valid[r] else None for r in range(n)]
                else:
                    vals = view(hc.fixed, 8 * n, np.int64)
                    out[name] = [int(vals[r]) if valid[r] else None for r in range(n)]
        return out


def _read_tabix_mode(mode, who, src, region, index_path, header, header_names, column_types, auto_detect, columns, attributes_map, device, max_blocks, stats):
    is_bytes = isinstance(src, (bytes, bytearray, memoryview, np.ndarray))
    index = None
    if not is_bytes:
        for p in ([index_path] if index_path else [os.fspath(src) + ".tbi", os.fspath(src) + ".csi"]):   # tbx_index_load2
            if os.path.exists(p):
                index = open(p, "rb").read()
                break
    regions = tabix_parse_regions(region)
    if regions and index is None:
        raise DhtsError("Region query requested but no tabix index found for: %s" % ("<bytes>" if is_bytes else os.fspath(src)))
    ctx = Context(device)
    try:
        sparse = None
        if len(regions) == 1 and not is_bytes and _is_bgzf(src):                               # one region: only its index windows are staged
            ibuf = np.frombuffer(index, dtype=np.uint8)
            beg, end, cnt = np.zeros(4096, np.uint64), np.zeros(4096, np.uint64), C.c_int64(0)
            rc = ctx._chk(ctx.L.dhts_tabix_region_segments(ctx.h, regions[0].encode(), ibuf.ctypes.data, ibuf.nbytes, beg.ctypes.data, end.ctypes.data, 4096, C.byref(cnt)))
            if rc == 0 and cnt.value >= 0 and mode != TABIX_GENERIC:          # (generic bind peeks at the head of the file)
                sparse = (beg[:cnt.value].copy(), end[:cnt.value].copy())
        if sparse is not None:
            ctx.open_segments(src, 0, *sparse)
        else:
            ctx.open(src)
        ctx.L.dhts_bgzf_index(ctx.h)
        sc = TabixScan(ctx, mode)
        if mode == TABIX_GENERIC:
            if index is not None:
                meta, skip = sc.index_conf(index)
                sc.set_conf(meta if meta else ord("#"), skip)
            schema = sc.bind(header, header_names, column_types, auto_detect, max_blocks)
            names, types = schema["names"], schema["types"]
        else:
            names, types = GXF_COLUMNS[:9] + (["attributes_map"] if attributes_map else []), GXF_TYPES + ([0] if attributes_map else [])
            if attributes_map:
                sc.set_projection(list(range(10)))
        if columns is not None:
            sc.set_projection(columns)
        pnames = [sc.col_name(i) for i in sc.projection]
        out = {"n_rows": 0, "status": 1, "names": names, "types": types}
        out.update({k: [] for k in pnames})
        nb = 0
        for rg in (regions if regions else [None]):
            if rg is not None:
                sc.set_region(rg)
                if not sc.load_index(index):
                    continue                                                 # tabix_advance_region_iterator passes over a region without an iterator
            while True:
                b = sc.next_batch(max_blocks)
                nb += 1
                if b.n_rows:
                    out["n_rows"] += int(b.n_rows)
                    for k, v in sc.batch_columns(b).items():
                        out[k].extend(v)
                out["status"] = int(b.status)
                if b.status != 0:
                    break
        if stats is not None:
            stats.update(resident_bytes=ctx.resident_bytes(), n_batches=nb, n_double_fast=sc.n_double_fast, n_double_patched=sc.n_double_patched)
        return out
    finally:
        ctx.close()


def read_tabix(src, region=None, index_path=None, header=False, header_names=None, column_types=None, auto_detect=False, columns=None, device=0, max_blocks=0, stats=None):
    """read_tabix(path, region := 'a,b', index_path, header, header_names, column_types, auto_detect): {"n_rows", "status", "names", "types"
    (the resolved schema, DUCKDB_TYPE_* codes), column: python list with None for NULL} for the projected columns (default all).  src: a path
    (uncompressed, BGZF or plain gzip) or the file's bytes.  The regions run one after another, each through its own index windows; one the
    index cannot resolve is passed over.  meta character and line_skip come from the index (src + ".tbi" / ".csi", or index_path)."""
    return _read_tabix_mode(TABIX_GENERIC, "read_tabix", src, region, index_path, header, header_names, column_types, auto_detect, columns, False, device, max_blocks, stats)


def read_gff(src, region=None, index_path=None, columns=None, attributes_map=False, device=0, max_blocks=0, stats=None):
    """read_gff: the nine GFF3 columns (GXF_COLUMNS) and, with attributes_map, the key=value pairs of column 9 as [(key, value), ...]"""
    return _read_tabix_mode(TABIX_GFF, "read_gff", src, region, index_path, False, None, None, False, columns, attributes_map, device, max_blocks, stats)


def read_gtf(src, region=None, index_path=None, columns=None, attributes_map=False, device=0, max_blocks=0, stats=None):
    """read_gtf: as read_gff with GTF's attribute grammar (key "value"; ...)"""
    return _read_tabix_mode(TABIX_GTF, "read_gtf", src, region, index_path, False, None, None, False, columns, attributes_map, device, max_blocks, stats)


def c_strtof(tok: bytes):
    """(float)strtod(tok, &end) in the C locale: NaN unless the whole token converts (vep_parse_float, src/vep_parser.c:222-235)"""
    global _LIBC
    try:
        _LIBC
    except NameError:
        _LIBC = C.CDLL(None)
        _LIBC.strtod.restype = C.c_double
        _LIBC.strtod.argtypes = [C.c_char_p, C.POINTER(C.c_char_p)]
    if not tok or b"\0" in tok:
        return float("nan")
    buf = C.create_string_buffer(tok)
    end = C.c_char_p()
    v = _LIBC.strtod(buf, C.byref(end))
    consumed = C.cast(end, C.c_void_p).value - C.addressof(buf)
    if consumed != len(tok):
        return float("nan")
    with np.errstate(over="ignore"):
        return float(np.float32(v))


def _concat_tables(parts, schema_cols):
    if not parts:
        return None
    out = []
    for k in range(len(parts[0]["cols"])):
        cs = [p["cols"][k] for p in parts]
        c = {"name": cs[0]["name"], "type": cs[0]["type"], "is_list": cs[0]["is_list"], "valid": np.concatenate([x["valid"] for x in cs])}

        def cat_off(key, bkey):
            base, offs = 0, []
            for x in cs:
                offs.append(x[key][:-1] + np.uint64(base))
                base += int(x[key][-1])
            return np.concatenate(offs + [np.array([base], np.uint64)]), np.concatenate([x[bkey] for x in cs])

        if not c["is_list"]:
            if "fixed" in cs[0]:
                c["fixed"] = np.concatenate([x["fixed"] for x in cs])
            else:
                c["soff"], c["sbytes"] = cat_off("soff", "sbytes")
        else:
            base, lo = 0, []
            for x in cs:
                lo.append(x["loff"] + np.uint64(base))
                base += x["child_n"]
            c["loff"], c["llen"], c["child_n"] = np.concatenate(lo), np.concatenate([x["llen"] for x in cs]), base
            if "cvalid" in cs[0]:
                c["cvalid"] = np.concatenate([x["cvalid"] for x in cs])
            if "cfixed" in cs[0]:
                c["cfixed"] = np.concatenate([x["cfixed"] for x in cs])
            else:
                c["csoff"], c["csbytes"] = cat_off("csoff", "csbytes")
        out.append(c)
    return out


def read_bcf(src, tidy=False, columns=None, device=0, max_blocks=0, block_range=None, region=None, index=None, stats=None, repair_stats=None):
    """Full sequential read_bcf scan (every record in file order); returns the canonical column table.
    columns: optional projection (names or schema ids), like DuckDB's projection pushdown.  stats: a dict that receives Context.debug_tile_stats();
    repair_stats: one that receives Context.bgzf_repair_stats()."""
    ctx = Context(device)
    try:
        ctx.open(src)
        ctx.bgzf_index()
        sc = BcfScan(ctx, tidy)
        if columns is not None:
            sc.set_projection(columns)
        if block_range is not None:
            sc.set_block_range(*block_range)
        parts, status, first, end = [], 0, None, None
        # region := 'a,b': chained union of single-region scans in the given order (src/bcf_reader.c:1327-1345)
        passes = [None] if region is None else ([r for r in region.split(",") if r] or [None])     # no non-empty token = no region
        for rg in passes:
            if rg is not None and not sc.set_region(rg):
                continue
            if rg is not None and index is not None and not sc.load_index(index):
                continue
            while True:
                b = sc.next_batch(max_blocks)
                if b.n_rows:
                    parts.append(sc.batch_table(b))
                    first = b.first_rec_uoff if first is None else first
                end = b.end_uoff
                status = b.status
                if b.status != 0:
                    break
        if stats is not None:
            stats.update(ctx.debug_tile_stats())
        if repair_stats is not None:
            repair_stats.update(ctx.bgzf_repair_stats())
        proj = [sc.schema[i] for i in sc.projection]
        cols = _concat_tables(parts, proj)
        if cols is None:
            cols = []
            for s_ in proj:
                c = {"name": s_["name"], "type": _CANON_TYPE[s_["type"]], "is_list": s_["is_list"], "valid": np.zeros(0, np.uint8)}
                varchar = s_["type"] == 17
                if not s_["is_list"]:
                    if varchar:
                        c["soff"], c["sbytes"] = np.zeros(1, np.uint64), np.zeros(0, np.uint8)
                    else:
                        c["fixed"] = np.zeros(0, np.uint64)
                else:
                    c["loff"], c["llen"], c["child_n"] = np.zeros(0, np.uint64), np.zeros(0, np.uint64), 0
                    if varchar:
                        c["csoff"], c["csbytes"] = np.zeros(1, np.uint64), np.zeros(0, np.uint8)
                    else:
                        c["cfixed"] = np.zeros(0, np.uint64)
                cols.append(c)
        return {"n_rows": sum(p["n_rows"] for p in parts), "status": status, "cols": cols, "by_name": {c["name"]: c for c in cols},
                "schema": sc.schema, "samples": sc.samples, "first_rec_uoff": first, "end_uoff": end, "header_first_rec_uoff": sc.first_rec_uoff}
    finally:
        ctx.close()


_STD_TAGS = None


def std_tags():
    """the reference's standard-tag table (src/bam_reader.c:54-70) as exposed by the library: [(name, type, subtype)]"""
    global _STD_TAGS
    if _STD_TAGS is None:
        L = lib()
        out = []
        for i in range(L.dhts_bam_std_tag_count()):
            nm, ty, sub = C.create_string_buffer(3), C.create_string_buffer(1), C.create_string_buffer(1)
            L.dhts_bam_std_tag_info(i, nm, ty, sub)
            out.append((nm.value.decode(), ty.raw.decode(), sub.raw.decode() if sub.raw != b"\0" else ""))
        _STD_TAGS = out
    return _STD_TAGS


def read_bam(src, device=0, max_blocks=0, shard=None, region=None, index=None, std_tags_cols=None, aux_map=None, overlap=None, sparse=None, overlap_bed=None,
             block_range=None, stats=None, repair_stats=None):
    """Full sequential scan (reference mode (i)): all rows in file order.
    block_range=(b0, b1, speculative): one shard of BGZF blocks (Context.set_block_range); the result carries first_rec_uoff / end_uoff.
    stats: a dict that receives Context.debug_tile_stats(); repair_stats: one that receives Context.bgzf_repair_stats().
    region: the reference's region := string (rows filtered on the device); index: BAI bytes narrowing the scan window.
    sparse=(header_bytes, beg[], end[]) with a path: only the header blocks and those file ranges are staged (Context.region_segments)."""
    ctx = Context(device)
    try:
        if sparse is not None:
            ctx.open_segments(src, *sparse)
        else:
            ctx.open(src)
        ctx.bgzf_index()
        hdr = ctx.bam_open()
        if shard is not None:
            ctx.set_shard(*shard)
        if block_range is not None:
            ctx.set_block_range(*block_range)
        if region is not None:
            if not ctx.set_regions(region):
                raise DhtsError(f"No reads found for region(s): {region}")
            if index is not None:
                ctx.load_index(index)
        if std_tags_cols is not None:
            ctx.set_tag_columns(std_tags_cols)
        if aux_map is not None:
            ctx.set_aux_map(True, bool(aux_map == "exclude_standard"))
        if overlap is not None:
            ctx.set_overlap_intervals(*overlap)          # (tid, beg, end) arrays: out["OVERLAPS"] = per-row arrays of interval ids
        n_bed = None
        if overlap_bed is not None:                      # BED text (bytes) or file (path): ids = read_bed row numbers
            n_bed = ctx.set_overlap_bed(overlap_bed); overlap = True
        parts, tparts, aparts, oparts = [], [], [], []
        status = 0
        first_uoff = end_uoff = None
        while True:
            b = ctx.next_batch(max_blocks)
            end_uoff = int(b.end_uoff)
            if b.n_rows:
                first_uoff = int(b.first_rec_uoff) if first_uoff is None else first_uoff
                parts.append(ctx.batch_to_host(b, hdr))
                if std_tags_cols is not None:
                    tparts.append(ctx.tag_table(b))
                if aux_map is not None:
                    aparts.append(ctx.aux_table(b))
                if overlap is not None:
                    oparts.append(ctx.overlap_lists(b))
            status = b.status
            if b.status != 0:
                break
        out = {"n_rows": sum(p["n_rows"] for p in parts), "status": status, "header": hdr, "first_rec_uoff": first_uoff, "end_uoff": end_uoff}
        if stats is not None:
            stats.update(ctx.debug_tile_stats())
        if repair_stats is not None:
            repair_stats.update(ctx.bgzf_repair_stats())
        if std_tags_cols is not None:
            out["tags"] = {"n_rows": out["n_rows"], "cols": _concat_tables(tparts, None) or []}
        if aux_map is not None:
            out["aux"] = {"n_rows": out["n_rows"], "cols": _concat_tables(aparts, None) or []}
        if n_bed is not None:
            out["n_bed_rows"] = n_bed
        if overlap is not None:
            out["OVERLAPS"] = [ids[off[i]:off[i + 1]] for off, ids in oparts for i in range(len(off) - 1)]
        for k in BAM_COLUMNS + ["tid", "mtid"]:
            vals = [p[k] for p in parts]
            if not vals:
                out[k] = []
            elif isinstance(vals[0], np.ndarray):
                out[k] = np.concatenate(vals)
            else:
                out[k] = [x for v in vals for x in v]
        return out
    finally:
        ctx.close()


def _bam_ctx(src, device, region, index):
    """a Context on `device` with src open as a BAM, its regions set and the index loaded: (ctx, header).  The caller closes it."""
    ctx = Context(device)
    try:
        ctx.open(src)
        ctx.bgzf_index()
        hdr = ctx.bam_open()
        if region is not None:
            if not ctx.set_regions(region):
                raise DhtsError(f"No reads found for region(s): {region}")
            if index is not None:
                ctx.load_index(index)
    except BaseException:
        ctx.close()
        raise
    return ctx, hdr


def _bed_ctx(device, bed):
    """a second Context on `device` with bed (a path or the file's bytes) open as read_bed opens it.  The caller closes it."""
    bctx = Context(device)
    try:
        bctx.open(bed)
        bctx.L.dhts_bgzf_index(bctx.h)
        bctx._chk(bctx.L.dhts_bed_open(bctx.h))
    except BaseException:
        bctx.close()
        raise
    return bctx


def _drain(next_fn):
    """every batch of a result: next_fn() -> (columns, status) until the status is not 0"""
    parts = []
    while True:
        cols, st = next_fn()
        parts.append(cols)
        if st != 0:
            return parts


def bam_bin_counts(src, bin_width=5000, min_mapq=0, include_flags=0, require_flags=0, exclude_flags=0, dedup="none", region=None, index=None, emit_zero_bins=False,
                   device=0, max_blocks=0, max_rows=0):
    """bam_bin_counts(path, bin_width :=, min_mapq :=, include_flags :=, require_flags :=, exclude_flags :=, dedup :=, region :=, index_path :=,
    emit_zero_bins :=): read-start counts in fixed-width bins, accumulated on the device (the contract: include/duckhts_amd.h).
    {"n_rows", "chrom": list of bytes, "start" .. "count_rev": int64 arrays, "stats": the seven counters, "status": how the stream ended}.
    index: BAI / CSI bytes narrowing the scan of a region query."""
    ctx, hdr = _bam_ctx(src, device, region, index)
    try:
        ctx.bam_bins_open(bin_width, min_mapq, include_flags, require_flags, exclude_flags, dedup, emit_zero_bins)
        status = ctx.bam_bins_scan(max_blocks)
        parts = _drain(lambda: ctx.bam_bins_next(max_rows))
        out = {k: np.concatenate([p[k] for p in parts]) for k in BINS_COLUMNS}
        names = [n.encode() if isinstance(n, str) else bytes(n) for n in hdr["ref_names"]]
        out["chrom"] = [names[t] for t in out["chrom"]]
        out["n_rows"] = len(out["chrom"])
        out["stats"] = {k: v for k, v in ctx.bam_bins_stats().items() if k.startswith("n_")}
        out["status"] = status
        return out
    finally:
        ctx.close()


def bam_bedcov(src, bed, min_mapq=0, require_flags=0, exclude_flags=0x704, include_flags=0, count_deletions=True, count_ref_skips=True, region=None, index=None,
               max_blocks=0, device=0, bed_max_blocks=0):
    """bam_bedcov(path, bed_path :=, min_mapq :=, require_flags :=, exclude_flags :=, include_flags :=, count_deletions :=, count_ref_skips :=,
    region :=, index_path :=): for every row of the BED (a path or the file's bytes) the summed per-base depth and the number of overlapping
    reads, accumulated on the device (the contract: include/duckhts_amd.h).  {"n_rows", "chrom", "name", "score", "strand": lists of bytes or
    None, "start", "end": lists of int or None, "bases_covered", "read_count": int64 arrays, "stats": the step counters, the BED's rows and
    the breakpoints, "status": how the BAM stream ended}.  index: BAI / CSI bytes narrowing the scan of a region query; max_blocks: BAM blocks
    per batch, bed_max_blocks: BED blocks per result batch."""
    (ctx, hdr), bctx = _bam_ctx(src, device, region, index), None
    try:
        bctx = _bed_ctx(device, bed)
        ctx.bam_bedcov_open(bctx, min_mapq, require_flags, exclude_flags, include_flags, count_deletions, count_ref_skips)
        status = ctx.bam_bedcov_scan(max_blocks)
        parts = _drain(lambda: ctx.bam_bedcov_next(bctx, bed_max_blocks))
        out = {}
        for k in BEDCOV_COLUMNS:
            vals = [p[k] for p in parts if k in p]
            out[k] = np.concatenate(vals) if k in ("bases_covered", "read_count") else [x for v in vals for x in v]
        out["n_rows"] = sum(p["n_rows"] for p in parts)
        out["stats"] = {k: v for k, v in ctx.bam_bedcov_stats().items() if k.startswith("n_")}
        out["status"] = status
        return out
    finally:
        if bctx is not None:
            bctx.close()
        ctx.close()


def bam_coverage(src, min_read_len=0, min_mapq=0, min_baseq=0, include_flags=0, require_flags=0, exclude_flags=0x704, min_depth=1, region=None, index=None,
                 device=0, max_blocks=0, max_rows=0):
    """bam_coverage(path, region :=, index_path :=, min_read_len :=, min_mapq :=, min_baseq :=, include_flags :=, require_flags :=, exclude_flags :=,
    min_depth :=): per contig, or per region given, what `samtools coverage` prints, accumulated on the device (the contract:
    include/duckhts_amd.h).  {"n_rows", "chrom": list of bytes, "start", "end", "numreads", "covbases": int64 arrays, "coverage", "meandepth",
    "meanbaseq", "meanmapq": float64 arrays, "sum_depth", "sum_baseq", "sum_mapq": int64 arrays, "stats": the step counters, "status": how the
    stream ended}.  index: BAI / CSI bytes narrowing the scan of a region query."""
    ctx, hdr = _bam_ctx(src, device, region, index)
    try:
        ctx.bam_coverage_open(min_read_len, min_mapq, min_baseq, include_flags, require_flags, exclude_flags, min_depth)
        status = ctx.bam_coverage_scan(max_blocks)
        parts = _drain(lambda: ctx.bam_coverage_next(max_rows))
        out = {k: np.concatenate([p[k] for p in parts]) for k in COVERAGE_COLUMNS}
        names = [n.encode() if isinstance(n, str) else bytes(n) for n in hdr["ref_names"]]
        out["chrom"] = [names[t] for t in out["chrom"]]
        out["n_rows"] = len(out["chrom"])
        out["stats"] = {k: v for k, v in ctx.bam_coverage_stats().items() if k.startswith("n_") and k != "n_target_rows"}
        out["status"] = status
        return out
    finally:
        ctx.close()


def bam_depth(src, region=None, index=None, bed=None, max_blocks=0, max_rows=0, columns=None, device=0, min_read_len=0, min_mapq=0, min_baseq=0,
              include_flags=0, require_flags=0, exclude_flags=0x704, include_deletions=0, all_positions=0):
    """bam_depth(path, region :=, index_path :=, bed_path :=, min_read_len :=, min_mapq :=, min_baseq :=, include_flags :=, require_flags :=,
    exclude_flags :=, include_deletions :=, all_positions := 0 | 1 (-a) | 2 (-aa)): per position what `samtools depth` prints, streamed page
    by page out of the depth table on the device (the contract: include/duckhts_amd.h) and concatenated here.  {"n_rows", "tid": int32 (the
    contig's id), "pos": int64 (1-based), "depth": int32 arrays -- None for a column that `columns` leaves out --, "contigs": the names by
    id, "stats": the step counters, the target rows, the skipped BED rows, the table's bytes and the result's rows, "status": how the stream
    ended}.  bed: a path or the file's bytes; index: BAI / CSI bytes narrowing the scan of a region query; max_rows: rows per page."""
    (ctx, hdr), bctx = _bam_ctx(src, device, region, index), None
    try:
        if bed is not None:
            bctx = _bed_ctx(device, bed)
        ctx.bam_depth_open(bctx, min_read_len, min_mapq, min_baseq, include_flags, require_flags, exclude_flags, include_deletions, all_positions)
        status = ctx.bam_depth_scan(max_blocks)
        parts = _drain(lambda: ctx.bam_depth_next(max_rows, columns))
        out = {k: None if parts[0][k] is None else np.concatenate([p[k] for p in parts]) for k in DEPTH_COLUMNS}
        out["n_rows"] = sum(p["n_rows"] for p in parts)
        out["pages"] = [p["n_rows"] for p in parts]
        out["contigs"] = [n.encode() if isinstance(n, str) else bytes(n) for n in hdr["ref_names"]]
        out["stats"] = {k: v for k, v in ctx.bam_depth_stats().items() if k != "status"}
        out["status"] = status
        return out
    finally:
        if bctx is not None:
            bctx.close()
        ctx.close()


def bam_bedgraph(src, region=None, index=None, bed=None, max_blocks=0, max_rows=0, columns=None, device=0, min_read_len=0, min_mapq=0, min_baseq=0,
                 include_flags=0, require_flags=0, exclude_flags=0x704, include_deletions=0, zero_runs=0, breaks=None):
    """bam_bedgraph(path, zero_runs :=, breaks :=, bed_path :=, region :=, index_path :=, min_read_len :=, min_mapq :=, min_baseq :=,
    include_deletions :=, include_flags :=, require_flags :=, exclude_flags :=): the depth as bedGraph rows, one per run of equal depth class, cut
    and paged on the device (the contract: include/duckhts_amd.h) and concatenated here.  {"n_rows", "tid": int32 (the contig's id), "start":
    int64 (0-based), "end": int64 (exclusive), "depth": int32 arrays -- None for a column that `columns` leaves out --, "contigs": the names by
    id, "stats": the step counters, the target rows, the skipped BED rows, the table's bytes and the result's runs, "status": how the stream
    ended}.  breaks: integers, or a string of them separated by commas; bed: a path or the file's bytes; index: BAI / CSI bytes narrowing the
    scan of a region query; max_rows: rows per page."""
    if isinstance(breaks, (str, bytes)):
        text = breaks.decode() if isinstance(breaks, bytes) else breaks
        try:
            breaks = [int(x) for x in text.split(",")]
        except ValueError:
            raise DhtsError("bam_bedgraph: breaks must be strictly increasing integers between 1 and 2147483647") from None
    (ctx, hdr), bctx = _bam_ctx(src, device, region, index), None
    try:
        if bed is not None:
            bctx = _bed_ctx(device, bed)
        ctx.bam_bedgraph_open(bctx, min_read_len, min_mapq, min_baseq, include_flags, require_flags, exclude_flags, include_deletions, zero_runs, breaks)
        status = ctx.bam_bedgraph_scan(max_blocks)
        parts = _drain(lambda: ctx.bam_bedgraph_next(max_rows, columns))
        out = {k: None if parts[0][k] is None else np.concatenate([p[k] for p in parts]) for k in BEDGRAPH_COLUMNS}
        out["n_rows"] = sum(p["n_rows"] for p in parts)
        out["pages"] = [p["n_rows"] for p in parts]
        out["contigs"] = [n.encode() if isinstance(n, str) else bytes(n) for n in hdr["ref_names"]]
        out["stats"] = {k: v for k, v in ctx.bam_bedgraph_stats().items() if k != "status"}
        out["status"] = status
        return out
    finally:
        if bctx is not None:
            bctx.close()
        ctx.close()


def _interval_result(ctx, parts, names_cols, status):
    out = {k: None if parts[0][k] is None else np.concatenate([p[k] for p in parts]) for k in names_cols}
    names = ctx.ivl_chrom_names()
    out["chrom"] = None if out["chrom"] is None else [names[i] for i in out["chrom"]]
    out["n_rows"] = sum(p["n_rows"] for p in parts)
    out["pages"] = [p["n_rows"] for p in parts]
    out["status"] = status
    return out


def interval_merge(bed, max_gap=0, columns=None, device=0, max_rows=0, max_blocks=0, stats=None):
    """interval_merge(path, max_gap := 0): the valid rows of a BED (a path, plain or bgzipped, or the file's bytes) sorted by (chrom, start) and
    merged into runs on the device (the contract: include/duckhts_amd.h).  {"n_rows", "chrom": list of bytes, "start", "end", "n_merged": int64
    arrays -- None for a column `columns` leaves out --, "pages": the rows of every page, "status": how the BED's stream ended}.  stats (a
    dict) receives n_rows, n_skipped, n_chroms, n_name_runs, sort_passes and n_runs; max_rows: rows per page; max_blocks: BGZF blocks per batch of
    the read."""
    if not 0 <= int(max_gap) <= INTERVAL_MAX_GAP:
        raise DhtsError("interval_merge: max_gap must be between 0 and 1099511627776")
    ctx = _bed_ctx(device, bed)
    try:
        ctx.ivl_load(max_blocks)
        ctx.ivl_merge_open(max_gap)
        parts = _drain(lambda: ctx.ivl_merge_next(max_rows, columns))
        st = ctx.ivl_stats()
        if stats is not None:
            stats.update({k: v for k, v in st.items() if k not in ("status", "n_pairs")})
        return _interval_result(ctx, parts, INTERVAL_MERGE_COLUMNS, st["status"])
    finally:
        ctx.close()


def interval_overlap(left, right, mode="any", columns=None, device=0, max_rows=0, max_blocks=0, stats=None):
    """interval_overlap(path, right_path :=, mode := 'any' | 'contain' | 'within'): one row per pair of valid rows of the two BED files (paths or
    bytes) on one chrom that satisfies the mode's predicate, joined on the device (the contract: include/duckhts_amd.h).  {"n_rows", "chrom":
    list of bytes, "start", "end", "left_row", "right_start", "right_end", "right_row", "overlap": int64 arrays -- None for a column `columns`
    leaves out --, "pages", "status"}.  stats (a dict) receives the left file's n_rows, n_skipped, n_chroms, n_name_runs, sort_passes and
    n_pairs, and the right file's under "right"."""
    if mode not in INTERVAL_MODES:
        raise DhtsError("interval_overlap: mode must be 'any', 'contain' or 'within'")
    if right is None:
        raise DhtsError("interval_overlap requires right_path")
    lctx, rctx = _bed_ctx(device, left), None
    try:
        rctx = _bed_ctx(device, right)
        lctx.ivl_load(max_blocks)
        rctx.ivl_load(max_blocks)
        lctx.ivl_overlap_open(rctx, mode)
        parts = _drain(lambda: lctx.ivl_overlap_next(max_rows, columns))
        st = lctx.ivl_stats()
        if stats is not None:
            stats.update({k: v for k, v in st.items() if k not in ("status", "n_runs")})
            stats["right"] = {k: v for k, v in rctx.ivl_stats().items() if k not in ("status", "n_runs", "n_pairs")}
        return _interval_result(lctx, parts, INTERVAL_OVERLAP_COLUMNS, st["status"])
    finally:
        if rctx is not None:
            rctx.close()
        lctx.close()


def interval_nearest(left, right, k=1, max_distance=None, ties="all", columns=None, device=0, max_rows=0, max_blocks=0, stats=None):
    """interval_nearest(path, right_path :=, k := 1, max_distance := NULL, ties := 'all' | 'first'): for every valid row of the left BED (paths or
    bytes) the k nearest valid rows of the right BED on its chrom, selected and written on the device (the contract: include/duckhts_amd.h).
    {"n_rows", "chrom": list of bytes, "start", "end", "left_row", "right_start", "right_end", "right_row", "overlap", "distance": int64 arrays --
    None for a column `columns` leaves out --, "pages", "status"}, ordered by left_row, then (right_start, right_row).  stats (a dict) receives the
    left file's n_rows, n_skipped, n_chroms, n_name_runs and sort_passes, the result's n_pairs, n_unmatched and end_sort_passes, and the right
    file's under "right"."""
    if right is None:
        raise DhtsError("interval_nearest requires right_path")
    if not 1 <= int(k) <= INTERVAL_MAX_K:
        raise DhtsError("interval_nearest: k must be between 1 and 1048576")
    if max_distance is not None and int(max_distance) < 0:
        raise DhtsError("interval_nearest: max_distance must not be negative")
    if ties not in INTERVAL_TIES:
        raise DhtsError("interval_nearest: ties must be 'all' or 'first'")
    lctx, rctx = _bed_ctx(device, left), None
    try:
        rctx = _bed_ctx(device, right)
        lctx.ivl_load(max_blocks)
        rctx.ivl_load(max_blocks)
        lctx.ivl_nearest_open(rctx, k, max_distance, ties)
        parts = _drain(lambda: lctx.ivl_nearest_next(max_rows, columns))
        st = lctx.ivl_stats()
        if stats is not None:
            stats.update({k_: v for k_, v in st.items() if k_ not in ("status", "n_runs", "n_pairs")})
            stats.update({k_: v for k_, v in lctx.ivl_nearest_stats().items() if k_ != "status"})
            stats["right"] = {k_: v for k_, v in rctx.ivl_stats().items() if k_ not in ("status", "n_runs", "n_pairs")}
        return _interval_result(lctx, parts, INTERVAL_NEAREST_COLUMNS, st["status"])
    finally:
        if rctx is not None:
            rctx.close()
        lctx.close()


def bam_bedgraph_export(src, out_path, index="tbi", level=-1, min_shift=0, overwrite=False, region=None, bam_index=None, bed=None, max_blocks=0, device=0, min_read_len=0,
                        min_mapq=0, min_baseq=0, include_flags=0, require_flags=0, exclude_flags=0x704, include_deletions=0, zero_runs=0, breaks=None, limits=None):
    """bam_bedgraph_export(path, out_path :=, index := 'tbi' | 'csi' | 'none', level :=, overwrite :=, and every parameter of bam_bedgraph): the
    bedGraph of bam_bedgraph written as out_path (a .bed.gz) with its tabix index, printed, compressed and indexed on the device (the contract:
    include/duckhts_amd.h).  -> the stats: {"n_rows", "bytes_text", "bytes_out", "bytes_index", "status", "output_path", "index_path", "stats":
    bam_bedgraph's}.  index: the kind of the index written (bam_index: BAI / CSI bytes narrowing the scan of a region query); limits: tests, the
    (page_rows, chunk_blocks) of debug_export_limits."""
    if isinstance(breaks, (str, bytes)):
        text = breaks.decode() if isinstance(breaks, bytes) else breaks
        try:
            breaks = [int(x) for x in text.split(",")]
        except ValueError:
            raise DhtsError("bam_bedgraph_export: breaks must be strictly increasing integers between 1 and 2147483647") from None
    (ctx, hdr), bctx = _bam_ctx(src, device, region, bam_index), None
    try:
        if bed is not None:
            bctx = _bed_ctx(device, bed)
        ctx.bam_bedgraph_open(bctx, min_read_len, min_mapq, min_baseq, include_flags, require_flags, exclude_flags, include_deletions, zero_runs, breaks)
        ctx.bam_bedgraph_scan(max_blocks)
        if limits is not None:
            ctx.debug_export_limits(*limits)
        out = ctx.bam_bedgraph_export(out_path, index, level, min_shift, overwrite)
        out["stats"] = {k: v for k, v in ctx.bam_bedgraph_stats().items() if k != "status"}
        return out
    finally:
        if bctx is not None:
            bctx.close()
        ctx.close()


def bam_depth_hist(src, region=None, index=None, bed=None, max_blocks=0, max_rows=0, columns=None, device=0, min_read_len=0, min_mapq=0, min_baseq=0,
                   include_flags=0, require_flags=0, exclude_flags=0x704, include_deletions=0, depth_cap=1000, per="row"):
    """bam_depth_hist(path, depth_cap :=, per :=, bed_path :=, region :=, index_path :=, min_read_len :=, min_mapq :=, min_baseq :=,
    include_deletions :=, include_flags :=, require_flags :=, exclude_flags :=): the positions of every group of target rows on every depth,
    binned and paged on the device (the contract: include/duckhts_amd.h) and concatenated here.  {"n_rows", "tid": int32 (the contig's id),
    "start": int64 (0-based), "end": int64 (exclusive), "depth": int32 (the bin: min(depth, depth_cap)), "n_positions", "n_at_least", "length":
    int64 arrays -- None for a column that `columns` leaves out --, "pages": the rows of every page, "contigs": the names by id, "stats": the
    step counters, the target rows, the groups, the skipped BED rows, the bytes of the two tables and the result's rows, "status": how the
    stream ended}.  per: 'row' or 'contig'; bed: a path or the file's bytes; index: BAI / CSI bytes narrowing the scan of a region query;
    max_rows: rows per page."""
    (ctx, hdr), bctx = _bam_ctx(src, device, region, index), None
    try:
        if bed is not None:
            bctx = _bed_ctx(device, bed)
        ctx.bam_depth_hist_open(bctx, min_read_len, min_mapq, min_baseq, include_flags, require_flags, exclude_flags, include_deletions, depth_cap, per)
        status = ctx.bam_depth_hist_scan(max_blocks)
        parts = _drain(lambda: ctx.bam_depth_hist_next(max_rows, columns))
        out = {k: None if parts[0][k] is None else np.concatenate([p[k] for p in parts]) for k in DEPTH_HIST_COLUMNS}
        out["n_rows"] = sum(p["n_rows"] for p in parts)
        out["pages"] = [p["n_rows"] for p in parts]
        out["contigs"] = [n.encode() if isinstance(n, str) else bytes(n) for n in hdr["ref_names"]]
        out["stats"] = {k: v for k, v in ctx.bam_depth_hist_stats().items() if k != "status"}
        out["status"] = status
        return out
    finally:
        if bctx is not None:
            bctx.close()
        ctx.close()


def bam_pileup(src, region=None, index=None, max_blocks=0, max_rows=0, columns=None, device=0, min_read_len=0, min_mapq=0, min_baseq=0,
               include_flags=0, require_flags=0, exclude_flags=0x704, include_deletions=1, include_insertions=0, distinguish_strands=1, min_nucleotide_depth=1,
               add_form=0):
    """bam_pileup(path, region :=, index_path :=, min_read_len :=, min_mapq :=, min_baseq :=, include_flags :=, require_flags :=, exclude_flags :=,
    include_deletions :=, include_insertions :=, distinguish_strands :=, min_nucleotide_depth :=): per position and strand the number of A C G T
    N = - + on it, counted on the device (the contract: include/duckhts_amd.h), streamed page by page and concatenated here.  {"n_rows", "tid":
    int32 (the contig's id), "pos": int64 (1-based), "strand", "nucleotide": uint8 (ASCII), "count": int32 arrays -- None for a column that
    `columns` leaves out --, "contigs": the names by id, "stats": the step counters, the target rows, the table's bytes and the result's rows,
    "status": how the stream ended}.  index: BAI / CSI bytes narrowing the scan of a region query; max_rows: rows per page; add_form: the
    debug hook's value (tests and benchmarks)."""
    ctx, hdr = _bam_ctx(src, device, region, index)
    try:
        if add_form:
            ctx.bam_pileup_add_form(add_form)
        ctx.bam_pileup_open(min_read_len, min_mapq, min_baseq, include_flags, require_flags, exclude_flags, include_deletions, include_insertions, distinguish_strands,
                            min_nucleotide_depth)
        status = ctx.bam_pileup_scan(max_blocks)
        parts = _drain(lambda: ctx.bam_pileup_next(max_rows, columns))
        out = {k: None if parts[0][k] is None else np.concatenate([p[k] for p in parts]) for k in PILEUP_COLUMNS}
        out["n_rows"] = sum(p["n_rows"] for p in parts)
        out["pages"] = [p["n_rows"] for p in parts]
        out["contigs"] = [n.encode() if isinstance(n, str) else bytes(n) for n in hdr["ref_names"]]
        out["stats"] = {k: v for k, v in ctx.bam_pileup_stats().items() if k != "status"}
        out["status"] = status
        return out
    finally:
        ctx.close()


def _udf_call(op, values, arg=None, device=0):
    ctx = Context(device)
    try:
        kind = "list" if op == "seq_decode_4bit" else "int" if UDF_OPS.index(op) >= _UDF_TEXT_OPS else "str"
        a0 = ctx.udf_upload(values, 0, kind=kind)
        if arg is not None and not isinstance(arg, (str, bytes, int)):
            arg = ctx.udf_upload(arg, 1, kind="int" if op == "sam_flag_has" else "str")
        return ctx.udf(op, a0, arg)
    finally:
        ctx.close()


def _udf_function(op, two):
    if two:
        def f(values, arg, device=0):
            return _udf_call(op, values, arg, device)
    else:
        def f(values, device=0):
            return _udf_call(op, values, None, device)
    f.__name__ = f.__qualname__ = op
    f.__doc__ = (f"{op} of the reference (src/kmer_udf.c) for a list of values, evaluated on the device: upload, one kernel, fetch.  None is NULL."
                 + ("  The second argument is one value for every row, or a list." if two else ""))
    return f


for _op in UDF_OPS:
    globals()[_op] = _udf_function(_op, _op in ("cigar_has_op", "sam_flag_has"))
del _op


def seq_kmers(strings, k, canonical=False, hash=False, text=True, max_rows=0, device=0):
    """seq_kmers over a list of sequences: {"row": index of the sequence, "pos": 1-based, "kmer": bytes (None: a canonical k-mer with a byte
    outside ACGTN), "hash": seq_hash_2bit(kmer) with hash = True (k <= 32)}"""
    ctx = Context(device)
    try:
        return ctx.udf_seq_kmers(ctx.udf_upload(strings, 0), k, canonical=canonical, text=text, hash=hash, max_rows=max_rows)
    finally:
        ctx.close()


def fasta_index(src, device=0):
    """fasta_index on the device: (.fai bytes, .gzi bytes) of a FASTA file (path or bytes), uncompressed or BGZF"""
    ctx = Context(device)
    try:
        ctx.open(src)
        ctx.bgzf_index()
        return ctx.fasta_build_index()
    finally:
        ctx.close()


def fasta_fetch(path, fai, regions, device=0):
    """read_fasta(region := ...): [(name, sequence)] of the regions by the .fai bytes; stages only what the regions read"""
    ctx = Context(device)
    try:
        ctx.fasta_load_index(fai)
        ctx.fasta_open_regions(path, regions)
        return ctx.fasta_fetch(regions)
    finally:
        ctx.close()


def shard_cut(coff, comp_len, rank, world):
    """Block range [b0, b1) of `rank` (same arithmetic as dhts_bam_set_shard; host only, no device needed)."""
    coff = np.ascontiguousarray(coff, dtype=np.uint64)
    b0, b1 = C.c_int64(0), C.c_int64(0)
    if lib().dhts_shard_cut(coff.ctypes.data, len(coff), int(comp_len), rank, world, C.byref(b0), C.byref(b1)) != 0:
        raise ValueError("bad shard arguments")
    return b0.value, b1.value


def shard_window(path, rank, world, header_bytes):
    """(win_begin, win_end, own_end) of `rank` when `world` ranks share ONE file (dhts_open_path_shard's cut; host only, no device)."""
    a, b, t = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    L = lib()
    L.dhts_shard_window.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    if L.dhts_shard_window(os.fsencode(path), rank, world, int(header_bytes), C.byref(a), C.byref(b), C.byref(t)) != 0:
        raise ValueError("bad shard arguments or unreadable file")
    return a.value, b.value, t.value


def check_handoff(spans):
    """spans: per-rank (first_rec_uoff, end_uoff, n_rows) in rank order, absolute inflated-stream offsets.
    Adjacent shards must chain exactly: the record after rank r's last one is rank r+1's first one."""
    for r in range(len(spans) - 1):
        if spans[r][1] != spans[r + 1][0]:
            raise RuntimeError(f"shard hand-off broken between rank {r} and {r + 1}: {spans[r][1]} != {spans[r + 1][0]}")
    return sum(s[2] for s in spans)
