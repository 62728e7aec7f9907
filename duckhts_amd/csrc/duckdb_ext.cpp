// duckdb_ext.cpp -- DuckDB C-API extension surface (outer drop-in boundary) over the MI355X scan path.
//
// The table functions live in the parts included below, one per reader family, over the shared helpers of duckdb_surface.h; read_bam and read_bcf run the batch pipeline of duckdb_pipeline.h (producer threads, pinned slots, parallel fill):
//   duckdb_bam.inc read_bam, duckdb_bins.inc bam_bin_counts, duckdb_bedcov.inc bam_bedcov, duckdb_bcf.inc read_bcf, duckdb_seq.inc read_fastq / read_fasta, duckdb_interval.inc read_bed / fasta_nuc, duckdb_interval_algebra.inc interval_merge / interval_overlap,
//   duckdb_tabix.inc read_tabix / read_gtf / read_gff, duckdb_udf.inc the k-mer family, duckdb_bedgraph.inc bam_bedgraph, duckdb_depth_hist.inc bam_depth_hist, duckdb_bedgraph_export.inc bam_bedgraph_export; duckdb_tools.cpp (its own translation unit) the writers.
// The htslib calls underneath are replaced by include/duckhts_amd.h (HIP kernels); DuckDB is reached only
// through the function-pointer table returned by access->get_api(info, "v1.2.0").
//
// Linkage (src/duckhts.c:13-16,54-55): register_read_bam_function / register_read_bcf_function have external
// linkage and read the DuckDB API through the global `duckdb_ext_api`, exactly like the reference's readers
// (DUCKDB_EXTENSION_EXTERN, duckdb_extension.h:1161), so a reference-built src/duckhts.c links against them
// unchanged.  This file also carries a weak definition of that global and a weak duckhts_init_c_api, which
// are what a stand-alone libduckhts_amd.so uses; strong definitions from src/duckhts.c win at link time.
#include "duckdb_surface.h"
#include "duckdb_pipeline.h"
#include "bam_filter_check.h"

#include <cmath>
#include <mutex>

// duckdb_ext_api_v1 viewed as an array of function pointers (duckdb_surface.h: API).  Weak: the definition
// DUCKDB_EXTENSION_GLOBAL emits in a reference-built src/duckhts.c (duckdb_extension.h:1151) replaces it.
extern "C" __attribute__((visibility("default"), weak)) const void *duckdb_ext_api[DUCKDB_ABI_V120_NSLOTS] = {nullptr};

// what DUCKDB_EXTENSION_API_INIT does (`duckdb_ext_api = *res`, duckdb_extension.h:1153-1158), for hosts that hold the table
extern "C" __attribute__((visibility("default"))) void dhts_set_duckdb_api(const void *api_table) {
    if (api_table) memcpy((void *)duckdb_ext_api, api_table, sizeof(void *) * DUCKDB_ABI_V120_NSLOTS);
}

extern "C" void dhts_debug_malloc_stats(uint64_t *calls, uint64_t *bytes, double *seconds);

#include "duckdb_bam.inc"
#include "duckdb_bins.inc"
#include "duckdb_bcf.inc"
#include "duckdb_seq.inc"
#include "duckdb_interval.inc"
#include "duckdb_interval_algebra.inc"
#include "duckdb_interval_nearest.inc"
#include "duckdb_bedcov.inc"
#include "duckdb_coverage.inc"
#include "duckdb_depth.inc"
#include "duckdb_pileup.inc"
#include "duckdb_bedgraph.inc"
#include "duckdb_depth_hist.inc"
#include "duckdb_bedgraph_export.inc"
#include "duckdb_tabix.inc"
#include "duckdb_udf.inc"

extern "C" __attribute__((visibility("default"), weak)) bool duckhts_init_c_api(duckdb_extension_info info, struct duckdb_extension_access *access) {
    // duckdb_extension.h:1151-1158,1182-1194: fetch the API table, connect, register, disconnect
    const void *api = access->get_api(info, DUCKHTS_API_VERSION);
    if (!api) return false;
    dhts_set_duckdb_api(api);
    duckdb_database *db = access->get_database(info);
    duckdb_connection conn = nullptr;
    if (API(duckdb_state, duckdb_connect, duckdb_database, duckdb_connection *)(*db, &conn) == DuckDBError) {
        access->set_error(info, "Failed to open connection to database");
        return false;
    }
    register_read_bcf_function(conn);                     // registration order of src/duckhts.c:54-71
    register_read_bam_function(conn);
    register_bgzip_function(conn); register_bgunzip_function(conn);           // (the readers between them in src/duckhts.c are not on this path)
    register_bam_index_function(conn); register_bcf_index_function(conn); register_tabix_index_function(conn);
    // read_fastq (src/duckhts.c registers it between the readers) is opt-in until the registered set is widened: DHTS_SEQ_FUNCTIONS=1
    // read_fasta and fasta_index are opt-in with it, in the reference's order (src/duckhts.c:56-58): read_fasta, read_fastq, fasta_index
    if (const char *e = getenv("DHTS_SEQ_FUNCTIONS")) if (atoi(e) == 1) { register_read_fasta_function(conn); register_read_fastq_function(conn); register_fasta_index_function(conn); }
    // read_bed follows fasta_index (src/duckhts.c:59), opt-in as well: DHTS_INTERVAL_FUNCTIONS=1
    if (const char *e = getenv("DHTS_INTERVAL_FUNCTIONS")) if (atoi(e) == 1) register_read_bed_function(conn);
    // fasta_nuc follows read_bed (src/duckhts.c:59-60), behind a variable of its own: DHTS_NUC_FUNCTIONS=1
    if (const char *e = getenv("DHTS_NUC_FUNCTIONS")) if (atoi(e) == 1) register_fasta_nuc_function(conn);
    if (const char *e = getenv("DHTS_ALGEBRA_FUNCTIONS")) if (atoi(e) == 1) { register_interval_merge_function(conn); register_interval_overlap_function(conn); }   // interval_merge, interval_overlap: their place in src/interval_udf.c (PLAN.md 10.5.2), behind a variable of their own
    if (const char *e = getenv("DHTS_NEAREST_FUNCTIONS")) if (atoi(e) == 1) register_interval_nearest_function(conn);   // interval_nearest: behind the two, its place in src/interval_udf.c, under a variable of its own
    // the k-mer family follows tabix_index and precedes read_tabix (src/duckhts.c:66), behind a variable of its own: DHTS_KMER_FUNCTIONS=1
    if (const char *e = getenv("DHTS_KMER_FUNCTIONS")) if (atoi(e) == 1) register_kmer_udf_functions(conn);
    // read_tabix, read_gtf, read_gff close the list (src/duckhts.c:67-69), opt-in: DHTS_TABIX_FUNCTIONS=1
    if (const char *e = getenv("DHTS_TABIX_FUNCTIONS")) if (atoi(e) == 1) { register_read_tabix_function(conn); register_read_gtf_function(conn); register_read_gff_function(conn); }
    // bam_bin_counts is not in src/duckhts.c (the reference plans it: .github/PLAN.md, Phase 10): last, behind a variable of its own, DHTS_COVERAGE_FUNCTIONS=1
    // bam_bedcov (PLAN.md 10.7.3) comes behind it under the same variable at the value 2: the set a host gets with 1 stays what it was
    if (const char *e = getenv("DHTS_COVERAGE_FUNCTIONS")) { const int v = atoi(e); if (v == 1 || v == 2) register_bam_bin_counts_function(conn); if (v == 2) register_bam_bedcov_function(conn); }
    // bam_coverage (PLAN.md 10.4 / 10.7.3) closes the list behind a variable of its own, DHTS_DEPTH_FUNCTIONS=1: the sets under DHTS_COVERAGE_FUNCTIONS stay what they were
    if (const char *e = getenv("DHTS_DEPTH_FUNCTIONS")) if (atoi(e) == 1) register_bam_coverage_function(conn);
    // bam_depth (PLAN.md 10.4 / 10.7.3) comes last, behind a variable of its own, DHTS_PERBASE_FUNCTIONS=1: no value of an existing variable changes its set
    if (const char *e = getenv("DHTS_PERBASE_FUNCTIONS")) if (atoi(e) == 1) register_bam_depth_function(conn);
    // bam_pileup (PLAN.md 10.4 / 10.7.3) comes last, behind a variable of its own, DHTS_PILEUP_FUNCTIONS=1: no value of an existing variable changes its set
    if (const char *e = getenv("DHTS_PILEUP_FUNCTIONS")) if (atoi(e) == 1) register_bam_pileup_function(conn);
    // bam_bedgraph (the run-length form of bam_depth) comes last, behind a variable of its own, DHTS_BEDGRAPH_FUNCTIONS=1: no value of an existing variable changes its set
    if (const char *e = getenv("DHTS_BEDGRAPH_FUNCTIONS")) if (atoi(e) == 1) register_bam_bedgraph_function(conn);
    // bam_depth_hist (the depth distribution per target row or contig) comes last, behind a variable of its own, DHTS_HIST_FUNCTIONS=1: no value of an existing variable changes its set
    if (const char *e = getenv("DHTS_HIST_FUNCTIONS")) if (atoi(e) == 1) register_bam_hist_function(conn);
    // bam_bedgraph_export (the writer layer of PLAN.md 10.5.4 / 10.7.4 for bam_bedgraph) comes last, behind a variable of its own, DHTS_EXPORT_FUNCTIONS=1: no value of an existing variable changes its set
    if (const char *e = getenv("DHTS_EXPORT_FUNCTIONS")) if (atoi(e) == 1) register_bedgraph_export_function(conn);
    API(void, duckdb_disconnect, duckdb_connection *)(&conn);
    return true;
}
