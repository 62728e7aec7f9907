// bam_filter_check.h -- the range checks of the read filters that bam_bin_counts, bam_bedcov, bam_coverage, bam_depth and bam_pileup share, for
// the C opens (dhts_api.hip) and the DuckDB binds (duckdb_ext.cpp) alike: plain C++, no HIP and no DuckDB.  The order -- min_read_len, min_mapq,
// min_baseq, include_flags, require_flags, exclude_flags -- and the wording are the contract's; a function's own parameters are checked by the
// function, in front of or behind this call.
#ifndef DHTS_BAM_FILTER_CHECK_H
#define DHTS_BAM_FILTER_CHECK_H
#include <stdint.h>
#include <stdio.h>

struct BamFilterMsg { char text[96]; };

// the first of the six that is out of range, as `fn`'s error in m.text; nullptr when all are in range.  has_min_read_len / has_min_baseq: the
// function has that parameter (bam_bin_counts and bam_bedcov have neither).
static inline const char *bam_filter_check(BamFilterMsg &m, const char *fn, int64_t min_read_len, int64_t min_mapq, int64_t min_baseq, int64_t include_flags,
                                           int64_t require_flags, int64_t exclude_flags, bool has_min_read_len, bool has_min_baseq) {
    if (has_min_read_len && min_read_len < 0) { snprintf(m.text, sizeof(m.text), "%s: min_read_len must be >= 0", fn); return m.text; }
    const struct { const char *name; int64_t v; int max; bool on; } r[5] = {{"min_mapq", min_mapq, 255, true}, {"min_baseq", min_baseq, 255, has_min_baseq},
        {"include_flags", include_flags, 65535, true}, {"require_flags", require_flags, 65535, true}, {"exclude_flags", exclude_flags, 65535, true}};
    for (const auto &x : r)
        if (x.on && (x.v < 0 || x.v > x.max)) { snprintf(m.text, sizeof(m.text), "%s: %s must be between 0 and %d", fn, x.name, x.max); return m.text; }
    return nullptr;
}
#endif
