"""A brute-force model of interval_nearest (the contract: include/duckhts_amd.h, "interval nearest") over interval_ref.rows_of.  Nothing here is
clever on purpose: every left row is tested against every right row of its chrom, the rows are ranked by (distance, right_start, right_row), cut
by k / ties / max_distance and put into the order of the result."""
import interval_ref as R

TIES = ("all", "first")
MAX_K = 1 << 20
ERR_NEAREST_PATH = "interval_nearest requires a file path"
ERR_RIGHT_PATH = "interval_nearest requires right_path"
ERR_K = "interval_nearest: k must be between 1 and 1048576"
ERR_MAX_DISTANCE = "interval_nearest: max_distance must not be negative"
ERR_TIES = "interval_nearest: ties must be 'all' or 'first'"
ERR_OPEN = R.ERR_OPEN
ERR_TOO_MANY = R.ERR_TOO_MANY
NEAREST_COLUMNS = R.OVERLAP_COLUMNS + ["distance"]


def distance(s, e, rs, re):
    """the gap in bases between [s, e) and [rs, re): 0 for rows that overlap or touch"""
    return max(0, rs - e, s - re)


def nearest(left_text, right_text, k=1, max_distance=None, ties="all", stats=None):
    """the rows of interval_nearest: [(chrom, start, end, left_row, right_start, right_end, right_row, overlap, distance)] by left_row, then
    (right_start, right_row); stats (a dict) receives n_pairs and n_unmatched"""
    if not 1 <= k <= MAX_K:
        raise ValueError(ERR_K)
    if max_distance is not None and max_distance < 0:
        raise ValueError(ERR_MAX_DISTANCE)
    if ties not in TIES:
        raise ValueError(ERR_TIES)
    lrows, lok = R.rows_of(left_text)
    rrows, rok = R.rows_of(right_text)
    by_chrom = {}
    for j in rok:
        by_chrom.setdefault(rrows[j][0], []).append(j)
    out, unmatched = [], 0
    for i in lok:
        c, s, e = lrows[i]
        ranked = sorted((distance(s, e, rrows[j][1], rrows[j][2]), rrows[j][1], j) for j in by_chrom.get(c, ()))
        if max_distance is not None:
            ranked = [t for t in ranked if t[0] <= max_distance]
        if len(ranked) > k:
            ranked = ranked[:k] if ties == "first" else [t for t in ranked if t[0] <= ranked[k - 1][0]]
        unmatched += not ranked
        for d, rs, j in sorted(ranked, key=lambda t: (t[1], t[2])):
            re = rrows[j][2]
            out.append((c, s, e, i, rs, re, j, max(0, min(e, re) - max(s, rs)), d))
    if stats is not None:
        stats.update(n_pairs=len(out), n_unmatched=unmatched)
    return out
