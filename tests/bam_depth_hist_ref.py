"""bam_depth_hist_ref.py -- CPU model of bam_depth_hist, the contract of include/duckhts_amd.h.  TEST INFRASTRUCTURE ONLY.

The depths are bam_depth_ref's: its per-position depth of every target row (the base-by-base walk), laid out as one array per row.  The rows
are put into groups, and a group's depths are clamped to depth_cap and counted with numpy's bincount.  No tiles, no spans, no LDS histogram,
no carries and no pages: nothing shared with the device code.
"""
import numpy as np

import bam_depth_ref as D
from bam_depth_ref import COUNTERS, DEFAULT_EXCLUDE, merge_bed, parse_bed, reads_from_bam, reads_from_cols, table_bytes  # noqa: F401

ERR_SHARD = "bam_depth_hist: a shard or block range of the file is not supported"
ERR_NOT_OPEN = "bam_depth_hist: dhts_bam_hist_open not called"
ERR_BAM_NOT_OPEN = "bam_depth_hist: dhts_bam_open not called"
ERR_READ_LEN = "bam_depth_hist: min_read_len must be >= 0"
ERR_DELETIONS = "bam_depth_hist: include_deletions must be 0 or 1"
ERR_DEPTH_CAP = "bam_depth_hist: depth_cap must be between 1 and 1048575"
ERR_PER = "bam_depth_hist: per must be 'row' or 'contig'"
ERR_BED_AND_REGION = "bam_depth_hist: a BED and regions cannot be combined (give the target rows one way)"
ERR_STALE = "bam_depth_hist: the batch is not the one dhts_bam_next_batch returned last"
ERR_BED_CTX = "bam_depth_hist: the BED context has to be a second context"
ERR_BED_NOT_OPEN = "bam_depth_hist: the BED context is not open"
COLUMNS = ["tid", "start", "end", "depth", "n_positions", "n_at_least", "length"]
STATS = COUNTERS + ["n_target_rows", "n_groups", "n_bed_skipped", "table_bytes", "hist_bytes", "n_result_rows"]
FILTERS = ("min_read_len", "min_mapq", "min_baseq", "include_flags", "require_flags", "exclude_flags", "include_deletions")
MAX_DEPTH_CAP = 1048575
MAX_HIST_BYTES = 1 << 30


def err_range(which):
    return f"bam_depth_hist: {which} must be between 0 and {255 if which in ('min_mapq', 'min_baseq') else 65535}"


def err_overlap(a, b):
    return f"bam_depth_hist: the regions '{a}' and '{b}' overlap (one row is answered per region: give disjoint regions)"


def err_table(need, cap):
    return f"bam_depth_hist: the depth table needs {need} bytes (4 per position of every row); at most {cap} are supported (fewer or shorter regions)"


def err_hist(need, cap):
    return f"bam_depth_hist: the histogram needs {need} bytes (8 per bin of every group); at most {cap} are supported (per := 'contig' or a smaller depth_cap)"


def row_depths(reads, refs, rows, **filters):
    """-> (per row an int64 array of bam_depth_ref's depth on every position of it, the step counters)"""
    res = D.depth(reads, refs, rows=rows, **filters)
    out = []
    for (t, b, e), have in zip(rows, res["per_row"]):
        d = np.zeros(max(e - b, 0), np.int64)
        for x, v in have.items():
            d[x - b] = v
        out.append(d)
    return out, res["stats"]


def groups_of(rows, per):
    """-> [(tid, start, end, length, [row indices])]: a group per non-empty row in the order given ('row'), or per contig that has a non-empty
    row, in header order, its rows by start ('contig')"""
    live = [r for r, (t, b, e) in enumerate(rows) if e > b]
    if per == "row":
        return [(rows[r][0], rows[r][1], rows[r][2], rows[r][2] - rows[r][1], [r]) for r in live]
    assert per == "contig", per
    out = []
    for t in sorted({rows[r][0] for r in live}):
        mine = sorted((r for r in live if rows[r][0] == t), key=lambda r: rows[r][1])
        out.append((t, min(rows[r][1] for r in mine), max(rows[r][2] for r in mine), sum(rows[r][2] - rows[r][1] for r in mine), mine))
    return out


def hist_bytes(rows, depth_cap, per):
    return len(groups_of(rows, per)) * (depth_cap + 1) * 8


def hist(reads, refs, rows=None, depth_cap=1000, per="row", **filters):
    """refs: [(name, length)]; rows: [(tid, beg, end)] already clipped, in the order they are answered in (None: one per reference).
    -> {"n_rows", the seven COLUMNS as int64 arrays, "stats": the counters, "n_groups", "per_row": the depth arrays, "groups"}"""
    if rows is None:
        rows = [(t, 0, l) for t, (_, l) in enumerate(refs)]
    depths, st = row_depths(reads, refs, rows, **filters)
    groups = groups_of(rows, per)
    cols = {k: [] for k in COLUMNS}
    for t, start, end, length, mine in groups:
        d = np.concatenate([depths[r] for r in mine])
        assert len(d) == length
        counts = np.bincount(np.minimum(d, depth_cap), minlength=depth_cap + 1)
        bins = np.flatnonzero(counts)
        at_least = np.cumsum(counts[::-1])[::-1]
        for k, v in (("tid", t), ("start", start), ("end", end), ("length", length)):
            cols[k].append(np.full(len(bins), v, np.int64))
        cols["depth"].append(bins)
        cols["n_positions"].append(counts[bins])
        cols["n_at_least"].append(at_least[bins])
    out = {k: np.concatenate(v).astype(np.int64) if v else np.zeros(0, np.int64) for k, v in cols.items()}
    out["n_rows"] = len(out["tid"])
    out["stats"] = st
    out["n_groups"] = len(groups)
    out["groups"] = groups
    out["per_row"] = depths
    return out


def from_bedgraph(res, rows, depth_cap, per):
    """the same seven columns from the rows of bam_bedgraph(zero_runs = 1) without breaks on the same target rows: the summed run lengths per
    group and min(depth, depth_cap).  res: tid, start, end, depth arrays; a run lies in the one row that contains it"""
    cols = {k: [] for k in COLUMNS}
    tid, start, end, depth = (np.asarray(res[k], np.int64) for k in ("tid", "start", "end", "depth"))
    for t, gs, ge, length, mine in groups_of(rows, per):
        counts = np.zeros(depth_cap + 1, np.int64)
        for r in mine:
            _, b, e = rows[r]
            sel = (tid == t) & (start >= b) & (end <= e)
            np.add.at(counts, np.minimum(depth[sel], depth_cap), end[sel] - start[sel])
        bins = np.flatnonzero(counts)
        at_least = np.cumsum(counts[::-1])[::-1]
        for k, v in (("tid", t), ("start", gs), ("end", ge), ("length", length)):
            cols[k].append(np.full(len(bins), v, np.int64))
        cols["depth"].append(bins)
        cols["n_positions"].append(counts[bins])
        cols["n_at_least"].append(at_least[bins])
    return {k: np.concatenate(v).astype(np.int64) if v else np.zeros(0, np.int64) for k, v in cols.items()}
