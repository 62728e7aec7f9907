"""bam_bedgraph_ref.py -- CPU model of bam_bedgraph, the contract of include/duckhts_amd.h.  TEST INFRASTRUCTURE ONLY.

numpy throughout, so that rows of millions of positions stay fast: per target row a difference array of the counted bases, its cumulative sum,
the classes of the depths and the flatnonzero of the class changes.  The read filter and the counted bases are bam_depth's, restated here per
CIGAR operation (bam_depth_ref walks base by base; test_bam_bedgraph_ref holds the two against each other).  No tiles, no carries, no suffix
pass and no pages: nothing shared with the device code.
"""
import numpy as np

from bam_depth_ref import COUNTERS, DEFAULT_EXCLUDE, merge_bed, parse_bed, reads_from_bam, reads_from_cols, table_bytes  # noqa: F401

ERR_SHARD = "bam_bedgraph: a shard or block range of the file is not supported"
ERR_NOT_OPEN = "bam_bedgraph: dhts_bam_bedgraph_open not called"
ERR_BAM_NOT_OPEN = "bam_bedgraph: dhts_bam_open not called"
ERR_READ_LEN = "bam_bedgraph: min_read_len must be >= 0"
ERR_ZERO_RUNS = "bam_bedgraph: zero_runs must be 0 or 1"
ERR_DELETIONS = "bam_bedgraph: include_deletions must be 0 or 1"
ERR_MANY_BREAKS = "bam_bedgraph: at most 16 breaks are supported"
ERR_BREAKS = "bam_bedgraph: breaks must be strictly increasing integers between 1 and 2147483647"
ERR_BED_AND_REGION = "bam_bedgraph: a BED and regions cannot be combined (give the target rows one way)"
ERR_STALE = "bam_bedgraph: the batch is not the one dhts_bam_next_batch returned last"
STATS = COUNTERS + ["n_target_rows", "n_bed_skipped", "table_bytes", "n_runs"]
FILTERS = ("min_read_len", "min_mapq", "min_baseq", "include_flags", "require_flags", "exclude_flags", "include_deletions")


def err_range(which):
    return f"bam_bedgraph: {which} must be between 0 and {255 if which in ('min_mapq', 'min_baseq') else 65535}"


def err_overlap(a, b):
    return f"bam_bedgraph: the regions '{a}' and '{b}' overlap (one row is answered per region: give disjoint regions)"


def err_table(need, cap):
    return f"bam_bedgraph: the depth table needs {need} bytes (4 per position of every row); at most {cap} are supported (fewer or shorter regions)"


def parse_breaks(breaks):
    """None, a list of integers or the table function's text '1,5,150' -> a list of integers"""
    if breaks is None:
        return []
    if isinstance(breaks, str):
        return [int(x) for x in breaks.split(",")]
    return [int(x) for x in breaks]


def classes(depth, breaks):
    """class(d) = the number of breaks <= d; d itself without breaks"""
    depth = np.asarray(depth, np.int64)
    return np.searchsorted(np.asarray(breaks, np.int64), depth, side="right") if len(breaks) else depth


def class_depth(cls, breaks):
    """the reported depth of a class: 0 for class 0, breaks[j - 1] for class j; the class itself without breaks"""
    cls = np.asarray(cls, np.int64)
    return np.concatenate([[0], np.asarray(breaks, np.int64)])[cls] if len(breaks) else cls


def row_depths(reads, refs, rows, min_read_len=0, min_mapq=0, min_baseq=0, include_flags=0, require_flags=0, exclude_flags=0, include_deletions=0):
    """-> (per row an int64 array of the depth on every position of it, the step counters)"""
    st = dict.fromkeys(COUNTERS, 0)
    diff = [np.zeros(e - b + 1, np.int64) for _, b, e in rows]

    def add(r, lo, hi):                      # [lo, hi) in reference coordinates, clipped to row r
        _, b, e = rows[r]
        lo, hi = max(lo, b), min(hi, e)
        if hi > lo:
            diff[r][lo - b] += 1
            diff[r][hi - b] -= 1

    for flag, tid, pos0, mapq, l_seq, cigar, qual in reads:
        st["n_rows"] += 1
        if (flag & require_flags) != require_flags or (flag & exclude_flags) != 0 or (include_flags != 0 and (flag & include_flags) == 0):
            st["n_flag_filtered"] += 1
            continue
        if tid < 0 or tid >= len(refs) or pos0 < 0:
            st["n_unplaced"] += 1
            continue
        if l_seq < min_read_len:
            st["n_short"] += 1
            continue
        if mapq < min_mapq:
            st["n_low_mapq"] += 1
            continue
        rlen = 0 if flag & 4 else sum(n for n, op in cigar if op in "MDN=X")
        lo, hi = pos0, pos0 + max(1, rlen)
        mine = [r for r, (t, b, e) in enumerate(rows) if t == tid and lo < e and hi > b]
        if not mine:
            st["n_outside"] += 1
            continue
        st["n_counted"] += 1
        if flag & 4:
            continue
        q8 = np.frombuffer(bytes(qual), np.uint8)
        x, q = pos0, 0
        for n, op in cigar:
            if op in "M=X":
                if min_baseq > 0:
                    qs = np.arange(q, q + n)
                    ok = qs >= l_seq                                           # a base behind SEQ counts; one inside it by its quality
                    ok[~ok] = q8[qs[~ok]] >= min_baseq
                    edges = np.flatnonzero(np.diff(np.concatenate([[0], ok.astype(np.int8), [0]])))          # starts and ends of the runs of counted bases
                    for s, t in zip(edges[0::2], edges[1::2]):
                        for r in mine:
                            add(r, x + int(s), x + int(t))
                else:
                    for r in mine:
                        add(r, x, x + n)
                x += n
                q += n
            elif op in "DN":
                if op == "D" and include_deletions:
                    for r in mine:
                        add(r, x, x + n)
                x += n
            elif op in "IS":
                q += n
    return [np.cumsum(d)[:-1] for d in diff], st


def bedgraph(reads, refs, rows=None, zero_runs=0, breaks=None, **filters):
    """refs: [(name, length)]; rows: [(tid, beg, end)] already clipped, in the order they are answered in (None: one per reference).
    -> {"n_rows", "tid", "start" (0-based), "end" (exclusive), "depth": int64 arrays, "stats": the counters, "per_row": the depth arrays}"""
    if rows is None:
        rows = [(t, 0, l) for t, (_, l) in enumerate(refs)]
    breaks = parse_breaks(breaks)
    depths, st = row_depths(reads, refs, rows, **filters)
    cols = {"tid": [], "start": [], "end": [], "depth": []}
    for (t, b, e), d in zip(rows, depths):
        if e <= b:
            continue
        cls = classes(d, breaks)
        starts = np.concatenate([[0], np.flatnonzero(cls[1:] != cls[:-1]) + 1])
        ends = np.concatenate([starts[1:], [e - b]])
        keep = np.ones(len(starts), bool) if zero_runs else cls[starts] > 0
        cols["tid"].append(np.full(int(keep.sum()), t, np.int64))
        cols["start"].append(starts[keep] + b)
        cols["end"].append(ends[keep] + b)
        cols["depth"].append(class_depth(cls[starts][keep], breaks))
    out = {k: np.concatenate(v).astype(np.int64) if v else np.zeros(0, np.int64) for k, v in cols.items()}
    out["n_rows"] = len(out["tid"])
    out["stats"] = st
    out["per_row"] = depths
    return out


def expand(res):
    """every row (tid, start, end, d) as the positions start + 1 .. end: (tid, pos 1-based, depth) int64 arrays, bam_depth's columns"""
    n = np.asarray(res["end"], np.int64) - np.asarray(res["start"], np.int64)
    first = np.repeat(np.asarray(res["start"], np.int64) + 1, n)
    within = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    return np.repeat(np.asarray(res["tid"], np.int64), n), first + within, np.repeat(np.asarray(res["depth"], np.int64), n)
