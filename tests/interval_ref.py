"""A brute-force model of interval_merge and interval_overlap (the contract: include/duckhts_amd.h, "interval algebra") over the rows
region_oracle.bed_rows gives for BED text, and a plain stable-sort model of the device sort's key.  Nothing here is clever on purpose: the
pairs are found by testing every left row against every right row of its chrom."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from region_oracle import bed_rows   # noqa: E402

POS_LIMIT = 1 << 62
MAX_GAP_LIMIT = 1 << 40
MODES = ("any", "contain", "within")
ERR_MAX_GAP = "interval_merge: max_gap must be between 0 and 1099511627776"
ERR_MODE = "interval_overlap: mode must be 'any', 'contain' or 'within'"
ERR_MERGE_PATH = "interval_merge requires a file path"
ERR_OVERLAP_PATH = "interval_overlap requires a file path"
ERR_RIGHT_PATH = "interval_overlap requires right_path"
ERR_OPEN = "read_bed: failed to open file: "
ERR_TOO_MANY = "more than 4294967279 rows"
MERGE_COLUMNS = ["chrom", "start", "end", "n_merged"]
OVERLAP_COLUMNS = ["chrom", "start", "end", "left_row", "right_start", "right_end", "right_row", "overlap"]


def valid(row):
    """a row takes part iff start and end are there, end >= start and both lie in [-2^62, 2^62)"""
    _, s, e = row
    return s is not None and e is not None and e >= s and -POS_LIMIT <= s < POS_LIMIT and -POS_LIMIT <= e < POS_LIMIT


def rows_of(text):
    """(rows as bed_rows gives them, the numbers of the valid ones)"""
    rows = bed_rows(bytes(text))
    return rows, [i for i, r in enumerate(rows) if valid(r)]


def table_stats(text):
    rows, ok = rows_of(text)
    return {"n_rows": len(rows), "n_skipped": len(rows) - len(ok), "n_chroms": len({r[0] for r in rows})}


def name_runs(text):
    """the fewest heads of name runs a single batch can show the host: the rows whose chrom differs from the row in front of them, where no
    meta line stands between the two (the head test compares with the LINE in front)"""
    lines = bytes(text).split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    heads, prev = 0, None
    for ln in lines:
        if ln.endswith(b"\r"):
            ln = ln[:-1]
        ln = ln.split(b"\0", 1)[0]
        if not ln or ln[:1] == b"#" or ln[:5] == b"track" or ln[:7] == b"browser":
            prev = None
            continue
        chrom = ln.split(b"\t")[0]
        heads += chrom != prev
        prev = chrom
    return heads


def merge(text, max_gap=0):
    """the rows of interval_merge: [(chrom, start, end, n_merged)] in (chrom byte order, start) order"""
    if not 0 <= max_gap <= MAX_GAP_LIMIT:
        raise ValueError(ERR_MAX_GAP)
    rows, ok = rows_of(text)
    order = sorted(ok, key=lambda i: (rows[i][0], rows[i][1]))        # bytes compare as memcmp does, the shorter first; sorted() is stable
    out = []
    for i in order:
        c, s, e = rows[i]
        if out and out[-1][0] == c and s <= out[-1][2] + max_gap:
            out[-1][2] = max(out[-1][2], e)
            out[-1][3] += 1
        else:
            out.append([c, s, e, 1])
    return [tuple(r) for r in out]


def predicate(mode, s, e, rs, re):
    if mode == "any":
        return rs < e and s < re
    if mode == "contain":
        return s <= rs and re <= e and rs < e
    if mode == "within":
        return rs <= s and e <= re and s < re
    raise ValueError(ERR_MODE)


def overlap(left_text, right_text, mode="any"):
    """the rows of interval_overlap: [(chrom, start, end, left_row, right_start, right_end, right_row, overlap)] by left_row, then
    (right_start, right_row)"""
    if mode not in MODES:
        raise ValueError(ERR_MODE)
    lrows, lok = rows_of(left_text)
    rrows, rok = rows_of(right_text)
    by_chrom = {}
    for j in rok:
        by_chrom.setdefault(rrows[j][0], []).append(j)
    out = []
    for i in lok:
        c, s, e = lrows[i]
        hits = [j for j in by_chrom.get(c, ()) if predicate(mode, s, e, rrows[j][1], rrows[j][2])]
        for j in sorted(hits, key=lambda j: (rrows[j][1], j)):
            rs, re = rrows[j][1], rrows[j][2]
            out.append((c, s, e, i, rs, re, j, max(0, min(e, re) - max(s, rs))))
    return out


def columns(rows, names):
    """a list of result rows as the Python functions return it: chrom a list of bytes, the other columns int64 arrays"""
    out = {"n_rows": len(rows), names[0]: [r[0] for r in rows]}
    for k, nm in enumerate(names[1:], 1):
        out[nm] = np.array([r[k] for r in rows], np.int64)
    return out


def sort_rows(keys, rank):
    """the device sort's answer for uint64 keys (compared unsigned) and uint32 ranks per row: the row numbers by (rank, key), rows of equal
    (rank, key) in input order -- numpy's stable lexsort, the last key the most significant"""
    k, r = np.asarray(keys, np.uint64), np.asarray(rank, np.uint32)
    return np.lexsort((k, r)).astype(np.uint32)


def sort_key(start):
    """the key of a start: two's complement with the sign bit flipped, so that unsigned order is signed order"""
    return np.asarray(start, np.int64).view(np.uint64) ^ np.uint64(1 << 63)


def bed_text(rows, eol=b"\n"):
    """BED text of (chrom, start, end) rows; start / end may be bytes (written as they are) or None (an empty field)"""
    def f(v):
        return b"" if v is None else v if isinstance(v, bytes) else str(v).encode()
    return b"".join(c + b"\t" + f(s) + b"\t" + f(e) + eol for c, s, e in rows)


def seeded_bed(seed, n, n_chroms=3, span=2000, max_len=120, empty_share=0.2, names=None):
    """n rows on n_chroms chroms inside int32, a fifth of them empty, unsorted"""
    rng = np.random.default_rng(seed)
    names = names or [b"chr%d" % (k + 1) for k in range(n_chroms)]
    rows = []
    for _ in range(n):
        s = int(rng.integers(0, span))
        ln = 0 if rng.random() < empty_share else int(rng.integers(1, max_len))
        rows.append((names[int(rng.integers(0, len(names)))], s, s + ln))
    return rows
