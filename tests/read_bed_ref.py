"""read_bed_ref.py -- CPU model of read_bed (src/interval_udf.c:127-195, 330-426).  TEST INFRASTRUCTURE ONLY.

next_bed_line: hts_getline lines (the '\\n' and a '\\r' in front of it dropped; a last line without '\\n' is a line), the C string ends at
the first NUL; empty lines and those starting with '#', 'track', 'browser' are skipped.  read_bed_scan: fewer than 3 tab-delimited
fields is an error that ends the scan; the five BIGINT columns are strtoll over the whole field, the VARCHAR columns are NULL when the
field is absent or empty, extra is everything behind the 12th tab.

Region queries: tbx_itr_querys looks the name up among the index's sequences; hts_itr_next keeps a line when tbx_parse1 -- under the
configuration the index was built with -- puts it on that sequence with end > beg_q and end_q > beg.  Valid for coordinate-sorted files
whose meta lines all precede the first record (inside an index chunk a line tabix cannot parse ends htslib's iteration).
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
from region_oracle import _strtoll_whole, parse_region   # noqa: E402

import hts_index_ref as R   # noqa: E402

COLUMNS = ["chrom", "start", "end", "name", "score", "strand", "thick_start", "thick_end", "item_rgb", "block_count", "block_sizes", "block_starts", "extra"]
INT_COLS = (1, 2, 6, 7, 9)
ERR = "read_bed: BED line has fewer than 3 tab-delimited fields"
ERR_ITER = "read_bed: failed to create region iterator"


class BedIteratorError(Exception):
    pass


def bed_lines(text):
    """(1-based line number, the line as next_bed_line's C string sees it) for every line of the text"""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for no, ln in enumerate(lines, 1):
        if ln.endswith(b"\r"):
            ln = ln[:-1]
        yield no, ln.split(b"\0", 1)[0]


def is_meta(ln):
    return not ln or ln[:1] == b"#" or ln[:5] == b"track" or ln[:7] == b"browser"


def row_of(ln):
    """the 13 values of one data line (None = NULL)"""
    f = ln.split(b"\t")
    vals = []
    for c in range(12):
        x = f[c] if c < len(f) else None
        if c in INT_COLS:
            vals.append(_strtoll_whole(x) if x else None)
        else:
            vals.append(x if x else None)
    rest = b"\t".join(f[12:]) if len(f) > 12 else None
    vals.append(rest if rest else None)
    return vals


def tabix_names(text, conf):
    """the index's sequences: names in order of first appearance among the lines the indexer does not pass over"""
    names = []
    for no, ln in bed_lines(text):
        if no <= conf[5] or ln[:1] == bytes([conf[4]]):
            continue
        iv = R.tbx_parse1(conf, ln.decode("latin-1"))
        if iv is not None and iv[0] not in names:
            names.append(iv[0])
    return names


def read_bed(text, columns=None, region=None, conf=R.CONF_BED):
    """-> {"n_rows", "status" (1 clean end, -4 a short line ended the scan), "error" (message with the 1-based line number, without it
    for a region query), column: list}.  columns: names or ids, default all 13."""
    ids = list(range(13)) if columns is None else [c if isinstance(c, int) else COLUMNS.index(c) for c in columns]
    q = None
    if region is not None and region != ".":
        names = tabix_names(text, conf)
        r = parse_region(names, region)
        if r is None:
            raise BedIteratorError(ERR_ITER)
        q = (names[r[0]], r[1], r[2])
    out = {"n_rows": 0, "status": 1, "error": None}
    out.update({COLUMNS[i]: [] for i in ids})
    for no, ln in bed_lines(text):
        if is_meta(ln):
            continue
        if q is not None:
            if no <= conf[5] or ln[:1] == bytes([conf[4]]):
                continue
            iv = R.tbx_parse1(conf, ln.decode("latin-1"))
            if iv is None or iv[0] != q[0] or not (iv[2] > q[1] and q[2] > iv[1]):
                continue
        if ln.count(b"\t") < 2:
            out["status"] = -4
            out["error"] = ERR + (" (line %d)" % no if region is None else "")
            break
        vals = row_of(ln)
        for i in ids:
            out[COLUMNS[i]].append(vals[i])
        out["n_rows"] += 1
    return out
