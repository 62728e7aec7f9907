"""bam_coverage_ref.py -- CPU model of bam_coverage, the contract of include/duckhts_amd.h statement by statement.  TEST INFRASTRUCTURE ONLY.

One sequential loop over the reads: flags, placement, length, MAPQ, the read's interval against the target rows, then a walk over the
CIGAR base by base that adds 1 to a per-row dict of depths for every counted base.  No runs, no difference table, no scan: nothing shared
with the device code.  The reads come from the file's own bytes (reads_from_bam: every QUAL byte as it is) or from the columns of a
read_bam result (reads_from_cols: the rows of a region query).
"""
import gzip
import re
import struct

import numpy as np

COLUMNS = ["chrom", "start", "end", "numreads", "covbases", "coverage", "meandepth", "meanbaseq", "meanmapq"]
SUMS = ["sum_depth", "sum_baseq", "sum_mapq"]
COUNTERS = ["n_rows", "n_flag_filtered", "n_unplaced", "n_short", "n_low_mapq", "n_outside", "n_counted"]
DEFAULT_EXCLUDE = 0x704                     # UNMAP, SECONDARY, QCFAIL, DUP: what the table function and the Python function default to
DEFAULT_CAP = 16 << 30
TILE = 1024
ERR_PATH = "bam_coverage requires a file path"
ERR_SHARD = "shard or block range"
ERR_NOT_OPEN = "dhts_bam_coverage_open not called"
ERR_READ_LEN = "bam_coverage: min_read_len must be >= 0"
ERR_DEPTH = "bam_coverage: min_depth must be >= 1"
OPS = "MIDNSHP=XB"


def err_range(which):
    return f"bam_coverage: {which} must be between 0 and {255 if which in ('min_mapq', 'min_baseq') else 65535}"


def err_overlap(a, b):
    return f"bam_coverage: the regions '{a}' and '{b}' overlap (one row is answered per region: give disjoint regions)"


def err_table(need, cap):
    return f"bam_coverage: the depth table needs {need} bytes (4 per position of every row); at most {cap} are supported (fewer or shorter regions)"


def table_bytes(rows):
    """what the depth table of these (tid, beg, end) rows takes: a span of (end - beg) + 1 slots each, rounded up to the tile"""
    return 4 * sum(-(-(e - b + 1) // TILE) * TILE for _, b, e in rows if e > b)


def cigar_ops(cigar):
    """[(length, operation)] of a CIGAR text ('*' or empty: none)"""
    if isinstance(cigar, (bytes, bytearray, memoryview)):
        cigar = bytes(cigar).decode()
    if not cigar or cigar == "*":
        return []
    return [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=XB])", cigar)]


def reads_from_bam(data):
    """(refs, reads) of a BAM file's bytes: refs = [(name, length)], a read = (flag, tid, pos0, mapq, l_seq, [(len, op)], qual bytes), the CIGAR
    the CG tag's where the record has one (the placeholder kS mN in front of SEQ with k = l_seq, and a CG:B,I tag at least as long)"""
    raw = gzip.decompress(data)
    assert raw[:4] == b"BAM\x01"
    l_text, = struct.unpack_from("<i", raw, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, p)
    p += 4
    refs = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, p)
        name = raw[p + 4:p + 4 + l_name - 1]
        l_ref, = struct.unpack_from("<i", raw, p + 4 + l_name)
        refs.append((name, l_ref))
        p += 8 + l_name
    reads = []
    while p + 4 <= len(raw):
        size, = struct.unpack_from("<i", raw, p)
        tid, pos, l_rn, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", raw, p + 4)
        o = p + 36 + l_rn
        cig = list(struct.unpack_from(f"<{n_cig}I", raw, o))
        o += 4 * n_cig + (l_seq + 1) // 2
        qual = raw[o:o + l_seq]
        aux, end = o + l_seq, p + 4 + size
        if n_cig and cig[0] == ((l_seq << 4) | 4) and tid >= 0 and pos >= 0:
            cg = _find_cg(raw, aux, end)
            if cg is not None and len(cg) >= n_cig:
                cig = cg
        reads.append((flag, tid, pos, mapq, l_seq, [(c >> 4, OPS[c & 15] if (c & 15) < len(OPS) else "?") for c in cig], qual))
        p = end
    return refs, reads


_AUX_SIZE = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def _find_cg(raw, p, end):
    while p + 3 <= end:
        tag, ty = raw[p:p + 2], chr(raw[p + 2])
        p += 3
        if ty in _AUX_SIZE:
            p += _AUX_SIZE[ty]
        elif ty in "ZH":
            p = raw.index(b"\x00", p) + 1
        elif ty == "B":
            sub, n = chr(raw[p]), struct.unpack_from("<I", raw, p + 1)[0]
            if tag == b"CG" and sub in "Ii":
                return list(struct.unpack_from(f"<{n}I", raw, p + 5))
            p += 5 + n * _AUX_SIZE[sub]
        else:
            return None
    return None


def reads_from_cols(cols):
    """the reads of a read_bam result (orc.bam_read or duckhts_amd.read_bam): QUAL as text, '*' = every byte 0xff"""
    out = []
    for i in range(len(cols["FLAG"])):
        seq, q = cols["SEQ"][i], cols["QUAL"][i]
        seq = bytes(seq).decode() if not isinstance(seq, str) else seq
        q = bytes(q).decode("latin-1") if not isinstance(q, str) else q
        l_seq = 0 if seq == "*" else len(seq)
        qual = b"\xff" * l_seq if q == "*" else bytes(ord(c) - 33 for c in q)
        assert len(qual) == l_seq
        out.append((int(cols["FLAG"][i]), int(cols["tid"][i]), int(cols["POS"][i]) - 1, int(cols["MAPQ"][i]), l_seq, cigar_ops(cols["CIGAR"][i]), qual))
    return out


def ratio(a, b):
    """one IEEE division of the two integers converted to double; 0.0 for a zero denominator"""
    return 0.0 if b == 0 else float(np.float64(a) / np.float64(b))


def coverage(reads, refs, rows=None, min_read_len=0, min_mapq=0, min_baseq=0, include_flags=0, require_flags=0, exclude_flags=0, min_depth=1):
    """refs: [(name, length)]; rows: [(tid, beg, end)] already clipped, in the order they are answered in (None: one per reference).
    -> {"n_rows", the nine columns and the three sums as lists, "stats": the counters, "depth": per row {position: depth}}"""
    if rows is None:
        rows = [(t, 0, l) for t, (_, l) in enumerate(refs)]
    st = dict.fromkeys(COUNTERS, 0)
    depth = [dict() for _ in rows]
    numreads, sum_mapq, sum_baseq = [0] * len(rows), [0] * len(rows), [0] * len(rows)
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
        for r in mine:
            numreads[r] += 1
            sum_mapq[r] += mapq
        if flag & 4:
            continue
        x, q = pos0, 0
        for n, op in cigar:
            if op in "M=X":
                for _ in range(n):
                    for r in mine:
                        if rows[r][1] <= x < rows[r][2] and (q >= l_seq or qual[q] >= min_baseq):
                            depth[r][x] = depth[r].get(x, 0) + 1
                            sum_baseq[r] += qual[q] if q < l_seq else 0
                    x += 1
                    q += 1
            elif op in "DN":
                x += n
            elif op in "IS":
                q += n
    out = {k: [] for k in COLUMNS + SUMS}
    for r, (t, b, e) in enumerate(rows):
        sum_depth = sum(depth[r].values())
        covbases = sum(1 for d in depth[r].values() if d >= min_depth)
        vals = [refs[t][0], b, e, numreads[r], covbases, ratio(100 * covbases, e - b), ratio(sum_depth, e - b), ratio(sum_baseq[r], sum_depth), ratio(sum_mapq[r], numreads[r]),
                sum_depth, sum_baseq[r], sum_mapq[r]]
        for k, v in zip(COLUMNS + SUMS, vals):
            out[k].append(v)
    out["n_rows"] = len(rows)
    out["stats"] = st
    out["depth"] = depth
    return out
