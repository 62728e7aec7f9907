"""bam_bedcov_ref.py -- CPU model of bam_bedcov, the contract of include/duckhts_amd.h statement by statement.  TEST INFRASTRUCTURE ONLY.

One sequential loop over the columns of a read_bam result (orc.bam_read, or duckhts_amd.read_bam for a region query): flags, placement,
MAPQ, then the read's interval and its depth segments from a walk over its CIGAR text.  The result sums max(0, min(b, e) - max(a, s))
over read x BED row directly: no breakpoints, no prefix sums, nothing shared with the device code.  The BED side is read_bed_ref's.
"""
import re

import read_bed_ref as B

COLUMNS = ["chrom", "start", "end", "name", "score", "strand", "bases_covered", "read_count"]
COUNTERS = ["n_rows", "n_flag_filtered", "n_unplaced", "n_low_mapq", "n_counted"]
MAX_BED_ROWS = 1 << 27
DEFAULT_EXCLUDE = 0x704                     # UNMAP, SECONDARY, QCFAIL, DUP: what the table function and the Python function default to
ERR_PATH = "bam_bedcov requires a file path"
ERR_BED_PATH = "bam_bedcov requires bed_path"
ERR_MAPQ = "bam_bedcov: min_mapq must be between 0 and 255"
ERR_SHARD = "shard or block range"
REF_OPS = "MDN=X"                           # the operations that consume the reference


def err_flags(which):
    return f"bam_bedcov: {which}_flags must be between 0 and 65535"


def cigar_ops(cigar):
    """[(length, operation)] of a CIGAR text ('*' or empty: none)"""
    if isinstance(cigar, (bytes, bytearray, memoryview)):
        cigar = bytes(cigar).decode()
    if not cigar or cigar == "*":
        return []
    return [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=XB])", cigar)]


def read_geometry(flag, pos0, cigar, count_deletions=True, count_ref_skips=True):
    """(rlen, [depth segments]) of one read: rlen = reference length of the CIGAR, 0 with FLAG & 4; the segments are the maximal runs of
    reference positions covered by M = X, by D with count_deletions and by N with count_ref_skips"""
    if flag & 4:
        return 0, []
    depth = "M=X" + ("D" if count_deletions else "") + ("N" if count_ref_skips else "")
    x, segs = pos0, []
    for n, op in cigar_ops(cigar):
        if op not in REF_OPS or n == 0:
            continue
        if op in depth:
            if segs and segs[-1][1] == x:
                segs[-1][1] = x + n
            else:
                segs.append([x, x + n])
        x += n
    return x - pos0, [tuple(s) for s in segs]


def counted_reads(cols, n_ref, min_mapq=0, include_flags=0, require_flags=0, exclude_flags=0, count_deletions=True, count_ref_skips=True):
    """the step counters, and per counted read (tid, read interval, depth segments)"""
    st = dict.fromkeys(COUNTERS, 0)
    reads = []
    for i in range(len(cols["FLAG"])):
        flag, tid, pos0, mapq = int(cols["FLAG"][i]), int(cols["tid"][i]), int(cols["POS"][i]) - 1, int(cols["MAPQ"][i])
        st["n_rows"] += 1
        if (flag & require_flags) != require_flags or (flag & exclude_flags) != 0 or (include_flags != 0 and (flag & include_flags) == 0):
            st["n_flag_filtered"] += 1
            continue
        if tid < 0 or tid >= n_ref or pos0 < 0:
            st["n_unplaced"] += 1
            continue
        if mapq < min_mapq:
            st["n_low_mapq"] += 1
            continue
        st["n_counted"] += 1
        rlen, segs = read_geometry(flag, pos0, cols["CIGAR"][i], count_deletions, count_ref_skips)
        reads.append((tid, (pos0, pos0 + max(1, rlen)), segs))
    return st, reads


def bedcov(cols, ref_names, bed_text, **params):
    """cols: {"FLAG", "tid", "POS" (1-based), "MAPQ", "CIGAR"} of the rows in file order; bed_text: the BED file's bytes.
    -> {"n_rows", the eight columns as lists (None = NULL), "stats": the counters}"""
    names = [n.encode() if isinstance(n, str) else bytes(n) for n in ref_names]
    tid_of = {}
    for t, n in enumerate(names):
        tid_of.setdefault(n, t)                                         # a name listed twice: the first @SQ
    bed = B.read_bed(bed_text, columns=COLUMNS[:6])
    if bed["status"] < 0:
        raise ValueError(bed["error"])
    st, reads = counted_reads(cols, len(names), **params)
    by_tid = {}
    for tid, iv, segs in reads:
        by_tid.setdefault(tid, []).append((iv, segs))
    out = {k: bed[k] for k in COLUMNS[:6]}
    out["bases_covered"], out["read_count"] = [], []
    for chrom, s, e in zip(bed["chrom"], bed["start"], bed["end"]):
        bases = count = 0
        tid = tid_of.get(chrom, -1) if chrom is not None else -1
        if tid >= 0 and s is not None and e is not None and e > s:
            for (p, q), segs in by_tid.get(tid, ()):
                if p < e and q > s:
                    count += 1
                for a, b in segs:
                    bases += max(0, min(b, e) - max(a, s))
        out["bases_covered"].append(bases)
        out["read_count"].append(count)
    out["n_rows"] = bed["n_rows"]
    out["stats"] = st
    return out
