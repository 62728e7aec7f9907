"""bam_pileup_ref.py -- CPU model of bam_pileup, the contract of include/duckhts_amd.h statement by statement.  TEST INFRASTRUCTURE ONLY.

bam_depth_ref's read loop (flags, placement, length, MAPQ, the read's interval against the target rows, then a walk over the CIGAR base by
base) that adds 1 to a dictionary {(row, position, strand, symbol): count}; the result is that dictionary sorted.  No table, no tiles, no
windows and no pages: nothing shared with the device code.  A read is bam_coverage_ref's tuple with the 4-bit codes of SEQ behind it.
"""
import gzip
import struct

import bam_coverage_ref as CV
from bam_coverage_ref import COUNTERS, DEFAULT_CAP, DEFAULT_EXCLUDE, TILE, cigar_ops  # noqa: F401

SYMBOLS = "ACGTN=-+"
SEQ_TEXT = "=ACMGRSVTWYHKDBN"                   # the text of the 4-bit codes
DEFAULTS = dict(min_read_len=0, min_mapq=0, min_baseq=0, include_flags=0, require_flags=0, exclude_flags=DEFAULT_EXCLUDE, include_deletions=1, include_insertions=0,
                distinguish_strands=1, min_nucleotide_depth=1)          # the table function's and the Python function's
ERR_SHARD = "bam_pileup: a shard or block range of the file is not supported"
ERR_NOT_OPEN = "bam_pileup: dhts_bam_pileup_open not called"
ERR_BAM_NOT_OPEN = "bam_pileup: dhts_bam_open not called"
ERR_READ_LEN = "bam_pileup: min_read_len must be >= 0"
ERR_MIN_DEPTH = "bam_pileup: min_nucleotide_depth must be >= 1"
ERR_STALE = "bam_pileup: the batch is not the one dhts_bam_next_batch returned last"
ERR_PATH = "bam_pileup requires a file path"
STATS = COUNTERS + ["n_target_rows", "table_bytes", "n_result_rows"]


def err_range(which):
    return f"bam_pileup: {which} must be between 0 and {255 if which in ('min_mapq', 'min_baseq') else 65535}"


def err_switch(which):
    return f"bam_pileup: {which} must be 0 or 1"


def err_overlap(a, b):
    return f"bam_pileup: the regions '{a}' and '{b}' overlap (one row is answered per region: give disjoint regions)"


def err_table(need, cap, strands):
    return f"bam_pileup: the count table needs {need} bytes ({64 if strands else 32} per position of every row); at most {cap} are supported (fewer or shorter regions)"


def table_bytes(rows, strands):
    """what the count table of these (tid, beg, end) rows takes: 4 bytes x 8 symbols x (2 with strands) per slot of bam_coverage's layout"""
    return CV.table_bytes(rows) * 8 * (2 if strands else 1)


def symbol_of(code):
    return {1: "A", 2: "C", 4: "G", 8: "T", 0: "="}.get(code, "N")


def reads_from_bam(data):
    """(refs, reads) of a BAM file's bytes: a read = bam_coverage_ref's (flag, tid, pos0, mapq, l_seq, [(len, op)], qual bytes) + (the 4-bit
    codes of SEQ,)"""
    refs, reads = CV.reads_from_bam(data)
    raw = gzip.decompress(data)
    l_text, = struct.unpack_from("<i", raw, 4)
    p = 12 + l_text
    for _ in refs:
        l_name, = struct.unpack_from("<i", raw, p)
        p += 8 + l_name
    out = []
    for r in reads:
        size, = struct.unpack_from("<i", raw, p)
        l_rn, n_cig, l_seq = raw[p + 12], struct.unpack_from("<H", raw, p + 16)[0], struct.unpack_from("<i", raw, p + 20)[0]
        o = p + 36 + l_rn + 4 * n_cig
        assert l_seq == r[4]
        out.append(r + ([(raw[o + q // 2] >> (0 if q & 1 else 4)) & 15 for q in range(l_seq)],))
        p += 4 + size
    assert p == len(raw)
    return refs, out


def reads_from_cols(cols):
    """the reads of a read_bam result, SEQ from its text"""
    base = CV.reads_from_cols(cols)
    out = []
    for i, r in enumerate(base):
        seq = cols["SEQ"][i]
        seq = bytes(seq).decode() if not isinstance(seq, str) else seq
        out.append(r + ([] if seq == "*" else [SEQ_TEXT.index(c) for c in seq],))
    return out


def pileup(reads, refs, rows=None, min_read_len=0, min_mapq=0, min_baseq=0, include_flags=0, require_flags=0, exclude_flags=0, include_deletions=0, include_insertions=0,
           distinguish_strands=0, min_nucleotide_depth=1):
    """refs: [(name, length)]; rows: [(tid, beg, end)] already clipped, in the order they are answered in (None: one per reference).
    -> {"n_rows", "tid", "pos" (1-based), "strand", "nucleotide" (characters), "count": lists, "stats": the counters,
    "counts": {(row, position 0-based, strand, symbol): count} before min_nucleotide_depth}"""
    if rows is None:
        rows = [(t, 0, l) for t, (_, l) in enumerate(refs)]
    st = dict.fromkeys(COUNTERS, 0)
    counts = {}
    for flag, tid, pos0, mapq, l_seq, cigar, qual, seq in reads:
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
        strand = ("-" if flag & 16 else "+") if distinguish_strands else "*"

        def add(x, sym):
            for r in mine:
                if rows[r][1] <= x < rows[r][2]:
                    counts[(r, x, strand, sym)] = counts.get((r, x, strand, sym), 0) + 1

        x, q, anchored = pos0, 0, False             # anchored: the last operation that consumed reference was M = X or D
        for n, op in cigar:
            if n == 0:
                continue
            if op in "M=X":
                for _ in range(n):
                    if q >= l_seq or qual[q] >= min_baseq:
                        add(x, "N" if q >= l_seq else symbol_of(seq[q]))
                    x += 1
                    q += 1
                anchored = True
            elif op == "D":
                if include_deletions:
                    for k in range(n):
                        add(x + k, "-")
                x += n
                anchored = True
            elif op == "N":
                x += n
                anchored = False
            elif op == "I":
                if include_insertions and anchored:
                    add(x - 1, "+")
                q += n
            elif op == "S":
                q += n
    out = {"tid": [], "pos": [], "strand": [], "nucleotide": [], "count": []}
    for (r, x, s, sym), n in sorted(counts.items(), key=lambda kv: (kv[0][0], kv[0][1], "+-*".index(kv[0][2]), SYMBOLS.index(kv[0][3]))):
        if n >= min_nucleotide_depth:
            out["tid"].append(rows[r][0])
            out["pos"].append(x + 1)
            out["strand"].append(s)
            out["nucleotide"].append(sym)
            out["count"].append(n)
    out["n_rows"] = len(out["pos"])
    out["stats"] = st
    out["counts"] = counts
    return out


def as_rows(res):
    """[(tid, pos, strand, nucleotide, count)] of a model or device result (the device's strand and nucleotide are ASCII bytes)"""
    ch = lambda v: v if isinstance(v, str) else chr(int(v))
    return [(int(t), int(p), ch(s), ch(n), int(c)) for t, p, s, n, c in zip(res["tid"], res["pos"], res["strand"], res["nucleotide"], res["count"])]
