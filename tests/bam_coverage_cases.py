"""Hand-written inputs of the bam_coverage tests, shared by the model's own test and the device tests."""
import struct

import bamwriter as W

REFS = [("c1", 100000), ("c2", 100000), ("c3", 100000)]
QUERY_OPS = (0, 1, 4, 7, 8)                 # M I S = X


def qlen_of(cigar):
    return sum(op >> 4 for op in W.parse_cigar(cigar) if (op & 15) in QUERY_OPS)


def read(flag=0, tid=0, pos0=0, mapq=30, cigar="10M", qual=30, **kw):
    """one read of a case.  qual: a number (every base), a list / bytes (one per query base), or a function of the query index"""
    return dict(flag=flag, tid=tid, pos0=pos0, mapq=mapq, cigar=cigar, qual=qual, **kw)


def record(i, r):
    """the BAM record of a read; the sequence has the CIGAR's query length ('A' throughout).  Keys besides read()'s: qname, cg (the real
    CIGAR of a record whose CIGAR field is the kS mN placeholder), l_seq / seq / raw_qual (bamwriter's)"""
    cigar = r.get("cg", r["cigar"])
    n = qlen_of(cigar)
    q = r["qual"]
    qual = bytes([q] * n) if isinstance(q, int) else bytes(q(k) for k in range(n)) if callable(q) else bytes(q)
    kw = dict(qname=r.get("qname", f"r{i}"), flag=r["flag"], tid=r["tid"], pos=r["pos0"], mapq=r["mapq"], seq=r.get("seq", "A" * n if n else "*"), qual=qual)
    if "cg" in r:
        ops = W.parse_cigar(cigar)
        rlen = sum(op >> 4 for op in ops if (op & 15) in (0, 2, 3, 7, 8))
        kw["raw_cigar"] = [(n << 4) | 4, (rlen << 4) | 3]
        kw["raw_aux"] = b"CGBI" + struct.pack("<I", len(ops)) + b"".join(struct.pack("<I", op) for op in ops)
    else:
        kw["cigar"] = cigar
    for k in ("l_seq", "raw_qual"):
        if k in r:
            kw[k] = r[k]
    return W.record(**kw)


def bam(refs, reads, one_record_per_block=False, **kw):
    recs = [record(i, r) for i, r in enumerate(reads)]
    if one_record_per_block:
        kw["cuts"] = [len(x) for x in recs]
    return W.bam_bytes(refs, recs, **kw)


# The table written out by hand.  exclude_flags = 0x704, min_mapq = 10, min_baseq = 20, min_read_len = 4, min_depth = 2.
HAND_REFS = [("c1", 100), ("c2", 50), ("c3", 0)]
HAND_PARAMS = dict(exclude_flags=0x704, min_mapq=10, min_baseq=20, min_read_len=4, min_depth=2)
HAND_READS = [
    read(0, 0, 10, 30, "10M", 30),                                         # 0  10..19, ten bases of quality 30
    read(16, 0, 15, 20, "5M2D5M", [30] * 5 + [10] * 5),                    # 1  15..19 count; 22..26 have quality 10 < 20
    read(0, 0, 18, 40, "2S4M2I4M", [40] * 2 + [25] * 4 + [5] * 2 + [25] * 4),   # 2  18..21 and 22..25: the I parts nothing, eight bases of 25
    read(0x400, 0, 10, 30, "10M", 30),                                     # 3  duplicate: flag-filtered
    read(0, 0, 10, 5, "10M", 30),                                          # 4  low MAPQ
    read(0, 0, 10, 30, "3M", 30),                                          # 5  l_seq 3 < 4: short (before MAPQ)
    read(4, -1, -1, 0, "*", 30),                                           # 6  UNMAP is excluded: flag-filtered
    read(0, 0, -1, 30, "4M", 30),                                          # 7  pos0 < 0: unplaced
    read(0, 1, 45, 30, "10M", 30),                                         # 8  c2 is 50 long: 45..49 count, 50..54 lie behind the row
    read(0, 1, 60, 30, "4M", 30),                                          # 9  behind c2's end: outside
    read(0, 0, 95, 30, "4M1N4M", [30, 30, 19, 30, 30, 30, 30, 30]),        # 10 95, 96, 98 count (97 has 19); 99 is skipped; 100..103 behind the row
    read(0, 0, 50, 30, "4S", 30),                                          # 11 no reference base: interval [50, 51), a read and no depth
]
HAND_STATS = {"n_rows": 12, "n_flag_filtered": 2, "n_unplaced": 1, "n_short": 1, "n_low_mapq": 1, "n_outside": 1, "n_counted": 6}
# c1: reads 0, 1, 2, 10, 11 -> numreads 5, sum_mapq 30 + 20 + 40 + 30 + 30 = 150.  depth 1 on 10..14, 2 on 15..17, 3 on 18..19, 1 on 20..25 and on
#     95, 96, 98: sum_depth 5 + 6 + 6 + 6 + 3 = 26 (= 10 + 5 + 8 + 3 counted bases); depth >= 2 on 15..19: covbases 5.
#     sum_baseq 300 + 150 + 200 + 90 = 740.
# c2: read 8 -> numreads 1, five bases of depth 1: covbases 0, sum_depth 5, sum_baseq 150.
# c3: length 0: zeros, and 0.0 for the four doubles.
HAND_EXPECTED = [
    # chrom, start, end, numreads, covbases, coverage, meandepth, meanbaseq, meanmapq, sum_depth, sum_baseq, sum_mapq
    (b"c1", 0, 100, 5, 5, 5.0, 0.26, 740 / 26, 30.0, 26, 740, 150),
    (b"c2", 0, 50, 1, 0, 0.0, 0.1, 30.0, 30.0, 5, 150, 30),
    (b"c3", 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0),
]
