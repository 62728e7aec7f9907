"""Hand-written inputs of the bam_bedcov tests, shared by the model's own test and the device tests."""
import bamwriter as W

REFS = [("c1", 100000), ("c2", 100000), ("c3", 100000)]
# a BED over tests/golden/range.bam: plain, nested, overlapping and repeated rows, a row before the first read, empty, inverted, negative,
# past the contig's end, a NULL start, a contig without reads and one the header lacks
GOLDEN_BED = (b"#a comment\n"
              b"CHROMOSOME_I\t900\t1000\tfirst\t5\t+\n"
              b"CHROMOSOME_I\t0\t914\n"
              b"CHROMOSOME_I\t1000\t2500\twide\t0\t-\n"
              b"CHROMOSOME_I\t1200\t1300\tnested\n"
              b"CHROMOSOME_I\t1200\t1300\tnested\n"
              b"CHROMOSOME_II\t1136\t1137\n"
              b"CHROMOSOME_II\t2000\t1000\tinverted\n"
              b"CHROMOSOME_II\t-50\t1200\n"
              b"CHROMOSOME_III\t1500\t1500\n"
              b"track name=x\n"
              b"CHROMOSOME_III\t2900\t9000\tpast_the_end\n"
              b"CHROMOSOME_IV\tx\t2000\n"
              b"CHROMOSOME_V\t0\t5000\n"
              b"chrNone\t0\t5000\n"
              b"CHROMOSOME_IV\t900\t3100\t.\t.\t.\n")

# The table written out by hand: reads on REFS, a BED, and the expected (bases_covered, read_count) per BED row under the four
# combinations (count_deletions, count_ref_skips) = (1, 1), (0, 1), (1, 0), (0, 0); exclude_flags = 0x704, min_mapq = 10.
# (flag, tid, pos0, mapq, cigar)
HAND_ROWS = [
    (0, 0, 100, 30, "10M"),                # 0  [100, 110)
    (16, 0, 105, 30, "5M3D5M"),            # 1  [105, 118): 105..109, deletion 110..112, 113..117
    (0, 0, 120, 30, "5M100N5M"),           # 2  [120, 230): 120..124, skip 125..224, 225..229
    (0, 0, 300, 30, "3S4M2I4M3S"),         # 3  [300, 308)
    (0, 0, 400, 30, "*"),                  # 4  mapped, no CIGAR: read interval [400, 401), no depth
    (0x400, 0, 100, 30, "10M"),            # 5  duplicate: flag-filtered
    (0, 0, 100, 5, "10M"),                 # 6  low MAPQ
    (4, -1, -1, 0, "*"),                   # 7  unplaced (and UNMAP is excluded first: flag-filtered)
    (0, 1, 100, 30, "4=1X4="),             # 8  contig 2: [100, 109)
    (0, 0, -1, 30, "4M"),                  # 9  pos0 < 0: unplaced
]
HAND_STATS = {"n_rows": 10, "n_flag_filtered": 2, "n_unplaced": 1, "n_low_mapq": 1, "n_counted": 6}
HAND_BED = (b"c1\t100\t110\n"              # read 0 whole (10), read 1's first five bases (5): 15 bases, 2 reads
            b"c1\t110\t113\n"              # inside read 1's deletion: 3 or 0 bases; 1 read either way
            b"c1\t0\t1000\n"               # everything on c1
            b"c1\t125\t225\n"              # inside read 2's ref-skip: 100 or 0 bases, 1 read
            b"c1\t400\t401\n"              # the read without a CIGAR: depth 0, 1 read
            b"c1\t401\t500\n"              # behind it: nothing
            b"c2\t100\t109\n"
            b"c2\t104\t105\n"              # the X of 4=1X4=
            b"c3\t0\t1000\n"               # no reads on c3
            b"c1\t110\t100\n")             # inverted
# per BED row: ((bases, reads) under (1, 1), (0, 1), (1, 0), (0, 0))
HAND_EXPECTED = [
    ((15, 2), (15, 2), (15, 2), (15, 2)),
    ((3, 1), (0, 1), (3, 1), (0, 1)),
    ((10 + 13 + 110 + 8 + 0, 5), (10 + 10 + 110 + 8, 5), (10 + 13 + 10 + 8, 5), (10 + 10 + 10 + 8, 5)),
    ((100, 1), (100, 1), (0, 1), (0, 1)),
    ((0, 1), (0, 1), (0, 1), (0, 1)),
    ((0, 0), (0, 0), (0, 0), (0, 0)),
    ((9, 1), (9, 1), (9, 1), (9, 1)),
    ((1, 1), (1, 1), (1, 1), (1, 1)),
    ((0, 0), (0, 0), (0, 0), (0, 0)),
    ((0, 0), (0, 0), (0, 0), (0, 0)),
]
OPTIONS = [(True, True), (False, True), (True, False), (False, False)]
HAND_PARAMS = dict(min_mapq=10, exclude_flags=0x704)


def records(rows):
    """rows: (flag, tid, pos0, mapq, cigar).  The sequence has the CIGAR's query length (bam_read1's check), 'A' throughout."""
    out = []
    for i, (f, t, p, q, cg) in enumerate(rows):
        qlen = sum(op >> 4 for op in W.parse_cigar(cg) if (op & 15) in (0, 1, 4, 7, 8))
        out.append(W.record(qname=f"r{i}", flag=f, tid=t, pos=p, mapq=q, cigar=cg, seq="A" * qlen if qlen else "*"))
    return out


def bam(refs, rows, one_record_per_block=False, **kw):
    """the rows as a BAM file; one_record_per_block: every record in a BGZF block of its own, so that a scan of k blocks per batch cuts
    between any two neighbours for some k"""
    recs = records(rows)
    if one_record_per_block:
        kw["cuts"] = [len(r) for r in recs]
    return W.bam_bytes(refs, recs, **kw)


def bed(rows):
    """(chrom, start, end[, name[, score[, strand]]]) tuples as BED text"""
    return b"".join(b"\t".join(str(x).encode() for x in r) + b"\n" for r in rows)


def pairs(res):
    """a result (model or device) as the list of (bases_covered, read_count) HAND_EXPECTED is written in"""
    return [(int(b), int(c)) for b, c in zip(res["bases_covered"], res["read_count"])]
