"""Hand-written inputs of the bam_pileup tests, shared by the model's own test and the device tests."""
import bam_coverage_cases as K

bam, read, REFS = K.bam, K.read, K.REFS
R = read

# The table written out by hand.  exclude_flags = 0x704, min_mapq = 10, min_read_len = 4; the switches at the table function's defaults
# (deletions, no insertions, strands, min_nucleotide_depth 1).
HAND_REFS = [("c1", 60), ("c2", 30), ("c3", 0), ("c4", 8)]
HAND_PARAMS = dict(exclude_flags=0x704, min_mapq=10, min_read_len=4, include_deletions=1, include_insertions=0, distinguish_strands=1, min_nucleotide_depth=1)
HAND_READS = [
    R(0, 0, 10, 30, "6M", [30, 30, 10, 30, 30, 30], seq="ACGTNA"),         # 0  + 10..15: A C G(quality 10) T N A
    R(16, 0, 12, 30, "3M2D3M", 30, seq="GGTACC"),                          # 1  - 12..14: G G T; D on 15, 16; 17..19: A C C
    R(0, 0, 12, 30, "2M2I2M", 30, seq="GCTTAA"),                           # 2  + 12, 13: G C; an I anchored on 13; 14, 15: A A
    R(0, 0, 30, 30, "2S3I4M", 30, seq="TTGGGACGT"),                        # 3  + an I with no reference in front of it: no anchor; 30..33: A C G T
    R(16, 1, 5, 30, "16M", 30, seq="=ACMGRSVTWYHKDBN"),                    # 4  - every 4-bit code on c2 5..20: = A C N G N N N T N N N N N N N
    R(0x400, 0, 10, 30, "6M", 30),                                         # 5  duplicate: flag-filtered
    R(0, 0, 10, 5, "6M", 30),                                              # 6  low MAPQ
    R(0, 0, 10, 30, "3M", 30),                                             # 7  l_seq 3 < 4: short
    R(0, 0, -1, 30, "4M", 30),                                             # 8  pos0 < 0: unplaced
    R(0, 1, 40, 30, "4M", 30),                                             # 9  behind c2's end: outside
    R(0, 1, 27, 30, "2M2N4M", 30, seq="ACGTAC"),                           # 10 + c2 is 30 long: 27, 28: A C; N on 29, 30; the rest behind the row
    R(16, 3, 2, 30, "4M2I", 30, seq="TTTTGG"),                             # 11 - c4 2..5: T; a trailing I anchored on 5
]
HAND_STATS = {"n_rows": 12, "n_flag_filtered": 1, "n_unplaced": 1, "n_short": 1, "n_low_mapq": 1, "n_outside": 1, "n_counted": 7}
_C2 = [(1, 6, "-", "=", 1), (1, 7, "-", "A", 1), (1, 8, "-", "C", 1), (1, 9, "-", "N", 1), (1, 10, "-", "G", 1), (1, 11, "-", "N", 1), (1, 12, "-", "N", 1), (1, 13, "-", "N", 1),
       (1, 14, "-", "T", 1), (1, 15, "-", "N", 1), (1, 16, "-", "N", 1), (1, 17, "-", "N", 1), (1, 18, "-", "N", 1), (1, 19, "-", "N", 1), (1, 20, "-", "N", 1), (1, 21, "-", "N", 1),
       (1, 28, "+", "A", 1), (1, 29, "+", "C", 1)]
_C4 = [(3, 3, "-", "T", 1), (3, 4, "-", "T", 1), (3, 5, "-", "T", 1), (3, 6, "-", "T", 1)]
_C1_TAIL = [(0, 17, "-", "-", 1), (0, 18, "-", "A", 1), (0, 19, "-", "C", 1), (0, 20, "-", "C", 1), (0, 31, "+", "A", 1), (0, 32, "+", "C", 1), (0, 33, "+", "G", 1), (0, 34, "+", "T", 1)]
# (tid, pos 1-based, strand, nucleotide, count) under HAND_PARAMS
HAND_ROWS = [(0, 11, "+", "A", 1), (0, 12, "+", "C", 1), (0, 13, "+", "G", 2), (0, 13, "-", "G", 1), (0, 14, "+", "C", 1), (0, 14, "+", "T", 1), (0, 14, "-", "G", 1),
             (0, 15, "+", "A", 1), (0, 15, "+", "N", 1), (0, 15, "-", "T", 1), (0, 16, "+", "A", 2), (0, 16, "-", "-", 1)] + _C1_TAIL + _C2 + _C4
# ... with include_insertions = 1: read 2's I on 14 (1-based) behind the + strand's bases, read 11's on c4's 6
HAND_ROWS_INS = [(0, 11, "+", "A", 1), (0, 12, "+", "C", 1), (0, 13, "+", "G", 2), (0, 13, "-", "G", 1), (0, 14, "+", "C", 1), (0, 14, "+", "T", 1), (0, 14, "+", "+", 1), (0, 14, "-", "G", 1),
                 (0, 15, "+", "A", 1), (0, 15, "+", "N", 1), (0, 15, "-", "T", 1), (0, 16, "+", "A", 2), (0, 16, "-", "-", 1)] + _C1_TAIL + _C2 + _C4 + [(3, 6, "-", "+", 1)]
# ... with distinguish_strands = 0
HAND_ROWS_NO_STRANDS = [(0, 11, "*", "A", 1), (0, 12, "*", "C", 1), (0, 13, "*", "G", 3), (0, 14, "*", "C", 1), (0, 14, "*", "G", 1), (0, 14, "*", "T", 1),
                        (0, 15, "*", "A", 1), (0, 15, "*", "T", 1), (0, 15, "*", "N", 1), (0, 16, "*", "A", 2), (0, 16, "*", "-", 1)] + \
                       [(t, p, "*", n, c) for t, p, _, n, c in _C1_TAIL + _C2 + _C4]
# ... with min_baseq = 20: read 0's G of quality 10 leaves 13
HAND_ROWS_BASEQ = [(0, 13, "+", "G", 1) if r == (0, 13, "+", "G", 2) else r for r in HAND_ROWS]
# ... with min_nucleotide_depth = 2
HAND_ROWS_DEPTH2 = [(0, 13, "+", "G", 2), (0, 16, "+", "A", 2)]
HAND_SETS = [({}, HAND_ROWS), ({"include_insertions": 1}, HAND_ROWS_INS), ({"distinguish_strands": 0}, HAND_ROWS_NO_STRANDS), ({"min_baseq": 20}, HAND_ROWS_BASEQ),
             ({"min_nucleotide_depth": 2}, HAND_ROWS_DEPTH2)]


def hand_bam():
    return K.bam(HAND_REFS, HAND_READS)


NT16 = "=ACMGRSVTWYHKDBN"
RANDOM_REFS = [("r1", 3000), ("r2", 1025), ("r3", 700)]


def random_seq(rng, n):
    """mostly A C G T, some N, '=' and ambiguity codes"""
    return "".join(NT16[int(c)] if rng.random() < 0.1 else "ACGT"[int(c) & 3] for c in rng.integers(0, 16, n))


def random_reads(seed, n, refs=RANDOM_REFS, sorted_=False):
    """n seeded reads with CIGARs over all nine operations (zero-length ones included), both strands, every flag the default mask drops,
    some reads off the contig's ends, MAPQ 0..60, qualities 0..41"""
    import numpy as np
    rng = np.random.default_rng(seed)
    reads = []
    for i in range(n):
        tid = int(rng.integers(0, len(refs)))
        ops = []
        for _ in range(int(rng.integers(1, 8))):
            op = "MMMM=XIDNSHP"[int(rng.integers(0, 12))]
            ops.append((int(rng.integers(0, 3)) if rng.random() < 0.1 else int(rng.integers(1, 40 if op in "M=X" else 6)), op))
        if not any(op in "M=XD" for _, op in ops):
            ops.append((int(rng.integers(1, 60)), "M"))
        cigar = "".join(f"{l}{op}" for l, op in ops)
        qn = K.qlen_of(cigar)
        flag = (16 if rng.random() < 0.5 else 0) | (int(rng.choice([0x4, 0x100, 0x200, 0x400])) if rng.random() < 0.1 else 0) | (1 if rng.random() < 0.3 else 0)
        pos0 = int(rng.integers(-1, refs[tid][1] + 20))
        reads.append(R(flag, tid, pos0, int(rng.integers(0, 61)), cigar, [int(v) for v in rng.integers(0, 42, qn)], seq=random_seq(rng, qn) if qn else "*", qname=f"q{i % 17 * 'x'}{i}"))
    if sorted_:
        reads.sort(key=lambda r: (r["tid"], r["pos0"]))
    return reads
