"""Hand-written inputs of the bam_depth tests, shared by the model's own test and the device tests."""
import bam_coverage_cases as K

bam, read, REFS = K.bam, K.read, K.REFS
R = read

# The table written out by hand.  exclude_flags = 0x704, min_mapq = 10, min_baseq = 20, min_read_len = 4.
HAND_REFS = [("c1", 60), ("c2", 30), ("c3", 0), ("c4", 8)]
HAND_PARAMS = dict(exclude_flags=0x704, min_mapq=10, min_baseq=20, min_read_len=4)
HAND_READS = [
    R(0, 0, 10, 30, "6M", 30),                                             # 0  10..15
    R(16, 0, 13, 20, "3M2D3M", [30, 30, 10, 30, 30, 30]),                  # 1  13, 14 count, 15 has quality 10; D on 16, 17; 18..20
    R(0, 0, 40, 30, "2D4M", 30),                                           # 2  a leading D on 40, 41; 42..45
    R(0x400, 0, 10, 30, "6M", 30),                                         # 3  duplicate: flag-filtered
    R(0, 0, 10, 5, "6M", 30),                                              # 4  low MAPQ
    R(0, 0, 10, 30, "3M", 30),                                             # 5  l_seq 3 < 4: short
    R(0, 0, -1, 30, "4M", 30),                                             # 6  pos0 < 0: unplaced
    R(0, 1, 27, 30, "2M2N4M", 30),                                         # 7  c2 is 30 long: 27, 28 count, N on 29, 30; 31..34 behind the row
    R(0, 1, 40, 30, "4M", 30),                                             # 8  behind c2's end: outside
    R(0, 3, 2, 30, "4S", 30),                                              # 9  no reference base: c4 is touched and has no depth
]
HAND_STATS = {"n_rows": 10, "n_flag_filtered": 1, "n_unplaced": 1, "n_short": 1, "n_low_mapq": 1, "n_outside": 1, "n_counted": 5}
# (tid, pos 1-based, depth) with include_deletions = 0 and all_positions = 0
HAND_ROWS = [(0, 11, 1), (0, 12, 1), (0, 13, 1), (0, 14, 2), (0, 15, 2), (0, 16, 1), (0, 19, 1), (0, 20, 1), (0, 21, 1), (0, 43, 1), (0, 44, 1), (0, 45, 1), (0, 46, 1),
             (1, 28, 1), (1, 29, 1)]
# ... with include_deletions = 1: 17, 18 (read 1's D) and 41, 42 (read 2's leading D) join
HAND_ROWS_DEL = [(0, 11, 1), (0, 12, 1), (0, 13, 1), (0, 14, 2), (0, 15, 2), (0, 16, 1), (0, 17, 1), (0, 18, 1), (0, 19, 1), (0, 20, 1), (0, 21, 1),
                 (0, 41, 1), (0, 42, 1), (0, 43, 1), (0, 44, 1), (0, 45, 1), (0, 46, 1), (1, 28, 1), (1, 29, 1)]
HAND_TOUCHED = {0, 1, 3}


def hand_rows_all(mode):
    """the hand-written result under all_positions = 1 (c1, c2, c4 are touched; c3 is empty anyway) or 2 (the same here: c3 has no position)"""
    have = {(t, p): d for t, p, d in HAND_ROWS}
    return [(t, p, have.get((t, p), 0)) for t, (_, n) in enumerate(HAND_REFS) for p in range(1, n + 1)]


# BED rows over REFS-like contigs [("c1", 1000), ("c2", 500), ("c3", 0)]: unsorted, overlapping, nested, adjacent, duplicate, clipped at both
# ends, an unknown contig twice, rows that are empty after clipping, an inverted row and a row on the empty contig
BED_REFS = [("c1", 1000), ("c2", 500), ("c3", 0)]
BED_ROWS = [(b"c2", 100, 200), (b"c1", 300, 400), (b"c1", 100, 200), (b"c1", 150, 250), (b"c1", 310, 320), (b"c1", 400, 450), (b"c1", 100, 200),
            (b"chrNone", 0, 100), (b"c1", 990, 2000), (b"c2", 480, 600), (b"c2", 700, 800), (b"c1", 600, 500), (b"c3", 0, 10), (b"chrOther", 5, 6), (b"c1", 0, 1)]
BED_MERGED = [(0, 0, 1), (0, 100, 250), (0, 300, 450), (0, 990, 1000), (1, 100, 200), (1, 480, 500)]
BED_SKIPPED = 2


def bed_text(rows):
    return b"".join(b"\t".join(x if isinstance(x, bytes) else str(x).encode() for x in r) + b"\n" for r in rows)
