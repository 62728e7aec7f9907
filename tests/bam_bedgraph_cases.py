"""Hand-written inputs of the bam_bedgraph tests, shared by the model's own test and the device tests.  A case is (refs, reads); the tile of the
depth table has 1,024 slots, and a row of length L takes L + 1 of them (the closing slot), rounded up to the tile."""
import bam_coverage_cases as K

bam, REFS = K.bam, K.REFS
R = K.read
TILE = 1024
COMBOS = [(0, None), (1, None), (0, "2,4"), (1, "2,4")]                      # (zero_runs, breaks): what every shape is run with


def at(tid, pos0, n, copies=1):
    """`copies` reads of n matched bases at pos0"""
    return [R(0, tid, pos0, 30, f"{n}M", 30)] * copies


# a run that ends on slot 1023 and one that starts on slot 0 of the next tile; a run over one tile edge; a run that covers three tiles with
# no boundary in the middle one (2000 .. 4200 covers the tiles of 2048 and 3072 whole)
def tile_edges():
    refs = [("a", 5000), ("b", 5000), ("c", 5000)]
    reads = at(0, 1000, 24) + at(0, 1024, 17, 2) + at(1, 1000, 101) + at(1, 990, 20, 3) + at(2, 2000, 2201) + at(2, 4150, 100, 4)
    return refs, reads


# rows of length 1, 1,023, 1,024 (the closing slot opens a tile of its own) and 1,025, each with a run up to its last position
def row_lengths():
    refs = [("one", 1), ("t1023", 1023), ("t1024", 1024), ("t1025", 1025), ("zero", 0), ("bare", 1024)]
    reads = at(0, 0, 5) + at(1, 1000, 30) + at(1, 0, 3, 2) + at(2, 1000, 24) + at(2, 1023, 5, 3) + at(2, 0, 1) + at(3, 1020, 10) + at(3, 1024, 1, 4)
    return refs, reads


# equal depth across the seam of two adjacent regions: c1 85 .. 144 has depth 2 throughout
SEAM_READS = at(0, 85, 60, 2) + at(0, 300, 10, 5)
SEAM_TWO, SEAM_ONE, SEAM_REVERSED = "c1:91-100,c1:101-110", "c1:91-110", "c1:101-110,c1:91-100"

# BED intervals that touch: merged into one row, and the run of depth 3 on 150 .. 249 goes through the seam at 200
TOUCH_REFS = [("a", 3000)]
TOUCH_BED = [(b"a", 100, 200), (b"a", 200, 300), (b"a", 1500, 2600)]
TOUCH_READS = at(0, 150, 100, 3) + at(0, 1400, 1300)

# depth 1 on 100 .. 109, 3 on 110 .. 119, 2 on 120 .. 129, 5 on 130 .. 139: under breaks 2,4 the classes are 0, 1, 1, 2
CLASS_REFS = [("k", 400)]
CLASS_READS = at(0, 100, 40) + at(0, 110, 30) + at(0, 110, 10) + at(0, 130, 10, 3)
CLASS_ROWS = {(0, None): [(0, 100, 110, 1), (0, 110, 120, 3), (0, 120, 130, 2), (0, 130, 140, 5)],
              (1, None): [(0, 0, 100, 0), (0, 100, 110, 1), (0, 110, 120, 3), (0, 120, 130, 2), (0, 130, 140, 5), (0, 140, 400, 0)],
              (0, "2,4"): [(0, 110, 130, 2), (0, 130, 140, 4)],
              (1, "2,4"): [(0, 0, 110, 0), (0, 110, 130, 2), (0, 130, 140, 4), (0, 140, 400, 0)]}

# one omitted zero run between two emitted ones, over a tile edge: the first one ends where the zero run starts
GAP_REFS = [("g", 4000)]
GAP_READS = at(0, 1000, 20, 2) + at(0, 2100, 20, 2)

# about 3,000 runs with zero_runs (1,500 reads apart from each other, every seventh with a step in it) on one contig, and a second contig whose zero run between 15 and 19,990 spans nineteen tiles
def many_runs():
    refs = [("m", 80000), ("far", 20000)]
    reads = [R(0, 0, 50 * i + 10, 30, "10M", 30) for i in range(1500)] + [R(0, 0, 50 * i + 12, 30, "4M", 30) for i in range(0, 1500, 7)] + at(1, 5, 10) + at(1, 19990, 10)
    return refs, reads


# more than 4,096 tiles, so that the suffix pass goes through its second level
LONG = 4300000
LONG_REFS = [("long", LONG)]
LONG_ENDS = at(0, 0, 10) + at(0, LONG - 10, 10)
LONG_DELETION = [R(0, 0, 20000, 30, "10M4250000D10M", 30)]
