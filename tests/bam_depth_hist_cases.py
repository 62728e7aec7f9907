"""Hand-written inputs of the bam_depth_hist tests, shared by the model's own test and the device tests.  A case is a dict: refs, reads, and
optionally region (the regions' text), bed (BED rows) and kw (parameters).  The tile of the depth table has 1,024 slots, and a row of length L
takes L + 1 of them (the closing slot), rounded up to the tile; a workgroup of the histogram pass owns duckhts_amd.depth_hist_span_tiles(ntiles)
consecutive tiles and counts bins below duckhts_amd.DEPTH_HIST_LDS_BINS in LDS."""
import bam_bedgraph_cases as G
import duckhts_amd

bam, REFS, R, at, TILE = G.bam, G.REFS, G.R, G.at, G.TILE
PERS = ("row", "contig")
LDS = duckhts_amd.DEPTH_HIST_LDS_BINS
CAPS = (5, LDS - 1, LDS, LDS + 1, 5000)                                       # depth_cap around the LDS limit, for STACK reads on one position
STACK = 4200


def rows_of_region(refs, region):
    """(tid, beg, end) per region token 'name' or 'name:a-b' (1-based, closed), clipped to the contig; refs' names as bytes or str"""
    names = [n.decode() if isinstance(n, bytes) else n for n, _ in refs]
    rows = []
    for tok in region.split(","):
        name, _, span = tok.partition(":")
        t = names.index(name)
        b, e = (0, refs[t][1]) if not span else (int(span.split("-")[0]) - 1, int(span.split("-")[1]))
        rows.append((t, min(b, refs[t][1]), min(e, refs[t][1])))
    return rows


def around_1024(tid, b):
    """reads in a row that begins at b: one that ends on slot 1,023, one that starts on it, one that straddles 1,023 / 1,024, one that starts on
    slot 1,024 (what lies behind the row's end is clipped), and depth at the row's first position"""
    return at(tid, b + 1000, 24) + at(tid, b + 1023, 1, 2) + at(tid, b + 1020, 10, 3) + at(tid, b + 1024, 1, 4) + at(tid, b, 2)


# one contig with rows of length 1, 1,023 (fills a tile exactly with its closing slot), 1,024 (spills) and 1,025
def row_lengths():
    starts = (0, 1000, 3000, 5000)
    reads = [r for b in starts for r in around_1024(0, b)]
    return dict(refs=[("a", 8000)], reads=reads, region="a:1-1,a:1001-2023,a:3001-4024,a:5001-6025")


# the same lengths as whole contigs (bam_bedgraph's case), an empty contig and an untouched one among them
def contig_lengths():
    refs, reads = G.row_lengths()
    return dict(refs=refs, reads=reads)


def span_tiles(length):
    return duckhts_amd.depth_hist_span_tiles((length + 1 + TILE - 1) // TILE)


# a contig of two spans and four tiles more: a workgroup's span holds several tiles, and the spans meet inside the one row.  Reads that end on,
# start on and straddle both seams, and a stretch over the whole second span
SPAN_LEN = (2 * duckhts_amd.DEPTH_HIST_SPAN_MIN_TILES + 4) * TILE


def spans():
    s = span_tiles(SPAN_LEN) * TILE
    assert SPAN_LEN > 2 * s and s >= 2 * TILE                                 # (what the case is for: read from the module, not assumed)
    reads = at(0, s - 10, 10) + at(0, s, 7, 2) + at(0, s - 3, 6, 3) + at(0, 2 * s - 1, 2, 4) + at(0, s + 5, s - 10, 2) + at(0, SPAN_LEN - 5, 5)
    return dict(refs=[("s", SPAN_LEN), ("t", 300)], reads=reads + at(1, 10, 20))


# three disjoint regions on one contig, out of order, one more on another contig, and one clipped to empty (behind c3's end)
def seams():
    reads = at(0, 85, 60, 2) + at(0, 300, 10, 5) + at(0, 5000, 100) + at(1, 95, 30, 3)
    return dict(refs=REFS, reads=reads, region="c1:301-400,c1:91-100,c3:100001-100200,c2:1-200,c1:5001-5050")


# two adjacent contigs whose tiles fall into one span (two tiles each), an untouched contig behind them, an empty one
def adjacent_contigs():
    refs = [("a", 1500), ("b", 1500), ("c", 7), ("e", 0), ("d", 1024)]
    return dict(refs=refs, reads=at(0, 100, 10, 3) + at(0, 1490, 10) + at(1, 0, 5) + at(1, 1020, 10, 2) + at(4, 1023, 1))


# STACK one-base reads on one position, other depths around it; run with every cap of CAPS and with depth_cap 1
def stack():
    return dict(refs=[("k", 3000), ("u", 10)], reads=at(0, 777, 1, STACK) + at(0, 700, 100) + at(0, 750, 10, 6) + at(0, 2000, 5, LDS) + at(0, 2002, 1))


# one depth across a whole tile (slots 1,024 .. 2,047 of the row: the wave-uniform add in all four waves), and the same with one slot differing
def flat(odd_one_out):
    reads = at(0, TILE - 4, TILE + 8, 3)
    if odd_one_out:
        reads = reads + at(0, TILE + 333, 1)
    return dict(refs=[("f", 4 * TILE)], reads=reads)


# overlapping and touching BED rows that merge, rows on two contigs, a row on a contig the header lacks, a row clipped to the contig's end
def bed():
    refs = [("a", 3000), ("b", 2000)]
    rows = [(b"a", 100, 200), (b"a", 200, 300), (b"a", 1500, 2600), (b"a", 2500, 2700), (b"nope", 5, 50), (b"b", 1900, 2500), (b"b", 0, 10)]
    return dict(refs=refs, reads=at(0, 150, 100, 3) + at(0, 1400, 1300) + at(1, 1950, 50, 2) + at(1, 5, 2), bed=rows)


ALL = {"row_lengths": row_lengths, "contig_lengths": contig_lengths, "spans": spans, "seams": seams, "adjacent_contigs": adjacent_contigs, "stack": stack,
       "flat": lambda: flat(False), "flat_but_one": lambda: flat(True), "bed": bed}
