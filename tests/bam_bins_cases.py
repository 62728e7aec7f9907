"""Hand-written inputs of the bam_bin_counts tests, shared by the model's own test and the device tests."""
import bamwriter as W

DEDUP_REFS = [("c1", 1000), ("c2", 1000)]
DEDUP_PARAMS = dict(bin_width=100, min_mapq=10, exclude_flags=0x200, dedup="adjacent")
# (flag, tid, pos0, mapq, mate pos0)                      what the adjacent rule makes of the row
DEDUP_ROWS = [
    (0x00, 0, 100, 30, -1),       # 0  counted, forward
    (0x00, 0, 100, 30, -1),       # 1  duplicate of 0 (unpaired: the start alone decides)
    (0x41, 0, 150, 30, 300),      # 2  counted
    (0x91, 0, 150, 30, 400),      # 3  paired, same start, another PNEXT: counted (reverse)
    (0x00, 0, 150, 30, -1),       # 4  unpaired behind a paired row with its start: duplicate
    (0x41, 0, 150, 30, 300),      # 5  paired, its predecessor (row 4, a duplicate itself) has another PNEXT: counted
    (0x00, 0, 200, 30, -1),       # 6  counted
    (0x200, 0, 200, 30, -1),      # 7  flag-filtered: invisible to the rule
    (0x00, 0, 200, 30, -1),       # 8  duplicate of 6, across the invisible row
    (0x10, 0, 300, 5, -1),        # 9  low MAPQ, but it is the predecessor of the next row
    (0x10, 0, 300, 30, -1),       # 10 duplicate of 9
    (0x00, 0, 500, 30, -1),       # 11 counted
    (0x00, 1, 500, 30, -1),       # 12 same start on the next contig: counted
    (0x04, -1, -1, 0, -1),        # 13 unplaced: invisible
    (0x00, 1, 500, 30, -1),       # 14 duplicate of 12, across the unplaced row
    (0x00, 1, 1000, 30, -1),      # 15 pos0 = ref_len: out of range
    (0x10, 1, 999, 30, -1),       # 16 the last base: the clipped last bin, reverse
]
DEDUP_STATS = {"n_rows": 17, "n_flag_filtered": 1, "n_unplaced": 1, "n_out_of_range": 1, "n_duplicate": 5, "n_low_mapq": 1, "n_counted": 8}
# chrom, start, end, bin_id, count_total, count_fwd, count_rev
DEDUP_TABLE = [
    (b"c1", 100, 200, 1, 4, 3, 1),
    (b"c1", 200, 300, 2, 1, 1, 0),
    (b"c1", 500, 600, 5, 1, 1, 0),
    (b"c2", 500, 600, 5, 1, 1, 0),
    (b"c2", 900, 1000, 9, 1, 0, 1),
]
# the same rows without the rule: the five duplicates are counted too
NODEDUP_STATS = dict(DEDUP_STATS, n_duplicate=0, n_counted=13)
NODEDUP_TABLE = [
    (b"c1", 100, 200, 1, 6, 5, 1),
    (b"c1", 200, 300, 2, 2, 2, 0),
    (b"c1", 300, 400, 3, 1, 0, 1),
    (b"c1", 500, 600, 5, 1, 1, 0),
    (b"c2", 500, 600, 5, 2, 2, 0),
    (b"c2", 900, 1000, 9, 1, 0, 1),
]


def records(rows):
    return [W.record(qname=f"r{i}", flag=f, tid=t, pos=p, mapq=q, mtid=(t if m >= 0 else -1), mpos=m, cigar="4M" if t >= 0 else "*", seq="ACGT") for i, (f, t, p, q, m) in enumerate(rows)]


def bam(refs, rows, one_record_per_block=False, **kw):
    """the rows as a BAM file; one_record_per_block: every record in a BGZF block of its own, so that a scan of k blocks per batch puts
    any two neighbours into different batches for some k"""
    recs = records(rows)
    if one_record_per_block:
        kw["cuts"] = [len(r) for r in recs]
    return W.bam_bytes(refs, recs, **kw)


def table_rows(res):
    """a result (model or device) as the list of tuples DEDUP_TABLE is written in"""
    return [tuple(bytes(res["chrom"][i]) if k == 0 else int(res[c][i]) for k, c in enumerate(("chrom", "start", "end", "bin_id", "count_total", "count_fwd", "count_rev")))
            for i in range(res["n_rows"])]
