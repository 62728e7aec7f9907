"""bam_depth_ref.py -- CPU model of bam_depth, the contract of include/duckhts_amd.h statement by statement.  TEST INFRASTRUCTURE ONLY.

The read loop of bam_coverage_ref (flags, placement, length, MAPQ, the read's interval against the target rows, then a walk over the CIGAR
base by base that adds 1 to a per-row dict of depths), with the positions of a D operation counted when include_deletions is on, the BED
merge, the three modes of all_positions, the error strings and the table's size.  No runs, no difference table, no scans, no tiles and no
pages: nothing shared with the device code.
"""
from bam_coverage_ref import COUNTERS, DEFAULT_CAP, DEFAULT_EXCLUDE, TILE, cigar_ops, reads_from_bam, reads_from_cols, table_bytes  # noqa: F401

ERR_SHARD = "bam_depth: a shard or block range of the file is not supported"
ERR_NOT_OPEN = "bam_depth: dhts_bam_depth_open not called"
ERR_BAM_NOT_OPEN = "bam_depth: dhts_bam_open not called"
ERR_READ_LEN = "bam_depth: min_read_len must be >= 0"
ERR_DELETIONS = "bam_depth: include_deletions must be 0 or 1"
ERR_ALL = "bam_depth: all_positions must be between 0 and 2"
ERR_BED_AND_REGION = "bam_depth: a BED and regions cannot be combined (give the target rows one way)"
ERR_SUPPRESS = "bam_depth: suppress_overlaps is not supported (mates are not paired on the device)"
ERR_STALE = "bam_depth: the batch is not the one dhts_bam_next_batch returned last"
STATS = COUNTERS + ["n_target_rows", "n_bed_skipped", "table_bytes", "n_positions"]


def err_range(which):
    return f"bam_depth: {which} must be between 0 and {255 if which in ('min_mapq', 'min_baseq') else 65535}"


def err_overlap(a, b):
    return f"bam_depth: the regions '{a}' and '{b}' overlap (one row is answered per region: give disjoint regions)"


def err_table(need, cap):
    return f"bam_depth: the depth table needs {need} bytes (4 per position of every row); at most {cap} are supported (fewer or shorter regions)"


def merge_bed(bed_rows, refs):
    """bed_rows: [(chrom name as bytes, start, end)], 0-based half-open -> ([(tid, beg, end)] the union of the rows: per contig in header
    order, sorted by start, overlapping, nested, duplicate and adjacent rows merged, clipped to the contig, empty ones dropped; the number
    of rows that name a contig the header lacks)"""
    names = {}
    for t, (n, _) in enumerate(refs):
        names.setdefault(n, t)                  # a name listed twice: the first @SQ
    skipped, per = 0, {}
    for name, s, e in bed_rows:
        if name not in names:
            skipped += 1
            continue
        t = names[name]
        s, e = max(s, 0), min(e, refs[t][1])
        if e > s:
            per.setdefault(t, []).append((s, e))
    out = []
    for t in sorted(per):
        cur = None
        for s, e in sorted(per[t]):
            if cur is not None and s <= cur[1]:
                cur[1] = max(cur[1], e)
            else:
                if cur is not None:
                    out.append((t, cur[0], cur[1]))
                cur = [s, e]
        out.append((t, cur[0], cur[1]))
    return out, skipped


def parse_bed(text):
    """the (chrom, start, end) of the data lines of a BED text (no comment, track or browser lines in the tests' files)"""
    rows = []
    for ln in text.splitlines():
        if not ln.strip() or ln.startswith(b"#"):
            continue
        f = ln.split(b"\t")
        rows.append((f[0], int(f[1]), int(f[2])))
    return rows


def depth(reads, refs, rows=None, min_read_len=0, min_mapq=0, min_baseq=0, include_flags=0, require_flags=0, exclude_flags=0, include_deletions=0, all_positions=0):
    """refs: [(name, length)]; rows: [(tid, beg, end)] already clipped, in the order they are answered in (None: one per reference).
    -> {"n_rows", "tid", "pos" (1-based), "depth": lists, "stats": the counters, "per_row": per row {position (0-based): depth},
    "touched": the contigs with a counted read}"""
    if rows is None:
        rows = [(t, 0, l) for t, (_, l) in enumerate(refs)]
    st = dict.fromkeys(COUNTERS, 0)
    per_row = [dict() for _ in rows]
    touched = set()
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
        touched.add(tid)
        if flag & 4:
            continue
        x, q = pos0, 0
        for n, op in cigar:
            if op in "M=X":
                for _ in range(n):
                    for r in mine:
                        if rows[r][1] <= x < rows[r][2] and (q >= l_seq or qual[q] >= min_baseq):
                            per_row[r][x] = per_row[r].get(x, 0) + 1
                    x += 1
                    q += 1
            elif op == "D" and include_deletions:
                for _ in range(n):
                    for r in mine:
                        if rows[r][1] <= x < rows[r][2]:
                            per_row[r][x] = per_row[r].get(x, 0) + 1
                    x += 1
            elif op in "DN":
                x += n
            elif op in "IS":
                q += n
    out = {"tid": [], "pos": [], "depth": []}
    for r, (t, b, e) in enumerate(rows):
        everything = all_positions == 2 or (all_positions == 1 and t in touched)
        for x in (range(b, e) if everything else sorted(per_row[r])):
            out["tid"].append(t)
            out["pos"].append(x + 1)
            out["depth"].append(per_row[r].get(x, 0))
    out["n_rows"] = len(out["pos"])
    out["stats"] = st
    out["per_row"] = per_row
    out["touched"] = touched
    return out
