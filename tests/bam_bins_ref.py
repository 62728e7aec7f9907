"""bam_bins_ref.py -- CPU model of bam_bin_counts, the contract of include/duckhts_amd.h statement by statement.  TEST INFRASTRUCTURE ONLY.

One sequential loop over the columns of a read_bam result (orc.bam_read, or duckhts_amd.read_bam for a region query): flags, placement, the
adjacent-start duplicate rule, MAPQ, then the bin.  Nothing is vectorised and nothing is shared with the device code.
"""
COLUMNS = ["chrom", "start", "end", "bin_id", "count_total", "count_fwd", "count_rev"]
COUNTERS = ["n_rows", "n_flag_filtered", "n_unplaced", "n_out_of_range", "n_duplicate", "n_low_mapq", "n_counted"]
MAX_BINS = 1 << 28
ERR_PATH = "bam_bin_counts requires a file path"
ERR_BIN_WIDTH = "bam_bin_counts: bin_width must be > 0"
ERR_MAPQ = "bam_bin_counts: min_mapq must be between 0 and 255"
ERR_DEDUP = "bam_bin_counts: dedup must be one of: none, adjacent"


def err_flags(which):
    return f"bam_bin_counts: {which}_flags must be between 0 and 65535"


class BinsError(Exception):
    pass


def check_params(bin_width=5000, min_mapq=0, include_flags=0, require_flags=0, exclude_flags=0, dedup="none"):
    """the parameter errors, in the order they are reported"""
    if bin_width <= 0:
        raise BinsError(ERR_BIN_WIDTH)
    if not 0 <= min_mapq <= 255:
        raise BinsError(ERR_MAPQ)
    for which, v in (("include", include_flags), ("require", require_flags), ("exclude", exclude_flags)):
        if not 0 <= v <= 65535:
            raise BinsError(err_flags(which))
    if dedup not in ("none", "adjacent"):
        raise BinsError(ERR_DEDUP)


def total_bins(ref_len, bin_width):
    return sum((int(n) + bin_width - 1) // bin_width for n in ref_len)


def bin_counts(cols, ref_names, ref_len, bin_width=5000, min_mapq=0, include_flags=0, require_flags=0, exclude_flags=0, dedup="none", emit_zero_bins=False,
               named_tids=None):
    """cols: {"FLAG", "tid", "POS" (1-based), "MAPQ", "PNEXT"} of the rows in file order.  named_tids: the contigs a region query names
    (None: no region, every contig).  -> {"n_rows", the seven columns as lists (chrom: bytes), "stats": the seven counters}"""
    check_params(bin_width, min_mapq, include_flags, require_flags, exclude_flags, dedup)
    ref_len = [int(x) for x in ref_len]
    if total_bins(ref_len, bin_width) > MAX_BINS:
        raise BinsError("too many bins")
    table = {}                                          # (tid, bin) -> [forward, reverse]
    st = dict.fromkeys(COUNTERS, 0)
    prev = None                                         # (tid, pos0, pnext) of the last row that passed steps 1 and 2
    n = len(cols["FLAG"])
    for i in range(n):
        flag, tid, pos0, mapq, pnext = int(cols["FLAG"][i]), int(cols["tid"][i]), int(cols["POS"][i]) - 1, int(cols["MAPQ"][i]), int(cols["PNEXT"][i])
        st["n_rows"] += 1
        # 1. flags
        if (flag & require_flags) != require_flags or (flag & exclude_flags) != 0 or (include_flags != 0 and (flag & include_flags) == 0):
            st["n_flag_filtered"] += 1
            continue
        # 2. placement
        if tid < 0 or pos0 < 0:
            st["n_unplaced"] += 1
            continue
        if pos0 >= ref_len[tid]:
            st["n_out_of_range"] += 1
            continue
        # 3. duplicate: the previous visible row, whatever became of it
        p, prev = prev, (tid, pos0, pnext)
        if dedup == "adjacent" and p is not None and p[0] == tid and p[1] == pos0 and ((flag & 1) == 0 or p[2] == pnext):
            st["n_duplicate"] += 1
            continue
        # 4. MAPQ
        if mapq < min_mapq:
            st["n_low_mapq"] += 1
            continue
        # 5. counted
        st["n_counted"] += 1
        table.setdefault((tid, pos0 // bin_width), [0, 0])[1 if flag & 0x10 else 0] += 1
    out = {k: [] for k in COLUMNS}
    for tid, length in enumerate(ref_len):
        zero_here = emit_zero_bins and (named_tids is None or tid in named_tids)
        for b in range((length + bin_width - 1) // bin_width) if zero_here else sorted(k[1] for k in table if k[0] == tid):
            fwd, rev = table.get((tid, b), (0, 0))
            name = ref_names[tid]
            out["chrom"].append(name.encode() if isinstance(name, str) else bytes(name))
            out["start"].append(b * bin_width)
            out["end"].append(min(b * bin_width + bin_width, length))
            out["bin_id"].append(b)
            out["count_total"].append(fwd + rev)
            out["count_fwd"].append(fwd)
            out["count_rev"].append(rev)
    out["n_rows"] = len(out["chrom"])
    out["stats"] = st
    return out
