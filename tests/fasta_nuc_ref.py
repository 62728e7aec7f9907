"""fasta_nuc_ref.py -- CPU model of fasta_nuc (src/interval_udf.c:451-836), statement by statement.  TEST INFRASTRUCTURE ONLY.

fasta_nuc_bind: the argument checks and their messages.  fasta_nuc_init: init_fasta_region (fai_parse_region with flags 0, then
fai_adjust_region, whose every non-zero result is "invalid FASTA region"), the BED file and, with a region and a tabix index, its iterator.
fasta_nuc_scan: next_fasta_nuc_bed_interval / next_fasta_nuc_bin_interval, faidx_fetch_seq64(start, end - 1) (htslib faidx.c:914-983:
faidx_adjust_position with end_adjust = 1, then fai_retrieve), count_nucleotides, the two fractions.

On top of fasta_index_ref (the .fai, region parsing) and read_bed_ref (lines, meta lines, the tabix iterator's filter).  One deliberate
difference from the reference: a missing .fai is never built; it is the bind error.
"""
import fasta_index_ref as F
import hts_index_ref as R
import read_bed_ref as B
from region_oracle import _strtoll_whole, parse_region

COLUMNS = ["chrom", "start", "end", "pct_at", "pct_gc", "num_a", "num_c", "num_g", "num_t", "num_n", "num_other", "seq_len", "seq"]
ERR_PATH = "fasta_nuc requires a FASTA path"
ERR_ONE_OF = "fasta_nuc requires exactly one of bed_path or bin_width"
ERR_BIN_WIDTH = "fasta_nuc bin_width must be > 0"
ERR_OPEN_INDEX = "fasta_nuc: failed to open FASTA index"
ERR_LOAD_INDEX = "fasta_nuc: failed to load FASTA index"
ERR_REGION = "fasta_nuc: invalid FASTA region"
ERR_OPEN_BED = "fasta_nuc: failed to open BED file"
ERR_BED_ITER = "fasta_nuc: failed to create BED region iterator"


class NucError(Exception):
    pass


def adjust_position(length, end_adjust, beg, end):
    """faidx_adjust_position (faidx.c:936-947) for a sequence of `length` bases -> (beg, end)"""
    if end < beg:
        beg = end
    if beg < 0:
        beg = 0
    elif length <= beg:
        beg = length
    if end < 0:
        end = 0
    elif length <= end:
        end = length - end_adjust
    return beg, end


def adjust_region(length, beg, end):
    """fai_adjust_region (faidx.c:952-970) -> (flags, beg, end)"""
    ob, oe = beg, end
    beg, end = adjust_position(length, 0, beg, end)
    return (1 if ob != beg else 0) | (2 if oe != end and oe < F.POS_MAX else 0), beg, end


def retrieve(text, ent, beg, end):
    """fai_retrieve (faidx.c:716-796), read by read -> the bytes, or None where it returns NULL"""
    ln, off, blen, llen = ent
    if blen <= 0:
        return None
    pos = off + beg // blen * llen + beg % blen
    buf = bytearray()
    s = 0
    short = False

    def rd(k):                                       # bgzf_read_small at pos; the bytes land at s, later reads overwrite the terminator
        nonlocal pos, short
        got = text[pos:pos + k] if pos < len(text) else b""
        pos += len(got)
        buf[s:s + len(got)] = got
        if len(got) < k:
            short = True

    remaining = end - beg
    first_blen = blen - beg % blen
    if remaining <= first_blen:
        rd(remaining)
        return None if short else bytes(buf[:remaining])
    rd(llen - beg % blen)
    if short:
        return None
    s += first_blen
    remaining -= first_blen
    while remaining > blen:
        rd(llen)
        if short:
            return None
        s += blen
        remaining -= blen
    if remaining > 0:
        rd(remaining)
        if short:
            return None
        s += remaining
    return bytes(buf[:s])


def fetch_seq(text, tab, name, beg, end):
    """faidx_fetch_seq64(name, beg, end) with an INCLUSIVE end -> the bytes, or None (unknown name, line_blen 0, a file that ends early)"""
    if name not in tab:
        return None
    beg, end = adjust_position(tab[name][0], 1, beg, end)
    return retrieve(text, tab[name], beg, end + 1)


def count_nucleotides(seq):
    """count_nucleotides (interval_udf.c:629-643): toupper in the C locale touches a-z only"""
    a = c = g = t = n = other = 0
    for b in seq:
        u = b - 32 if 0x61 <= b <= 0x7A else b
        if u == 0x41:
            a += 1
        elif u == 0x43:
            c += 1
        elif u == 0x47:
            g += 1
        elif u == 0x54:
            t += 1
        elif u == 0x4E:
            n += 1
        else:
            other += 1
    return a, c, g, t, n, other


def init_region(names, tab, region):
    """init_fasta_region -> None (no region) or (tid, beg, end); NucError for a region the reference calls invalid"""
    if not region:
        return None
    r = F.parse_region(tab, region if isinstance(region, bytes) else region.encode())
    if r is None:                                    # (with flags 0 hts_parse_region returns the end of the string or NULL)
        raise NucError(ERR_REGION)
    name, beg, end = r
    flags, beg, end = adjust_region(tab[name][0], beg, end)
    if flags != 0:
        raise NucError(ERR_REGION)
    return names.index(name), beg, end


def bin_intervals(names, tab, bin_width, rg):
    """next_fasta_nuc_bin_interval, call by call"""
    if rg is not None:
        tid, nxt, cur_end = rg
    else:
        if not names:
            return
        tid, nxt, cur_end = 0, 0, tab[names[0]][0]
    while tid < len(names):
        seq_len = cur_end if rg is not None and tid == rg[0] else tab[names[tid]][0]
        if nxt >= seq_len:
            if rg is not None:
                return
            tid += 1
            if tid >= len(names):
                return
            nxt, cur_end = 0, tab[names[tid]][0]
            continue
        bin_end = min(nxt + bin_width, seq_len)
        yield names[tid], nxt, bin_end
        nxt = bin_end


def bed_intervals(bed_text, names, rg, region=None, bed_indexed=False, conf=R.CONF_BED):
    """next_fasta_nuc_bed_interval over the BED's lines; with bed_indexed the lines are those the tabix iterator of `region` returns"""
    q = None
    if region and bed_indexed:
        tnames = B.tabix_names(bed_text, conf)
        r = parse_region(tnames, region if isinstance(region, str) else region.decode())
        if r is None:
            raise NucError(ERR_BED_ITER)
        q = (tnames[r[0]], r[1], r[2])
    for no, ln in B.bed_lines(bed_text):
        if q is not None:
            if no <= conf[5] or ln[:1] == bytes([conf[4]]):
                continue
            iv = R.tbx_parse1(conf, ln.decode("latin-1"))
            if iv is None or iv[0] != q[0] or not (iv[2] > q[1] and q[2] > iv[1]):
                continue
        if B.is_meta(ln):
            continue
        f = ln.split(b"\t")
        if len(f) < 3:                               # get_field_span of a missing field is NULL: the line is passed over
            continue
        s = _strtoll_whole(f[1]) if f[1] else None
        e = _strtoll_whole(f[2]) if f[2] else None
        if s is None or e is None:
            continue
        if rg is not None:                           # bed_overlap_region
            if f[0] != names[rg[0]] or not (e > rg[1] and s < rg[2]):
                continue
        yield f[0], s, e


def row_of(text, tab, chrom, start, end):
    """one pass of fasta_nuc_scan's loop -> the 13 values, or None where it `continue`s"""
    seq_len = end - start
    a = c = g = t = n = other = 0
    pct_at = pct_gc = 0.0
    seq = None
    if seq_len > 0:
        seq = fetch_seq(text, tab, chrom, start, end - 1)
        if seq is None:
            return None
        seq_len = len(seq)
        a, c, g, t, n, other = count_nucleotides(seq)
        if seq_len > 0:
            pct_at = float(a + t) / float(seq_len)
            pct_gc = float(c + g) / float(seq_len)
    return [chrom, start, end, pct_at, pct_gc, a, c, g, t, n, other, seq_len, seq]


def rows_of(text, tab, intervals, include_seq=False, columns=None):
    ids = list(range(13 if include_seq else 12)) if columns is None else [c if isinstance(c, int) else COLUMNS.index(c) for c in columns]
    out = {"n_rows": 0}
    out.update({COLUMNS[i]: [] for i in ids})
    for chrom, start, end in intervals:
        v = row_of(text, tab, chrom, start, end)
        if v is None:
            continue
        if not include_seq:
            v[12] = None
        for i in ids:
            out[COLUMNS[i]].append(v[i])
        out["n_rows"] += 1
    return out


def fasta_nuc(fasta_text, fai, bed_text=None, bin_width=None, region=None, bed_indexed=False, include_seq=False, columns=None, fasta_path="x.fa", conf=R.CONF_BED):
    """bind + init + scan -> {"n_rows", column: list}.  fai: the .fai's bytes, or None for a missing one; bed_indexed: a tabix index of
    the BED was found (it matters only with a region)."""
    if not fasta_path:
        raise NucError(ERR_PATH)
    if (bed_text is None) == (bin_width is None):
        raise NucError(ERR_ONE_OF)
    if bin_width is not None and bin_width <= 0:
        raise NucError(ERR_BIN_WIDTH)
    if fai is None:
        raise NucError(ERR_OPEN_INDEX)
    names, tab = F.read(fai)
    rg = init_region(names, tab, region)
    if bed_text is not None:
        ivs = bed_intervals(bed_text, names, rg, region, bed_indexed, conf)
    else:
        ivs = bin_intervals(names, tab, bin_width, rg)
    return rows_of(fasta_text, tab, ivs, include_seq, columns)
