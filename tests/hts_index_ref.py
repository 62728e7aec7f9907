"""A plain record-by-record model of htslib's index builder (test tooling: no GPU, no project code).

It follows hts.c as it reads -- hts_idx_init, hts_idx_push, insert_to_b, insert_to_l, update_loff, compress_binning, hts_idx_finish,
hts_adjust_csi_settings -- with a dict per sequence (bin -> list of (u, v)) and a list for the linear index.  One push() per record, then
finish().  Nothing here is restructured into runs or extents: the value of the model is that it is the other algorithm.

Row sources turn files into the arguments of push(): BAM records out of BGZF bytes (sam_index, sam.c), BCF records (bcf_index, vcf.c) and
tabix text lines (tbx_index / tbx_parse1, tbx.c).  The virtual offset behind a record follows bgzf_read / bgzf_getline (bgzf.c): a read that
ends exactly at the end of a block leaves the reader at the address of whatever follows that block, with in-block offset 0; at the end of
the file the failing read does not move the reader any more, so the final offset is the address behind the last block that holds data.

Every object adds to `tags` (a set of strings) when it goes through a branch worth knowing about; tests/test_gpu_index_writer.py asserts
that its inputs reach all of them.
"""
import gzip
import struct
import zlib

NONE = 0xFFFFFFFFFFFFFFFF
MIN_MARKER_DIST = 0x10000           # HTS_MIN_MARKER_DIST
WAVE_EDGES = (63, 64, 65, 255, 256, 257)


class IndexBuildError(Exception):
    pass


class UnsortedPositions(IndexBuildError):
    pass


class BlocksNotContinuous(IndexBuildError):
    pass


class NoCoorNotLast(IndexBuildError):
    pass


class EndBeforeBegin(IndexBuildError):
    pass


class BeyondMaxPos(IndexBuildError):
    pass


def bin_first(l):
    return ((1 << (3 * l)) - 1) // 7


def bin_parent(b):
    return (b - 1) >> 3


def bin_level(b):
    l = 0
    while b >= bin_first(l + 1):
        l += 1
    return l


def bin_bot(b, n_lvls):
    l = bin_level(b)
    return (b - bin_first(l)) << ((n_lvls - l) * 3)


def bin_maxpos(min_shift, n_lvls):
    return 1 << (min_shift + 3 * n_lvls)


def reg2bin(beg, end, min_shift, n_lvls):
    """hts_reg2bin (htslib/hts.h)"""
    s, t = min_shift, ((1 << (3 * n_lvls)) - 1) // 7
    end -= 1
    l = n_lvls
    while l > 0:
        if beg >> s == end >> s:
            return t + (beg >> s)
        l -= 1
        s += 3
        t -= 1 << (3 * l)
    return 0


def adjust_csi_settings(max_len_in, min_shift, n_lvls):
    """hts_adjust_csi_settings -> (min_shift, n_lvls)"""
    max_len = max_len_in + 256
    if max_len <= bin_maxpos(min_shift, 9):
        maxpos = bin_maxpos(min_shift, n_lvls)
        while max_len > maxpos:
            n_lvls += 1
            maxpos *= 8
    else:
        n_lvls = 9
        maxpos = bin_maxpos(min_shift, n_lvls)
        while max_len > maxpos:
            min_shift += 1
            maxpos *= 2
    return min_shift, n_lvls


class HtsIdx:
    """hts_idx_t and the functions that fill it.  fmt: "bai", "csi" or "tbi"."""

    def __init__(self, n, fmt, offset0, min_shift, n_lvls, tags=None):
        self.fmt, self.min_shift, self.n_lvls = fmt, min_shift, n_lvls
        self.n_bins = ((1 << (3 * n_lvls + 3)) - 1) // 7
        self.n = n
        self.bidx = [None] * n                    # per sequence: None or {bin: [[u, v], ...]}
        self.lidx = [[] for _ in range(n)]
        self.loff = [dict() for _ in range(n)]
        self.n_no_coor = 0
        self.save_tid = self.last_tid = -1
        self.save_bin = self.last_bin = 0xFFFFFFFF
        self.save_off = self.last_off = self.off_beg = self.off_end = offset0
        self.last_coor = 0xFFFFFFFF
        self.n_mapped = self.n_unmapped = 0
        self.finished = False
        self.tags = tags if tags is not None else set()
        self.tags.add("fmt_" + fmt)
        if fmt != "bai":
            self.tags.add("min_shift_%d" % min_shift)
            self.tags.add("depth_%d" % n_lvls)
        self.row = 0
        self.row_tid = []
        self._ew_max, self._ew_prev, self._prev_inside = -1, -1, False

    def meta_bin(self):
        return self.n_bins + 1

    def _grow(self, tid):
        while self.n < tid + 1:
            self.bidx.append(None)
            self.lidx.append([])
            self.loff.append({})
            self.n += 1

    def _insert_to_b(self, tid, b, beg, end):
        self.bidx[tid].setdefault(b, []).append([beg, end])

    def _insert_to_l(self, tid, beg_, end_, offset):
        l = self.lidx[tid]
        beg, end = beg_ >> self.min_shift, (end_ - 1) >> self.min_shift
        if len(l) < end + 1:
            l.extend([NONE] * (end + 1 - len(l)))
        for i in range(beg, end + 1):
            if l[i] == NONE:
                l[i] = offset
        if end - beg + 1 >= 64:
            self.tags.add("read_covers_64_windows")
        return end

    def _edge(self, what):
        if self.row in WAVE_EDGES:
            self.tags.add("%s_at_row_%d" % (what, self.row))

    def push(self, tid, beg, end, offset, is_mapped):
        """hts_idx_push; offset: the virtual offset behind the record"""
        where = "wave_edge" if self.row % 64 == 0 else "in_wave"
        if tid < 0:
            beg, end = -1, 0
        maxpos = bin_maxpos(self.min_shift, self.n_lvls)
        if not (tid < 0 or (beg <= maxpos and end <= maxpos)):
            self.tags.add("err_maxpos_" + self.fmt)
            raise BeyondMaxPos("Region %d..%d cannot be stored in a %s index" % (beg, end, self.fmt))
        self._grow(tid)
        if self.finished:
            return
        if self.last_tid != tid or (self.last_tid >= 0 and tid < 0):
            if tid >= 0 and self.n_no_coor:
                self.tags.add("err_nocoor")
                raise NoCoorNotLast("NO_COOR reads not in a single block at the end %d %d" % (tid, self.last_tid))
            if tid >= 0 and self.bidx[tid] is not None:
                self.tags.add("err_not_continuous")
                raise BlocksNotContinuous("Chromosome blocks not continuous")
            self._edge("tid_change")
            self.last_tid = tid
            self.last_bin = 0xFFFFFFFF
            self._ew_max, self._ew_prev, self._prev_inside = -1, -1, False
        elif tid >= 0 and self.last_coor > beg:
            self.tags.add("err_unsorted_" + where)
            raise UnsortedPositions("Unsorted positions on sequence #%d: %d followed by %d" % (tid + 1, self.last_coor + 1, beg + 1))
        if end < beg:
            self.tags.add("err_end_lt_beg")
            raise EndBeforeBegin("Invalid record on sequence #%d: end %d < begin %d" % (tid + 1, end, beg + 1))
        if tid >= 0:
            if self.bidx[tid] is None:
                self.bidx[tid] = {}
            if beg < 0:
                beg = 0
                self.tags.add("pos_clamped")
            if end <= 0:
                end = 1
            ew = self._insert_to_l(tid, beg, end, self.last_off)
            # (what the row passes of the writer have to get right: a read inside an earlier, longer one, then one that reaches beyond it)
            if self._prev_inside and self._ew_prev < ew <= self._ew_max:
                self.tags.add("lin_long_short_medium")
            self._prev_inside = ew < self._ew_max
            self._ew_prev = ew
            self._ew_max = max(self._ew_max, ew)
        else:
            self.n_no_coor += 1
        b = reg2bin(beg, end, self.min_shift, self.n_lvls)
        if self.last_bin != b:
            if self.last_bin != 0xFFFFFFFF:
                self._edge("bin_change")
            if self.save_bin != 0xFFFFFFFF:
                self._insert_to_b(self.save_tid, self.save_bin, self.save_off, self.last_off)
            if self.last_bin == 0xFFFFFFFF and self.save_bin != 0xFFFFFFFF:
                self.off_end = self.last_off
                self._insert_to_b(self.save_tid, self.meta_bin(), self.off_beg, self.off_end)
                self._insert_to_b(self.save_tid, self.meta_bin(), self.n_mapped, self.n_unmapped)
                self.n_mapped = self.n_unmapped = 0
                self.off_beg = self.off_end
            self.save_off = self.last_off
            self.save_bin = self.last_bin = b
            self.save_tid = tid
        if is_mapped:
            self.n_mapped += 1
        else:
            self.n_unmapped += 1
        self.last_off = offset
        self.last_coor = beg
        self.row_tid.append(tid)
        self.row += 1

    def _update_loff(self, i):
        l = self.lidx[i]
        for k in range(len(l) - 2, -1, -1):
            if l[k] == NONE:
                l[k] = l[k + 1]
                self.tags.add("lin_empty_window_filled_from_right")
        if self.bidx[i] is None:
            return
        for b in self.bidx[i]:
            if b < self.n_bins:
                bot = bin_bot(b, self.n_lvls)
                self.loff[i][b] = l[bot] if bot < len(l) else 0
            else:
                self.loff[i][b] = 0

    def _compress_binning(self, i):
        bidx = self.bidx[i]
        if bidx is None:
            return
        own_small = {b: (c[-1][1] >> 16) - (c[0][0] >> 16) < MIN_MARKER_DIST for b, c in bidx.items() if b < self.n_bins}
        got, chain = set(), {}
        for l in range(self.n_lvls, 0, -1):
            start = bin_first(l)
            for b in list(bidx):
                if b not in bidx or b >= self.n_bins or b < start:
                    continue
                p = bidx[b]
                if l < self.n_lvls and len(p) > 1:
                    p.sort(key=lambda c: c[0])
                lvl = bin_level(b)
                if (p[-1][1] >> 16) - (p[0][0] >> 16) < MIN_MARKER_DIST:
                    par = bin_parent(b)
                    if par not in bidx:
                        if lvl == l:
                            self.tags.add("bin_stays_parent_absent")
                        continue
                    bidx[par].extend(p)
                    del bidx[b]
                    self.tags.add("bin_joins_parent")
                    got.add(par)
                    chain[par] = max(chain.get(par, 0), chain.get(b, 0) + 1)
                    if par == 0 and chain[par] >= 3:
                        self.tags.add("join_chain_3_levels_into_bin0")
                elif lvl == l:
                    self.tags.add("bin_stays_64k_level_%s" % ("deepest" if l == self.n_lvls else "mid"))
                    self.tags.add("bin_stays_64k_at_level_%d_of_%s" % (l, self.fmt))
                    if l < self.n_lvls and b in got and own_small[b]:
                        self.tags.add("mid_bin_stays_widened_by_children")
        if 0 in bidx:
            bidx[0].sort(key=lambda c: c[0])
        for b, p in bidx.items():
            if b >= self.n_bins:
                continue
            m = 0
            for k in range(1, len(p)):
                if p[m][1] >> 16 >= p[k][0] >> 16:
                    self.tags.add("chunks_coalesced_same_block")
                    if p[m][1] < p[k][1]:
                        p[m][1] = p[k][1]
                else:
                    self.tags.add("chunks_not_coalesced")
                    m += 1
                    p[m] = p[k]
            del p[m + 1:]

    def finish(self, final_offset):
        """hts_idx_finish"""
        if self.finished:
            return
        if self.save_tid >= 0:
            self._insert_to_b(self.save_tid, self.save_bin, self.save_off, final_offset)
            self._insert_to_b(self.save_tid, self.meta_bin(), self.off_beg, final_offset)
            self._insert_to_b(self.save_tid, self.meta_bin(), self.n_mapped, self.n_unmapped)
        for i in range(self.n):
            self._update_loff(i)
            self._compress_binning(i)
        self.finished = True
        have = [i for i in range(self.n) if self.bidx[i] is not None]
        if have and any(self.bidx[i] is None for i in range(have[0], have[-1])):
            self.tags.add("empty_sequence_between")
        self._row_tags()

    def _row_tags(self):
        n = len(self.row_tid)
        if n in (1,) + WAVE_EDGES:
            self.tags.add("nrows_%d" % n)
        for w in range(0, n, 64):
            t = self.row_tid[w:w + 64]
            if len(t) < 64:
                self.tags.add("partial_last_wave")
            kinds = len(set(t))
            if kinds == 1 and len(t) == 64 and t[0] >= 0:
                self.tags.add("wave_one_sequence")
            if len(set(x for x in t if x >= 0)) >= 3:
                self.tags.add("wave_three_sequences")
            if t[0] >= 0 and t[-1] < 0:
                self.tags.add("wave_placed_to_unplaced")

    # ---- the finished index in the shape the tests' parsers return ----
    def parsed_bai(self):
        """like _parse_bai: ([({bin: [(u, v)]}, linear index)], n_no_coor)"""
        refs = []
        for i in range(self.n):
            bins = {b: [tuple(c) for c in p] for b, p in (self.bidx[i] or {}).items()}
            refs.append((bins, list(self.lidx[i])))
        return refs, self.n_no_coor

    def parsed_csi(self, l_aux=0):
        """like _parse_csi: (min_shift, depth, l_aux, [{bin: (loff, [(u, v)])}], n_no_coor)"""
        refs = []
        for i in range(self.n):
            refs.append({b: (self.loff[i][b], [tuple(c) for c in p]) for b, p in (self.bidx[i] or {}).items()})
        return self.min_shift, self.n_lvls, l_aux, refs, self.n_no_coor

    def parsed_tabix(self, conf, names):
        """like parse_tabix"""
        out = {"kind": "tbi" if self.fmt == "tbi" else "csi", "min_shift": self.min_shift, "depth": self.n_lvls, "conf": tuple(conf),
               "names": list(names), "n_no_coor": self.n_no_coor}
        csi = self.fmt != "tbi"
        out["refs"] = [{b: (self.loff[i][b] if csi else 0, [tuple(c) for c in p]) for b, p in (self.bidx[i] or {}).items()} for i in range(self.n)]
        out["lin"] = [] if csi else [list(l) for l in self.lidx]
        return out

    def parsed(self, conf=None, names=None, l_aux=0):
        if conf is not None:
            return self.parsed_tabix(conf, names)
        return self.parsed_bai() if self.fmt == "bai" else self.parsed_csi(l_aux)


# ---- BGZF: blocks, the inflated stream, the reader's virtual offsets ---------------------------------------------------------------------
class Bgzf:
    def __init__(self, data, tags=None):
        self.tags = tags if tags is not None else set()
        self.coff, self.clen, self.ustart, self.ulen = [], [], [], []
        parts, p, u = [], 0, 0
        while p < len(data):
            assert data[p:p + 4] == b"\x1f\x8b\x08\x04", "not a BGZF block"
            xlen = struct.unpack_from("<H", data, p + 10)[0]
            q, bsize = p + 12, None
            while q < p + 12 + xlen:
                si1, si2, slen = struct.unpack_from("<BBH", data, q)
                if (si1, si2) == (66, 67):
                    bsize = struct.unpack_from("<H", data, q + 4)[0] + 1
                q += 4 + slen
            raw = zlib.decompress(data[p + 12 + xlen:p + bsize - 8], -15)
            self.coff.append(p); self.clen.append(bsize); self.ustart.append(u); self.ulen.append(len(raw))
            parts.append(raw)
            u += len(raw)
            p += bsize
        self.size = len(data)
        self.raw = b"".join(parts)
        self.data_blocks = [k for k in range(len(self.coff)) if self.ulen[k]]
        self._starts = [self.ustart[k] for k in self.data_blocks]
        last = self.data_blocks[-1] if self.data_blocks else -1
        if any(self.ulen[k] == 0 for k in range(last)):
            self.tags.add("empty_block_mid_file")
        trailing = len(self.coff) - 1 - last
        self.tags.add("final_eof_absent" if trailing == 0 else "final_eof_present" if trailing == 1 else "final_several_empty_blocks")
        if len(self.coff) > 16384:
            self.tags.add("more_than_16384_blocks")

    def block_of(self, u):
        """index (into data_blocks) of the block holding inflated byte u"""
        import bisect
        return bisect.bisect_right(self._starts, u) - 1

    def tell(self, u):
        """bgzf_tell after the reader has consumed the inflated stream up to u (u > 0)"""
        k = self.data_blocks[self.block_of(u - 1)]
        if u == self.ustart[k] + self.ulen[k]:
            return (self.coff[k] + self.clen[k]) << 16
        return (self.coff[k] << 16) | (u - self.ustart[k])

    def final(self):
        """bgzf_tell after the read that found the end of the file"""
        if not self.data_blocks:
            return 0
        k = self.data_blocks[-1]
        return (self.coff[k] + self.clen[k]) << 16

    def note_record(self, u0, u1, first):
        k0, k1 = self.block_of(u0), self.block_of(u1 - 1)
        if k1 - k0 >= 2:
            self.tags.add("record_spans_3_blocks")
        kb = self.data_blocks[k1]
        if u1 == self.ustart[kb] + self.ulen[kb] and k1 + 1 < len(self.data_blocks):
            self.tags.add("record_ends_at_block_end")
        if first:
            self.tags.add("first_record_at_offset_0" if u0 == self.ustart[self.data_blocks[k0]] else "first_record_at_nonzero_offset")


CIGAR_REF = {0, 2, 3, 7, 8}          # M D N = X consume the reference (bam_cigar2rlen)


def bam_rows(data, tags=None):
    """-> dict(refs [(name, len)], rows [(tid, beg, end, offset_after, is_mapped)], offset0, final, batch_rows)"""
    tags = tags if tags is not None else set()
    z = Bgzf(data, tags)
    raw = z.raw
    assert raw[:4] == b"BAM\x01"
    l_text = struct.unpack_from("<i", raw, 4)[0]
    p = 8 + l_text
    n_ref = struct.unpack_from("<i", raw, p)[0]; p += 4
    refs = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", raw, p)[0]; p += 4
        name = raw[p:p + l_name - 1].decode(); p += l_name
        refs.append((name, struct.unpack_from("<I", raw, p)[0])); p += 4
    offset0 = z.tell(p)
    rows, first = [], True
    first_batch_rows = None
    while p < len(raw):
        bs = struct.unpack_from("<i", raw, p)[0]
        tid, pos, l_qn, _mq, _bin, n_cig, flag = struct.unpack_from("<iiBBHHH", raw, p + 4)
        cg = p + 36 + l_qn
        rlen = 0
        if not flag & 4:
            for j in range(n_cig):
                op = struct.unpack_from("<I", raw, cg + 4 * j)[0]
                tags.add("cigar_op_" + "MIDNSHP=XB"[op & 15])
                if (op & 15) in CIGAR_REF:
                    rlen += op >> 4
            if n_cig == 0 and tid >= 0:
                tags.add("mapped_no_cigar")
        elif tid >= 0 and n_cig:
            tags.add("placed_unmapped_with_cigar")
        if rlen == 0:
            rlen = 1
        end_u = p + 4 + bs
        z.note_record(p, end_u, first)
        # the rows of a scan's first batch: the records that end inside the 16384 blocks that begin with the first record's block
        if first:
            cut = z.data_blocks[z.block_of(p)] + 16384
        if first_batch_rows is None and len(z.coff) > cut and end_u > z.ustart[cut]:
            first_batch_rows = len(rows)
        first = False
        if tid >= 0 and tid < n_ref and pos > refs[tid][1] + (1 << 20):
            tags.add("read_1mb_beyond_header_length")
        rows.append((tid, pos, pos + rlen, z.tell(end_u), not flag & 4))
        p = end_u
    if any(l > 1 << 29 for _, l in refs):
        tags.add("ref_len_gt_2^29")
    return {"refs": refs, "rows": rows, "offset0": offset0, "final": z.final(), "first_batch_rows": first_batch_rows, "n_blocks": len(z.coff)}


def _feed(idx, src, tags):
    if src.get("first_batch_rows"):
        k = src["first_batch_rows"]
        a, b = src["rows"][k - 1], src["rows"][k]
        same_bin = reg2bin(max(a[1], 0), a[2], idx.min_shift, idx.n_lvls) == reg2bin(max(b[1], 0), b[2], idx.min_shift, idx.n_lvls)
        if a[0] == b[0] and a[0] >= 0 and same_bin:
            tags.add("run_straddles_batch_boundary")
        if a[0] != b[0] and a[0] >= 0 and b[0] >= 0:
            tags.add("tid_change_at_batch_boundary")
    batch2 = src.get("first_batch_rows")
    for i, r in enumerate(src["rows"]):
        try:
            idx.push(*r)
        except IndexBuildError:
            if batch2 is not None and i == batch2:
                tags.add("err_at_batch_boundary")
            raise
    idx.finish(src["final"])
    return idx


def bam_index(data, min_shift=0, tags=None):
    """sam_index (sam.c): BAI for min_shift <= 0, else CSI with the depth the longest reference asks for"""
    tags = tags if tags is not None else set()
    src = bam_rows(data, tags)
    if min_shift > 0:
        max_len = max([l for _, l in src["refs"]], default=0)
        min_shift, n_lvls = adjust_csi_settings(max_len, min_shift, 0)
        fmt = "csi"
    else:
        min_shift, n_lvls, fmt = 14, 5, "bai"
    idx = HtsIdx(len(src["refs"]), fmt, src["offset0"], min_shift, n_lvls, tags)
    return _feed(idx, src, tags)


def sam_text_index(data, min_shift=0, tags=None):
    """sam_index over bgzipped SAM text: the same rows, read line by line (bgzf_getline)"""
    tags = tags if tags is not None else set()
    z = Bgzf(data, tags)
    raw, p, refs, rows = z.raw, 0, [], []
    while p < len(raw) and raw[p:p + 1] == b"@":
        q = raw.index(b"\n", p)
        f = raw[p:q].decode("latin-1").split("\t")
        if f[0] == "@SQ":
            kv = dict(x.split(":", 1) for x in f[1:])
            refs.append((kv["SN"], int(kv["LN"])))
        p = q + 1
    offset0 = z.tell(p) if p else 0
    names = {n: i for i, (n, _) in enumerate(refs)}
    while p < len(raw):
        q = raw.find(b"\n", p)
        nxt = len(raw) if q < 0 else q + 1
        f = raw[p:nxt].decode("latin-1").rstrip("\r\n").split("\t")
        flag, tid, pos = int(f[1]), names.get(f[2], -1), int(f[3]) - 1
        rlen, num = 0, ""
        for ch in f[5] if f[5] != "*" else "":
            if ch.isdigit():
                num += ch
            else:
                if ch in "MDN=X" and not flag & 4:
                    rlen += int(num)
                num = ""
        rows.append((tid, pos, pos + (rlen or 1), z.tell(nxt), not flag & 4))
        p = nxt
    if min_shift > 0:
        min_shift, n_lvls = adjust_csi_settings(max([l for _, l in refs], default=0), min_shift, 0)
        fmt = "csi"
    else:
        min_shift, n_lvls, fmt = 14, 5, "bai"
    idx = HtsIdx(len(refs), fmt, offset0, min_shift, n_lvls, tags)
    return _feed(idx, {"rows": rows, "final": z.final()}, tags)


# ---- BCF -----------------------------------------------------------------------------------------------------------------------------------
def _contigs(header_text):
    """[(name, length or 0)] of the ##contig lines, in order"""
    out = []
    for line in header_text.split("\n"):
        if line.startswith("##contig=<"):
            body = line[len("##contig=<"):].rstrip(">")
            kv = dict(f.split("=", 1) for f in body.split(",") if "=" in f)
            out.append((kv.get("ID"), int(kv.get("length", "0") or 0)))
    return out


def bcf_index(data, min_shift=14, tags=None):
    """bcf_index (vcf.c): CSI; rows (rid, pos, pos + rlen)"""
    tags = tags if tags is not None else set()
    tags.add("src_bcf")
    z = Bgzf(data, tags)
    raw = z.raw
    assert raw[:5] == b"BCF\x02\x02"
    l_text = struct.unpack_from("<I", raw, 5)[0]
    ctg = _contigs(raw[9:9 + l_text].rstrip(b"\0").decode())
    max_len = max([l for _, l in ctg], default=0) or (1 << 31) - 1
    min_shift, n_lvls = adjust_csi_settings(max_len, min_shift, 0)
    p = 9 + l_text
    idx = HtsIdx(len(ctg), "csi", z.tell(p), min_shift, n_lvls, tags)
    first = True
    while p < len(raw):
        l_shared, l_indiv, rid, pos, rlen = struct.unpack_from("<IIiii", raw, p)
        end_u = p + 8 + l_shared + l_indiv
        z.note_record(p, end_u, first)
        first = False
        idx.push(rid, pos, pos + rlen, z.tell(end_u), True)
        p = end_u
    idx.finish(z.final())
    return idx


# ---- tabix text ----------------------------------------------------------------------------------------------------------------------------
TBX_GENERIC, TBX_SAM, TBX_VCF, TBX_UCSC = 0, 1, 2, 0x10000
CONF_GFF = (0, 1, 4, 5, ord("#"), 0)
CONF_BED = (0x10000, 1, 2, 3, ord("#"), 0)
CONF_SAM = (1, 3, 4, 0, ord("@"), 0)
CONF_VCF = (2, 1, 2, 0, ord("#"), 0)


def _strtoll(s):
    """(value, number of characters used) of a leading base-10 integer"""
    k = 0
    while k < len(s) and s[k] in " \t":
        k += 1
    j = k
    if j < len(s) and s[j] in "+-":
        j += 1
    d = j
    while j < len(s) and s[j].isdigit():
        j += 1
    if j == d:
        return 0, 0
    return int(s[k:j]), j


def _svlen_alt(a):
    return a.startswith("<") and a[1:4] in ("DEL", "DUP", "CNV", "INV") and (a[4:5] in (">", ":"))


def tbx_parse1(conf, line):
    """tbx_parse1 (tbx.c) -> (name, beg, end) or None"""
    preset, sc, bc, ec = conf[0], conf[1], conf[2], conf[3]
    kind = preset & 0xFFFF
    f = line.split("\t")
    name, beg, end = None, -1, -1
    reflen = svlen = fmtlen = 0
    alts, getlen, lenpos = [], False, -1
    for k, x in enumerate(f):
        col = k + 1
        if col == sc:
            name = x
        elif col == bc:
            beg, used = _strtoll(x)
            if bc <= ec:
                end = beg
            if not used:
                return None
            if not preset & TBX_UCSC:
                beg -= 1
            elif bc <= ec:
                end += 1
            if beg < 0:
                beg = 0
            if end < 1:
                end = 1
        elif kind == TBX_GENERIC:
            if col == ec:
                end, used = _strtoll(x)
                if not used:
                    return None
        elif kind == TBX_SAM:
            if col == 6:
                l, num = 0, ""
                for ch in x:
                    if ch.isdigit():
                        num += ch
                    else:
                        if ch.upper() in "MDN" and num:
                            l += int(num)
                        num = ""
                end = beg + (l or 1)
        elif kind == TBX_VCF:
            if col == 4:
                if x:
                    end = beg + len(x)
                reflen = len(x)
            elif col == 5:
                alts = x.split(",")
                getlen = any(a in ("<*>", "<NON_REF>") for a in alts if not _svlen_alt(a))
            elif col == 8:
                at = 4 if x.startswith("END=") else (x.find(";END=") + 5 if ";END=" in x else -1)
                if at >= 0 and x[at:at + 1] != ".":
                    e, _ = _strtoll(x[at:])
                    if e > beg:
                        end = e
                at = 6 if x.startswith("SVLEN=") else (x.find(";SVLEN=") + 7 if ";SVLEN=" in x else -1)
                if at >= 0:
                    vals = x[at:].split(";")[0].split(",")
                    for d, v in enumerate(vals[:len(alts)]):
                        t = abs(_strtoll(v)[0]) if _svlen_alt(alts[d]) else 1
                        svlen = max(svlen, t)
            elif col == 9 and getlen:
                keys = x.split(":")
                lenpos = keys.index("LEN") if "LEN" in keys else -1
                if lenpos < 0:
                    break
            elif col > 9 and getlen and lenpos >= 0:
                parts = x.split(":")
                if lenpos < len(parts):
                    fmtlen = max(fmtlen, _strtoll(parts[lenpos])[0])
    if kind == TBX_VCF:
        end = max(end, max(reflen, svlen, fmtlen) + beg)
    if name is None or beg < 0 or end < 0:
        return None
    return name, beg, end


def tabix_index(data, conf, min_shift=0, tags=None):
    """tbx_index (tbx.c) over bgzipped text -> (HtsIdx, names in order of first appearance)"""
    tags = tags if tags is not None else set()
    tags.add("src_text_%s_%s" % ({0: "generic", 1: "sam", 2: "vcf"}[conf[0] & 0xFFFF], "csi" if min_shift > 0 else "tbi"))
    z = Bgzf(data, tags)
    raw = z.raw
    meta, skip = bytes([conf[4]]), conf[5]
    if min_shift > 0:
        n_lvls, fmt = (31 - min_shift + 2) // 3, "csi"
    else:
        min_shift, n_lvls, fmt = 14, 5, "tbi"
    idx, names, tids = None, [], {}
    last_off, max_ref_len, lineno, p, first = 0, 0, 0, 0, True
    while p < len(raw):
        q = raw.find(b"\n", p)
        nxt = len(raw) if q < 0 else q + 1
        line = raw[p:len(raw) if q < 0 else q]
        if line.endswith(b"\r"):
            line = line[:-1]
        lineno += 1
        off = z.tell(nxt)
        if line[:1] == meta and fmt == "csi":
            s = line.decode("latin-1")
            if conf[0] == TBX_SAM and s.startswith("@SQ") and "\tLN:" in s:
                max_ref_len = max(max_ref_len, _strtoll(s[s.index("\tLN:") + 4:])[0])
            if conf[0] == TBX_VCF and s.startswith("##contig") and "length" in s[8:]:
                max_ref_len = max(max_ref_len, _strtoll(s[s.index("length", 8) + 6:].lstrip(" ="))[0])
        if lineno <= skip or line[:1] == meta:
            last_off = off
            p = nxt
            continue
        if idx is None:
            if fmt == "csi":
                if max_ref_len:
                    min_shift, n_lvls = adjust_csi_settings(max_ref_len, min_shift, n_lvls)
                else:
                    n_lvls = 9 if min_shift < 10 else 9 - (min_shift - 10) // 3 if min_shift < 25 else 4
            idx = HtsIdx(0, fmt, last_off, min_shift, n_lvls, tags)
        iv = tbx_parse1(conf, line.decode("latin-1"))
        if iv is None:
            raise IndexBuildError("Failed to parse line %d" % lineno)
        z.note_record(p, nxt, first)
        first = False
        tid = tids.setdefault(iv[0], len(tids))
        if tid == len(names):
            names.append(iv[0].encode("latin-1"))
        idx.push(tid, iv[1], iv[2], off, True)
        p = nxt
    if idx is None:
        idx = HtsIdx(0, fmt, last_off, min_shift, n_lvls, tags)
    idx.finish(z.final())
    return idx, names


def maybe_gunzip(d):
    return gzip.decompress(d) if d[:2] == b"\x1f\x8b" else d
