"""Plain-Python model of the record stage's speculation rule (test tooling).

read_bam and read_bcf cut a batch of inflated bytes into 8 KiB tiles that count from the batch buffer's first byte.  One wave per tile takes
the FIRST offset in its tile that passes a cheap filter and whose next two hops pass it too (a hop that runs out of the stream ends the
test in the candidate's favour), and walks the record chain from there to the tile's end.  Tile 0 starts on the known first record, or --
in a shard that begins mid-stream -- keeps looking through the whole batch, from `spec_from` on.  The filter is written here from the
kernels' comments and from what sam.c (bam_read1, sam_read1_bam) and vcf.c (bcf_read1_core, bcf_record_check) test on the fixed-size core
of a record; nothing here calls the library.

The model answers, per tile: which offset the scan speculates, whether that is the tile's true first record, where the speculated chain
leaves the tile, and which of the filter's three evaluations read beyond the staged window (tile + 1 KiB halo; the kernels then read
global memory instead of LDS)."""
import struct
from bisect import bisect_left

TILE = 8192
HALO = 1024
OK, INVALID, INCOMPLETE = 0, 1, 2


def _u32(u, o):
    return struct.unpack_from("<I", u, o)[0]


def _i32(u, o):
    return struct.unpack_from("<i", u, o)[0]


class BamRule:
    """block_size, then the 32-byte core: refID pos l_read_name|mapq|bin n_cigar|flag l_seq next_refID next_pos tlen"""
    need = 300          # bytes behind a candidate that must lie inside the staged window for the LDS form of the filter (core + longest QNAME)

    def __init__(self, n_ref):
        self.n_ref = n_ref

    def _core(self, u, o):
        n = len(u)
        if n - o < 4:
            return INCOMPLETE, None
        bl = _i32(u, o)
        if bl < 32:
            return INVALID, None
        if n - o - 4 < 32:
            return INCOMPLETE, None
        tid, l_qname, n_cigar, l_seq, mtid = _i32(u, o + 4), u[o + 12], _u32(u, o + 16) & 0xffff, _i32(u, o + 20), _i32(u, o + 24)
        body = bl - 32
        if l_seq < 0 or l_qname < 1:
            return INVALID, None
        core = 4 * n_cigar + l_qname + (l_seq + 1) // 2 + l_seq
        if core > body:
            return INVALID, None
        return OK, (bl, tid, mtid, l_qname, body, core)

    def filter(self, u, o):
        """the speculation filter: (verdict, bytes to the next record)"""
        rc, f = self._core(u, o)
        if rc != OK:
            return rc, 0
        bl, tid, mtid, l_qname, body, core = f
        if not (-1 <= tid < self.n_ref and -1 <= mtid < self.n_ref):
            return INVALID, 0
        if body - core > 8 * core + 65536:
            return INVALID, 0
        if len(u) - o - 36 < body:
            return INCOMPLETE, 0
        if u[o + 36 + l_qname - 1] != 0:
            return INVALID, 0
        return OK, 4 + bl

    def hop(self, u, o):
        """a hop of the tile scan's chain walk: block_size alone (it must not stand still and must not leave the stream)"""
        n = len(u)
        if n - o < 4:
            return INCOMPLETE, 0
        bl = _i32(u, o)
        if bl < 32:
            return INVALID, 0
        if n - o - 4 < bl:
            return INCOMPLETE, 0
        return OK, 4 + bl

    def hop_strict(self, u, o):
        """a hop of the repair rounds' walk: bam_read1's tests on the core plus the header range test"""
        rc, f = self._core(u, o)
        if rc != OK:
            return rc, 0
        bl, tid, mtid, l_qname, body, core = f
        if len(u) - o - 36 < body:
            return INCOMPLETE, 0
        if not (-1 <= tid < self.n_ref and -1 <= mtid < self.n_ref):
            return INVALID, 0
        return OK, 4 + bl


class BcfRule:
    """l_shared l_indiv, then CHROM POS rlen QUAL n_info|n_allele<<16 n_sample|n_fmt<<24"""
    need = 32

    def __init__(self, n_ctg, n_smp):
        self.n_ctg, self.n_smp = n_ctg, n_smp

    def _hop(self, u, o, spec):
        n = len(u)
        if n - o < 32:
            return INCOMPLETE, 0
        l_shared, l_indiv, rid = _u32(u, o), _u32(u, o + 4), _i32(u, o + 8)
        if l_shared < 24:
            return INVALID, 0
        if rid < 0 or rid >= self.n_ctg:
            return INVALID, 0
        if (_u32(u, o + 24) >> 16) < 1:
            return INVALID, 0
        if spec:
            if l_shared > (1 << 28) or l_indiv > (1 << 30):
                return INVALID, 0
            x = _u32(u, o + 28)
            if (x >> 24) != 0 and (x & 0xffffff) != 0 and (x & 0xffffff) != self.n_smp:
                return INVALID, 0
        sz = 8 + l_shared + l_indiv
        if n - o < sz:
            return INCOMPLETE, 0
        return OK, sz

    def filter(self, u, o):
        return self._hop(u, o, True)

    def hop(self, u, o):
        return self._hop(u, o, False)

    hop_strict = hop


def speculate(rule, u, t, spec_from=0, skip=()):
    """the candidate tile t takes (None: none), and for the three filter evaluations that accepted it "lds" or "global".
    Tile 0 is asked only for a shard that starts mid-stream: it looks through the whole batch, from spec_from on, and passes over the
    offsets in `skip` (the retries of such a shard: record starts on the chains of failed candidates)."""
    n = len(u)
    tb = t * TILE
    te = min(tb + TILE, n)
    win = min(n - tb, TILE + HALO)
    lim = n if t == 0 else te
    for o in range(max(tb, spec_from) if t == 0 else tb, lim):
        if o in skip:
            continue
        paths = ["lds" if (o - tb) + rule.need <= win else "global"]
        rc, sz = rule.filter(u, o)
        if rc != OK:
            continue
        ok, o2 = True, o + sz
        for _ in range(2):
            paths.append("lds" if o2 >= tb and (o2 - tb) + rule.need <= win else "global")
            rc, sz = rule.filter(u, o2)
            if rc == INVALID:
                ok = False
                break
            if rc == INCOMPLETE:
                break
            o2 += sz
        if ok:
            return o, paths
    return None, []


def walk(rule, u, first, te, final_batch=True, hop=None):
    """the chain walk from `first` to the tile's end: (end_next, count, err)"""
    hop = hop or rule.hop
    o, cnt = first, 0
    while o < te:
        rc, sz = hop(u, o)
        if rc == INCOMPLETE:
            return o, cnt, int(final_batch and o < len(u))
        if rc == INVALID:
            return o, cnt, 1
        cnt += 1
        o += sz
    return o, cnt, 0


def tile_table(rule, stream, origin, starts, start0=None, final_batch=True, ulen=None):
    """One entry per tile of the batch whose buffer begins at stream[origin] (tiles count from the batch buffer's first byte: the batch's
    first block minus the carry) and holds ulen bytes (default: the rest of the stream).  starts: the true record offsets in the stream, in
    order.  start0: offset in the stream of the batch's known first record (None: tile 0 speculates too).  Entry: t, spec (speculated
    first record, offset in the batch, or None), true (the tile's true first record or None), mis (they differ), end_next / count / err of the
    speculated chain, paths."""
    u = bytes(stream[origin:] if ulen is None else stream[origin:origin + ulen])
    n = len(u)
    rel = [s - origin for s in starts if origin <= s < origin + n]
    out = []
    for t in range(max(1, (n + TILE - 1) // TILE)):
        tb, te = t * TILE, min(t * TILE + TILE, n)
        k = bisect_left(rel, tb)
        true = rel[k] if k < len(rel) and rel[k] < te else None
        if t == 0 and start0 is not None:
            spec, paths = start0 - origin, []
        else:
            spec, paths = speculate(rule, u, t)
        e = {"t": t, "true": true, "paths": paths, "first_abs": spec}
        if spec is not None and spec < te:
            e["spec"] = spec
            e["end_next"], e["count"], e["err"] = walk(rule, u, spec, te, final_batch)
        else:
            e["spec"] = None
            e["end_next"], e["count"], e["err"] = spec, 0, 0
        e["mis"] = e["spec"] != true
        out.append(e)
    return out


def mis_count(table):
    return sum(e["mis"] for e in table)


def longest_mis_run(table):
    best = run = 0
    for e in table:
        run = run + 1 if e["mis"] else 0
        best = max(best, run)
    return best


def correct_behind_mis(table):
    """correctly speculated tiles directly behind a mis-speculated one"""
    return sum(1 for a, b in zip(table, table[1:]) if a["mis"] and not b["mis"])


def chain_members(rule, u, first):
    """the record starts on the chain from `first` up to its break (or the end of the batch)"""
    out, o = [], first
    while o < len(u):
        rc, sz = rule.hop(u, o)
        if rc != OK:
            break
        out.append(o)
        o += sz
    return out


def shard_candidates(rule, stream, origin, starts, ulen=None, skip_members=True):
    """The candidates a shard that starts mid-stream at stream[origin] goes through before it reaches a true record: [(offset in the stream,
    "breaks" | "holds", offset where its chain breaks or None)], then the true record it settles on (None: none left).  A chain "holds" when
    it reaches the end of the batch: only the full validation of its records can refuse such a candidate.
    skip_members: as the driver does, a retry passes over every record start on the chain of a candidate that failed (it would walk the
    same hops to the same break); of a chain that holds only the candidate itself is passed over (the model has no full validation: it takes
    the candidate for the refused record).  Without it: every offset the plain three-deep rule would try."""
    u = bytes(stream[origin:] if ulen is None else stream[origin:origin + ulen])
    true = set(s - origin for s in starts)
    out, spec_from, skip = [], 0, set()
    while True:
        c, _ = speculate(rule, u, 0, spec_from, skip)
        if c is None or c in true:
            return out, (None if c is None else c + origin)
        en, _, err = walk(rule, u, c, len(u), True)
        en2, _, err2 = walk(rule, u, c, len(u), True, rule.hop_strict)
        assert (en, err) == (en2, err2), "the scan's walk and the repair rounds' walk leave this candidate's chain at different places"
        out.append((c + origin, "breaks" if err else "holds", en + origin if err else None))
        if skip_members and err:
            skip.update(chain_members(rule, u, c))
        spec_from = c + 1
