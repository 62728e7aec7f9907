"""The rules of the reference's sequence, CIGAR and flag functions (src/kmer_udf.c) restated in Python: the model the device functions
are compared with.  Strings are bytes, NULL is None.  Every function names the lines it restates; tests/test_kmer_udf_ref.py pins the
model on the reference's published statements (test/sql/duckhts.test:624-782, recorded in tests/golden/kmer_udf_statements.json)."""

_COMP = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A"), ord("N"): ord("N")}
_IUPAC = {"A": 1, "C": 2, "G": 4, "T": 8, "M": 3, "R": 5, "S": 6, "V": 7, "W": 9, "Y": 10, "H": 11, "K": 12, "D": 13, "B": 14, "N": 15}      # :109-128
_BASE_OF = {v: ord(k) for k, v in _IUPAC.items()}                                                                                             # :130-149
CIGAR_OPS = b"MIDNSHP=X"
FLAG_FIELDS = ["is_paired", "is_proper_pair", "is_unmapped", "is_next_segment_unmapped", "is_reverse_complemented", "is_next_segment_reverse_complemented",
               "is_first_segment", "is_last_segment", "is_secondary", "is_qc_fail", "is_duplicate", "is_supplementary"]                      # :21-34, masks :36-49 = bit 0 .. 11
# the registration order of :1223-1254: (name, parameter types, return type)
_FLAG_STRUCT = "STRUCT(" + ", ".join(f + " BOOLEAN" for f in FLAG_FIELDS) + ")"
REGISTERED = [("seq_revcomp", ["VARCHAR"], "VARCHAR"), ("seq_canonical", ["VARCHAR"], "VARCHAR"), ("seq_hash_2bit", ["VARCHAR"], "UBIGINT"),
              ("seq_encode_4bit", ["VARCHAR"], "UTINYINT[]"), ("seq_decode_4bit", ["UTINYINT[]"], "VARCHAR"), ("seq_gc_content", ["VARCHAR"], "DOUBLE"),
              ("seq_kmers", ["VARCHAR", "BIGINT"], "TABLE(pos BIGINT, kmer VARCHAR)"),
              ("cigar_has_soft_clip", ["VARCHAR"], "BOOLEAN"), ("cigar_has_hard_clip", ["VARCHAR"], "BOOLEAN"), ("cigar_left_soft_clip", ["VARCHAR"], "BIGINT"),
              ("cigar_right_soft_clip", ["VARCHAR"], "BIGINT"), ("cigar_query_length", ["VARCHAR"], "BIGINT"), ("cigar_aligned_query_length", ["VARCHAR"], "BIGINT"),
              ("cigar_reference_length", ["VARCHAR"], "BIGINT"), ("cigar_has_op", ["VARCHAR", "VARCHAR"], "BOOLEAN"),
              ("sam_flag_bits", ["USMALLINT"], _FLAG_STRUCT), ("sam_flag_has", ["USMALLINT", "USMALLINT"], "BOOLEAN"), ("is_forward_aligned", ["BIGINT"], "BOOLEAN")] + \
             [(f, ["USMALLINT"], "BOOLEAN") for f in FLAG_FIELDS]


def _upper(c):
    """toupper in the C locale, on one byte value"""
    return c - 32 if 97 <= c <= 122 else c


# byte -> what the reference's switch statements make of it, as translate tables (0 = the default branch)
_COMP_TAB = bytes(_COMP.get(_upper(c), 0) for c in range(256))                               # dna_complement :88-97
_IUPAC_TAB = bytes(_IUPAC.get(chr(_upper(c)), 0) if c < 128 else 0 for c in range(256))       # iupac_to_4bit :109-128 (no code is 0)
_UPPER_TAB = bytes(_upper(c) for c in range(256))


def seq_revcomp(s):                                                   # :297-336
    if s is None:
        return None
    out = s[::-1].translate(_COMP_TAB)
    return None if 0 in out else out


def seq_canonical(s):                                                 # :338-388
    if s is None:
        return None
    fwd = s.translate(_UPPER_TAB)
    rev = s[::-1].translate(_COMP_TAB)
    if 0 in rev:                                                      # (fwd's own test, {A,C,G,T,N} after toupper, fails on the same bytes)
        return None
    return fwd if fwd <= rev else rev                                 # memcmp(fwd, rev) <= 0: a tie keeps fwd


def seq_hash_2bit(s):                                                 # :390-427
    if s is None or len(s) > 32:
        return None
    h = 0
    for c in s:
        code = b"ACGT".find(bytes([_upper(c)]))
        if code < 0:
            return None
        h = (h << 2) | code
    return h


def seq_encode_4bit(s):                                               # :429-480
    if s is None:
        return None
    out = s.translate(_IUPAC_TAB)
    return None if 0 in out else list(out)


def seq_decode_4bit(codes):                                           # :482-528; a NULL child is None
    if codes is None:
        return None
    out = [_BASE_OF.get(c) if c is not None else None for c in codes]
    return None if None in out else bytes(out)


def gc_counts(s):
    """(gc, called) of :549-573, or None for a row that is NULL"""
    if s is None or len(s) == 0:
        return None
    u = s.translate(_UPPER_TAB)
    g, c, a, t, n = (u.count(x) for x in (b"G", b"C", b"A", b"T", b"N"))
    if g + c + a + t + n != len(u):
        return None
    return (g + c, g + c + a + t) if g + c + a + t else None


def seq_gc_content(s):                                                # :530-581: one IEEE division of two exactly representable counts
    g = gc_counts(s)
    return None if g is None else g[0] / g[1]


def cigar_metrics(s):
    """parse_cigar_metrics :197-269 -> dict, or None"""
    if s is None or len(s) == 0 or s == b"*":
        return None
    m = dict(has_soft_clip=False, has_hard_clip=False, left_soft_clip=0, right_soft_clip=0, query_length=0, aligned_query_length=0, reference_length=0)
    op_len = 0; first = last = None
    for c in s:
        if 48 <= c <= 57:
            op_len = op_len * 10 + (c - 48)
            continue
        if op_len <= 0:
            return None
        if c in b"M=X":
            m["query_length"] += op_len; m["aligned_query_length"] += op_len; m["reference_length"] += op_len
        elif c == ord("I"):
            m["query_length"] += op_len
        elif c == ord("S"):
            m["query_length"] += op_len; m["has_soft_clip"] = True
        elif c == ord("H"):
            m["has_hard_clip"] = True
        elif c in b"DN":
            m["reference_length"] += op_len
        elif c != ord("P"):
            return None
        if first is None:
            first = (c, op_len)
        last = (c, op_len)
        op_len = 0
    if first is None or op_len != 0:
        return None
    if first[0] == ord("S"):
        m["left_soft_clip"] = first[1]
    if last[0] == ord("S"):
        m["right_soft_clip"] = last[1]
    return m


def cigar_metric(name, s):
    """cigar_<name> (:695-742), name = has_soft_clip ... reference_length"""
    m = cigar_metrics(s)
    return None if m is None else m[name]


def cigar_has_op(s, op):                                              # :744-790 over :271-295
    if s is None or op is None or len(op) != 1:
        return None
    want = _upper(op[0])
    if want not in CIGAR_OPS:
        return None
    if len(s) == 0 or s == b"*":
        return False
    op_len = 0
    for c in s:
        if 48 <= c <= 57:
            op_len = op_len * 10 + (c - 48)
            continue
        if op_len <= 0:
            return None
        if c == want:
            return True                                               # at the first match, whatever follows
        op_len = 0
    return None if op_len != 0 else False


def _flag(v):
    return None if v is None or v < 0 or v > 0xffff else v


def sam_flag_has(flag, mask):                                         # :636-656
    f, m = _flag(flag), _flag(mask)
    return None if f is None or m is None else (f & m) != 0


def flag_predicate(name, flag):                                       # :583-609
    return sam_flag_has(flag, 1 << FLAG_FIELDS.index(name))


def is_forward_aligned(flag):                                         # :611-634
    f = _flag(flag)
    return None if f is None or f & 4 else (f & 16) == 0


def sam_flag_bits(flag):                                              # :658-693: 12 booleans in FLAG_FIELDS' order
    f = _flag(flag)
    return None if f is None else [bool(f >> k & 1) for k in range(12)]


def seq_kmers(s, k, canonical=False):                                 # :820-974: [(pos, kmer)], pos 1-based
    if k <= 0:
        raise ValueError("seq_kmers: k must be > 0")
    if s is None:
        return []
    return [(i + 1, seq_canonical(s[i:i + k]) if canonical else s[i:i + k]) for i in range(len(s) - k + 1)]


def seq_kmers_column(col, k, canonical=False):
    """the whole-column form: [(row, pos, kmer, hash)], hash = seq_hash_2bit(kmer) (None for k > 32 as for any NULL)"""
    out = []
    for r, s in enumerate(col):
        for pos, km in seq_kmers(s, k, canonical):
            out.append((r, pos, km, seq_hash_2bit(km)))
    return out


def call(name, *args):
    """the scalar function `name` of REGISTERED on one row"""
    if name.startswith("cigar_") and name != "cigar_has_op":
        return cigar_metric(name[len("cigar_"):], *args)
    if name in FLAG_FIELDS:
        return flag_predicate(name, *args)
    return globals()[name](*args)
