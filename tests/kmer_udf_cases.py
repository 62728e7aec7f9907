"""Inputs shared by the CPU and GPU tests of the seq_* / cigar_* / flag functions: a hand-written edge table (expected values worked out
from the cited lines of src/kmer_udf.c by hand, not by the model) and seeded columns whose lengths lie on both sides of every 16-byte
piece, lane group, wave and tile a kernel could use."""
import random

N = None
IUPAC15 = [1, 2, 4, 8, 5, 10, 6, 9, 12, 3, 14, 13, 11, 7, 15]
_M = ["cigar_has_soft_clip", "cigar_has_hard_clip", "cigar_left_soft_clip", "cigar_right_soft_clip", "cigar_query_length", "cigar_aligned_query_length", "cigar_reference_length"]

# (function, arguments, expected); strings are bytes, None is NULL
EDGE = [
    ("seq_revcomp", (b"ACGTN",), b"NACGT"), ("seq_revcomp", (b"acgtn",), b"NACGT"), ("seq_revcomp", (b"",), b""), ("seq_revcomp", (b"ACGU",), N),
    ("seq_revcomp", (N,), N), ("seq_revcomp", (b"A",), b"T"), ("seq_revcomp", (b"AC\x80",), N), ("seq_revcomp", (b"AAAAAAAAAAAAAAAAC",), b"GTTTTTTTTTTTTTTTT"),
    ("seq_canonical", (b"ACGT",), b"ACGT"), ("seq_canonical", (b"AAT",), b"AAT"), ("seq_canonical", (b"ATT",), b"AAT"), ("seq_canonical", (b"TTA",), b"TAA"),
    ("seq_canonical", (b"tta",), b"TAA"), ("seq_canonical", (b"acgt",), b"ACGT"), ("seq_canonical", (b"",), b""), ("seq_canonical", (b"ACXT",), N),
    ("seq_canonical", (b"NNN",), b"NNN"), ("seq_canonical", (N,), N), ("seq_canonical", (b"TN",), b"NA"), ("seq_canonical", (b"T",), b"A"),
    ("seq_hash_2bit", (b"",), 0), ("seq_hash_2bit", (b"A" * 32,), 0), ("seq_hash_2bit", (b"T" * 32,), 2 ** 64 - 1), ("seq_hash_2bit", (b"A" * 33,), N),
    ("seq_hash_2bit", (b"ACGT",), 27), ("seq_hash_2bit", (b"acgt",), 27), ("seq_hash_2bit", (b"ACNT",), N), ("seq_hash_2bit", (b"C" + b"A" * 31,), 1 << 62),
    ("seq_hash_2bit", (b"A" * 16 + b"C",), 1), ("seq_hash_2bit", (N,), N),
    ("seq_encode_4bit", (b"ACGTRYSWKMBDHVN",), IUPAC15), ("seq_encode_4bit", (b"acgt",), [1, 2, 4, 8]), ("seq_encode_4bit", (b"",), []), ("seq_encode_4bit", (b"ACGU",), N),
    ("seq_encode_4bit", (b"AC=T",), N), ("seq_encode_4bit", (N,), N),
    ("seq_decode_4bit", ([0],), N), ("seq_decode_4bit", ([16],), N), ("seq_decode_4bit", ([],), b""), ("seq_decode_4bit", ([1, N],), N),
    ("seq_decode_4bit", ([1, 2, 4, 8],), b"ACGT"), ("seq_decode_4bit", ([15],), b"N"), ("seq_decode_4bit", (IUPAC15,), b"ACGTRYSWKMBDHVN"), ("seq_decode_4bit", (N,), N),
    ("seq_decode_4bit", ([1, 255],), N),
    ("seq_gc_content", (b"nnnn",), N), ("seq_gc_content", (b"NNNN",), N), ("seq_gc_content", (b"",), N), ("seq_gc_content", (b"acgt",), 0.5), ("seq_gc_content", (b"ACGT",), 0.5),
    ("seq_gc_content", (b"ACGTNN",), 0.5), ("seq_gc_content", (b"GGC",), 1.0), ("seq_gc_content", (b"AAT",), 0.0), ("seq_gc_content", (b"GCA",), 2 / 3), ("seq_gc_content", (b"ACGX",), N),
    ("seq_gc_content", (N,), N),
] + [(f, (s,), N) for f in _M for s in (b"*", b"", b"5M!", b"0M", b"M", b"5", b"5B", b"5?", b"5M3", N)] + [
    ("cigar_has_soft_clip", (b"5S90M5S",), True), ("cigar_has_soft_clip", (b"90M",), False), ("cigar_has_hard_clip", (b"5H95M",), True), ("cigar_has_hard_clip", (b"5S95M",), False),
    ("cigar_left_soft_clip", (b"5S90M7S",), 5), ("cigar_right_soft_clip", (b"5S90M7S",), 7), ("cigar_left_soft_clip", (b"5H3S90M",), 0), ("cigar_right_soft_clip", (b"90M3S5H",), 0),
    ("cigar_left_soft_clip", (b"3S",), 3), ("cigar_right_soft_clip", (b"3S",), 3),
    ("cigar_query_length", (b"5S90M5I",), 100), ("cigar_aligned_query_length", (b"5S90M5I",), 90), ("cigar_reference_length", (b"90M5D",), 95),
    ("cigar_query_length", (b"10M2P3M",), 13), ("cigar_reference_length", (b"10=2X3N4D5I6S7H8P",), 19), ("cigar_query_length", (b"10=2X3N4D5I6S7H8P",), 23),
    ("cigar_aligned_query_length", (b"10=2X3N4D5I6S7H8P",), 12), ("cigar_reference_length", (b"1000000000000M",), 10 ** 12),
    ("cigar_has_op", (b"*", b"M"), False), ("cigar_has_op", (b"", b"M"), False), ("cigar_has_op", (b"5M!", b"M"), True), ("cigar_has_op", (b"5M!", b"S"), N),
    ("cigar_has_op", (b"0M", b"M"), N), ("cigar_has_op", (b"M", b"M"), N), ("cigar_has_op", (b"5", b"M"), N), ("cigar_has_op", (b"5M", b"B"), N),
    ("cigar_has_op", (b"5S90M", b"s"), True), ("cigar_has_op", (b"5S90M", b"S"), True), ("cigar_has_op", (b"5M", b"MM"), N), ("cigar_has_op", (b"5M", b""), N),
    ("cigar_has_op", (b"5M", N), N), ("cigar_has_op", (N, b"M"), N), ("cigar_has_op", (b"5!5M", b"M"), True), ("cigar_has_op", (b"90M5D", b"I"), False),
    ("cigar_has_op", (b"*", b"B"), N), ("cigar_has_op", (b"5M", b"="), False), ("cigar_has_op", (b"5=", b"="), True),
    ("is_forward_aligned", (-1,), N), ("is_forward_aligned", (65536,), N), ("is_forward_aligned", (4,), N), ("is_forward_aligned", (0,), True), ("is_forward_aligned", (16,), False),
    ("is_forward_aligned", (N,), N), ("is_forward_aligned", (20,), N),
    ("is_paired", (1,), True), ("is_paired", (2,), False), ("is_paired", (65536,), N), ("is_paired", (-1,), N), ("is_paired", (N,), N), ("is_proper_pair", (2,), True),
    ("is_unmapped", (4,), True), ("is_next_segment_unmapped", (8,), True), ("is_reverse_complemented", (16,), True), ("is_next_segment_reverse_complemented", (32,), True),
    ("is_first_segment", (64,), True), ("is_last_segment", (128,), True), ("is_secondary", (256,), True), ("is_qc_fail", (512,), True), ("is_duplicate", (1024,), True),
    ("is_supplementary", (2048,), True), ("is_supplementary", (2047,), False), ("is_supplementary", (65535,), True),
    ("sam_flag_has", (3, 2), True), ("sam_flag_has", (3, 4), False), ("sam_flag_has", (3, 65536), N), ("sam_flag_has", (N, 1), N), ("sam_flag_has", (3, N), N), ("sam_flag_has", (-1, 1), N),
    ("sam_flag_bits", (1 | 16 | 128,), [True, False, False, False, True, False, False, True, False, False, False, False]), ("sam_flag_bits", (65536,), N),
    ("sam_flag_bits", (0,), [False] * 12), ("sam_flag_bits", (4095,), [True] * 12), ("sam_flag_bits", (N,), N),
]

LENGTHS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097]
_RC = bytes.maketrans(b"ACGTN", b"TGCAN")
_cache = {}


def _kind_row(rng, n, kind):
    if kind == "null":
        return None
    alpha = {"acgt": b"ACGT", "n": b"ACGTN", "mixed": b"ACGTNacgtn", "iupac": b"ACGTRYSWKMBDHVNacgtrysw"}.get(kind, b"ACGT")
    s = bytearray(rng.choices(alpha, k=n))
    if n == 0:
        return bytes(s)
    if kind == "bad_first":
        s[0] = ord("X")
    elif kind == "bad_mid":
        s[n // 2] = ord("-")
    elif kind == "bad_last":
        s[n - 1] = ord("u")
    elif kind == "high":
        s[rng.randrange(n)] = rng.randrange(0x80, 0x100)
    elif kind == "palindrome":                                 # its own reverse complement (even lengths; an odd one gets N in the middle)
        half = bytes(s[: n // 2])
        s = bytearray(half + (b"N" if n % 2 else b"") + half[::-1].translate(_RC))
    elif kind in ("last_lt", "last_gt") and n >= 2:            # differs from its reverse complement only at the last position memcmp reaches
        half = bytes(s[: n // 2])
        s = bytearray(half + (b"N" if n % 2 else b"") + half[::-1].translate(_RC))
        # position n - 1 of fwd is s[n - 1], of rev comp(s[0]); position 0 would differ as well, so keep s[0] and s[n - 1] a pair and
        # break the pair in the middle instead: fwd[m - 1] vs rev[m - 1] = comp(s[n - m]), the last position before the halves mirror
        m = n // 2
        a, b = (b"A", b"G") if kind == "last_lt" else (b"T", b"G")        # fwd holds a, rev holds comp(b) = C: A < C < T
        s[m - 1:m] = a
        s[n - m:n - m + 1] = b
    return bytes(s)


KINDS = ["acgt", "acgt", "n", "mixed", "bad_first", "bad_mid", "bad_last", "high", "palindrome", "last_lt", "last_gt", "null", "iupac"]


def seq_column(seed=20261018, rows=3000):
    """the seeded SEQ-like column: every length of LENGTHS with every kind, then random pairs, and one row of 70,001 bases"""
    key = ("seq", seed, rows)
    if key not in _cache:
        rng = random.Random(seed)
        col = [_kind_row(rng, n, k) for n in LENGTHS[:18] for k in KINDS] + [_kind_row(rng, n, k) for n in LENGTHS[18:] for k in KINDS[1:]]
        short = LENGTHS[:18]
        while len(col) < rows - 1:
            col.append(_kind_row(rng, rng.choice(short if rng.random() < 0.97 else LENGTHS), rng.choice(KINDS)))
        col.insert(rows // 2, _kind_row(rng, 70001, "mixed"))
        _cache[key] = col
    return _cache[key]


def code_column(seed=7, rows=3000):
    """LIST(UTINYINT) rows for seq_decode_4bit: valid codes, a 0, a code above 15, a NULL child, NULL rows"""
    key = ("code", seed, rows)
    if key not in _cache:
        rng = random.Random(seed)
        col = []
        lens = LENGTHS[:18] * 8 + LENGTHS[18:]
        while len(col) < rows:
            n = rng.choice(lens); kind = rng.choice(["ok", "ok", "ok", "zero", "big", "nullchild", "null"])
            if kind == "null":
                col.append(None); continue
            r = [rng.randrange(1, 16) for _ in range(n)]
            if n and kind == "zero":
                r[rng.randrange(n)] = 0
            elif n and kind == "big":
                r[rng.randrange(n)] = rng.choice([16, 17, 128, 255])
            elif n and kind == "nullchild":
                r[rng.choice([0, n // 2, n - 1])] = None
            col.append(r)
        _cache[key] = col
    return _cache[key]


def cigar_column(seed=11, rows=3000):
    """CIGAR strings: well-formed ones of 1 .. 40 operators, and ones broken in each way the parser tells apart"""
    key = ("cigar", seed, rows)
    if key not in _cache:
        rng = random.Random(seed)
        col = [b"*", b"", None, b"5M!", b"0M", b"M", b"5", b"5B", b"5?"]
        while len(col) < rows:
            nops = rng.choice([1, 1, 2, 3, 3, 5, 8, 40])
            ops = [(rng.choice([1, 2, 9, 10, 76, 150, 1000, 123456789]), rng.choice("MIDNSHP=X")) for _ in range(nops)]
            kind = rng.choice(["ok"] * 6 + ["zero", "noop", "trail", "badop", "lower", "null", "star", "clip"])
            if kind == "clip":
                ops = [(rng.randrange(1, 50), "S")] + ops + [(rng.randrange(1, 50), "S")]
            s = "".join(f"{n}{o}" for n, o in ops)
            if kind == "zero":
                s = s.replace(str(ops[-1][0]) + ops[-1][1], "0" + ops[-1][1])
            elif kind == "noop":
                s = s + "M" if rng.random() < 0.5 else "M" + s
            elif kind == "trail":
                s += "17"
            elif kind == "badop":
                i = rng.randrange(nops); s = s.replace(ops[i][1], rng.choice("B?m "), 1)
            elif kind == "lower":
                s = s.lower()
            col.append(None if kind == "null" else b"*" if kind == "star" else s.encode())
        _cache[key] = col
    return _cache[key]


def flag_column(seed=13, rows=3000):
    key = ("flag", seed, rows)
    if key not in _cache:
        rng = random.Random(seed)
        _cache[key] = [0, 4, 16, 20, 65535, 65536, -1, None, 2 ** 40, -2 ** 40] + [rng.choice([rng.randrange(0, 4096), rng.randrange(0, 65536), rng.randrange(-5, 70000), None]) for _ in range(rows - 10)]
    return _cache[key]
