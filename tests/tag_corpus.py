"""Hostile aux data for the standard-tag columns and AUXILIARY_TAGS: one record per case, shared by the CPU model test and the GPU tests.

Every family is built once per CARRIER tag: one column of each kind (NM: i, MD: Z, TS: A, ML / FZ / CG: B of C / S / I) and XT, which only
the map sees.  A record carries a healthy standard tag and a healthy non-standard one in front of the case field (UQ:C, YA:Z) and, where the
case field can be walked over, a second pair behind it (AS:c, YB:Z): the result shows whether the walk went on or stopped.

corpus() -> [(name, record bytes, the aux bytes as bam_aux_get sees them)]; a name begins with its family, "F1 " .. "F7 ".
field / barray / cg_tag / cg_record are also the builders of test_gpu_aux_walk.py."""
import functools
import random
import struct

import bamwriter as BW

REFS = [("chr1", 100000000)]
FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4, "d": 8}
VALID = "AcCsSiIfdZHB"
CARRIERS = [b"NM", b"MD", b"TS", b"ML", b"FZ", b"CG", b"XT"]
PRE = b"UQC\x07" + b"YAZya\0"
POST = b"ASc\xfb" + b"YBZyb\0"
INT_RANGE = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (-2**31, 2**31 - 1), "I": (0, 2**32 - 1)}
INT_FMT = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}
# the words of bcf_cases.qual_records(), then the edges of the widening: denormals, the smallest normal, the largest finite, zeros, infinities, NaNs
QUAL_WORDS = [0x7F800002, 0x7FC00000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000000, 0x7F800001, 0x3DCCCCCD, 0x7F7FFFFF, 0x00800000, 0x007FFFFF, 0xFFC12345]
F3_WORDS = QUAL_WORDS + [0x00000001, 0x007fffff, 0x00800000, 0x80000001, 0x7f7fffff, 0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7f800001, 0xffc12345]
F3_DOUBLES = [struct.pack("<d", v) for v in (5e-324, 1.7976931348623157e308, 0.1, 1e-5, 0.0001, 100000.0, 1e6, 123456789.0, -0.0, float("inf"), float("-inf"))] + \
             [struct.pack("<Q", 0x7ff8000000000000), struct.pack("<Q", 0xfff8000000000001)]
F7_POSITIONS = ["first", "middle", "middle, TS behind", "last", "only"]


def field(type_byte, tag=b"XT"):
    """a field of that type with a payload of the right size where the type has one (4 bytes otherwise)"""
    t = bytes([type_byte]); ch = chr(type_byte)
    if ch in FIXED:
        return tag + t + bytes(range(1, 1 + FIXED[ch]))
    if ch in "ZH":
        return tag + t + b"ab\0"
    if ch == "B":
        return tag + t + b"c" + struct.pack("<I", 2) + b"\x01\x02"
    return tag + t + b"\x01\x02\x03\x04"


def barray(sub, n, tag=b"XB", payload=None):
    """a B field of n elements of that sub-type (Z, H and B count as elements of their own byte value, sam.c aux_type2size)"""
    size = FIXED[sub] if sub in FIXED else ord(sub)
    if payload is None:
        payload = bytes((7 * k + 1) & 0x7f for k in range(size * n))
    assert len(payload) == size * n
    return tag + b"B" + sub.encode() + struct.pack("<I", n) + payload


def cg_record(i, aux, far, n_real=3):
    """a record whose CIGAR is the placeholder <l_seq>S<ref>N: the CG walk runs over its aux data"""
    n = 900 if far else 40
    rnd = random.Random(i)
    return BW.record(qname="c%d" % i, flag=0, tid=0, pos=i, mapq=20, raw_cigar=[(n << 4) | 4, (n << 4) | 3], seq="".join(rnd.choice("ACGT") for _ in range(n)),
                     qual=bytes(rnd.randrange(1, 60) for _ in range(n)), raw_aux=aux)


def cg_tag(n):
    ops = [(10 << 4) | 0] * (n // 10) + ([((n % 10) << 4) | 0] if n % 10 else [])
    return b"CGBI" + struct.pack("<I", len(ops)) + b"".join(struct.pack("<I", o) for o in ops)


def healthy(tag, k=0):
    """the carrier in the type its column expects, two different values"""
    return {b"NM": [b"NMi" + struct.pack("<i", 77), b"NMc\xfb"], b"MD": [b"MDZ10A5\0", b"MDZ7\0"], b"TS": [b"TSA+", b"TSA-"],
            b"ML": [barray("C", 3, b"ML", b"\x01\x02\xff"), barray("C", 1, b"ML", b"\x09")], b"FZ": [barray("S", 2, b"FZ", b"\xff\xff\x01\x00"), barray("S", 1, b"FZ", b"\x03\x00")],
            b"CG": [barray("I", 2, b"CG", b"\x50\0\0\0\xff\xff\xff\xff"), barray("I", 1, b"CG", b"\x64\0\0\0")], b"XT": [b"XTZxt\0", b"XTi\x05\0\0\0"]}[tag][k]


def wrong_type(tag):
    return {b"NM": b"NMZoops\0", b"MD": b"MDi\x05\0\0\0", b"TS": b"TSZ++\0", b"ML": b"MLZnotB\0", b"FZ": b"FZA!", b"CG": b"CGZ4M\0", b"XT": b"XTA!"}[tag]


def int_array(sub, n):
    lo, hi = INT_RANGE[sub]
    vals = [lo, hi, 0, hi - 1, lo + 1, 1, hi // 2]
    return b"".join(struct.pack("<" + INT_FMT[sub], vals[k % 7]) for k in range(n))


def f4_fields(tag):
    """(name, bytes) of the truncated and overrunning fields and of stray bytes: each ends its record"""
    out = []
    for ch, sz in FIXED.items():
        for short in range(1, sz + 1):
            out.append(("%s %d short" % (ch, short), tag + ch.encode() + b"\x05" * (sz - short)))
    out += [("Z without NUL", tag + b"Zabc"), ("H without NUL", tag + b"H1AE3")]
    for k in range(5):
        out.append(("B header cut after %d" % k, tag + b"B" + (b"I" + struct.pack("<I", 1))[:k]))
    for n, have in ((3, 8), (1 << 20, 16), (0xffffffff, 0), (0x40000001, 8)):
        out.append(("B:I count %d overruns" % n, tag + b"BI" + struct.pack("<I", n) + b"\x01" * have))
    # bytes behind the last field that are no field: one, two, and a tag name with a type byte but no payload
    out += [("1 stray byte", tag[:1]), ("2 stray bytes", tag), ("tag and i, no payload", tag + b"i"), ("tag and Z, no payload", tag + b"Z"), ("tag and B, no payload", tag + b"B")]
    return out


def _plain(i, aux):
    return BW.record(qname="t%d" % i, flag=0, tid=0, pos=i, mapq=20, cigar="4M", seq="ACGT", qual=b"\x1e\x1f\x20\x21", raw_aux=aux)


@functools.lru_cache(maxsize=None)
def corpus():
    out = []

    def add(name, aux):
        out.append((name, _plain(len(out), aux), aux))

    def add_cg(name, aux, seen):
        out.append((name, cg_record(len(out), aux, False), seen))

    for tag in CARRIERS:
        T = tag.decode()
        # F1 type x kind: the carrier stored as every type byte; the integer types once more at their limits
        for t in range(256):
            add("F1 %s type %d" % (T, t), PRE + field(t, tag) + (POST if chr(t) in VALID else b""))
        for sub, (lo, hi) in INT_RANGE.items():
            for v in (lo, hi):
                add("F1 %s %s %d" % (T, sub, v), PRE + tag + sub.encode() + struct.pack("<" + INT_FMT[sub], v) + POST)
        # F2 arrays of every sub-type aux_type2size accepts
        for sub in "cCsSiIfdAZHB":
            for n in (0, 1, 7, 300):
                add("F2 %s B:%s x%d" % (T, sub, n), PRE + barray(sub, n, tag, int_array(sub, n) if sub in INT_RANGE else None) + POST)
        # F3 float words as f and inside B:f of 1 and 5, the payload at an odd offset of the aux area; d scalars
        for k, w in enumerate(F3_WORDS):
            front = PRE + b"XAA!"
            one = front + tag + b"f" + struct.pack("<I", w) + POST
            assert (len(front) + 3) % 2 == 1
            add("F3 %s f %08x #%d" % (T, w, k), one)
            front = PRE + b"XAA!" + b"YCZo\0"                                   # (a 5-byte field more: the 8-byte B header then ends at an odd offset)
            assert (len(front) + 8) % 2 == 1
            add("F3 %s B:f x1 %08x #%d" % (T, w, k), front + barray("f", 1, tag, struct.pack("<I", w)) + POST)
            five = struct.pack("<5I", 0x3f800000, w, F3_WORDS[(k + 1) % len(F3_WORDS)], w ^ 0x80000000, 0xc0490fdb)
            add("F3 %s B:f x5 %08x #%d" % (T, w, k), front + barray("f", 5, tag, five) + POST)
        for k, d in enumerate(F3_DOUBLES):
            add("F3 %s d #%d" % (T, k), PRE + b"XAA!" + tag + b"d" + d + POST)
        # F4 truncation: the field ends the record
        for name, f in f4_fields(tag):
            add("F4 %s %s" % (T, name), PRE + f)
        # F5 duplicates
        add("F5 %s twice" % T, PRE + healthy(tag, 0) + healthy(tag, 1) + POST)
        add("F5 %s wrong type first" % T, PRE + wrong_type(tag) + healthy(tag) + POST)
        add("F5 %s then a corrupt copy" % T, PRE + healthy(tag) + POST + tag + b"i\x01\x02")
        add("F5 %s behind a corrupt field" % T, PRE + b"XQ?\x01\x02" + healthy(tag) + POST)
        add("F5 %s in front of a corrupt field" % T, PRE + healthy(tag) + b"XQi\x01\x02")
        # F6 byte values through the carrier
        for v in (0x00, 0xe9):
            add("F6 %s A 0x%02x" % (T, v), PRE + tag + b"A" + bytes([v]) + POST)
        add("F6 %s Z empty" % T, PRE + tag + b"Z\0" + POST)
        add("F6 %s Z high bytes" % T, PRE + tag + b"Z\x80\xff\xc3\xa9\x7f\0" + POST)
        # F7 the CG splice: every F4 field behind a swapped CG tag
        for name, f in f4_fields(tag):
            add_cg("F7 %s behind CG: %s" % (T, name), PRE + cg_tag(40) + f, PRE + f)
    # F6 keys, sizes
    for nm in (b"\0X", b"X\0", b"\0\0", b"\xffZ", b"NX", b"XM"):
        add("F6 key %r" % nm, PRE + nm + b"i\x2a\0\0\0" + POST)
    add("F6 Z of 70000", PRE + b"MDZ" + bytes(33 + k % 90 for k in range(70000)) + b"\0" + POST)
    add("F6 3000 fields", PRE + b"".join(bytes([48 + k // 75, 48 + k % 75, 67, k & 0xff]) for k in range(3000)) + POST)
    for aux in (b"", b"N", b"NM", b"NMi"):
        add("F6 aux of %d bytes" % len(aux), aux)
    # F7 positions of a swapped CG tag among one healthy field of each column kind
    L = healthy(b"NM") + healthy(b"MD") + healthy(b"TS") + healthy(b"ML") + b"YAZya\0"
    R = b"UQC\x07" + b"PGZbwa\0" + healthy(b"FZ") + b"YBZyb\0"
    Lm, Rm = healthy(b"NM") + healthy(b"MD") + healthy(b"ML") + b"YAZya\0", R + healthy(b"TS")
    for name, l, r in zip(F7_POSITIONS, (b"", L, Lm, L + R, b""), (L + R, R, Rm, b"", b"")):
        add_cg("F7 CG " + name, l + cg_tag(40) + r, l + r)
    short = PRE + b"CGBI" + struct.pack("<I", 1) + struct.pack("<I", 40 << 4) + POST
    add_cg("F7 CG shorter than the CIGAR stays", short, short)
    return out


@functools.lru_cache(maxsize=None)
def files():
    """the corpus as BAM, twice: the writer's default BGZF payload, and 700 bytes so that records and the long Z straddle blocks"""
    recs = [r for _, r, _ in corpus()]
    return BW.bam_bytes(REFS, recs), BW.bam_bytes(REFS, recs, payload=700)


def file_of(n, **kw):
    return BW.bam_bytes(REFS, [r for _, r, _ in corpus()[:n]], **kw)
