"""bam_tags_ref.py -- CPU model of read_bam(standard_tags := true) and AUXILIARY_TAGS on one record's aux bytes.  TEST INFRASTRUCTURE ONLY.

Restates the reference's src/bam_reader.c:54-183 (the tag table, bam_assign_list_int / _double, bam_aux_to_string) and 920-1027 (the tag
columns and the map) over htslib's sam.c: aux_type2size 732-748, skip_aux 4785-4809, bam_aux_first / next / get 4811-4855,
get_int_aux_val 5093-5107, bam_aux2i / 2f / 2A / 2Z 5109-5141, bam_auxB_len / B2i / B2f 5143-5171.  One function per function there, byte
by byte, in plain Python: nothing shared with the device code or with the C oracle.

The aux bytes are the record's as bam_aux_get sees them: after a long-CIGAR swap (bam_tag2cigar sam.c:675-730) the CG field has been cut
out of them, so the caller passes them without it.

Three places where the reference reads memory behind the record; each is defined here, as INTEGRATION.md defines it:
  * a corrupt field (skip_aux answers NULL) ends the walk of the map and is listed with an EMPTY value (bam_aux_to_string would format
    whatever follows the record);
  * a Z / H value without a NUL is not corrupt to skip_aux (it answers `end`): in the map its value is the bytes up to the record's end
    (kputs would run on behind it); bam_aux_get refuses it (sam.c:4842), so the tag's column is NULL;
  * skip_aux tests a B field with `end - s < size * n`, a product of an int and a uint32_t, which is taken modulo 2^32: a count of
    0x40000001 four-byte elements passes as 4 bytes, and bam_auxB_len then sends the list and the map through a gigabyte behind the
    record.  The product is taken exactly here, so such a field is corrupt like every other array that overruns its record.
"""
import struct

# src/bam_reader.c:54-70: (tag, column kind), in the table's order
STD_TAGS = [("AM", "i"), ("AS", "i"), ("BC", "Z"), ("BQ", "Z"), ("BZ", "Z"), ("CB", "Z"), ("CC", "Z"), ("CG", "B"), ("CM", "i"), ("CO", "Z"), ("CP", "i"), ("CQ", "Z"),
            ("CR", "Z"), ("CS", "Z"), ("CT", "Z"), ("CY", "Z"), ("E2", "Z"), ("FI", "i"), ("FS", "Z"), ("FZ", "B"), ("H0", "i"), ("H1", "i"), ("H2", "i"), ("HI", "i"),
            ("IH", "i"), ("LB", "Z"), ("MC", "Z"), ("MD", "Z"), ("MI", "Z"), ("ML", "B"), ("MM", "Z"), ("MN", "i"), ("MQ", "i"), ("NH", "i"), ("NM", "i"), ("OA", "Z"),
            ("OC", "Z"), ("OP", "i"), ("OQ", "Z"), ("OX", "Z"), ("PG", "Z"), ("PQ", "i"), ("PT", "Z"), ("PU", "Z"), ("Q2", "Z"), ("QT", "Z"), ("QX", "Z"), ("R2", "Z"),
            ("RG", "Z"), ("RX", "Z"), ("SA", "Z"), ("SM", "i"), ("TC", "i"), ("TS", "A"), ("U2", "Z"), ("UQ", "i")]
assert len(STD_TAGS) == 56
BAD = "bad"                                     # skip_aux's NULL


def aux_type2size(t):                           # sam.c:732-748
    if t in b"AcC":
        return 1
    if t in b"sS":
        return 2
    if t in b"iIf":
        return 4
    if t == ord("d"):
        return 8
    if t in b"ZHB":
        return t
    return 0


def skip_aux(a, s):
    """sam.c:4785-4809; s = index of the type byte, end = len(a).  The index behind the field, or BAD"""
    end = len(a)
    if s >= end:
        return end
    size = aux_type2size(a[s]); s += 1
    if size in (ord("Z"), ord("H")):            # memchr(s, 0, end - s): s + 1 behind the NUL, `end` where there is none
        z = a.find(b"\0", s)
        return z + 1 if z >= 0 else end
    if size == ord("B"):
        if end - s < 5:
            return BAD
        size = aux_type2size(a[s]); s += 1
        n = struct.unpack_from("<I", a, s)[0]; s += 4
        if size == 0 or end - s < size * n:     # (the exact product: see the module's text)
            return BAD
        return s + size * n
    if size == 0:
        return BAD
    if end - s < size:
        return BAD
    return s + size


def aux_first(a):                               # sam.c:4811-4817
    return None if len(a) <= 2 else 2


def aux_next(a, s):
    """sam.c:4819-4832 -> (index of the next type byte or None, corrupt)"""
    nxt = skip_aux(a, s)
    if nxt == BAD:
        return None, True
    if len(a) - nxt <= 2:
        return None, False
    return nxt + 2, False


def aux_get(a, tag):                            # sam.c:4834-4855
    s = aux_first(a)
    while s is not None:
        if a[s - 2] == tag[0] and a[s - 1] == tag[1]:
            e = skip_aux(a, s)
            if e == BAD:
                return None
            if a[s] in b"ZH" and a[e - 1] != 0:
                return None
            return s
        s, _ = aux_next(a, s)
    return None


def get_int_aux_val(t, a, s, idx):              # sam.c:5093-5107; any other type: 0
    fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}.get(chr(t))
    if fmt is None:
        return 0
    return struct.unpack_from(fmt, a, s + struct.calcsize(fmt) * idx)[0]


def f32_to_f64_bits(w):
    """the word of a float -> the word of the same value as a double, on integers (le_to_float, then C's float -> double)"""
    sign, e, m = w >> 31, (w >> 23) & 0xff, w & 0x7fffff
    if e == 0xff:                               # inf; a NaN keeps its payload and becomes quiet
        return sign << 63 | 0x7ff << 52 | m << 29 | ((1 << 51) if m else 0)
    if e == 0:
        if m == 0:
            return sign << 63
        sh = 24 - m.bit_length()                # a denormal: m * 2^-149, normalised
        return sign << 63 | (1023 - 126 - sh) << 52 | ((m << sh) & 0x7fffff) << 29
    return sign << 63 | (e - 127 + 1023) << 52 | m << 29


def aux_b2f_bits(a, s, idx):                    # bam_auxB2f sam.c:5162-5171 as the word of the double: 'f' widened, anything else through
    if a[s + 1] == ord("f"):                    # get_int_aux_val (so 'd' reads 0.0)
        return f32_to_f64_bits(struct.unpack_from("<I", a, s + 6 + 4 * idx)[0])
    return struct.unpack("<Q", struct.pack("<d", float(get_int_aux_val(a[s + 1], a, s + 6, idx))))[0]


def aux_b_len(a, s):                            # sam.c:5143-5150
    return struct.unpack_from("<I", a, s + 2)[0] if a[s] == ord("B") else 0


def std_tags(aux):
    """the 56 cells of bam_reader.c:920-966: None = NULL, int (BIGINT), bytes (VARCHAR), list of int (LIST(BIGINT); the word of the double
    where the stored sub-type is f or d: bam_assign_list_double writes doubles into the BIGINT child)"""
    a = bytes(aux)
    out = []
    for tag, kind in STD_TAGS:
        s = aux_get(a, tag.encode())
        if s is None:
            out.append(None)
        elif kind == "A":                       # bam_aux2A sam.c:5125-5132, assigned as the C string {ch, 0}
            ch = a[s + 1] if a[s] == ord("A") else 0
            out.append(bytes([ch]) if ch else b"")
        elif kind == "Z":                       # bam_aux2Z sam.c:5134-5141, assigned as a C string
            out.append(a[s + 1:a.index(b"\0", s + 1)] if a[s] in b"ZH" else None)
        elif kind == "i":                       # bam_aux2i sam.c:5109-5114
            out.append(get_int_aux_val(a[s], a, s + 1, 0))
        else:                                   # bam_reader.c:954-961
            n = aux_b_len(a, s)
            if a[s + 1] in b"fd":
                out.append([aux_b2f_bits(a, s, i) for i in range(n)])
            else:
                out.append([get_int_aux_val(a[s + 1], a, s + 6, i) for i in range(n)])
    return out


def fmt_g(bits):
    """printf("%g") of the double with that word: Python's %g for finite values and the infinities; glibc prints a NaN by its sign bit"""
    if (bits >> 52) & 0x7ff == 0x7ff and bits & ((1 << 52) - 1):
        return b"-nan" if bits >> 63 else b"nan"
    return b"%g" % struct.unpack("<d", struct.pack("<Q", bits))[0]


def aux_to_string(a, s, e):
    """bam_aux_to_string bam_reader.c:140-183 of the field at s, which ends at e"""
    t = chr(a[s])
    if t == "A":
        return a[s + 1:s + 2]
    if t in "cCsSiI":
        return b"%d" % get_int_aux_val(a[s], a, s + 1, 0)
    if t == "f":                                # bam_aux2f sam.c:5116-5123
        return fmt_g(f32_to_f64_bits(struct.unpack_from("<I", a, s + 1)[0]))
    if t == "d":
        return fmt_g(struct.unpack_from("<Q", a, s + 1)[0])
    if t in "ZH":
        return a[s + 1:e]                       # (cut at its NUL by the caller; without one: the bytes up to the record's end)
    sub = a[s + 1]
    n = aux_b_len(a, s)
    if sub in b"fd":
        return bytes([sub]) + b"".join(b"," + fmt_g(aux_b2f_bits(a, s, i)) for i in range(n))
    return bytes([sub]) + b"".join(b",%d" % get_int_aux_val(sub, a, s + 6, i) for i in range(n))


def cstr(b):
    return b.split(b"\0")[0]


_STD = {t.encode() for t, _ in STD_TAGS}


def aux_map(aux, exclude_standard):
    """bam_reader.c:967-1027: None where no field is listed (the MAP cell is NULL), else (keys, values), both cut at the first NUL as
    duckdb_vector_assign_string_element cuts them.  A field is excluded by bam_std_tag_index of its two-byte name (bam_reader.c:72-81)."""
    a = bytes(aux)
    keys, vals = [], []
    s = aux_first(a)
    while s is not None:
        tag = a[s - 2:s]
        e = skip_aux(a, s)
        if not (exclude_standard and tag in _STD):
            keys.append(cstr(tag))
            vals.append(b"" if e == BAD else cstr(aux_to_string(a, s, e)))      # corrupt: listed with an empty value (the module's text)
        s, _ = aux_next(a, s)
    return (keys, vals) if keys else None
