"""A plain Python model of read_tabix / read_gtf / read_gff (src/tabix_reader.c of the reference): bind (the peek, the schema rules,
auto_detect), the scan (line classes, line_skip, the header line, typed fields), the two attribute grammars and parse_regions.  No device,
no library: the GPU tests compare the device's columns with this, and test_read_tabix_ref.py pins it on the reference's recorded answers."""
import gzip
import re
import struct

GENERIC, GTF, GFF = 0, 1, 2
T_INTEGER, T_BIGINT, T_DOUBLE, T_VARCHAR = 4, 5, 11, 17
MAX_COLS = 256
NUM_BUF = 128
GXF_NAMES = ["seqname", "source", "feature", "start", "end", "score", "strand", "frame", "attributes"]
GXF_TYPES = [T_VARCHAR, T_VARCHAR, T_VARCHAR, T_BIGINT, T_BIGINT, T_DOUBLE, T_VARCHAR, T_VARCHAR, T_VARCHAR]
GXF_MAP = 9

# ---- numbers: strtoll / strtod over a whole field (parse_int64_span, parse_double_span: the field is copied into a C string) ---------------
_WS = rb"[ \t\n\v\f\r]*"
_INT_RE = re.compile(_WS + rb"([+-]?)([0-9]+)\Z")
_DEC_RE = re.compile(_WS + rb"[+-]?(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?\Z")
_HEX_RE = re.compile(_WS + rb"[+-]?0[xX](?:[0-9a-fA-F]+\.?[0-9a-fA-F]*|\.[0-9a-fA-F]+)(?:[pP][+-]?[0-9]+)?\Z")
_INF_RE = re.compile(_WS + rb"([+-]?)(?:inf|infinity)\Z", re.I)
_NAN_RE = re.compile(_WS + rb"([+-]?)nan(?:\([0-9A-Za-z_]*\))?\Z", re.I)


def strtoll_whole(tok: bytes):
    """strtoll(tok, &end, 10) when it consumes the whole token, else None; out of range saturates (errno is not looked at)"""
    m = _INT_RE.match(tok)
    if not m:
        return None
    v = int(m.group(2))
    if m.group(1) == b"-":
        v = -v
    return max(-(1 << 63), min((1 << 63) - 1, v))


def strtod_whole(tok: bytes):
    """strtod(tok, &end) in the C locale when it consumes the whole token, else None.  Decimal, hex, inf / infinity, nan / nan(chars);
    leading white space; nothing behind.  (Python's float() alone would also take '1_0' and trailing blanks.)"""
    if _DEC_RE.match(tok):
        return float(tok.strip(b" \t\n\v\f\r").decode("ascii"))
    if _HEX_RE.match(tok):
        return float.fromhex(tok.strip(b" \t\n\v\f\r").decode("ascii"))
    m = _INF_RE.match(tok)
    if m:
        return float("-inf") if m.group(1) == b"-" else float("inf")
    m = _NAN_RE.match(tok)
    if m:
        return struct.unpack("<d", struct.pack("<Q", 0xfff8000000000000 if m.group(1) == b"-" else 0x7ff8000000000000))[0]   # (glibc puts nan(chars) into the mantissa: not modelled)
    return None


def dbl_bits(v):
    return None if v is None else struct.unpack("<Q", struct.pack("<d", v))[0]


def fast_path_takes(tok: bytes):
    """the tokens vcf_str2dbl_fast converts on the device: decimal, at most 15 significant digits, and a power of ten one exact IEEE
    multiplication or division covers (after moving spare digits into the significand, |exponent| <= 22)"""
    if not _DEC_RE.match(tok):
        return False
    t = tok.strip(b" \t\n\v\f\r").lstrip(b"+-").lower()
    mant, _, ex = t.partition(b"e")
    ip, _, fp = mant.partition(b".")
    digits = (ip + fp).lstrip(b"0")
    nd = len(digits)
    if nd > 15:
        return False
    if nd == 0:
        return True
    e10 = (int(ex) if ex else 0) - len(fp)
    while e10 > 22 and nd < 15:
        nd += 1
        e10 -= 1
    return -22 <= e10 <= 22


# ---- lines ------------------------------------------------------------------------------------------------------------------------------------
def getlines(text: bytes):
    """hts_getline: (C string of the line, line.l).  A CR in front of the newline is dropped; the C string ends at the first NUL, line.l does
    not; a last line without a newline is a line."""
    parts = text.split(b"\n")
    if parts and parts[-1] == b"":
        parts.pop()
    out = []
    for ln in parts:
        if ln.endswith(b"\r"):
            ln = ln[:-1]
        out.append((ln.split(b"\0", 1)[0], len(ln)))
    return out


def get_field(s: bytes, idx: int):
    f = s.split(b"\t")
    return f[idx] if idx < len(f) else None


def count_fields(s: bytes):
    return s.count(b"\t") + 1


def trim(b: bytes):
    return b.strip(b" \t")


def is_missing(f):
    return f is None or f == b"" or f == b"."


# ---- attributes --------------------------------------------------------------------------------------------------------------------------------
def gff_pairs(s: bytes):
    """fill_attr_map with is_gff: key=value between ';'; a token without '=' is skipped"""
    out, p, n = [], 0, len(s)
    while p < n:
        while p < n and s[p] in b"; \t":
            p += 1
        if p >= n:
            break
        key = p
        while p < n and s[p] not in b"=;":
            p += 1
        if p >= n or s[p] != 0x3d:
            continue
        k = s[key:p]
        p += 1
        val = p
        while p < n and s[p] != 0x3b:
            p += 1
        k, v = trim(k), trim(s[val:p])
        if k:
            out.append((k, v))
        if p < n:
            p += 1
    return out


def gtf_pairs(s: bytes):
    """fill_attr_map for GTF: the key runs to a blank or ';', the value is quoted up to the next '"' or bare up to ';'"""
    out, p, n = [], 0, len(s)
    while p < n:
        while p < n and s[p] in b"; \t":
            p += 1
        if p >= n:
            break
        key = p
        while p < n and s[p] not in b" \t;":
            p += 1
        k = s[key:p]
        while p < n and s[p] in b" \t":
            p += 1
        if p < n and s[p] == 0x22:
            p += 1
            val = p
            while p < n and s[p] != 0x22:
                p += 1
            v = s[val:p]
            if p < n:
                p += 1
        else:
            val = p
            while p < n and s[p] != 0x3b:
                p += 1
            v = s[val:p]
        k, v = trim(k), trim(v)
        if k:
            out.append((k, v))
        while p < n and s[p] != 0x3b:
            p += 1
        if p < n:
            p += 1
    return out


def attr_map(field, is_gff):
    """None = NULL map (field 8 missing, empty or '.'); else the list of (key, value)"""
    if is_missing(field):
        return None
    return gff_pairs(field) if is_gff else gtf_pairs(field)


# ---- regions -----------------------------------------------------------------------------------------------------------------------------------
def parse_regions(s):
    """comma-separated, trimmed of blanks and tabs, empty tokens dropped"""
    if not s:
        return []
    return [t.strip(" \t") for t in s.split(",") if t.strip(" \t")]


def tbi_conf(index_bytes: bytes):
    """(preset, sc, bc, ec, meta, skip, names) of a .tbi"""
    d = gzip.decompress(index_bytes) if index_bytes[:2] == b"\x1f\x8b" else index_bytes
    assert d[:4] == b"TBI\x01"
    n_ref, preset, sc, bc, ec, meta, skip, l_nm = struct.unpack_from("<8i", d, 4)
    names = [x.decode() for x in d[36:36 + l_nm].split(b"\0") if x]
    return preset, sc, bc, ec, meta, skip, names


def region_interval(tok, names):
    """'name' or 'name:beg-end' (1-based, closed) -> (name, beg0, end) or None when the index does not know the sequence"""
    name, beg, end = tok, 0, (1 << 62)
    if tok not in names and ":" in tok:
        name, _, rng = tok.rpartition(":")
        a, _, b = rng.replace(",", "").partition("-")
        beg = max(int(a) - 1, 0)
        end = int(b) if b else (1 << 62)
    if name not in names:
        return None
    return name, beg, end


# ---- bind -----------------------------------------------------------------------------------------------------------------------------------------
def type_of_name(s):
    u = s.upper()
    if u in ("INT", "INTEGER"):
        return T_INTEGER
    if u in ("BIGINT", "LONG"):
        return T_BIGINT
    if u in ("DOUBLE", "FLOAT", "REAL"):
        return T_DOUBLE
    return T_VARCHAR


def sniff(text, header, have_names, meta_char=ord("#"), line_skip=0):
    """the peek of bind: (n_fields of the first data line, header candidate or None, candidate_from_skip)"""
    want = header and not have_names
    cand, from_skip, n_fields, skip = None, False, 0, line_skip
    for s, l in getlines(text):
        if l == 0:
            continue
        if skip > 0:
            if want:
                cand, from_skip = s, True
            skip -= 1
            continue
        if meta_char and s[:1] == bytes([meta_char]):
            continue
        if want and cand is None:
            cand = s
        else:
            n_fields = count_fields(s)
            break
    return n_fields, cand, from_skip


class BindError(Exception):
    pass


def data_lines(text, meta_char, line_skip, skip_header_line, in_region=False):
    """the C strings of the lines tabix_scan turns into rows"""
    skip, hdr = line_skip, skip_header_line
    for s, l in getlines(text):
        if l == 0:
            continue
        if not in_region and skip > 0:
            skip -= 1
            continue
        if meta_char and s[:1] == bytes([meta_char]):
            continue
        if not in_region and hdr:
            hdr = False
            continue
        yield s


def bind(text, header=False, header_names=None, column_types=None, auto_detect=False, meta_char=ord("#"), line_skip=0):
    """generic bind: {"n_cols", "names", "types", "skip_header_line"}"""
    n_fields, cand, from_skip = sniff(text, header, bool(header_names), meta_char, line_skip)
    names, n_cols, skip_header_line = [], n_fields, False
    if header_names:
        names, n_cols, skip_header_line = [x.encode() if isinstance(x, str) else x for x in header_names], len(header_names), bool(header)
    elif header and cand is not None:
        names = [trim(f) for f in cand.split(b"\t")]
        n_cols, skip_header_line = len(names), not from_skip
    n_cols = min(n_cols or 1, MAX_COLS)
    if column_types:
        if len(column_types) != n_cols:
            raise BindError("column_types length does not match detected column count")
        types = [type_of_name(t) for t in column_types]
    else:
        types = [T_VARCHAR] * n_cols
        if auto_detect:
            state = [T_BIGINT] * n_cols
            for seen, s in enumerate(data_lines(text, meta_char, line_skip, skip_header_line)):
                if seen >= 100:
                    break
                for i in range(n_cols):
                    f = get_field(s, i)
                    if is_missing(f):
                        continue
                    if re.match(rb"[+-]?[0-9]+\Z", f):
                        continue
                    if strtod_whole(f) is not None:
                        if state[i] != T_VARCHAR:
                            state[i] = T_DOUBLE
                    else:
                        state[i] = T_VARCHAR
            types = state
    out_names = [(names[i].decode() if i < len(names) and names[i] else "column%d" % i) for i in range(n_cols)]
    return {"n_cols": n_cols, "names": out_names, "types": types, "skip_header_line": skip_header_line}


# ---- scan -----------------------------------------------------------------------------------------------------------------------------------------
def cell(f, ty, gxf):
    """one value: bytes, int, float or None"""
    if is_missing(f):
        if gxf:
            return 0 if ty == T_BIGINT else None if ty == T_DOUBLE else b"."
        return None
    if ty == T_VARCHAR:
        return f
    if len(f) >= NUM_BUF:
        return None
    return strtod_whole(f) if ty == T_DOUBLE else strtoll_whole(f)


def scan(text, mode=GENERIC, types=None, meta_char=ord("#"), line_skip=0, skip_header_line=False, in_region=False, keep=None):
    """rows of every column (GTF / GFF: the nine columns and, last, attributes_map); keep(line) filters the lines of a region query"""
    gxf = mode != GENERIC
    if gxf:
        types, meta_char, line_skip, skip_header_line = GXF_TYPES, ord("#"), 0, False
    rows = []
    for s in data_lines(text, meta_char, line_skip, skip_header_line, in_region):
        if keep is not None and not keep(s):
            continue
        row = [cell(get_field(s, i), types[i], gxf) for i in range(len(types))]
        if gxf:
            row.append(attr_map(get_field(s, 8), mode == GFF))
        rows.append(row)
    return rows


def region_scan(text, conf, regions, mode=GENERIC, types=None, meta_char=ord("#")):
    """the chained union of region := 'a,b,...' on a sorted file: for every region the index resolves, the data lines whose tabix interval
    (columns sc / bc / ec of the index, 1-based closed coordinates) overlaps it, in file order"""
    preset, sc, bc, ec, _meta, _skip, names = conf
    assert (preset & 0xffff) == 0 and not (preset & 0x10000)
    rows = []
    for tok in parse_regions(regions):
        iv = region_interval(tok, names)
        if iv is None:
            continue
        name, qb, qe = iv

        def keep(s):
            f = s.split(b"\t")
            if len(f) < max(sc, bc, ec or 0) or f[sc - 1].decode() != name:
                return False
            b = int(f[bc - 1]) - 1
            e = int(f[ec - 1]) if ec and ec != bc else b + 1
            return e > qb and qe > b
        rows += scan(text, mode, types, meta_char, 0, False, True, keep)
    return rows
