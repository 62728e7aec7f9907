"""A plain-Python restatement of htslib's FASTA index, character by character: fai_build_core (faidx.c:132-349), fai_save (:352-377),
fai_read (:380-446), fai_parse_region / hts_parse_region with flags 0 (hts.c:3995-4150), fai_get_val's clamping (faidx.c:798-827),
fai_retrieve (:716-796) and the .gzi the single-threaded read path records (bgzf.c:1225-1236, 2382-2408).  The yardstick of the device
code (tests/test_gpu_fasta.py); pinned on htslib's own fixtures by tests/test_fasta_index_ref.py."""
import struct
import zlib

POS_MAX = (1 << 63) - 1


class FaidxError(Exception):
    pass


def _isspace(c):
    return c == 0x20 or 0x09 <= c <= 0x0D


def _isgraph(c):
    return 0x21 <= c <= 0x7E


def _isprint(c):
    return 0x20 <= c <= 0x7E


def build(text):
    """fai_build_core on FASTA bytes -> [(name, len, seq_offset, line_blen, line_len)]; FaidxError carries htslib's message"""
    OUT_READ, IN_NAME, IN_SEQ = 0, 1, 2
    n = len(text)
    p = 0

    def getc():
        nonlocal p
        if p >= n:
            return -1
        p += 1
        return text[p - 1]

    entries, seen = [], set()

    def insert(name, seq_len, line_len, char_len, seq_offset):
        name = bytes(name)
        if name in seen:
            return
        seen.add(name)
        entries.append((name, seq_len, seq_offset, char_len & 0xFFFFFFFF, line_len & 0xFFFFFFFF))

    fmt = None
    state, read_done, line_num = OUT_READ, False, 1
    name = bytearray()
    seq_offset = seq_len = char_len = line_len = 0
    c = getc()
    while c >= 0:
        if state == OUT_READ:
            if c == ord(">"):
                if fmt == "fastq":
                    raise FaidxError("Found '>' in a FASTQ file, error at line %d" % line_num)
                fmt, state = "fasta", IN_NAME
            elif c == ord("@"):
                if fmt == "fasta":
                    raise FaidxError("Found '@' in a FASTA file, error at line %d" % line_num)
                raise FaidxError("FASTQ")          # a FASTQ index (six columns) is outside this restatement
            elif c == 0x0D:
                if getc() == 0x0A:
                    line_num += 1
                else:
                    raise FaidxError("Format error, carriage return not followed by new line at line %d" % line_num)
            elif c == 0x0A:
                line_num += 1
            else:
                raise FaidxError("Format error, unexpected %s at line %d" % ('"%c"' % c if _isprint(c) else "character", line_num))
        elif state == IN_NAME:
            if read_done:
                insert(name, seq_len, line_len, char_len, seq_offset)
                read_done = False
            name = bytearray()
            while c >= 0:
                if not _isspace(c):
                    name.append(c)
                elif len(name) > 0 or c == 0x0A:
                    break
                c = getc()
            if c < 0:
                raise FaidxError("The last entry '%s' has no sequence at line %d" % (name.decode("latin-1"), line_num))
            if c != 0x0A:
                c = getc()
                while c >= 0 and c != 0x0A:
                    c = getc()
            state = IN_SEQ
            seq_len = char_len = line_len = 0
            seq_offset = p
            line_num += 1
        else:                                      # IN_SEQ, FASTA
            if c == 0x0A:
                state = OUT_READ
                line_num += 1
                c = getc()
                continue
            if c == ord(">"):
                state = IN_NAME
                c = getc()
                continue
            ll = cl = 0
            read_done = True
            while True:
                ll += 1
                if _isgraph(c):
                    cl += 1
                c = getc()
                if not (c >= 0 and c != 0x0A):
                    break
            ll += 1
            seq_len += cl
            if line_len == 0:
                line_len, char_len = ll, cl
            elif line_len > ll:
                state = OUT_READ
            elif line_len < ll:
                raise FaidxError("Different line length in sequence '%s' at line %d" % (name.decode("latin-1"), line_num))
            line_num += 1
        c = getc()
    if read_done:
        insert(name, seq_len, line_len, char_len, seq_offset)
    else:
        raise FaidxError("File truncated at line %d" % line_num)
    return entries


def save(entries):
    """fai_save"""
    return b"".join(nm + b"\t%d\t%d\t%d\t%d\n" % (ln, off, blen, llen) for nm, ln, off, blen, llen in entries)


def read(fai):
    """fai_read -> (names in order, {name: (len, seq_offset, line_blen, line_len)}); the first of equal names stays"""
    names, tab = [], {}
    lnum = 1
    for line in fai.splitlines(keepends=True):
        k = 0
        while k < len(line) and not _isspace(line[k]):
            k += 1
        nm, rest = line[:k], line[k + 1:].split()
        try:
            ln, off, blen, llen = (int(x) for x in rest[:4])
        except ValueError:
            raise FaidxError("Could not understand FASTA index line %d" % lnum)
        if nm not in tab:
            tab[nm] = (ln, off, blen & 0xFFFFFFFF, llen & 0xFFFFFFFF)
            names.append(nm)
        lnum += 1
    return names, tab


def _parse_decimal(s):
    """hts_parse_decimal with HTS_PARSE_THOUSANDS_SEP on bytes -> (value, rest); rest is s itself when there is no digit"""
    i = 0
    while i < len(s) and _isspace(s[i]):
        i += 1
    sign = 1
    if i < len(s) and s[i] in b"+-":
        sign = -1 if s[i] == ord("-") else 1
        i += 1
    v = digits = decimals = e = 0
    while i < len(s):
        if 0x30 <= s[i] <= 0x39:
            digits += 1
            v = v * 10 + s[i] - 0x30
            i += 1
        elif s[i] == ord(","):
            i += 1
        else:
            break
    if i < len(s) and s[i] == ord("."):
        i += 1
        while i < len(s) and 0x30 <= s[i] <= 0x39:
            decimals += 1
            digits += 1
            v = v * 10 + s[i] - 0x30
            i += 1
    if i < len(s) and s[i] in b"eE":
        i += 1
        es = 1
        if i < len(s) and s[i] in b"+-":
            es = -1 if s[i] == ord("-") else 1
            i += 1
        while i < len(s) and 0x30 <= s[i] <= 0x39:
            e = e * 10 + s[i] - 0x30
            i += 1
        e *= es
    elif i < len(s) and s[i] in b"kK":
        e, i = e + 3, i + 1
    elif i < len(s) and s[i] in b"mM":
        e, i = e + 6, i + 1
    elif i < len(s) and s[i] in b"gG":
        e, i = e + 9, i + 1
    e -= decimals
    if e > 0:
        v *= 10 ** e
    elif e < 0:
        v //= 10 ** (-e)
    return (sign * v, s[i:]) if digits else (sign * v, s)


def parse_region(tab, s):
    """hts_parse_region(flags = 0) with the index as name2id -> (name, beg, end) 0-based half-open, or None"""
    quoted = False
    colon = -1
    if s[:1] == b"{":
        close = s.find(b"}")
        if close < 0:
            return None
        name = s[1:close]
        quoted = True
        if s[close + 1:close + 2] == b":":
            colon = close + 1
        if colon < 0:
            return (name, 0, POS_MAX) if name in tab else None
    else:
        colon = s.rfind(b":")
        if colon < 0:
            return (s, 0, POS_MAX) if s in tab else None
        if s in tab:                               # the whole string is a name; ambiguous when the part before the colon is one too
            return None if s[:colon] in tab else (s, 0, POS_MAX)
        name = s[:colon]
    if name not in tab:
        return None
    rest = s[colon + 1:]
    beg, hy = _parse_decimal(rest)
    beg -= 1
    if beg < 0:
        if beg != -1 and hy[:1] == b"-" and len(rest) > 0:
            return None
        if hy == b"" or 0x30 <= hy[0] <= 0x39 or hy[:1] == b",":
            return (name, 0, POS_MAX if beg == -1 else -(beg + 1))
        if beg < -1:
            return None
    if hy == b"":
        end = POS_MAX
    elif hy[:1] == b"-":
        end, h2 = _parse_decimal(hy[1:])
        if h2 != b"" and h2[:1] != b",":
            return None
    else:
        return None
    if end == 0:
        end = POS_MAX
    if beg >= end:
        return None
    return name, beg, end


def fetch(text, tab, region):
    """fai_fetch64: the bytes of `region` (fai_get_val, then fai_retrieve read by read); FaidxError where htslib returns NULL"""
    r = parse_region(tab, region)
    if r is None:
        raise FaidxError("Reference %s not found in FASTA file" % region.decode("latin-1"))
    name, beg, end = r
    ln, off, blen, llen = tab[name]
    beg, end = min(beg, ln), min(end, ln)
    if beg > end:
        beg = end
    if blen <= 0:
        raise FaidxError("Invalid line length in index: %d" % blen)
    pos = off + beg // blen * llen + beg % blen      # bgzf_useek

    def rd(k):
        nonlocal pos
        got = text[pos:pos + k] if pos < len(text) else b""
        pos += len(got)
        if len(got) < k:
            raise FaidxError("Failed to retrieve block: unexpected end of file")
        return got

    remaining = end - beg
    first_blen = blen - beg % blen
    if remaining <= first_blen:
        return rd(remaining)
    buf = bytearray()
    s = 0

    def put(b):                                      # a read lands at s; later reads overwrite the terminator it brought along
        buf[s:s + len(b)] = b

    put(rd(llen - beg % blen))
    s += first_blen
    remaining -= first_blen
    while remaining > blen:
        put(rd(llen))
        s += blen
        remaining -= blen
    if remaining > 0:
        put(rd(remaining))
        s += remaining
    return bytes(buf[:s])


def split_regions(region_str):
    """parse_regions_duckdb (src/seq_reader.c:192-229): split at commas, trim blanks and tabs, drop empty pieces"""
    out = []
    for tok in region_str.split(b","):
        tok = tok.strip(b" \t")
        if tok:
            out.append(tok)
    return out


def gzi(coff, uoff, isize):
    """the .gzi bytes the read path leaves for a block table: one (caddr, uaddr) per non-empty block behind the first"""
    rec = [(int(c), int(u)) for c, u, n in zip(coff, uoff, isize) if n > 0][1:]
    return struct.pack("<Q", len(rec)) + b"".join(struct.pack("<QQ", c, u) for c, u in rec)


def bgzf_blocks(data):
    """(coff, uoff, isize) of the blocks of BGZF bytes, walked by their BSIZE fields and inflated by zlib"""
    coff, uoff, isize = [], [], []
    p = u = 0
    while p + 18 <= len(data):
        bsize = struct.unpack_from("<H", data, p + 16)[0] + 1
        raw = zlib.decompress(data[p + 18:p + bsize - 8], -15)
        coff.append(p)
        uoff.append(u)
        isize.append(len(raw))
        u += len(raw)
        p += bsize
    return coff, uoff, isize


CE_NAMES = [(b"CHROMOSOME_I", 1009800), (b"CHROMOSOME_II", 5000), (b"CHROMOSOME_III", 5000), (b"CHROMOSOME_IV", 5000),
            (b"CHROMOSOME_V", 5000), (b"CHROMOSOME_X", 5000), (b"CHROMOSOME_MtDNA", 5000)]


def ce_shaped(seed=7):
    """a FASTA of the shape of htslib's test/ce.fa: its seven names and lengths, 50 bases a line, bare >NAME headers"""
    import random
    rng = random.Random(seed)
    out = bytearray()
    for nm, ln in CE_NAMES:
        out += b">" + nm + b"\n"
        seq = bytes(rng.choice(b"ACGT") for _ in range(5000)) * (ln // 5000) + bytes(rng.choice(b"acgtn") for _ in range(ln % 5000))
        for i in range(0, ln, 50):
            out += seq[i:i + 50] + b"\n"
    return bytes(out)
