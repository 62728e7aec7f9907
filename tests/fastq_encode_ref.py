"""CPU restatement of htslib's FASTQ / FASTA reader with default options: fastq_parse1 (sam.c:3919-4120) + bam_set1 (sam.c:526-646) +
bam_write1 -> the BAM records read_bam's device encoder (duckhts_amd/csrc/fastq_text.hip) has to produce, byte for byte.  It walks the
lines one after the other as the reference does; the device finds the records another way (prefix sums and pointer jumping)."""
import struct

import bamwriter as W
import sam_encode_ref as R

SPACE = b" \t\n\v\f\r"


def detect(text: bytes):
    """hts_detect_format2 on the first KiB (hts.c:693-733): 'sam' for a header line, 'fasta', 'fastq', or None (not raw reads)"""
    s = text[:1024]
    if s[:4] in (b"@HD\t", b"@SQ\t", b"@RG\t", b"@PG\t", b"@CO\t"):
        return "sam"

    def is_fastaq():
        eol = s.find(b"\n")
        first = s if eol < 0 else s[:eol]
        if any(not (b >= 32 or b in b"\t\r\n") for b in first):
            return False
        if eol < 0:
            return True
        p = eol + 1
        while p < len(s) and (R.NT16[s[p]] != 15 or s[p] in b"Nn"):
            if s[p] == ord("="):
                return False
            p += 1
        return p == len(s) or s[p] in b"\r\n"
    if s[:1] == b">" and is_fastaq():
        return "fasta"
    if s[:1] == b"@" and is_fastaq():
        return "fastq"
    return None


def split_lines(text: bytes):
    """bgzf_getline: lines end at '\\n' (a last line without one counts), one trailing '\\r' is dropped"""
    parts = text.split(b"\n")
    if parts and parts[-1] == b"":
        parts.pop()
    return [l[:-1] if l.endswith(b"\r") else l for l in parts]


def record(name: bytes, seq: bytes, qual):
    """bam_set1 + bam_write1 of an unmapped read; name still carries its /1 /2 suffix.  None: bam_set1 refuses it"""
    flag = 4
    line = b"@" + name                                        # (name.l counts the prefix character)
    if len(line) > 2 and line[-2:-1] == b"/" and line[-1:].isdigit():
        flag |= 1 | 8 | {b"1": 64, b"2": 128}.get(line[-1:], 192)
        line = line[:-2]
    qn = line[1:] or b"*"
    if len(qn) > 254:
        return None
    z = qn.find(b"\0")
    if z >= 0:
        qn = qn[:z] + b"\0" * (len(qn) - z)                   # (strncpy)
    n = len(seq)
    codes = [R.NT16[b] for b in seq] + [0]
    packed = bytes((codes[i] << 4) | codes[i + 1] for i in range(0, n, 2))
    ql = b"\xff" * n if qual is None else bytes((b - 33) & 0xff for b in qual)
    body = struct.pack("<iiIIiiii", -1, -1, (R.reg2bin(-1, 0) << 16) | (len(qn) + 1), flag << 16, n, -1, -1, 0)
    body += qn + b"\0" + packed + ql
    return struct.pack("<I", len(body)) + body


def encode_text(text: bytes, fasta=None):
    """-> ([record bytes in front of the first record the reader refuses], True when it stopped at one (a truncated last record included))"""
    if fasta is None:
        fasta = detect(text) == "fasta"
    lines = split_lines(text)
    recs, i, n = [], 0, len(lines)
    while i < n:
        l = lines[i]
        if l[:1] != (b">" if fasta else b"@"):
            return recs, True
        k = 1
        while k < len(l) and l[k] not in SPACE:
            k += 1
        name = l[1:k]
        i += 1
        seq = b""
        while True:
            if i >= n:
                if not fasta:
                    return recs, True
                break
            if lines[i][:1] == (b">" if fasta else b"+"):
                break
            seq += lines[i]
            i += 1
        qual = None
        if not fasta:
            i += 1                                            # the '+' line
            qual, rem = b"", len(seq)
            while True:
                if i >= n or len(lines[i]) > rem:
                    return recs, True
                qual += lines[i]
                rem -= len(lines[i])
                i += 1
                if rem == 0:
                    break
        r = record(name, seq, qual)
        if r is None:
            return recs, True
        recs.append(r)
    return recs, False


def fastq_to_bam(text: bytes, **kw) -> bytes:
    """the BAM file (empty header) of the records htslib would read from this FASTQ / FASTA text before it stops"""
    recs, _ = encode_text(text)
    return W.bgzf_file(W.bam_header([], text=b"") + b"".join(recs), **kw)


def sam_columns(rec: bytes):
    """columns 1-11 of the SAM line sam_format1 writes for one of these records"""
    l_qname = rec[12]
    flag = struct.unpack_from("<H", rec, 18)[0]
    n = struct.unpack_from("<I", rec, 20)[0]
    qn = rec[36:36 + l_qname - 1]
    z = qn.find(b"\0")
    qn = qn if z < 0 else qn[:z]
    sq = rec[36 + l_qname:36 + l_qname + (n + 1) // 2]
    seq = "".join(W.NT16[(sq[k >> 1] >> (4 if k % 2 == 0 else 0)) & 15] for k in range(n)) or "*"
    ql = rec[36 + l_qname + (n + 1) // 2:36 + l_qname + (n + 1) // 2 + n]
    qual = "*" if n == 0 or ql[0] == 0xff else "".join(chr(b + 33) for b in ql)
    return [qn.decode("latin-1"), str(flag), "*", "0", "0", "*", "*", "0", "0", seq, qual]
