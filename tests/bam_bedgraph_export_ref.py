"""bam_bedgraph_export_ref.py -- CPU model of bam_bedgraph_export, the contract of include/duckhts_amd.h.  TEST INFRASTRUCTURE ONLY.

The file is the bgzipped text of bam_bedgraph's rows: `name \\t start \\t end \\t depth \\n` per row, cut into blocks of 0xff00 bytes.  The rows are
the bedGraph model's (bam_bedgraph_ref.bedgraph), the text is Python's own %d formatting; nothing here is shared with the device code.
"""
import bam_bedgraph_ref as B

BLOCK = 0xFF00                                                         # the bytes of the row stream one BGZF block holds
EOF_BLOCK = bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 0x42, 0x43, 2, 0, 0x1B, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
CONF_BED = (0x10000, 1, 2, 3, ord("#"), 0)                             # the tabix configuration of the index: 0-based half-open, columns 1 / 2 / 3
INDEX_KINDS = ("tbi", "csi", "none")

ERR_NOT_OPEN = "bam_bedgraph_export: dhts_bam_bedgraph_open not called"
ERR_ORDER = "bam_bedgraph_export: the regions are not in file order (an indexed file needs each contig's regions together and ascending)"
ERR_INDEX_KIND = "bam_bedgraph_export: index must be one of: tbi, csi, none"
ERR_NO_OUT_PATH = "bam_bedgraph_export requires out_path"
ERR_NO_PATH = "bam_bedgraph_export requires a file path"
ERR_OPEN_OUTPUT = "bam_bedgraph_export: cannot open output "


def err_exists(path):
    return f"bam_bedgraph_export: output '{path}' already exists (overwrite is off)"


def as_export(msg):
    """one of bam_bedgraph's bind errors under this function's prefix"""
    assert msg.startswith("bam_bedgraph:")
    return "bam_bedgraph_export:" + msg[len("bam_bedgraph:"):]


def name_bytes(n):
    return n if isinstance(n, bytes) else n.encode()


def text(rows, refs):
    """rows: the result of bam_bedgraph_ref.bedgraph (or any dict of tid, start, end, depth); refs: [(name, length)] -> the file's text"""
    names = [name_bytes(n) for n, _ in refs]
    return b"".join(b"%s\t%d\t%d\t%d\n" % (names[int(t)], int(s), int(e), int(d)) for t, s, e, d in zip(rows["tid"], rows["start"], rows["end"], rows["depth"]))


def parse(data):
    """the text back as [(name, start, end, depth)]"""
    out = []
    for line in data.split(b"\n")[:-1]:
        name, s, e, d = line.split(b"\t")
        out.append((name, int(s), int(e), int(d)))
    assert data == b"" or data.endswith(b"\n")
    return out


def rows_of(rows, refs):
    """the model's rows as parse() gives them"""
    names = [name_bytes(n) for n, _ in refs]
    return [(names[int(t)], int(s), int(e), int(d)) for t, s, e, d in zip(rows["tid"], rows["start"], rows["end"], rows["depth"])]


def n_blocks(data):
    """the data blocks of the file (the EOF block is one more)"""
    return -(-len(data) // BLOCK)


def straddlers(data):
    """the rows of the text that lie on both sides of a block boundary"""
    n, at = 0, 0
    for line in data.split(b"\n")[:-1]:
        end = at + len(line) + 1
        n += at // BLOCK != (end - 1) // BLOCK
        at = end
    return n


def overlapping(rows, name, beg, end):
    """the rows [(name, start, end, depth)] that a tabix query of name:beg+1-end (0-based half-open [beg, end)) returns"""
    return [r for r in rows if r[0] == name and r[1] < end and r[2] > beg]


def in_file_order(target_rows):
    """target_rows: [(tid, beg, end)] in the order they are answered in: every contig's rows together and ascending"""
    seen, last = set(), None
    for t, b, _e in target_rows:
        if last is not None and last[0] == t:
            if b < last[1]:
                return False
        elif t in seen:
            return False
        seen.add(t)
        last = (t, b)
    return True


def export(reads, refs, rows=None, **kw):
    """-> (the text, the bedGraph model's result)"""
    res = B.bedgraph(reads, refs, rows=rows, **kw)
    return text(res, refs), res
