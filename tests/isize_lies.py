"""BGZF files whose ISIZE trailer fields lie (CPU helper, no GPU import).

htslib never reads the ISIZE field of a BGZF block: a block is whatever its DEFLATE stream inflates to, valid when the CRC-32 agrees.  A
file that differs from a clean one in ISIZE fields only is therefore the SAME file to the reference, and every reader here must return
what it returns for the clean file.  `lie` rewrites nothing but the chosen four-byte fields; `PLANS` names which blocks lie, `VALUES` what
they claim."""
import struct
import zlib

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")

# what a block of true length L claims; an empty block claims 777 instead of 0
VALUES = {
    "zero": lambda L: 0 if L else 777,
    "minus1": lambda L: (L - 1) & 0xFFFFFFFF,
    "plus1": lambda L: L + 1,
    "64k": lambda L: 65536,
    "64k1": lambda L: 65537,
    "70000": lambda L: 70000,
    "64M": lambda L: 0x04000000,
    "high_bit": lambda L: 0x80000000 | L,
    "ffff0000": lambda L: 0xFFFF0000 + L,
    "all_ones": lambda L: 0xFFFFFFFF,
}
ALL_VALUES = tuple(VALUES)
OVERSTATING = ("plus1", "64k", "64k1", "70000", "64M", "high_bit", "ffff0000", "all_ones")       # more than L for every L < 65536
PLANS = ("block0", "first_record_block", "one_mid", "last_data_block", "eof_block", "run8", "all", "net_zero", "empty_mid")


def blocks(data):
    """(offset, length) of every BGZF block, walked by BSIZE; the walk must consume the whole file"""
    out, p = [], 0
    while p < len(data):
        assert p + 18 <= len(data) and data[p:p + 4] == b"\x1f\x8b\x08\x04" and data[p + 12:p + 16] == b"BC\x02\x00", f"no BGZF block at {p}"
        bl = struct.unpack_from("<H", data, p + 16)[0] + 1
        assert bl >= 26 and p + bl <= len(data), f"block at {p} runs past the end"
        out.append((p, bl)); p += bl
    assert p == len(data)
    return out


def isize(data, blk):
    return struct.unpack_from("<I", data, blk[0] + blk[1] - 4)[0]


def inflate_block(data, blk):
    """the block's payload by raw zlib (never looks at ISIZE), checked against its CRC-32"""
    o, bl = blk
    raw = zlib.decompress(bytes(data[o + 18:o + bl - 8]), -15)
    assert zlib.crc32(raw) == struct.unpack_from("<I", data, o + bl - 8)[0], f"CRC of the block at {o}"
    return raw


def inflate_all(data):
    return b"".join(inflate_block(data, b) for b in blocks(data))


def first_record_block(data):
    """index of the block that holds the first byte behind the header: BAM (magic, l_text, references), BCF (magic, l_text); for text
    formats the block behind the first one (or block 0 of a file with one data block)"""
    bl = blocks(data)
    lens = [isize(data, b) for b in bl]
    head = b""
    k = 0
    need = 12

    def more(n):
        nonlocal head, k
        while len(head) < n and k < len(bl):
            head += inflate_block(data, bl[k]); k += 1
        return len(head) >= n
    more(need)
    if head[:4] == b"BAM\x01":
        p = 8 + struct.unpack_from("<I", head, 4)[0]
        assert more(p + 4)
        n_ref = struct.unpack_from("<i", head, p)[0]; p += 4
        for _ in range(n_ref):
            assert more(p + 4)
            p += 4 + struct.unpack_from("<i", head, p)[0] + 4
            assert more(p)
    elif head[:5] == b"BCF\x02\x02":
        p = 9 + struct.unpack_from("<I", head, 5)[0]
    else:
        return 1 if sum(1 for x in lens if x) > 1 else 0
    u = 0
    for i, x in enumerate(lens):
        if u + x > p:
            return i
        u += x
    return len(bl) - 1


def data_blocks(data):
    bl = blocks(data)
    return [i for i, b in enumerate(bl) if isize(data, b) > 0]


def plan_blocks(data, plan):
    """block indices that lie under `plan` (on the file `clean_for(data, plan)`)"""
    bl = blocks(data)
    db = data_blocks(data)
    if plan == "block0":
        return [0]
    if plan == "first_record_block":
        return [first_record_block(data)]
    if plan == "one_mid":
        return [db[len(db) // 2]]
    if plan == "last_data_block":
        return [db[-1]]
    if plan == "eof_block":
        assert isize(data, bl[-1]) == 0
        return [len(bl) - 1]
    if plan == "run8":
        s = max(0, len(db) // 2 - 4)
        return db[s:s + 8]
    if plan == "all":
        return list(range(len(bl)))
    if plan == "net_zero":
        i = next(k for k in range(len(db) // 2, len(db) - 1) if db[k + 1] == db[k] + 1 and isize(data, bl[db[k]]) >= 30)
        return [db[i], db[i] + 1]
    if plan == "empty_mid":
        return [db[len(db) // 2]]            # (the inserted empty block takes this index in clean_for's file)
    raise ValueError(plan)


def clean_for(data, plan):
    """the clean file a plan's lying file is compared with: the file itself, except empty_mid (an empty block inserted between data blocks)"""
    if plan != "empty_mid":
        return bytes(data)
    at = blocks(data)[plan_blocks(data, plan)[0]][0]
    return bytes(data[:at]) + EOF_BLOCK + bytes(data[at:])


def set_isize(data, idx_values):
    """the file with the ISIZE field of block i set to v for every (i, v); nothing else changes"""
    d = bytearray(data)
    bl = blocks(data)
    for i, v in idx_values:
        struct.pack_into("<I", d, bl[i][0] + bl[i][1] - 4, v & 0xFFFFFFFF)
    return bytes(d)


def lie(data, plan, values=ALL_VALUES, only=None):
    """the lying counterpart of clean_for(data, plan).  plan: a name of PLANS or a list of block indices; values: one name of VALUES or a
    sequence of names the lying blocks cycle through (net_zero claims L-30 / L+30 and empty_mid 100 whatever `values` says).
    only: restrict the plan to block indices for which only(i) is true."""
    base = clean_for(data, plan) if isinstance(plan, str) else bytes(data)
    idx = plan_blocks(data, plan) if isinstance(plan, str) else list(plan)
    if only is not None:
        idx = [i for i in idx if only(i)]
    bl = blocks(base)
    if plan == "net_zero":
        a, b = idx
        return set_isize(base, [(a, isize(base, bl[a]) - 30), (b, isize(base, bl[b]) + 30)])
    if plan == "empty_mid":
        assert isize(base, bl[idx[0]]) == 0
        return set_isize(base, [(idx[0], 100)])
    if isinstance(values, str):
        values = (values,)
    return set_isize(base, [(i, VALUES[values[k % len(values)]](isize(base, bl[i]))) for k, i in enumerate(idx)])


def small_understatement(data, ks):
    """blocks ks[0..2] claim L-1, L-5, L-40: 46 bytes short in all (under half of the 256 pad bytes every stream buffer carries)"""
    bl = blocks(data)
    assert len(ks) == 3 and all(isize(data, bl[k]) >= 40 for k in ks)
    return set_isize(data, [(k, isize(data, bl[k]) - s) for k, s in zip(ks, (1, 5, 40))])


def lying_blocks(clean, lying):
    """indices of the blocks whose ISIZE fields differ; asserts that nothing else does"""
    assert len(clean) == len(lying)
    bl = blocks(clean)
    assert blocks(lying) == bl
    out, c, l = [], bytearray(clean), bytearray(lying)
    for i, (o, n) in enumerate(bl):
        if c[o + n - 4:o + n] != l[o + n - 4:o + n]:
            out.append(i)
            l[o + n - 4:o + n] = c[o + n - 4:o + n]
    assert c == l, "a lie changed bytes outside ISIZE fields"
    return out
