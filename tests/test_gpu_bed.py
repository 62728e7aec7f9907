"""read_bed on the device (bed_text.hip, dhts_bed_scan.inc) through the Python mirror, against the CPU model tests/read_bed_ref.py:
every column with its validity in the three containers, batches that cut lines, projections, the short-line error, region queries."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import read_bed_ref as M
from conftest import read_golden

pytestmark = pytest.mark.gpu

INTS = [b" 12", b"+5", b"-7", b"-", b"12 ", b"0x10", b"1e3", b"\v12", b"999999999999999999", b"9223372036854775807", b"9223372036854775808",
        b"-9223372036854775808", b"-9223372036854775809", b"99999999999999999999", b"-99999999999999999999", b"1000000000000000000"]


def corner_text():
    """every corner the kernels can get wrong, spread over more than three 65,280-byte pieces"""
    L = []
    full = [b"chrE", b"1", b"2", b"n", b"5", b"+", b"7", b"8", b"9,9", b"10", b"11,", b"12,", b"x13", b"x14", b"x15", b"x16"]
    for nf in range(3, 17):                                       # 3 to 16 fields: extra keeps its tabs
        L.append(b"\t".join(full[:nf]))
    L += [b"#comment", b"", b"track name=t", b"browser position chr1", b"tracker1\t1\t2", b"\r", b"\0chr\t1\t2"]
    for pos in range(14):                                         # an empty field in every position
        f = list(full[:14]); f[pos] = b""
        L.append(b"\t".join(f))
    L += [b"chrT\t1\t2\t", b"chrT\t1\t", b"\t".join(full[:12]) + b"\t", b"\t".join(full[:13]) + b"\t"]      # trailing tabs
    L += [b"chrR\t1\t2\tcr\r", b"chrR\t1\t2\t\r", b"\t".join(full[:13]) + b"\r", b"#meta\r"]                  # CRLF
    L += [b"chrN\t1\t2\tna\0me\t5\t+", b"chrN\t1\t2\t3\t4\t5\t6\t7\t8\t9\t10\t11\tex\0tra\tmore", b"chrN\t1\t2\0\t3"]    # NUL in the middle
    for x in INTS:                                                # integers in every BIGINT column
        L.append(b"\t".join([b"chrI", x, x, b"n", b"s", b"+", x, x, b"rgb", x]))
    L += [b"", b"#again", b"browser hide all"]
    for n in range(1, 49):                                        # every tab / newline position modulo 16
        L.append(b"#" * n if n < 5 else b"c" * (n - 4) + b"\t1\t2")
        if n >= 5:
            L.append(b"c\t1\t" + b"7" * (n - 4))
            L.append(b"c\t" + b"3" * (n - 4) + b"\t2")
    L.append(b"chrL\t1\t2\t" + b"N" * 5000 + b"\t0")              # longer than a 4 KiB chunk
    for i in range(2200):                                         # ordinary BED12 rows between the corners
        L.append(b"chr%d\t%d\t%d\tname%d\t%d\t%s\t%d\t%d\t%d,0,0\t2\t10,20\t0,30" % (i % 5, i * 10, i * 10 + 50, i, i % 1000, b"+-"[i % 2:i % 2 + 1], i * 10, i * 10 + 50, i % 256))
        if i % 97 == 0:
            L += [b"", b"track x%d" % i]
    L.append(b"chrX\t1\t2\t" + b"\t".join([b"f"] * 9) + b"\t" + (b"0123456789\tabcdef" * 4200))      # > 64 KiB: crosses a BGZF block
    for i in range(400):
        L.append(b"chrZ\t%d\t%d\tz%d" % (i, i + 1, i))
    L.append(b"chrEnd\t5\t6\tlast\t0\t-")                         # a last line without a newline
    return b"\n".join(L)


@pytest.fixture(scope="module")
def corner():
    text = corner_text()
    assert 3 * 65280 < len(text) < 400_000
    return text, M.read_bed(text)


def containers(text):
    import duckhts_amd
    ctx = duckhts_amd.Context(0)
    try:
        z = ctx.bgzf_compress(text)
    finally:
        ctx.close()
    assert gzip.decompress(z) == text
    return {"plain": text, "bgzf": z, "gzip": gzip.compress(text, 6)}


def same(got, exp, cols=M.COLUMNS):
    assert got["n_rows"] == exp["n_rows"]
    for k in cols:
        assert len(got[k]) == len(exp[k]), k
        bad = [i for i in range(len(exp[k])) if got[k][i] != exp[k][i]]
        assert not bad, (k, bad[:5], [(got[k][i], exp[k][i]) for i in bad[:2]])


@pytest.fixture(scope="module")
def corner_files(corner):
    return containers(corner[0])


@pytest.mark.parametrize("kind", ["plain", "bgzf", "gzip"])
def test_every_column_in_every_container(corner, corner_files, kind):
    import duckhts_amd
    exp = corner[1]
    assert exp["n_rows"] > 2000 and exp["status"] == 1
    whole, st1, st2 = {}, {}, {}
    whole = duckhts_amd.read_bed(corner_files[kind], stats=st1)
    assert whole["status"] == 1 and whole["error"] is None
    same(whole, exp)
    cut = duckhts_amd.read_bed(corner_files[kind], max_blocks=1, stats=st2)        # lines straddle the batches
    assert st2["n_batches"] >= 3 and cut["status"] == 1
    same(cut, exp)
    for k in M.COLUMNS:
        assert cut[k] == whole[k]


def test_targets_bed(corner):
    import duckhts_amd
    got = duckhts_amd.read_bed(read_golden("targets.bed"))
    same(got, M.read_bed(read_golden("targets.bed")))
    assert got["n_rows"] == 4 and got["extra"][3] == b"extra_note=foo" and got["score"][0] == b"100"


@pytest.mark.parametrize("cols", [[c] for c in M.COLUMNS] + [["extra", "start", "strand"], []], ids=lambda c: "+".join(c) or "none")
def test_projections(corner, corner_files, cols):
    import duckhts_amd
    got = duckhts_amd.read_bed(corner_files["bgzf"], columns=cols, max_blocks=2)
    assert sorted(k for k in got if k in M.COLUMNS) == sorted(cols)
    same(got, corner[1], cols)


def _small(nlines=60):
    return [b"chr1\t%d\t%d\tr%d\t%d" % (i * 3, i * 3 + 2, i, i) if i % 7 else b"# note %d" % i for i in range(nlines)]


@pytest.mark.parametrize("k", [1, 2, 31, 60])
def test_short_line_at_line_k(k):
    import duckhts_amd
    L = _small()
    L[k - 1] = b"chr1\t5"
    text = b"\n".join(L) + (b"\n" if k != 60 else b"")
    exp = M.read_bed(text)
    assert exp["error"] == M.ERR + " (line %d)" % k
    got = duckhts_amd.read_bed(text)
    assert got["status"] < 0 and got["error"] == exp["error"]
    same(got, exp)


def test_short_line_in_a_later_batch(corner):
    """the line number counts the lines of the batches in front; the rows of those batches have been delivered"""
    import duckhts_amd
    lines = corner[0].split(b"\n")
    k = len(lines) - 100
    lines[k - 1] = b"only\ttwo"
    text = b"\n".join(lines)
    exp = M.read_bed(text)
    st = {}
    got = duckhts_amd.read_bed(text, max_blocks=1, stats=st)
    assert st["n_batches"] >= 3 and got["status"] < 0 and got["error"] == M.ERR + " (line %d)" % k == exp["error"]
    same(got, exp)


def test_refusals_on_a_bed_context():
    import duckhts_amd
    L = duckhts_amd.lib()
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(b"c\t1\t2\n")
        L.dhts_bgzf_index(ctx.h)
        sc = duckhts_amd.BedScan(ctx)
        with pytest.raises(duckhts_amd.DhtsError, match="uncompressed text"):
            sc.set_region("c:1-2")
        with pytest.raises(duckhts_amd.DhtsError, match="BED"):
            ctx.set_shard(0, 2)
        L.dhts_tabix_build_index.restype = C.c_int64; L.dhts_tabix_build_index.argtypes = [C.c_void_p] + [C.c_int] * 7
        assert L.dhts_tabix_build_index(ctx.h, 0x10000, 1, 2, 3, ord("#"), 0, 0) < 0 and b"BED" in L.dhts_error(ctx.h)
        b = sc.next_batch()
        assert b.n_rows == 1 and b.status == 1
    finally:
        ctx.close()
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(gzip.compress(b"c\t1\t2\n"))
        L.dhts_bgzf_index(ctx.h)
        with pytest.raises(duckhts_amd.DhtsError, match="plain .* gzip"):
            duckhts_amd.BedScan(ctx).set_region("c")
    finally:
        ctx.close()


# ---- regions ---------------------------------------------------------------------------------------------------------------------

def sorted_bed():
    L = [b"#sorted three-sequence BED"]
    for s, name in enumerate((b"seqA", b"seqB", b"seqC")):
        for i in range(3000):
            beg = i * 50 + s
            L.append(b"%s\t%d\t%d\tr%d_%d\t%d\t+" % (name, beg, beg + 30 + (i % 5) * 20, s, i, i % 900))
    return b"\n".join(L) + b"\n"


def build_index(bgzf, conf, min_shift):
    import duckhts_amd
    L = duckhts_amd.lib()
    L.dhts_tabix_build_index.restype = C.c_int64; L.dhts_tabix_build_index.argtypes = [C.c_void_p] + [C.c_int] * 7
    L.dhts_bgzf_wrap.restype = C.c_int64; L.dhts_bgzf_wrap.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(bgzf); ctx.bgzf_index()
        n = L.dhts_tabix_build_index(ctx.h, conf[0], conf[1], conf[2], conf[3], conf[4], conf[5], min_shift)
        assert n > 0, L.dhts_error(ctx.h)
        raw = np.zeros(n, np.uint8)
        assert L.dhts_bam_index_bytes(ctx.h, raw.ctypes.data, n) == 0
    finally:
        ctx.close()
    need = L.dhts_bgzf_wrap(raw.ctypes.data, n, None, 0)
    out = np.zeros(need, np.uint8)
    got = L.dhts_bgzf_wrap(raw.ctypes.data, n, out.ctypes.data, need)
    return out[:got].tobytes()


CONF_ONE_BASED = (0, 1, 2, 3, ord("#"), 0)


@pytest.fixture(scope="module")
def region_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("bed_region")
    text = sorted_bed()
    z = containers(text)["bgzf"]
    assert len(z) > 2 * 20000 and len(text) > 2 * 65280
    path = str(d / "sorted.bed.gz")
    open(path, "wb").write(z)
    open(path + ".tbi", "wb").write(build_index(z, M.R.CONF_BED, 0))
    open(str(d / "elsewhere.csi"), "wb").write(build_index(z, M.R.CONF_BED, 14))
    open(str(d / "one_based.tbi"), "wb").write(build_index(z, CONF_ONE_BASED, 0))
    open(str(d / "plain.bed"), "wb").write(text)
    return {"dir": str(d), "path": path, "text": text, "size": len(z)}


# row 100 of seqB is [5001, 5031): the ranges below touch its beg / end exactly, from both sides
REGIONS = ["seqB", "seqA:20,001-30,000", "seqC:200,000-300,000", "seqB:5001-5001", "seqB:5002-5002", "seqB:5031-5031", "seqB:5032-5032",
           "seqA:1,000-2,000", ".", "seqC:3-3", "seqA:99,000"]


@pytest.mark.parametrize("index", ["tbi", "csi"])
@pytest.mark.parametrize("region", REGIONS)
def test_region_rows(region_files, region, index):
    import duckhts_amd
    exp = M.read_bed(region_files["text"], region=region)
    st = {}
    got = duckhts_amd.read_bed(region_files["path"], region=region, index_path=None if index == "tbi" else os.path.join(region_files["dir"], "elsewhere.csi"), stats=st)
    assert got["status"] == 1
    same(got, exp)
    if region == "seqC:200,000-300,000":
        assert exp["n_rows"] == 0
    elif region != ".":
        assert 0 < exp["n_rows"] < 9000
    if region not in (".", "seqB"):
        assert st["resident_bytes"] < region_files["size"], (st, region_files["size"])             # only the index windows were staged


def test_region_under_the_index_configuration(region_files):
    """an index built with 1-based columns (sc 1, bc 2, ec 3, no UCSC flag) reads [start - 1, end): the row set follows it"""
    import duckhts_amd
    idx = os.path.join(region_files["dir"], "one_based.tbi")
    differs = 0
    for region in ("seqB:5001-5001", "seqB:5031-5031", "seqA:20,001-30,000", "seqC:3-3"):
        exp = M.read_bed(region_files["text"], region=region, conf=CONF_ONE_BASED)
        same(duckhts_amd.read_bed(region_files["path"], region=region, index_path=idx), exp)
        differs += exp["name"] != M.read_bed(region_files["text"], region=region)["name"]
    assert differs >= 2


def test_region_errors(region_files):
    import duckhts_amd
    with pytest.raises(duckhts_amd.BedIteratorError, match="read_bed: failed to create region iterator"):
        duckhts_amd.read_bed(region_files["path"], region="nope:1-10")
    with pytest.raises(duckhts_amd.DhtsError, match="read_bed: region queries require a tabix index"):
        duckhts_amd.read_bed(region_files["path"], region="seqA", index_path=os.path.join(region_files["dir"], "missing.tbi"))
    with pytest.raises(duckhts_amd.DhtsError, match="read_bed: region queries require a tabix index"):
        duckhts_amd.read_bed(os.path.join(region_files["dir"], "plain.bed"), region="seqA")
    with pytest.raises(duckhts_amd.DhtsError, match="uncompressed text"):
        duckhts_amd.read_bed(os.path.join(region_files["dir"], "plain.bed"), region="seqA", index_path=region_files["path"] + ".tbi")
