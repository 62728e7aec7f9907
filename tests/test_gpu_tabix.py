"""read_tabix / read_gtf / read_gff on the device (tabix_text.hip, dhts_tabix_scan.inc) through the Python mirror, against the CPU model
tests/read_tabix_ref.py, exactly (doubles by their 64 bits): every column in the three containers and the three modes, both DOUBLE paths,
bind, line_skip and the header line across batches, projections, the attribute grammars, chained regions, refusals, the golden fixtures."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import read_tabix_ref as M
from conftest import ROOT

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden")
DBL_FAST = [b"0", b"-0.0", b"1.5", b".5", b"5.", b"1e22", b"1e-22", b"123456789012345", b"1e23"]       # 1e23 = 10 * 1e22 is one exact multiplication
DBL_PATCH = [b"1234567890123456", b"1e38", b"1e-23", b"1e400", b"4.9e-324", b"inf", b"-Infinity", b"nan", b"0x1p-3", b"1e", b"1.5x"]
INTS = [b" 5", b"+5", b"5x", b"99999999999999999999", b"-99999999999999999999", b"-", b"12 ", b"0x10"]
BASE = [b"chr1", b"src", b"exon", b"100", b"200", b"1.5", b"+", b"0", b"ID=e1;Name=x"]
GXF_TYPE_NAMES = ["VARCHAR", "VARCHAR", "VARCHAR", "BIGINT", "BIGINT", "DOUBLE", "VARCHAR", "VARCHAR", "VARCHAR"]


def with_(**kw):
    f = list(BASE)
    for k, v in kw.items():
        f[int(k[1:])] = v
    return b"\t".join(f)


def corner_text():
    """every corner the kernels can get wrong, over more than three 65,280-byte pieces; the first data line has nine fields"""
    L = [b"##gff-version 3", b"\t".join(BASE)]
    for n in range(1, 49):                                        # every tab / newline position modulo 16
        L.append(b"s" * n + b"\tv\tf\t%d\t%d\t.\t-\t.\tk=%d" % (n, n + 5, n))
    for n in (63, 64, 65, 200, 5000):                             # around the 64-byte switch of the gather; longer than a 4 KiB chunk
        L.append(with_(f1=b"L" * n, f8=b"ID=" + b"V" * n + b';note "q"'))
    for n in (127, 128):
        L.append(with_(f3=b"0" * (n - 1) + b"1", f4=b"0" * (n - 1) + b"1", f5=b"0" * (n - 1) + b"1"))
    for x in INTS:
        L.append(with_(f3=x, f4=x))
    for x in DBL_FAST + DBL_PATCH + [b" 2.5", b"+.5e1", b"-"]:
        L.append(with_(f5=x))
    L += [with_(f0=b"crlf") + b"\r", b"\r", b"", b"#meta between rows", b"", with_(f0=b"after")]
    L += [with_(f0=b"nu\0l"), with_(f3=b"1\0" + b"2"), with_(f5=b"2.\0" + b"5"), with_(f8=b"ID=a;b=\0c;d=e"), b"\0\tx\ty", b"x\0\r"]
    L += [b"onefield", b"\t".join(BASE + [b"ten", b"eleven", b"twelve"]), b"a\tb\t", b"\t\t\t\t\t\t\t\t", with_(f0=b".", f1=b"", f3=b".", f4=b"", f5=b".", f8=b".")]
    for i in range(2600):                                         # ordinary GFF3 rows between the corners, a numeric score on part of them
        sc = (b"%d.%d" % (i % 97, i % 10)) if i % 3 == 0 else b"."
        L.append(b"chr%d\tsrc\t%s\t%d\t%d\t%s\t%s\t%d\tID=f%d;Parent=g%d;Note=n %d" % (i % 4, (b"exon", b"CDS", b"gene")[i % 3], i * 10 + 1, i * 10 + 60, sc, b"+-"[i % 2:i % 2 + 1], i % 3, i, i // 7, i))
        if i % 131 == 0:
            L += [b"", b"#note %d" % i]
    L.append(with_(f1=b"0123456789abcdef" * 4200))                # > 64 KiB: crosses a BGZF block
    L.append(with_(f0=b"last", f8=b"ID=end"))                     # a last line without a newline
    return b"\n".join(L)


def containers(text):
    import duckhts_amd
    ctx = duckhts_amd.Context(0)
    try:
        z = ctx.bgzf_compress(text)
    finally:
        ctx.close()
    assert gzip.decompress(z) == text
    return {"plain": text, "bgzf": z, "gzip": gzip.compress(text, 6)}


@pytest.fixture(scope="module")
def corner():
    text = corner_text()
    assert 3 * 65280 < len(text) < 500_000
    exp = {M.GFF: M.scan(text, M.GFF), M.GTF: M.scan(text, M.GTF), M.GENERIC: M.scan(text, M.GENERIC, M.GXF_TYPES)}
    return text, containers(text), exp


def norm(v):
    return ("d", M.dbl_bits(float(v))) if isinstance(v, float) else v


def table(got, names):
    """the result dict as rows in the order of `names`"""
    cols = [[norm(v) for v in got[k]] for k in names]
    assert all(len(c) == got["n_rows"] for c in cols), (got["n_rows"], [len(c) for c in cols])
    return [list(r) for r in zip(*cols)] if cols else [[] for _ in range(got["n_rows"])]


def expect(rows, ids):
    return [[norm(r[i]) for i in ids] for r in rows]


def same(got_rows, exp_rows):
    assert len(got_rows) == len(exp_rows)
    bad = [i for i in range(len(exp_rows)) if got_rows[i] != exp_rows[i]]
    assert not bad, (bad[:5], [(got_rows[i], exp_rows[i]) for i in bad[:2]])


def token_counts(rows_text, field=5):
    """DOUBLE tokens of the data lines that the device converts itself / hands to the host"""
    fast = patch = 0
    for s in M.data_lines(rows_text, ord("#"), 0, False):
        f = M.get_field(s, field)
        if M.is_missing(f) or len(f) >= M.NUM_BUF:
            continue
        if M.fast_path_takes(f):
            fast += 1
        else:
            patch += 1
    return fast, patch


@pytest.mark.parametrize("kind", ["plain", "bgzf", "gzip"])
@pytest.mark.parametrize("mode", ["gff", "gtf", "tabix"])
def test_every_column_in_every_container(corner, kind, mode):
    import duckhts_amd as D
    text, files, exp = corner
    fast, patch = token_counts(text)
    assert fast > 800 and patch == len(DBL_PATCH) + 1               # the eleven tokens and "-"; "2.\\0" + "5" reads as "2.", which the device converts
    for mb in (0, 1):
        st = {}
        if mode == "tabix":
            got = D.read_tabix(files[kind], column_types=GXF_TYPE_NAMES, max_blocks=mb, stats=st)
            assert got["names"] == ["column%d" % i for i in range(9)] and got["types"] == M.GXF_TYPES
            same(table(got, got["names"]), expect(exp[M.GENERIC], range(9)))
        else:
            fn, m = (D.read_gff, M.GFF) if mode == "gff" else (D.read_gtf, M.GTF)
            got = fn(files[kind], attributes_map=True, max_blocks=mb, stats=st)
            assert got["names"] == D.GXF_COLUMNS
            same(table(got, D.GXF_COLUMNS), expect(exp[m], range(10)))
        assert got["status"] == 1 and got["n_rows"] > 2700
        assert (st["n_double_fast"], st["n_double_patched"]) == (fast, patch)
        assert st["n_batches"] >= (3 if mb else 1)


def test_double_values_take_both_paths():
    import duckhts_amd as D
    toks = DBL_FAST + DBL_PATCH
    text = b"".join(b"r%d\t%s\n" % (i, t) for i, t in enumerate(toks))
    st = {}
    got = D.read_tabix(text, column_types=["VARCHAR", "DOUBLE"], stats=st)
    exp = M.scan(text, M.GENERIC, [M.T_VARCHAR, M.T_DOUBLE])
    same(table(got, got["names"]), expect(exp, range(2)))
    assert all(M.fast_path_takes(t) for t in DBL_FAST) and not any(M.fast_path_takes(t) for t in DBL_PATCH)
    assert (st["n_double_fast"], st["n_double_patched"]) == (len(DBL_FAST), len(DBL_PATCH))
    vals = dict(zip(toks, got["column1"]))
    assert vals[b"1e"] is None and vals[b"1.5x"] is None and vals[b"1e400"] == float("inf") and vals[b"0x1p-3"] == 0.125
    assert M.dbl_bits(float(vals[b"-0.0"])) == 1 << 63 and M.dbl_bits(float(vals[b"4.9e-324"])) == 1 and M.dbl_bits(float(vals[b"nan"])) == 0x7ff8000000000000
    assert isinstance(got["column1"][2], float)


# ---- bind ---------------------------------------------------------------------------------------------------------------------------------
def generic(src, meta=ord("#"), skip=0, header=False, header_names=None, column_types=None, auto_detect=False, columns=None, max_blocks=0):
    """read_tabix with a configuration no index supplies, through TabixScan: (schema, rows in projection order, batches)"""
    import duckhts_amd as D
    ctx = D.Context(0)
    try:
        ctx.open(src)
        ctx.L.dhts_bgzf_index(ctx.h)
        sc = D.TabixScan(ctx)
        sc.set_conf(meta, skip)
        sch = sc.bind(header, header_names, column_types, auto_detect)
        if columns is not None:
            sc.set_projection(columns)
        names = [sc.col_name(i) for i in sc.projection]
        out = {"n_rows": 0}
        out.update({k: [] for k in names})
        nb = 0
        while True:
            b = sc.next_batch(max_blocks)
            nb += 1
            out["n_rows"] += int(b.n_rows)
            if b.n_rows:
                for k, v in sc.batch_columns(b).items():
                    out[k].extend(v)
            if b.status != 0:
                assert b.status == 1
                break
        return sch, table(out, names), nb
    finally:
        ctx.close()


def model(text, meta=ord("#"), skip=0, **kw):
    b = M.bind(text, meta_char=meta, line_skip=skip, **kw)
    return b, M.scan(text, M.GENERIC, b["types"], meta, skip, b["skip_header_line"])


def check_bind(text, **kw):
    sch, rows, _ = generic(text, **kw)
    b, exp = model(text, **kw)
    assert {k: sch[k] for k in ("n_cols", "names", "types", "skip_header_line")} == b
    same(rows, expect(exp, range(b["n_cols"])))
    return sch, rows


def test_schema_of_a_300_field_line():
    text = b"\t".join(b"f%d" % i for i in range(300)) + b"\nshort\t1\n"
    sch, rows = check_bind(text)
    assert sch["n_cols"] == 256 and rows[0][255] == b"f255" and rows[1][:3] == [b"short", b"1", None]


def test_header_with_and_without_line_skip():
    text = b"#meta\nskipped one\tx\n\n chrom \tpos\t\nchr1\t1\t2.5\nchr1\t2\t.\n"
    sch, rows = check_bind(text, header=True)                                  # the first data line is the header line, and is skipped
    assert sch["names"] == ["skipped one", "x"] and sch["skip_header_line"] and len(rows) == 3
    sch, rows = check_bind(text, header=True, skip=3)                          # "#meta" counts against line_skip; the last skipped line names the columns
    assert sch["names"] == ["chrom", "pos", "column2"] and not sch["skip_header_line"] and rows[0] == [b"chr1", b"1", b"2.5"]
    sch, rows = check_bind(text, skip=1)
    assert sch["names"] == ["column0", "column1"] and len(rows) == 4
    check_bind(text, header=True, skip=50)                                     # more than the file has: the last line is the candidate, no rows
    check_bind(b"", header=True)
    check_bind(b"\n\n#only meta\n", header=True, auto_detect=True)


def test_header_names_shorter_and_longer_than_the_lines():
    text = b"a\t1\t2\t3\nb\t4\n"
    sch, rows = check_bind(text, header_names=["x", "y"])
    assert rows == [[b"a", b"1"], [b"b", b"4"]]
    sch, rows = check_bind(text, header_names=["x", "", "z", "w", "v"], header=True)
    assert sch["names"] == ["x", "column1", "z", "w", "v"] and rows == [[b"b", b"4", None, None, None]]


def test_column_types():
    import duckhts_amd as D
    text = b"a\t1\t2.5\t7\nb\tx\t1e400\t99999999999\n"
    sch, rows = check_bind(text, column_types=["string", "LONG", "real", "int"])
    assert sch["types"] == [M.T_VARCHAR, M.T_BIGINT, M.T_DOUBLE, M.T_INTEGER] and rows[1][1] is None and rows[1][3] == 99999999999
    sch, rows = check_bind(text, column_types=["geometry", "bigint", "Float", "nope"])
    assert sch["types"] == [M.T_VARCHAR, M.T_BIGINT, M.T_DOUBLE, M.T_VARCHAR]
    with pytest.raises(D.DhtsError, match="column_types length does not match detected column count"):
        generic(text, column_types=["VARCHAR", "BIGINT"])
    check_bind(text, column_types=["BIGINT", "BIGINT"], header_names=["p", "q"])


@pytest.mark.parametrize("odd_row", [99, 100])
def test_auto_detect_decides_over_exactly_100_rows(odd_row):
    L = [b"r%d\t%d\t%d\t%s" % (i, i, i, b"." if i % 2 else b"7") for i in range(120)]
    f = L[odd_row].split(b"\t"); f[1] = b"word"; f[2] = b"2.5"; L[odd_row] = b"\t".join(f)
    sch, rows = check_bind(b"#m\n" + b"\n".join(L) + b"\n", auto_detect=True)
    if odd_row == 99:
        assert sch["types"] == [M.T_VARCHAR, M.T_VARCHAR, M.T_DOUBLE, M.T_BIGINT]
    else:
        assert sch["types"] == [M.T_VARCHAR, M.T_BIGINT, M.T_BIGINT, M.T_BIGINT] and rows[100][1] is None and rows[100][2] is None
    check_bind(b"#m\n" + b"\n".join(L) + b"\n", auto_detect=True, column_types=["VARCHAR"] * 4)      # ignored beside column_types


# ---- skips across batches ---------------------------------------------------------------------------------------------------------------------
def test_line_skip_and_header_line_across_batches():
    big = [b"skip%d\t" % i + b"x" * 50000 for i in range(2)]
    L = [big[0], b"", b"#meta counts", big[1], b"#meta does not count any more", b"", b"name\tvalue\tscore"]
    L += [b"r%d\t%d\t%d.5" % (i, i * 3, i) for i in range(5000)]
    text = b"\n".join(L) + b"\n"
    z = containers(text)["bgzf"]
    kw = dict(skip=3, header=True, header_names=["a", "b", "c"], column_types=["VARCHAR", "BIGINT", "DOUBLE"])
    b, exp = model(text, **kw)
    assert b["skip_header_line"] and len(exp) == 5000 and exp[0][0] == b"r0"
    sch, whole, nb1 = generic(z, **kw)
    sch2, cut, nb = generic(z, max_blocks=1, **kw)                              # the first batch holds one whole line, the second none
    assert nb >= 4 and sch == sch2
    same(whole, expect(exp, range(3)))
    same(cut, whole)
    # header names from the skip prefix: the line behind it is a row
    b, exp = model(text, skip=3, header=True)
    assert b["names"][0] == "skip1" and not b["skip_header_line"] and exp[0][0] == b"name"
    sch, rows, nb = generic(z, skip=3, header=True, max_blocks=1, columns=[0])
    assert sch["names"] == b["names"]
    same(rows, expect(exp, [0]))


# ---- projections ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [[c] for c in range(10)] + [[9, 4, 0], [5, 8, 3], []], ids=lambda c: "+".join(map(str, c)) or "none")
def test_projections(corner, cols):
    import duckhts_amd as D
    text, files, exp = corner
    got = D.read_gff(files["bgzf"], columns=cols, attributes_map=True, max_blocks=2)
    names = [D.GXF_COLUMNS[i] for i in cols]
    assert sorted(k for k in got if k in D.GXF_COLUMNS) == sorted(names) and got["n_rows"] == len(exp[M.GFF])
    same(table(got, names), expect(exp[M.GFF], cols))


def test_projection_of_a_generic_schema(corner):
    text, files, exp = corner
    sch, rows, _ = generic(files["gzip"], column_types=GXF_TYPE_NAMES, columns=[5, 0, 3], max_blocks=1)
    same(rows, expect(exp[M.GENERIC], [5, 0, 3]))
    sch, rows, _ = generic(files["plain"], columns=[])
    assert len(rows) == len(exp[M.GENERIC])


# ---- attribute grammars ------------------------------------------------------------------------------------------------------------------------
P40 = [(b"k%d" % i, b"v%d" % i) for i in range(40)]
ATTR_CASES = [
    # (field 8 or None for a line without it, GFF pairs, GTF pairs)
    (b'gene_id "a;b"; n 5', [], [(b"gene_id", b"a;b"), (b"n", b"5")]),
    (b'tag "never closed; x=1', [(b"x", b"1")], [(b"tag", b"never closed; x=1")]),
    (b"ID=1;bare", [(b"ID", b"1")], [(b"ID=1", b""), (b"bare", b"")]),
    (b";; ID = 1 ;;=novalue;k=; ", [(b"ID", b"1"), (b"k", b"")], [(b"ID", b"= 1"), (b"=novalue", b""), (b"k=", b"")]),
    (b"keyonly", [], [(b"keyonly", b"")]),
    (b'"" x; a ""', [], [(b'""', b"x"), (b"a", b"")]),
    (b".", None, None),
    (b"", None, None),
    (None, None, None),
    (b";".join(k + b"=" + v for k, v in P40), P40, [(k + b"=" + v, b"") for k, v in P40]),
    (b"; ".join(k + b' "' + v + b'"' for k, v in P40), [], P40),
    (b"ID=" + b"v" * 300 + b';k "' + b"w" * 300 + b'"', [(b"ID", b"v" * 300)], [(b"ID=" + b"v" * 300, b""), (b"k", b"w" * 300)]),
    (b"a=1; ;", [(b"a", b"1")], [(b"a=1", b"")]),
]


@pytest.mark.parametrize("mode", ["gff", "gtf"])
def test_attribute_grammars(mode):
    import duckhts_amd as D
    lines = [b"\t".join(BASE[:8] + ([f] if f is not None else [])) for f, _, _ in ATTR_CASES]
    text = b"\n".join(lines) + b"\n"
    fn, m, k = (D.read_gff, M.GFF, 1) if mode == "gff" else (D.read_gtf, M.GTF, 2)
    got = fn(text, attributes_map=True, columns=["attributes_map", "attributes"])
    written = [c[k] for c in ATTR_CASES]
    assert [r[9] for r in M.scan(text, m)] == written                        # the model agrees with what is written out above
    assert got["attributes_map"] == written
    assert got["attributes"] == [f if f not in (None, b"", b".") else b"." for f, _, _ in ATTR_CASES]


# ---- regions ----------------------------------------------------------------------------------------------------------------------------------
CONF_GFF = (0, 1, 4, 5, ord("#"), 0)
CONF_SKIP2 = (0, 1, 4, 5, ord("#"), 2)


def sorted_gff():
    L = [b"##gff-version 3"]
    for s, name in enumerate((b"seqA", b"seqB", b"seqC")):
        for i in range(2000):
            beg = i * 50 + 1 + s
            L.append(b"%s\tsrc\texon\t%d\t%d\t%d.5\t+\t.\tID=e%d_%d" % (name, beg, beg + 29 + (i % 5) * 20, i % 50, s, i))
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


@pytest.fixture(scope="module")
def region_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("tabix_region")
    text = sorted_gff()
    z = containers(text)["bgzf"]
    assert len(text) > 3 * 65280
    path = str(d / "sorted.gff.gz")
    open(path, "wb").write(z)
    open(path + ".tbi", "wb").write(build_index(z, CONF_GFF, 0))
    open(str(d / "elsewhere.csi"), "wb").write(build_index(z, CONF_GFF, 14))
    open(str(d / "skip2.tbi"), "wb").write(build_index(z, CONF_SKIP2, 0))
    noidx = str(d / "noindex.gff.gz")
    open(noidx, "wb").write(z)
    names = [b"seqA", b"seqB", b"seqC"]
    return {"dir": str(d), "path": path, "noidx": noidx, "text": text, "size": len(z), "conf": CONF_GFF + ([n.decode() for n in names],)}


# row 100 of seqB is [5002, 5031] (1-based, closed): the ranges touch its ends from both sides.  (A comma always separates regions here.)
REGIONS = ["seqB", "seqB:5002-5002", "seqB:5001-5001", "seqB:5031-5031", "seqB:5032-5032", "seqA:20001-30000", "seqC:200000-300000",
           "seqA:1-3000,seqA:2000-4000", "seqC:1-500,nosuch:1-10,seqA:1-500", "nosuch,alsonot:5-9", " seqB:100-900 ,, \tseqA:7-90 , ", "seqC,seqA"]


@pytest.mark.parametrize("index", ["tbi", "csi"])
@pytest.mark.parametrize("region", REGIONS)
def test_region_rows(region_files, region, index):
    import duckhts_amd as D
    exp = M.region_scan(region_files["text"], region_files["conf"], region, M.GFF)
    st = {}
    got = D.read_gff(region_files["path"], region=region, attributes_map=True, stats=st,
                     index_path=None if index == "tbi" else os.path.join(region_files["dir"], "elsewhere.csi"))
    assert got["status"] == 1
    same(table(got, D.GXF_COLUMNS), expect(exp, range(10)))
    if region in ("seqC:200000-300000", "nosuch,alsonot:5-9"):
        assert exp == []
    else:
        assert 0 < len(exp) <= 4000
    if region == "seqA:1-3000,seqA:2000-4000":
        ids = [r[8] for r in exp]
        assert len(set(ids)) < len(ids)                                      # overlapping regions repeat rows
    if "," not in region and region != "seqB":
        assert st["resident_bytes"] < region_files["size"]                   # one region: only its index windows were staged


def test_region_generic_mode_and_skip_rules_inside_a_window(region_files):
    import duckhts_amd as D
    text, path = region_files["text"], region_files["path"]
    types = ["VARCHAR", "VARCHAR", "VARCHAR", "BIGINT", "BIGINT", "DOUBLE", "VARCHAR", "VARCHAR", "VARCHAR"]
    exp = M.region_scan(text, region_files["conf"], "seqA:1-700", M.GENERIC, M.GXF_TYPES)
    # header := true takes the first data line for the names and a sequential scan skips it; a window does not
    got = D.read_tabix(path, region="seqA:1-700", header=True, column_types=types)
    assert got["names"][0] == "seqA" and got["names"][8] == "ID=e0_0"
    same(table(got, got["names"]), expect(exp, range(9)))
    assert exp[0][3] == 1
    seq = D.read_tabix(path, header=True, column_types=types)
    assert seq["n_rows"] == 5999 and seq[seq["names"][3]][0] == 51
    # an index that says line_skip = 2: the sequential scan passes over two lines, a window over none
    idx = os.path.join(region_files["dir"], "skip2.tbi")
    seq = D.read_tabix(path, index_path=idx, column_types=types)
    assert seq["n_rows"] == 5999 and seq["column3"][0] == 51
    got = D.read_tabix(path, index_path=idx, region="seqB:1-700,seqA:40-700", column_types=types)
    conf = CONF_SKIP2 + (region_files["conf"][6],)
    same(table(got, got["names"]), expect(M.region_scan(text, conf, "seqB:1-700,seqA:40-700", M.GENERIC, M.GXF_TYPES), range(9)))
    assert got["n_rows"] > 20


def test_region_errors(region_files):
    import duckhts_amd as D
    with pytest.raises(D.DhtsError, match="Region query requested but no tabix index found for: " + region_files["noidx"].replace(".", r"\.")):
        D.read_gff(region_files["noidx"], region="seqA")
    with pytest.raises(D.DhtsError, match="Region query requested but no tabix index found for: "):
        D.read_tabix(region_files["path"], region="seqA", index_path=os.path.join(region_files["dir"], "missing.tbi"))
    got = D.read_tabix(region_files["path"], region="nosuch")
    assert got["n_rows"] == 0 and got["status"] == 1 and got["column0"] == []
    assert D.read_gff(region_files["noidx"], region=" , ")["n_rows"] == 6000    # no region is left: a sequential scan, no index needed


def test_refusals_on_a_tabix_context():
    import duckhts_amd as D
    L = D.lib()
    ctx = D.Context(0)
    try:
        ctx.open(b"c\t1\t2\n")
        L.dhts_bgzf_index(ctx.h)
        sc = D.TabixScan(ctx, D.TABIX_GFF)
        with pytest.raises(D.DhtsError, match="read_gff: region queries need a BGZF file"):
            sc.set_region("c:1-2")
        with pytest.raises(D.DhtsError, match="a shard is not supported on a tabix text context"):
            ctx.set_shard(0, 2)
        assert L.dhts_bam_set_block_range(ctx.h, 0, 1, 0) < 0 and b"a block range is not supported on a tabix text context" in L.dhts_error(ctx.h)
        L.dhts_tabix_build_index.restype = C.c_int64; L.dhts_tabix_build_index.argtypes = [C.c_void_p] + [C.c_int] * 7
        assert L.dhts_tabix_build_index(ctx.h, 0, 1, 4, 5, ord("#"), 0, 0) < 0 and b"tabix_index is not supported on a tabix text context" in L.dhts_error(ctx.h)
        with pytest.raises(D.DhtsError, match="fixed"):
            sc.set_conf(ord("#"), 1)
        with pytest.raises(D.DhtsError, match="bad projection"):
            sc.set_projection([10])
        b = sc.next_batch()
        assert b.n_rows == 1 and b.status == 1
    finally:
        ctx.close()


# ---- the golden fixtures, with the answers the reference records (test/sql/duckhts.test:406-519) ---------------------------------------------------
def test_golden_gff():
    import collections
    import duckhts_amd as D
    p = os.path.join(GOLD, "gff_file.gff.gz")
    text = gzip.decompress(open(p, "rb").read())
    got = D.read_gff(p, attributes_map=True)
    assert got["n_rows"] == 62
    same(table(got, D.GXF_COLUMNS), expect(M.scan(text, M.GFF), range(10)))
    assert [got[k][0] for k in D.GXF_COLUMNS[:5]] == [b"X", b"Vega", b"exon", 2934816, 2935190]
    assert collections.Counter(got["feature"]) == {b"exon": 23, b"intron": 19, b"CDS": 15, b"transcript": 4, b"gene": 1}
    assert sum(m is not None for m in got["attributes_map"]) == 62 and set(got["score"]) == {None}
    assert D.read_gff(p, columns=["feature"])["feature"][0] == b"exon"
    t = D.read_tabix(p, columns=[0, 2])
    assert t["n_rows"] == 62 and len(t["names"]) == 9 and list(zip(t["column0"], t["column2"]))[:2] == [(b"X", b"exon"), (b"X", b"gene")]
    for fn in (D.read_gff, D.read_tabix):
        a, b = fn(p, region="X:2934816-2935190", columns=[])["n_rows"], fn(p, region="X:2937010-2937500", columns=[])["n_rows"]
        assert (a, b) == (4, 3) and fn(p, region="X:2934816-2935190,X:2937010-2937500", columns=[])["n_rows"] == 7


def test_golden_meta_and_header_tabix():
    import duckhts_amd as D
    meta, hdr = os.path.join(GOLD, "meta_tabix.tsv.gz"), os.path.join(GOLD, "header_tabix.tsv.gz")
    got = D.read_tabix(meta)
    assert (got["column0"][0], got["column1"][0]) == (b"chr1", b"1")
    got = D.read_tabix(meta, header_names=["chrom", "pos", "value"])
    assert got["names"] == ["chrom", "pos", "value"] and (got["chrom"][0], got["pos"][0]) == (b"chr1", b"1")
    got = D.read_tabix(meta, auto_detect=True)
    assert got["types"][1] == M.T_BIGINT and got["column1"][0] == 1
    got = D.read_tabix(hdr, header=True)
    assert got["names"] == ["chrom", "pos", "value"] and (got["chrom"][0], got["pos"][0]) == (b"chr1", b"1")
    got = D.read_tabix(hdr, header=True, column_types=["VARCHAR", "BIGINT", "VARCHAR"])
    assert got["pos"][0] + 1 == 2
    for p, kw in ((meta, {}), (meta, {"auto_detect": True}), (hdr, {"header": True})):
        text = gzip.decompress(open(p, "rb").read())
        conf = M.tbi_conf(open(p + ".tbi", "rb").read())
        b, exp = model(text, meta=conf[4], skip=conf[5], **kw)
        got = D.read_tabix(p, **kw)
        assert (got["names"], got["types"]) == (b["names"], b["types"])
        same(table(got, got["names"]), expect(exp, range(b["n_cols"])))
