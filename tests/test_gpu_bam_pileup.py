"""bam_pileup on the device (dhts_bam_pileup_*, csrc/bam_pileup.hip) against the CPU model bam_pileup_ref, row for row: tid, pos, strand,
nucleotide, count, the counters and the stats; every comparison is exact.  SEQ and QUAL at every offset, the operations and the insertion
anchors, the edges of rows and tiles, many reads on few positions, pages of every size, min_nucleotide_depth, regions, the table cap, the
parameter ranges, the ABI's states, the cross-check against bam_depth on the device, and seeded random files.  Every add form the library
has is run through the debug hook."""
import ctypes as C

import numpy as np
import pytest

import bam_coverage_cases as K
import bam_pileup_cases as P
import bam_pileup_ref as M
import duckhts_amd
from conftest import read_golden
from test_gpu_bam_coverage import CIGARS, low_at, parse_rows, ramp

pytestmark = pytest.mark.gpu
R = K.read
FORMS = [1, 2]                                                             # direct, window
FILTERS = tuple(M.DEFAULTS)
form_param = pytest.mark.parametrize("form", FORMS)


def model_params(kw):
    return {**M.DEFAULTS, **{k: v for k, v in kw.items() if k in FILTERS}}     # the Python function's defaults


def same(got, exp, rows=None, strands=1):
    assert {k: got["stats"][k] for k in M.COUNTERS} == exp["stats"]
    assert sum(got["stats"][k] for k in M.COUNTERS[1:]) == got["stats"]["n_rows"]
    assert got["n_rows"] == exp["n_rows"] == got["stats"]["n_result_rows"] == sum(got["pages"])
    for k, dt in zip(duckhts_amd.PILEUP_COLUMNS, duckhts_amd.PILEUP_DTYPES):
        assert got[k].dtype == dt and len(got[k]) == exp["n_rows"]
        want = np.array([ord(c) for c in exp[k]], dt) if k in ("strand", "nucleotide") else np.array(exp[k], dt)
        assert np.array_equal(got[k], want), (k, got[k].tolist()[:40], want.tolist()[:40])
    if rows is not None:
        assert got["stats"]["n_target_rows"] == len(rows) and got["stats"]["table_bytes"] == M.table_bytes(rows, strands)


def check(data, form, **kw):
    got = duckhts_amd.bam_pileup(data, add_form=form, **kw)
    refs, reads = M.reads_from_bam(data)
    p = model_params(kw)
    same(got, M.pileup(reads, refs, **p), rows=[(t, 0, l) for t, (_, l) in enumerate(refs)], strands=p["distinguish_strands"])
    assert got["status"] == 1 and got["contigs"] == [n for n, _ in refs]
    return got


def check_region(data, form, region, index=None, **kw):
    """the model's reads are the rows of read_bam's own region query"""
    scanned = duckhts_amd.read_bam(data, region=region, index=index)
    refs, _ = M.reads_from_bam(data)
    rows = parse_rows(refs, region)
    got = duckhts_amd.bam_pileup(data, region=region, index=index, add_form=form, **kw)
    p = model_params(kw)
    same(got, M.pileup(M.reads_from_cols(scanned), refs, rows=rows, **p), rows=rows, strands=p["distinguish_strands"])
    assert got["stats"]["n_rows"] == scanned["n_rows"]
    return got


def open_ctx(data, form=0):
    ctx = duckhts_amd.Context(0)
    ctx.open(data)
    ctx.bgzf_index()
    ctx.bam_open()
    if form:
        ctx.bam_pileup_add_form(form)
    return ctx


def drain(ctx, max_rows=0, columns=None):
    parts = []
    while True:
        cols, st = ctx.bam_pileup_next(max_rows, columns)
        parts.append(cols)
        if st:
            return {k: None if parts[0][k] is None else np.concatenate([p[k] for p in parts]) for k in duckhts_amd.PILEUP_COLUMNS}, [p["n_rows"] for p in parts]


def seq_of(n, k=0):
    """n bases that differ from their neighbours and from read to read, every 4-bit code among them"""
    return "".join(P.NT16[(5 * i + 3 * k + i // 16) % 16] if (i + k) % 5 == 0 else "ACGT"[(i * 7 + k + i // 4) % 4] for i in range(n))


def RS(flag, tid, pos0, mapq, cigar, qual, k=0, **kw):
    """a read whose sequence is seq_of(its query length)"""
    n = K.qlen_of(kw.get("cg", cigar))
    return R(flag, tid, pos0, mapq, cigar, qual, seq=seq_of(n, k) if n else "*", **kw)


BOTH = [dict(include_deletions=d, include_insertions=i) for d in (0, 1) for i in (0, 1)]


# ---- 1. SEQ and QUAL extraction ----
M_LENGTHS = [1, 2, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 257]


@form_param
@pytest.mark.parametrize("min_baseq", [0, 20])
def test_seq_and_qual_at_every_offset_mod_16(form, min_baseq):
    # the qname's length moves CIGAR, SEQ and QUAL by a byte each; odd and even l_seq move QUAL by (l_seq + 1) / 2
    reads = [RS(16 * (i & 1), 0, 1000 + i, 30, f"{30 + (i * 3 + j) % 9}M", lambda k: 5 + (k * 11) % 40, k=i, qname="q" * (1 + i % 16)) for i in range(32) for j in (0, 1)]
    seq_offs, qual_offs, p = set(), set(), 0
    for i, r in enumerate(reads):
        seq_offs.add((p + 36 + len(r["qname"]) + 1 + 4) % 16)
        qual_offs.add((p + 36 + len(r["qname"]) + 1 + 4 + (K.qlen_of(r["cigar"]) + 1) // 2) % 16)
        p += len(K.record(i, r))
    assert seq_offs == qual_offs == set(range(16))
    check(K.bam(K.REFS, reads), form, min_baseq=min_baseq)


@form_param
@pytest.mark.parametrize("min_baseq", [0, 20])
def test_m_lengths_and_odd_query_starts(form, min_baseq):
    reads = [RS(16 * (i & 1), 0, 1000 + 300 * i, 30, f"{n}M", ramp, k=i, qname="n" * (1 + i)) for i, n in enumerate(M_LENGTHS)]
    # an odd-length S and an odd-length I in front of an M: the query index is odd where the piece starts
    reads += [RS(0, 1, 1000 + 300 * i, 30, f"{s}S{n}M", ramp, k=i, qname="s" * (1 + i)) for i, (s, n) in enumerate([(1, 40), (3, 33), (5, 17), (15, 16), (17, 129), (2, 31)])]
    reads += [RS(16, 1, 5000 + 300 * i, 30, f"{a}M{ins}I{n}M", ramp, k=i, qname="i" * (2 + i)) for i, (a, ins, n) in enumerate([(4, 1, 40), (7, 3, 33), (16, 5, 129), (1, 1, 1), (30, 2, 20)])]
    reads.append(R(0, 2, 100, 30, "16M", 30, seq=P.NT16))                                       # all sixteen codes in one read
    reads.append(R(16, 2, 101, 30, "1S16M", 30, seq="A" + P.NT16[::-1]))                        # ... from an odd query index
    reads.append(R(0, 2, 300, 30, "10M", [], seq="*"))                                          # SEQ = *: ten N whatever min_baseq is
    reads.append(R(0, 2, 400, 30, "9M", b"\xff" * 9, seq="ACGTACGTA"))                          # 0xff qualities
    reads.append(RS(0, 2, 500, 30, "1S1N", ramp, cg="30M5D2I30M10N17M"))                        # the real CIGAR in the CG tag
    got = check(K.bam(K.REFS, reads), form, min_baseq=min_baseq, include_insertions=1)
    on3 = got["tid"] == 2
    assert bytes(got["nucleotide"][on3 & (got["pos"] > 300) & (got["pos"] <= 310)]) == b"N" * 10
    assert bytes(got["nucleotide"][on3 & (got["pos"] > 400) & (got["pos"] <= 409)]) == b"ACGTACGTA"


@form_param
@pytest.mark.parametrize("min_baseq", [1, 20, 31, 255])
def test_low_bases_on_both_sides_of_every_16_byte_boundary(form, min_baseq):
    reads = [RS(0, 0, 1000, 30, "40M", low_at(40, {0})), RS(0, 0, 1100, 30, "40M", low_at(40, {39})), RS(16, 0, 1300, 30, "40M", 3),
             RS(0, 0, 1400, 30, "41M", low_at(41, set(range(0, 41, 2)))), RS(0, 0, 1500, 30, "41M", low_at(41, set(range(1, 41, 2)))),
             RS(0, 0, 1600, 30, "20M3D20M", low_at(40, {19, 20})), RS(0, 0, 1700, 30, "20M3I20M", low_at(43, {19, 23}))]
    reads += [RS(0, 1, 2000 + 100 * j, 30, "64M", low_at(64, {j, j + 16, j + 32}), k=j, qname="n" * (1 + j % 5)) for j in range(16)]
    reads += [RS(16, 1, 5000 + 100 * j, 30, "32M1D32M", low_at(64, set(range(64)) - {j, j + 17, j + 40}), k=j) for j in range(16)]
    check(K.bam(K.REFS, reads), form, min_baseq=min_baseq, include_insertions=1)


@form_param
def test_a_cigar_longer_than_l_seq_ends_the_stream_with_its_rows_counted(form):
    reads = [RS(0, 0, 1000, 30, "20M", 30), R(0, 0, 1100, 30, "20M", [30] * 10, seq="ACGTACGTAC", l_seq=10), RS(0, 0, 1200, 30, "20M", 30)]
    data = K.bam(K.REFS, reads)
    got = duckhts_amd.bam_pileup(data, add_form=form)
    scanned = duckhts_amd.read_bam(data)
    refs, mreads = M.reads_from_bam(data)
    assert got["status"] < 0 and got["status"] == scanned["status"] and scanned["n_rows"] < 3
    same(got, M.pileup(mreads[:scanned["n_rows"]], refs, **M.DEFAULTS))
    reads[1] = R(4, 0, 1100, 30, "20M", [30] * 10, seq="ACGTACGTAC")                           # with FLAG & 4 the record is taken, and such a read contributes nothing
    got = check(K.bam(K.REFS, reads), form, exclude_flags=0)
    assert got["n_rows"] == 40 and got["stats"]["n_counted"] == 3


# ---- 2. operations ----
@form_param
@pytest.mark.parametrize("kw", BOTH, ids=str)
def test_every_cigar_operation(form, kw):
    reads = [RS(16 * (i & 1), i % 2, 1000 + 40 * i, 30, cg, lambda k: 12 + (k * 5) % 17, k=i) for i, cg in enumerate(CIGARS)]
    reads.append(RS(0, 2, 500, 30, "1S1N", ramp, cg="30M5D2I30M10N17M"))
    got = check(K.bam(K.REFS, reads), form, min_baseq=15, **kw)
    assert got["stats"]["n_counted"] == len(reads)
    assert (ord("-") in got["nucleotide"]) == bool(kw["include_deletions"]) and (ord("+") in got["nucleotide"]) == bool(kw["include_insertions"])


ANCHOR_CIGARS = ["5S3I10M", "10M2I5D3I10M", "10M100N2I10M", "10M2I2P3I10M", "3D2I", "4M0D2N0M3I4M", "4M2N1D3I4M", "2I4M1I", "10M1I1I10M"]


@form_param
@pytest.mark.parametrize("include_deletions", [0, 1])
def test_insertion_anchors_and_deletions_at_row_and_tile_edges(form, include_deletions):
    refs = [("a", 1000), ("b", 3000)]
    reads = [RS(16 * (i & 1), 1, 100 + 150 * i, 30, cg, ramp, k=i) for i, cg in enumerate(ANCHOR_CIGARS)]
    reads += [RS(0, 0, 0, 30, "3D5M", ramp), RS(0, 0, 990, 30, "8M6D8M", ramp), RS(0, 0, 995, 30, "2M3D", ramp), RS(16, 0, 997, 30, "3D5M", ramp),     # D at a row's first and last position
              RS(0, 1, 1015, 30, "8M6D8M", ramp), RS(0, 1, 1019, 30, "5M5D5M", ramp), RS(0, 1, 1014, 30, "10M4D4M", ramp), RS(0, 1, 2040, 30, "8D", ramp),  # ... at a tile's edge
              RS(0, 0, 990, 30, "10M2I", ramp), RS(0, 1, 2990, 30, "10M3I5M", ramp)]                                                                  # an I anchored on a row's last position
    got = check(K.bam(refs, reads), form, include_deletions=include_deletions, include_insertions=1)
    plus = sorted(zip(got["tid"][got["nucleotide"] == ord("+")].tolist(), got["pos"][got["nucleotide"] == ord("+")].tolist(), got["count"][got["nucleotide"] == ord("+")].tolist()))
    # 5S3I10M none; 10M2I5D3I10M on 260 and 265; ...100N2I... none; 10M2I2P3I10M twice on 560; 3D2I on 703; none; 4M2N1D3I4M on 1007; 2I4M1I on 1154; 10M1I1I10M twice on 1310
    assert plus == [(0, 1000, 1), (1, 260, 1), (1, 265, 1), (1, 560, 2), (1, 703, 1), (1, 1007, 1), (1, 1154, 1), (1, 1310, 2), (1, 3000, 1)]
    minus = got["pos"][(got["nucleotide"] == ord("-")) & (got["tid"] == 0)].tolist()
    assert minus == ([1, 2, 3, 998, 998, 999, 999, 1000, 1000] if include_deletions else [])     # (the + strand's rows, then the - strand's 3D5M at every position)


@form_param
def test_an_insertion_whose_anchor_lies_one_position_in_front_of_the_row(form):
    reads = [RS(0, 0, 90, 30, "10M2I10M", ramp), RS(0, 0, 91, 30, "10M2I10M", ramp), RS(16, 0, 105, 30, "5M1I5M", ramp)]
    got = check_region(K.bam(K.REFS, reads), form, "c1:101-110", include_insertions=1)
    sel = got["nucleotide"] == ord("+")
    assert list(zip(got["pos"][sel].tolist(), got["strand"][sel].tolist())) == [(101, ord("+")), (110, ord("-"))]     # the anchor 100 lies in front of the row


# ---- 3. edges of rows and tiles ----
TILE_REFS = [("zero", 0), ("one", 1), ("t1023", 1023), ("t1024", 1024), ("t1025", 1025), ("t3073", 3 * 1024 + 1)]
TILE_READS = [RS(0, 1, 0, 30, "1M", ramp), RS(16, 1, 0, 30, "5M", ramp),
              RS(0, 2, 0, 30, "10M", ramp), RS(16, 2, 1000, 30, "30M", ramp), RS(0, 2, 1022, 30, "1M", ramp),
              RS(0, 3, 1000, 30, "24M", ramp), RS(16, 3, 1023, 30, "5M", ramp), RS(0, 3, 500, 30, "10M5D10M", ramp),
              RS(0, 4, 1000, 30, "25M", ramp), RS(16, 4, 1020, 30, "10M", ramp), RS(0, 4, 1024, 30, "1M", ramp),
              RS(0, 5, 1000, 30, "60M", ramp), RS(16, 5, 1010, 30, "30M", ramp), RS(0, 5, 1023, 30, "2M", ramp), RS(16, 5, 60, 30, "10M", ramp, k=1), RS(0, 5, 63, 30, "3M1I3M", ramp, k=2),
              RS(0, 5, 3060, 30, "20M", ramp), RS(16, 5, 3072, 30, "1M", ramp), RS(0, 5, 5, 30, "3M", ramp),
              RS(0, 5, 0, 30, "1500M", ramp, k=3), RS(16, 5, 1500, 30, "1573M", ramp, k=4)]                      # every position of the last contig: a result of more than three pages of 1,025
PAGE_SIZES = [1, 2, 255, 256, 257, 1024, 1025, 0]


@pytest.fixture(scope="module")
def tile_file():
    data = K.bam(TILE_REFS, TILE_READS)
    refs, reads = M.reads_from_bam(data)
    return data, {s: M.pileup(reads, refs, **{**M.DEFAULTS, "include_insertions": 1, "distinguish_strands": s}) for s in (0, 1)}


@form_param
@pytest.mark.parametrize("strands", [0, 1])
def test_contigs_around_the_tile(tile_file, form, strands):
    data, exp = tile_file
    got = check(data, form, include_insertions=1, distinguish_strands=strands)
    assert got["n_rows"] == exp[strands]["n_rows"] > 3 * 1025 and sorted(set(got["tid"].tolist())) == [1, 2, 3, 4, 5]
    assert got["stats"]["table_bytes"] == (1024 * 2 + 2048 * 2 + 4096) * (64 if strands else 32)    # (the empty contig has no span)


@form_param
def test_a_read_over_two_adjacent_regions_and_regions_out_of_order(form):
    reads = [RS(0, 0, 85, 30, "60M", ramp), RS(16, 0, 95, 30, "10M", ramp), RS(0, 0, 99, 30, "1M", ramp), RS(16, 0, 100, 30, "1M", ramp), RS(0, 0, 90, 30, "8M6D8M", ramp),
             RS(0, 0, 104, 30, "5M20N5M", ramp), RS(16, 0, 60, 30, "20M", ramp), RS(0, 1, 95, 30, "30M", ramp), RS(0, 0, 140, 30, "3S10M", ramp), RS(0, 0, 96, 30, "4M2I4M", ramp)]
    region = "c1:121-130,c1:91-100,c2:100-100,c1:101-110,c1:141-141"
    for max_rows in (0, 7):
        got = check_region(K.bam(K.REFS, reads), form, region, min_baseq=15, include_insertions=1, max_rows=max_rows)
        assert got["pos"][0] >= 121 and got["tid"].tolist().count(1) == 1 and int(got["pos"][-1]) == 141


def test_regions_with_and_without_the_index():
    rng = read_golden("range.bam")
    bai = read_golden("range.bam.bai")
    region = "CHROMOSOME_I:1001-1100,CHROMOSOME_I:901-1000,CHROMOSOME_II:1-5000,CHROMOSOME_I:1101-1150,CHROMOSOME_I:1151-1151"
    for form in FORMS:
        a = check_region(rng, form, region, index=bai)
        b = check_region(rng, form, region, min_baseq=25, max_rows=77)                  # without the index: the whole file is scanned and filtered
        assert a["n_rows"] > 0 and b["n_rows"] > 0
    check_region(rng, 0, "CHROMOSOME_I", distinguish_strands=0)


@form_param
def test_last_kilobase_of_a_long_contig(form):
    n = (1 << 31) - 1
    refs = [("small", 5000), ("long", n)]
    reads = [RS(0, 0, 100 + i, 30, "10M", ramp) for i in range(10)] + [RS(16 * (i & 1), 1, n - 1000 + 7 * i, 30, "20M3D2I20M", ramp, k=i) for i in range(130)] + [RS(0, 1, n - 2, 30, "10M", ramp)]
    got = check_region(K.bam(refs, reads), form, f"long:{n - 999}-{n}", min_baseq=15, include_insertions=1)
    assert int(got["pos"][-1]) == n and n - 999 <= int(got["pos"][0]) <= n - 990 and got["n_rows"] > 1000


# ---- 4. many reads on few positions, reads around the window ----
@form_param
@pytest.mark.parametrize("n", [31, 32, 33, 63, 64, 65, 129])
def test_reads_around_a_turn(form, n):
    reads = [RS(16 * (i & 1), i % 3, 1000 + i, 30, "10M2D1I10M", ramp, k=i) for i in range(n)]
    got = check(K.bam(K.REFS, reads), form, min_baseq=15, include_insertions=1)
    assert got["stats"]["n_counted"] == n


@form_param
@pytest.mark.parametrize("order", ["sorted", "reverse"])
def test_reads_around_the_window(form, order):
    W = 512                                                                 # the window's positions (PIL_WINDOW): starts W - 1, W and W + 1 apart
    reads, pos = [], 100
    for step in (W - 1, W, W + 1, 10, W - 30, 5, 2 * W, 3):
        pos += step
        reads.append(RS(16 * (len(reads) & 1), 0, pos, 30, "40M2D1I40M", ramp, k=len(reads)))
    reads += [RS(0, 0, pos + 20, 30, f"10M{W + 5}N10M", ramp), RS(0, 0, pos + 30, 30, f"5M{W + 5}D5M", ramp), RS(16, 0, pos + W - 20, 30, "60M", ramp),   # an N and a D longer than the window; in and out
              RS(0, 1, 50, 30, "30M", ramp), RS(16, 1, 60, 30, "30M", ramp), RS(0, 2, 70, 30, "30M", ramp), RS(0, 2, 70 + 3 * W, 30, "30M", ramp)]               # three contigs inside one turn
    if order == "reverse":
        reads = reads[::-1]
    check(K.bam(K.REFS, reads), form, include_insertions=1)
    check(K.bam(K.REFS, reads), form, min_baseq=15, distinguish_strands=0)


@form_param
def test_5000_identical_reads_and_70000_one_base_reads(form):
    data = K.bam(K.REFS, [R(0, 0, 777, 30, "1M1D2M1I1M", [30, 10, 30, 30, 30], seq="ACGTT")] * 5000)
    got = check(data, form, min_baseq=20, include_insertions=1)
    assert M.as_rows(got) == [(0, 778, "+", "A", 5000), (0, 779, "+", "-", 5000), (0, 781, "+", "G", 5000), (0, 781, "+", "+", 5000), (0, 782, "+", "T", 5000)]
    data = K.bam(K.REFS, [R(16, 1, 4242, 30, "1M", 30, seq="G", qname="r")] * 70000)
    got = duckhts_amd.bam_pileup(data, add_form=form)                                            # no counter of 16 bits may wrap
    assert M.as_rows(got) == [(1, 4243, "-", "G", 70000)] and got["stats"]["n_counted"] == 70000


# ---- 5. paging and projection ----
@form_param
@pytest.mark.parametrize("max_rows", PAGE_SIZES)
def test_pages_of_every_size(tile_file, form, max_rows):
    data, exp = tile_file
    got = duckhts_amd.bam_pileup(data, add_form=form, include_insertions=1, max_rows=max_rows)
    same(got, exp[1])
    n = exp[1]["n_rows"]
    if max_rows:
        assert got["pages"][:-1] == [max_rows] * ((n - 1) // max_rows) and 0 <= got["pages"][-1] <= max_rows
    else:
        assert got["pages"] == [n]


@pytest.mark.parametrize("max_rows", [1, 2])
def test_a_position_cut_by_a_page(max_rows):
    reads = [R(0, 0, 50, 30, "1M", 30, seq="A"), R(0, 0, 50, 30, "1M", 30, seq="C"), R(16, 0, 50, 30, "1M", 30, seq="A")]
    got = check(K.bam(K.REFS, reads), 0, max_rows=max_rows)
    assert M.as_rows(got) == [(0, 51, "+", "A", 1), (0, 51, "+", "C", 1), (0, 51, "-", "A", 1)] and got["pages"] == ([1, 1, 1] if max_rows == 1 else [2, 1])


def test_projection(tile_file):
    data, exp = tile_file
    full = duckhts_amd.bam_pileup(data, include_insertions=1, max_rows=300)
    for cols in [[k] for k in duckhts_amd.PILEUP_COLUMNS] + [["tid", "pos", "strand", "nucleotide"], []]:
        got = duckhts_amd.bam_pileup(data, include_insertions=1, max_rows=300, columns=cols)
        assert got["n_rows"] == full["n_rows"] == exp[1]["n_rows"] and got["pages"] == full["pages"]
        for k in duckhts_amd.PILEUP_COLUMNS:
            assert (got[k] is None) if k not in cols else np.array_equal(got[k], full[k]), k
    ctx = open_ctx(data)
    try:
        ctx.bam_pileup_open(exclude_flags=0x704)
        ctx.bam_pileup_scan()
        b = duckhts_amd.BedBatch()
        ctx._chk(ctx.L.dhts_bam_pileup_next(ctx.h, 100, 1 << duckhts_amd.PILEUP_COLUMNS.index("nucleotide"), C.byref(b)))
        assert b.n_rows == 100 and b.n_cols == 5 and [bool(b.cols[i].fixed) for i in range(5)] == [False, False, False, True, False] and not b.cols[3].valid
        assert ctx.L.dhts_bam_pileup_batch_host_bytes(C.byref(b)) == 104
    finally:
        ctx.close()


# ---- 6. min_nucleotide_depth ----
@form_param
@pytest.mark.parametrize("depth", [1, 2, 1000])
def test_min_nucleotide_depth(form, depth):
    reads = [RS(16 * (i % 3 == 0), 0, 1000 + 2 * (i % 7), 30, "20M1D10M", ramp, k=i % 2) for i in range(40)]
    got = check(K.bam(K.REFS, reads), form, min_nucleotide_depth=depth)
    assert (got["n_rows"] == 0 and got["pages"] == [0]) if depth == 1000 else int(got["count"].min()) >= depth


# ---- 7. regions and the cap ----
def test_overlapping_regions_are_refused():
    rng = read_golden("range.bam")
    with pytest.raises(duckhts_amd.DhtsError) as e:
        duckhts_amd.bam_pileup(rng, region="CHROMOSOME_I:1-1000,CHROMOSOME_II:1-10,CHROMOSOME_I:1000-1200")
    assert str(e.value) == M.err_overlap("CHROMOSOME_I:1-1000", "CHROMOSOME_I:1000-1200")
    duckhts_amd.bam_pileup(rng, region="CHROMOSOME_I:1-1000,CHROMOSOME_I:1001-1200")       # adjacent


@pytest.mark.parametrize("strands", [0, 1])
def test_the_table_cap(strands):
    rng = read_golden("range.bam")
    refs, _ = M.reads_from_bam(rng)
    need = M.table_bytes([(t, 0, l) for t, (_, l) in enumerate(refs)], strands)
    ctx = open_ctx(rng)
    L = ctx.L
    try:
        L.dhts_debug_coverage_max_table_bytes(need - 1)
        with pytest.raises(duckhts_amd.DhtsError) as e:
            ctx.bam_pileup_open(distinguish_strands=strands)
        assert str(e.value) == M.err_table(need, need - 1, strands)
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_NOT_OPEN):    # an open that failed leaves nothing open
            ctx.bam_pileup_stats()
        L.dhts_debug_coverage_max_table_bytes(need)
        ctx.bam_pileup_open(distinguish_strands=strands)
        assert ctx.bam_pileup_stats()["table_bytes"] == need
    finally:
        L.dhts_debug_coverage_max_table_bytes(0)
        ctx.close()


# ---- 8. and 9. parameter ranges and states ----
def test_calls_in_the_wrong_state_and_refusals():
    rng = read_golden("range.bam")
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(rng)
        ctx.bgzf_index()
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_BAM_NOT_OPEN):
            ctx.bam_pileup_open()
        ctx.bam_open()
        b = ctx.next_batch(0, duckhts_amd.PILEUP_COLMASK)
        for call in (lambda: ctx.bam_pileup_accumulate(b), ctx.bam_pileup_scan, ctx.bam_pileup_stats, ctx.bam_pileup_next):
            with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_NOT_OPEN):
                call()
        for kw, msg in ((dict(min_mapq=256), M.err_range("min_mapq")), (dict(min_mapq=-1), M.err_range("min_mapq")), (dict(min_baseq=256), M.err_range("min_baseq")),
                        (dict(min_baseq=-1), M.err_range("min_baseq")), (dict(include_flags=65536), M.err_range("include_flags")), (dict(require_flags=-1), M.err_range("require_flags")),
                        (dict(exclude_flags=70000), M.err_range("exclude_flags")), (dict(min_read_len=-1), M.ERR_READ_LEN), (dict(include_deletions=2), M.err_switch("include_deletions")),
                        (dict(include_insertions=-1), M.err_switch("include_insertions")), (dict(distinguish_strands=2), M.err_switch("distinguish_strands")),
                        (dict(min_nucleotide_depth=0), M.ERR_MIN_DEPTH),
                        # wrong in two ways: the first in the order of the checks is reported
                        (dict(min_read_len=-1, min_mapq=256), M.ERR_READ_LEN), (dict(min_baseq=-1, include_flags=65536), M.err_range("min_baseq")),
                        (dict(require_flags=-1, exclude_flags=70000), M.err_range("require_flags")), (dict(include_deletions=2, exclude_flags=70000), M.err_range("exclude_flags")),
                        (dict(distinguish_strands=2, min_nucleotide_depth=0), M.err_switch("distinguish_strands"))):
            with pytest.raises(duckhts_amd.DhtsError) as e:
                ctx.bam_pileup_open(**kw)
            assert str(e.value) == msg
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_NOT_OPEN):
            ctx.bam_pileup_stats()
        with pytest.raises(duckhts_amd.DhtsError, match="bam_pileup: add form 7 is not built"):
            ctx.bam_pileup_add_form(7)
        # a shard or a block range of the file
        ctx.set_shard(0, 2)
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_SHARD):
            ctx.bam_pileup_open()
        ctx.set_shard(0, 1)
        ctx.bam_pileup_open()
        ctx.set_block_range(0, 1, 1)
        with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_SHARD):
            ctx.bam_pileup_scan()
    finally:
        ctx.close()


@form_param
def test_accumulate_after_a_page_two_batches_and_a_second_open(form):
    reads = [RS(16 * (i & 1), i % 3, 100 + 5 * i, 30, "10M1D1I4M", ramp, k=i) for i in range(12)]
    data = K.bam(K.REFS, reads, one_record_per_block=True)
    refs, mreads = M.reads_from_bam(data)
    kw = dict(min_baseq=15, include_deletions=1, include_insertions=1, distinguish_strands=1)
    ctx = open_ctx(data, form)
    try:
        ctx.bam_pileup_open(**kw)
        assert ctx.bam_pileup_stats()["n_result_rows"] == 0
        seen, stale = 0, None
        while True:
            b = ctx.next_batch(1, duckhts_amd.PILEUP_COLMASK)
            if stale is not None and b.n_rows:
                with pytest.raises(duckhts_amd.DhtsError, match=M.ERR_STALE):
                    ctx.bam_pileup_accumulate(stale)
                stale = None
            ctx.bam_pileup_accumulate(b)
            seen += int(b.n_rows)
            if seen == 1 and stale is None:
                stale = duckhts_amd.BamBatch()
                C.memmove(C.byref(stale), C.byref(b), C.sizeof(b))
            if seen == 5:                                                  # a whole result in the middle: the reads so far; the table and the counters stay intact
                exp = M.pileup(mreads[:seen], refs, **kw)
                cols, sizes = drain(ctx, 7)
                assert sum(sizes) == exp["n_rows"] and M.as_rows(cols) == M.as_rows(exp) and ctx.bam_pileup_stats()["n_result_rows"] == exp["n_rows"]
            if seen == 9:                                                  # one page of a result taken: the next accumulate starts the result over
                exp = M.pileup(mreads[:seen], refs, **kw)
                cols, st = ctx.bam_pileup_next(4)
                assert cols["n_rows"] == 4 and st == 0 and M.as_rows(cols) == M.as_rows(exp)[:4]
            if b.status:
                break
        exp = M.pileup(mreads, refs, **kw)
        assert ctx.bam_pileup_stats()["n_result_rows"] == 0                # (no result of the table as it is now was taken)
        cols, sizes = drain(ctx)
        assert sizes == [exp["n_rows"]] and M.as_rows(cols) == M.as_rows(exp)
        st = ctx.bam_pileup_stats()
        assert {k: st[k] for k in M.COUNTERS} == exp["stats"] and st["n_result_rows"] == exp["n_rows"] and st["status"] == 1
        cols, st = ctx.bam_pileup_next()                                    # behind the last page: nothing, and still the end
        assert cols["n_rows"] == 0 and st == 1
        whole = duckhts_amd.bam_pileup(data, add_form=form, exclude_flags=0, **kw)           # twelve batches against one
        assert M.as_rows(whole) == M.as_rows(exp)
        ctx.bam_pileup_open(distinguish_strands=0)                          # a second open zeroes everything
        st = ctx.bam_pileup_stats()
        assert st["n_rows"] == 0 and st["status"] == 0 and st["n_target_rows"] == 3 and st["n_result_rows"] == 0 and st["table_bytes"] == M.table_bytes([(t, 0, l) for t, (_, l) in enumerate(refs)], 0)
        cols, sizes = drain(ctx)
        assert sizes == [0]
    finally:
        ctx.close()


# ---- 10. the cross-check on the device: bam_depth's depths ----
def cross_check(data, form, **kw):
    got = check(data, form, include_deletions=1, include_insertions=1, **kw)
    n_ref = len(got["contigs"])
    key = got["tid"].astype(np.int64) * (1 << 32) + got["pos"]
    for with_del in (0, 1):
        dep = duckhts_amd.bam_depth(data, include_deletions=with_del, **kw)
        sel = np.isin(got["nucleotide"], list(b"ACGTN=-" if with_del else b"ACGTN="))
        k, inv = np.unique(key[sel], return_inverse=True)
        tot = np.bincount(inv, weights=got["count"][sel]).astype(np.int64)
        assert np.array_equal(k, dep["tid"].astype(np.int64) * (1 << 32) + dep["pos"]) and np.array_equal(tot, dep["depth"].astype(np.int64))
        assert {c: got["stats"][c] for c in M.COUNTERS} == {c: dep["stats"][c] for c in M.COUNTERS} and len(dep["contigs"]) == n_ref


@form_param
@pytest.mark.parametrize("min_baseq", [0, 25])
def test_the_bases_sum_to_bam_depth_on_the_golden_file(form, min_baseq):
    cross_check(read_golden("range.bam"), form, min_baseq=min_baseq)


@form_param
def test_the_bases_sum_to_bam_depth_on_2000_random_reads(form):
    cross_check(P.bam(P.RANDOM_REFS, P.random_reads(5, 2000, sorted_=True)), form, min_baseq=12, min_mapq=3)


# ---- 11. random files ----
RANDOM_SETS = [dict(), dict(include_insertions=1, min_baseq=20), dict(include_deletions=0, distinguish_strands=0, min_mapq=20), dict(exclude_flags=0, include_insertions=1, min_read_len=30),
               dict(require_flags=1, min_nucleotide_depth=2, include_insertions=1), dict(include_flags=16, distinguish_strands=0, include_insertions=1, min_baseq=41)]


@pytest.fixture(scope="module")
def random_file():
    return P.bam(P.RANDOM_REFS, P.random_reads(23, 200))


@form_param
@pytest.mark.parametrize("kw", RANDOM_SETS, ids=str)
def test_random_reads(random_file, form, kw):
    got = check(random_file, form, **kw)
    assert got["n_rows"] > 0


@form_param
def test_the_hand_written_table(form):
    data = P.hand_bam()
    for extra, rows in P.HAND_SETS:
        got = check(data, form, **{**P.HAND_PARAMS, **extra})
        assert M.as_rows(got) == rows and {k: got["stats"][k] for k in M.COUNTERS} == P.HAND_STATS
