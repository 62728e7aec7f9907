"""read_bam on FASTQ / FASTA text: record discovery and the device encoder (duckhts_amd/csrc/fastq_text.hip) in front of the unchanged BAM
record stage.

Every htslib fixture is read as committed, inside plain gzip, and re-wrapped in 777-byte BGZF blocks so that lines straddle blocks; the
encoder's records must equal tests/fastq_encode_ref.py byte for byte, and read_bam on the text must equal read_bam on the restatement's
BAM column for column.  The same holds with small batches (records straddle them) and for a few hundred generated files that mix
four-line and wrapped records, '@' / '+' / '>'-led quality lines, the edge cases of test_fastq_ref.py and damage at a random line."""
import gzip
import os
import random

import pytest

import bamwriter as W
import fastq_encode_ref as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "htslib_fastq")
FIXTURES = ["minimal", "multiline", "single", "interleaved", "r1", "r2"]
FILES = [n + e for n in FIXTURES for e in (".fq", ".fa")] + ["longline.fq", "mate_mismatch_r1.fq", "mate_mismatch_r2.fq", "odd_interleaved.fq"]
HEADER_ERROR = "Failed to read SAM/BAM/CRAM header"


def _forms(raw):
    """(name, bytes, dhts_bam_is_text of a FASTQ in that form; FASTA is 2 more)"""
    return [("plain", raw, 4), ("gzip", gzip.compress(raw), 4), ("bgzf777", W.bgzf_file(raw, payload=777), 3)]


def device_records(data, max_blocks=0):
    """-> (the BAM records the device encoder made, batch after batch, concatenated; their number; is_text; the scan's last status)"""
    import duckhts_amd
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(data)
        ctx.bgzf_index()
        hdr = ctx.bam_open()
        assert hdr["n_ref"] == 0 and hdr["text"] in (b"", "")
        got, n = [], 0
        while True:
            b = ctx.next_batch(max_blocks)
            recs_b, nb = ctx.debug_fastq_records()
            assert nb == b.n_rows
            got.append(recs_b)
            n += nb
            if b.status != 0:
                break
        return b"".join(got), n, ctx.bam_is_text(), b.status
    finally:
        ctx.close()


def check(raw, data, kind=None, max_blocks=0, what=""):
    """the device's records and read_bam's columns for `data` (a form of the text `raw`) against the restatement"""
    import duckhts_amd
    recs, stopped = F.encode_text(raw)
    if F.detect(raw) is None or not recs:
        # the first record is refused: the header error; not raw reads at all by hts_detect_format2's rule: some refusal
        with pytest.raises(duckhts_amd.DhtsError, match=HEADER_ERROR if F.detect(raw) else None):
            duckhts_amd.read_bam(data)
        return 0
    got, n, is_text, status = device_records(data, max_blocks)
    assert n == len(recs) and got == b"".join(recs), what
    assert (status < 0) if stopped else (status == 1), (what, status, stopped)
    if kind is not None:
        assert is_text == kind + (2 if F.detect(raw) == "fasta" else 0), what
    exp = duckhts_amd.read_bam(F.fastq_to_bam(raw))
    t = duckhts_amd.read_bam(data, max_blocks=max_blocks)
    assert t["n_rows"] == exp["n_rows"] == len(recs), what
    assert (t["status"] < 0) if stopped else (t["status"] == 1), what
    for k in duckhts_amd.BAM_COLUMNS:
        assert list(t[k]) == list(exp[k]), (what, k)
    return len(recs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FILES)
def test_fastq_fixture_three_forms(name):
    raw = open(os.path.join(GOLD, name), "rb").read()
    for form, data, kind in _forms(raw):
        assert check(raw, data, kind, what=(name, form)) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", FILES)
def test_fastq_fixture_small_batches(name):
    raw = open(os.path.join(GOLD, name), "rb").read()
    for mb in (1, 2):
        assert check(raw, W.bgzf_file(raw, payload=97), 3, max_blocks=mb, what=(name, mb)) > 0


@pytest.mark.gpu
def test_read_bam_r1_columns():
    import duckhts_amd
    t = duckhts_amd.read_bam(open(os.path.join(GOLD, "r1.fq"), "rb").read())
    exp = [l.split("\t") for l in open(os.path.join(GOLD, "r1.sam")).read().split("\n") if l and not l.startswith("@")]
    assert t["n_rows"] == 5 and t["status"] == 1
    assert [q.decode() for q in t["QNAME"]] == [e[0] for e in exp] and [int(f) for f in t["FLAG"]] == [int(e[1]) for e in exp]
    assert [s.decode() for s in t["SEQ"]] == [e[9] for e in exp] and [q.decode() for q in t["QUAL"]] == [e[10] for e in exp]
    assert list(t["tid"]) == [-1] * 5 and list(t["mtid"]) == [-1] * 5 and t["header"]["n_ref"] == 0


BASES = b"ACGTNacgtnRYKMSWBDHV"


def _gen_record(rng, fasta, k):
    """one record's lines (without newlines)"""
    shape = rng.random()
    name = b"r%d" % k
    r = rng.random()
    if r < 0.15:
        name += rng.choice([b"/1", b"/2", b"/7", b"/x"])
    elif r < 0.2:
        name = rng.choice([b"/1", b"1", b"/", b"", b"n" * 254, b"n" * 252 + b"/2"])
    if rng.random() < 0.3:
        name += rng.choice([b" ", b"\t", b"  "]) + rng.choice([b"comment", b"1:N:0:ACGT", b"x/1", b""])
    n = 0 if shape < 0.05 else rng.randrange(1, 40) if shape < 0.6 else rng.randrange(40, 400)
    seq = bytes(rng.choice(BASES[:5] if rng.random() < 0.8 else BASES) for _ in range(n))
    qual = bytes(rng.randrange(33, 127) for _ in range(n))
    lead = rng.random()
    if n and lead < 0.3:
        qual = rng.choice([b"@", b"+", b">", b" "]) + qual[1:]
    lines = [(b">" if fasta else b"@") + name]
    if shape < 0.6 and rng.random() < 0.7:                     # one line each
        seq_lines, qual_lines = [seq], [qual]
        if n == 0 and rng.random() < 0.5:
            seq_lines = []
    else:                                                      # wrapped, the two parts not alike; empty lines in between
        def wrap(b):
            out, p = [], 0
            while p < len(b):
                w = rng.randrange(1, 80)
                out.append(b[p:p + w])
                p += w
                if rng.random() < 0.05:
                    out.append(b"")
            return out
        seq_lines, qual_lines = wrap(seq), wrap(qual)
        if not qual_lines or qual_lines[-1] == b"":
            qual_lines = [l for l in qual_lines if l] or [b""]
    lines += seq_lines
    if not fasta:
        lines.append(b"+" + (name if rng.random() < 0.2 else b""))
        lines += qual_lines
    return lines


def gen_file(rng, nrec=None):
    fasta = rng.random() < 0.25
    nrec = nrec if nrec is not None else rng.randrange(1, 60)
    lines = []
    for k in range(nrec):
        lines += _gen_record(rng, fasta, k)
    d = rng.random()
    if d < 0.35 and lines:                                     # damage at a random line
        i = rng.randrange(len(lines))
        kind = rng.randrange(5)
        if kind == 0:
            del lines[i]
        elif kind == 1:
            lines.insert(i, rng.choice([b"", b"ACGT", b"+", b"@x", b">y"]))
        elif kind == 2:
            lines[i] = lines[i] + b"A"
        elif kind == 3:
            lines[i] = lines[i][1:]
        else:
            lines = lines[:i + 1]                              # truncated
    eol = b"\r\n" if rng.random() < 0.2 else b"\n"
    text = eol.join(lines) + (eol if rng.random() < 0.85 else b"")
    return text


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", range(6))
def test_generated_files(chunk):
    rng = random.Random(20240 + chunk)
    rows = 0
    for k in range(50):                                        # 6 x 50 files, every one compared
        raw = gen_file(rng)
        form = rng.randrange(3)
        data = raw if form == 0 else gzip.compress(raw) if form == 1 else W.bgzf_file(raw, payload=rng.choice([61, 777, 4000]))
        mb = rng.choice([0, 0, 1, 3]) if form == 2 else 0
        rows += check(raw, data, max_blocks=mb, what=(chunk, k, form, mb))
    assert rows > 200


@pytest.mark.gpu
def test_many_records_cross_discovery_tiles_and_batches():
    """far more lines than one discovery tile (2048), records that straddle tiles and batches, '@'-led quality lines throughout"""
    rng = random.Random(7)
    lines = []
    for k in range(30000):
        lines += _gen_record(rng, False, k)
    raw = b"\n".join(lines) + b"\n"
    assert check(raw, W.bgzf_file(raw, payload=65280), 3, max_blocks=7, what="many") > 25000
    four = b"".join(b"@q%d\nACGTACGTAC\n+\n@@@@@@@@@@\n" % k for k in range(50000))
    assert check(four, four, 4, what="four-line") == 50000


@pytest.mark.gpu
def test_long_fasta_record_grows_the_carry():
    """a 3 MB chromosome is one read: with 2-block batches the carry grows until the next '>' (or the end of the file) completes it"""
    rng = random.Random(11)
    seq = bytes(rng.choice(b"ACGT") for _ in range(60 * 50000))
    body = b"\n".join(seq[p:p + 60] for p in range(0, len(seq), 60))
    raw = b">chrA first\n" + body + b"\n>chrB\nACGT\nAC\n"
    assert check(raw, W.bgzf_file(raw), 3, max_blocks=2, what="long fasta") == 2


@pytest.mark.gpu
def test_refusals_name_fastq_fasta():
    import duckhts_amd
    raw = open(os.path.join(GOLD, "r1.fq"), "rb").read()
    calls = [lambda c: c.set_regions("x"), lambda c: c.set_shard(1, 2), lambda c: c.load_index(b"BAI\1" + b"\0" * 8), lambda c: c.build_index()]
    for data in (raw, W.bgzf_file(raw)):
        for call in calls:
            ctx = duckhts_amd.Context(0)
            try:
                ctx.open(data)
                ctx.bgzf_index()
                ctx.bam_open()
                with pytest.raises(duckhts_amd.DhtsError, match="FASTQ/FASTA"):
                    call(ctx)
            finally:
                ctx.close()


@pytest.mark.gpu
def test_first_record_refused_keeps_the_header_error():
    import duckhts_amd
    for bad in (b"@XY\tAA:b\n", b"@r\nACGT\n+\nIII\n", b"@r\nACGT\n", b"@" + b"n" * 255 + b"\nA\n+\nI\n"):
        assert F.detect(bad) == "fastq"
        with pytest.raises(duckhts_amd.DhtsError, match=HEADER_ERROR):
            duckhts_amd.read_bam(bad)
    with pytest.raises(duckhts_amd.DhtsError, match=HEADER_ERROR):
        duckhts_amd.read_bam(b"@XY\tAA:b\n" + b"r\t0\t*\t0\t0\t*\t*\t0\t0\tA\tI\n")


@pytest.mark.gpu
def test_sam_hook_and_is_text_unchanged_for_sam():
    import duckhts_amd
    ctx = duckhts_amd.Context(0)
    try:
        ctx.open(b"@HD\tVN:1.6\nr\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\n")
        ctx.bgzf_index()
        ctx.bam_open()
        assert ctx.bam_is_text() == 2
        b = ctx.next_batch(0)
        assert b.n_rows == 1 and ctx.debug_sam_records()[1] == 1
        with pytest.raises(duckhts_amd.DhtsError):
            ctx.debug_fastq_records()
    finally:
        ctx.close()
