"""tests/hts_index_ref.py (the record-by-record model of htslib's index builder) against index files htslib itself wrote.  No GPU: this is
what entitles the model to judge the device writers in tests/test_gpu_index_writer.py.  Bin order inside a sequence is not compared (htslib
writes khash order)."""
import gzip
import os
import struct

import pytest

import bamwriter as bw
import hts_index_ref as R
from test_gpu_bam import _parse_bai
from test_gpu_bcf import _parse_csi
from test_vcf_region import index_vcf_gz, parse_tabix

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _gold(name):
    return open(os.path.join(GOLD, name), "rb").read()


@pytest.mark.parametrize("name", ["range.bam", "colons.bam"])
def test_model_reproduces_htslib_bai(name):
    exp = _parse_bai(_gold(name + ".bai"))
    got = R.bam_index(_gold(name)).parsed()
    assert got[1] == exp[1]
    assert len(got[0]) == len(exp[0])
    for t, (g, e) in enumerate(zip(got[0], exp[0])):
        assert g == e, (name, t)


def test_model_reproduces_htslib_bam_csi():
    """no_hdr_sq_1.bam.csi: a CSI of a BAM -- min_shift, the depth from the longest reference, every bin's loff"""
    exp = _parse_csi(R.maybe_gunzip(_gold("no_hdr_sq_1.bam.csi")))
    got = R.bam_index(_gold("no_hdr_sq_1.bam"), exp[0]).parsed()
    assert got == exp


def test_model_reproduces_htslib_sam_gz_csi():
    """rg.sam.gz.csi carries no tabix header: it is sam_index's CSI of bgzipped SAM text (the same pushes as for a BAM, offsets per line)"""
    exp = _parse_csi(R.maybe_gunzip(_gold("rg.sam.gz.csi")))
    assert exp[2] == 0
    assert R.sam_text_index(_gold("rg.sam.gz"), exp[0]).parsed() == exp


def test_model_reproduces_htslib_bcf_csi():
    exp = _parse_csi(gzip.decompress(_gold("vcf_file.bcf.csi")))
    got = R.bcf_index(_gold("vcf_file.bcf"), 14).parsed()
    assert got == exp


TABIX = [("index.vcf.gz", "index.vcf.gz.tbi", R.CONF_VCF, 0), ("index.vcf.gz", "index.vcf.gz.csi", R.CONF_VCF, None),
         ("formatcols.vcf.gz", "formatcols.vcf.gz.csi", R.CONF_VCF, None), ("no_contig.vcf.gz", "no_contig.vcf.gz.tbi", R.CONF_VCF, 0),
         ("gff_file.gff.gz", "gff_file.gff.gz.tbi", R.CONF_GFF, 0), ("header_tabix.tsv.gz", "header_tabix.tsv.gz.tbi", (0, 1, 2, 2, ord("#"), 1), 0),
         ("meta_tabix.tsv.gz", "meta_tabix.tsv.gz.tbi", (0, 1, 2, 2, ord("#"), 1), 0), ("rg.sam.gz", "rg.sam.gz.tbi", R.CONF_SAM, 0)]


@pytest.mark.parametrize("data,index,conf,min_shift", TABIX, ids=[t[1] for t in TABIX])
def test_model_reproduces_htslib_tabix(data, index, conf, min_shift):
    exp = parse_tabix(_gold(index))
    if min_shift is None:                           # a CSI: built with the min_shift the file records (the depth is the model's to find)
        min_shift = exp["min_shift"]
    assert tuple(exp["conf"]) == conf
    idx, names = R.tabix_index(index_vcf_gz() if data == "index.vcf.gz" else _gold(data), conf, min_shift)
    assert idx.parsed(exp["conf"], names) == exp


def test_adjust_csi_settings():
    """hts_adjust_csi_settings: levels grow by 8x until length + 256 fits; beyond nine levels min_shift grows"""
    assert R.adjust_csi_settings(0, 14, 0) == (14, 0)
    assert R.adjust_csi_settings((1 << 14) - 256, 14, 0) == (14, 0)
    assert R.adjust_csi_settings((1 << 14) - 255, 14, 0) == (14, 1)
    assert R.adjust_csi_settings((1 << 29) - 256, 14, 0) == (14, 5)
    assert R.adjust_csi_settings(1 << 29, 14, 0) == (14, 6)
    assert R.adjust_csi_settings((1 << 31) - 1, 14, 0) == (14, 6)
    assert R.adjust_csi_settings(1 << 40, 12, 0) == (14, 9)


def test_final_offset_without_eof_block_and_with_several():
    """Where the reader stands after the read that finds the end of the file.  No golden index confirms these two: the expectation rests on
    reading bgzf.c only.  bgzf_read leaves block_address at the address behind the block a read ended in (bgzf.c:1282-1285);
    bgzf_read_block then skips empty blocks with a local address and returns at the end of the file without storing it (1145-1155).  So
    the final offset is the address behind the last block that holds data: the file's size without an EOF block, and the FIRST of several
    trailing empty blocks."""
    recs = [bw.record(qname="q%d" % i, tid=0, pos=10 * i, cigar="4M", seq="ACGT") for i in range(5)]
    base = bw.bam_bytes([("a", 1000)], recs, level=0, eof=False)
    for tail, want in ((b"", len(base)), (bw.EOF_BLOCK, len(base)), (bw.EOF_BLOCK * 3, len(base))):
        refs, nnc = R.bam_index(base + tail).parsed()
        bins = refs[0][0]
        assert bins[4681][-1][1] == want << 16 and bins[37450][0][1] == want << 16 and nnc == 0


def test_tell_rule():
    """a record that ends exactly at a block end is followed by the NEXT block's address, an empty block's included"""
    recs = [bw.record(qname="q", tid=0, pos=i, cigar="4M", seq="ACGT") for i in range(4)]
    n = len(recs[0])
    hdr = bw.bgzf_file(bw.bam_header([("a", 100)]), eof=False, level=0)
    body = bw.bgzf_block(recs[0] + recs[1][:10], 0) + bw.bgzf_block(recs[1][10:], 0) + bw.bgzf_block(b"", 0) + bw.bgzf_block(recs[2] + recs[3], 0)
    src = R.bam_rows(hdr + body + bw.EOF_BLOCK)
    b1 = len(hdr)
    b2 = b1 + len(bw.bgzf_block(recs[0] + recs[1][:10], 0))
    b3 = b2 + len(bw.bgzf_block(recs[1][10:], 0))
    b4 = b3 + len(bw.bgzf_block(b"", 0))
    assert src["offset0"] == b1 << 16
    assert [r[3] for r in src["rows"]] == [(b1 << 16) | n, b3 << 16, (b4 << 16) | n, (b4 + len(bw.bgzf_block(recs[2] + recs[3], 0))) << 16]
    assert src["final"] == src["rows"][-1][3]


def test_model_errors_are_distinct():
    def build(rows, fmt="bai", n=2):
        idx = R.HtsIdx(n, fmt, 0, 14, 5)
        for k, r in enumerate(rows):
            idx.push(r[0], r[1], r[2], (k + 1) << 16, True)
        idx.finish((len(rows) + 1) << 16)
    with pytest.raises(R.UnsortedPositions):
        build([(0, 100, 110), (0, 50, 60)])
    with pytest.raises(R.BlocksNotContinuous):
        build([(0, 100, 110), (1, 50, 60), (0, 200, 210)])
    with pytest.raises(R.NoCoorNotLast):
        build([(0, 100, 110), (-1, 0, 0), (1, 5, 6)])
    with pytest.raises(R.EndBeforeBegin):
        build([(0, 100, 90)])
    with pytest.raises(R.BeyondMaxPos):
        build([(0, (1 << 29) + 1, (1 << 29) + 2)])
    build([(0, -1, 3), (0, 0, 4)])
    with pytest.raises(R.UnsortedPositions):          # last_coor is the clamped begin: POS 0 twice is "unsorted" to htslib
        build([(0, -1, 3), (0, -1, 3)])
