"""bam_tag_dir / bam_tag_cells / bam_aux_list on the hostile corpus (tag_corpus.py): the 56 tag columns and AUXILIARY_TAGS against the
plain model (bam_tags_ref.py) cell for cell, and against the oracle's table so that a failure names its column and row."""
import functools

import pytest

import bam_tags_ref as R
import duckhts_amd
import orc
import tag_corpus as TC
from test_bam_tags_ref import map_cells, model, table_cells
from test_gpu_aux_walk import _same

pytestmark = pytest.mark.gpu

FILES = ["default_payload", "payload_700"]
COL = {t: i for i, (t, _) in enumerate(R.STD_TAGS)}


@functools.lru_cache(maxsize=None)
def _oracle(which):
    data = TC.files()[which]
    return orc.bam_read(data), orc.bam_read_std_tags(data), {e: orc.bam_read_aux_map(data, e) for e in (True, False)}


@functools.lru_cache(maxsize=None)
def _full(which):
    """all 56 columns of one file, read once"""
    return duckhts_amd.read_bam(TC.files()[which], std_tags_cols=list(range(56)))


def _tags_equal_model(got, n, ctx, cols=range(56)):
    rows = table_cells(got["tags"])
    assert got["n_rows"] == n == len(rows), (ctx, got["n_rows"], n)
    for (name, _, _), cells, (want, _, _) in zip(TC.corpus(), rows, model()):
        for g, j in zip(cells, cols):
            assert g == want[j], f"{ctx}: {name}: column {R.STD_TAGS[j][0]}: device {g!r:.120} model {want[j]!r:.120}"


def _map_equal_model(got, excl, n, ctx):
    rows = map_cells(got["aux"])
    assert got["n_rows"] == n == len(rows), (ctx, got["n_rows"], n)
    for (name, _, _), g, m in zip(TC.corpus(), rows, model()):
        want = m[1] if excl else m[2]
        assert g == want, f"{ctx}: {name}: device {g!r:.200} model {want!r:.200}"


@pytest.mark.parametrize("max_blocks", [0, 1])
@pytest.mark.parametrize("which", [0, 1], ids=FILES)
def test_all_tag_columns(which, max_blocks):
    n = len(TC.corpus())
    got = _full(which) if max_blocks == 0 else duckhts_amd.read_bam(TC.files()[which], std_tags_cols=list(range(56)), max_blocks=max_blocks)
    assert got["status"] >= 0
    _tags_equal_model(got, n, FILES[which])
    d = orc.bcf_cols_diff(_oracle(which)[1], got["tags"])
    assert d is None, d
    _same(got, _oracle(which)[0], "core columns beside the tag columns")           # the tag passes read rec_off after compaction


@pytest.mark.parametrize("excl", [True, False], ids=["exclude_standard", "all"])
@pytest.mark.parametrize("max_blocks", [0, 1])
@pytest.mark.parametrize("which", [0, 1], ids=FILES)
def test_the_map(which, max_blocks, excl):
    got = duckhts_amd.read_bam(TC.files()[which], aux_map="exclude_standard" if excl else "all", max_blocks=max_blocks)
    exp = _oracle(which)[2][excl]
    d = orc.bcf_cols_diff({"n_rows": exp["n_rows"], "cols": exp["cols"]}, got["aux"])
    assert d is None, d
    _map_equal_model(got, excl, len(TC.corpus()), FILES[which])
    _same(got, _oracle(which)[0], "core columns beside the map")


def test_tag_columns_and_map_together():
    got = duckhts_amd.read_bam(TC.files()[1], std_tags_cols=list(range(56)), aux_map="exclude_standard")
    _tags_equal_model(got, len(TC.corpus()), "together")
    _map_equal_model(got, True, len(TC.corpus()), "together")
    _same(got, _oracle(1)[0], "core columns beside both")


@pytest.mark.parametrize("sel", [["NM"], ["MD"], ["TS"], ["ML"], ["CG"], "reversed"], ids=lambda s: s if isinstance(s, str) else s[0])
def test_projections(sel):
    """a column read alone, and all of them in reverse, equal the same columns of the full read"""
    idx = list(range(55, -1, -1)) if sel == "reversed" else [COL[t] for t in sel]
    got = duckhts_amd.read_bam(TC.files()[0], std_tags_cols=idx)
    full = _full(0)["tags"]
    d = orc.bcf_cols_diff({"n_rows": full["n_rows"], "cols": [full["cols"][i] for i in idx]}, got["tags"])
    assert d is None, d
    _tags_equal_model(got, len(TC.corpus()), "projection", idx)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_row_counts_at_the_edge_of_a_256_thread_block(n):
    data = TC.file_of(n)
    got = duckhts_amd.read_bam(data, std_tags_cols=list(range(56)), aux_map="all")
    _tags_equal_model(got, n, "first %d" % n)
    _map_equal_model(got, False, n, "first %d" % n)
    _same(got, orc.bam_read(data), "first %d" % n)
