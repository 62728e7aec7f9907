"""The line table the text readers share, alone (dhts_debug_line_table: line_table of csrc/dhts_text_lines.inc with both kernel pairs),
against the model in text_lines_ref.py on the smallest texts at which the kernels and the host tail can go wrong: lengths around a lane's 16
bytes and a chunk's 4096, newlines on either side of those boundaries, a text of nothing but newlines, every t0 / open_last_ok / lim the
contract distinguishes, and the tab part's tabs and NULs.  Every comparison is exact."""
import numpy as np
import pytest

import duckhts_amd
import text_lines_ref as ref

pytestmark = pytest.mark.gpu

TEXTS = ref.texts()


@pytest.fixture(scope="module")
def ctx():
    c = duckhts_amd.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", list(TEXTS))
def test_line_table_against_the_model(ctx, name):
    text = TEXTS[name]
    n = len(text)
    for t0, ok, lim in ref.combos(name, text):
        exp = ref.line_table(text, t0, ok, lim, tabs=True)
        plain = ctx.debug_line_table(text, t0, ok, lim, tabs=False)
        tabbed = ctx.debug_line_table(text, t0, ok, lim, tabs=True)
        key = (name, t0, ok, lim)
        for f in ref.FIELDS:
            assert tabbed[f] == exp[f], (key, "tabs", f, tabbed[f], exp[f])
            if f != "ntabs":
                assert plain[f] == exp[f], (key, "plain", f, plain[f], exp[f])
        assert np.array_equal(plain["line_off"], exp["line_off"]), key
        assert np.array_equal(tabbed["line_off"], plain["line_off"]), key          # the two kernel pairs cut the same lines
        for f in ("tab_off", "tab0", "has_nul"):
            assert np.array_equal(tabbed[f], exp[f]), (key, f)
        # what the contract says in words, on the device's own numbers
        if plain["last_open"]:
            assert ok and plain["line_off"][-1] == n + 1 and plain["carry_start"] == n and plain["last_start"] < n
        if lim is not None and lim < n and t0 < n:
            assert (plain["line_off"][:plain["nlines"]] < lim).all()
            if plain["finished"] and plain["carry_start"] < n:
                assert plain["carry_start"] >= lim and plain["last_open"] == 0
        else:
            assert plain["finished"] == 0
