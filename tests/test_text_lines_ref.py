"""The line-table model (text_lines_ref.py) against bytes.split(b"\\n") and plain loops, on the cases the device test runs (no GPU)."""
import bisect
import re

import pytest

import text_lines_ref as ref

TEXTS = ref.texts()


def by_split(text, t0, open_last_ok, lim, tabs):
    """the contract restated with bytes.split and loops"""
    n = len(text)
    if t0 >= n:
        return dict(nl=0, nlines=0, last_start=n, carry_start=n, last_open=0, finished=0, lines=[], starts=[])
    parts = bytes(text[t0:]).split(b"\n")
    lines, tail = parts[:-1], parts[-1]
    starts, at = [], t0
    for ln in lines:
        starts.append(at)
        at += len(ln) + 1
    last_start = at
    assert last_start + len(tail) == n
    nl, last_open, carry = len(lines), 0, last_start
    if open_last_ok and tail:
        lines, starts, last_open, carry = lines + [tail], starts + [last_start], 1, n
    finished = 0
    if lim is not None and lim < n:
        keep = [i for i, s in enumerate(starts) if s < lim]
        assert keep == list(range(len(keep)))
        if len(keep) < len(starts):
            carry, finished, last_open = starts[len(keep)], 1, 0
            lines, starts = lines[:len(keep)], starts[:len(keep)]
        elif carry >= lim:
            finished = 1
    out = dict(nl=nl, nlines=len(lines), last_start=last_start, carry_start=carry, last_open=last_open, finished=finished, lines=lines, starts=starts)
    if tabs:
        out["ntabs"] = bytes(text[t0:]).count(b"\t")
        out["tab_off"] = [m.start() for m in re.finditer(rb"\t", bytes(text)) if m.start() >= t0]
        out["tab0"] = [bisect.bisect_left(out["tab_off"], s) for s in starts + [carry]]      # tabs in front of every start, and of what follows the lines
        out["has_nul"] = [int(b"\0" in ln) for ln in lines]
    return out


@pytest.mark.parametrize("name", [k for k in TEXTS if k != "huge"])
def test_model_against_split(name):
    text = TEXTS[name]
    for t0, ok, lim in ref.combos(name, text):
        for tabs in (False, True):
            got, exp = ref.line_table(text, t0, ok, lim, tabs), by_split(text, t0, ok, lim, tabs)
            key = (name, t0, ok, lim, tabs)
            for f in ("nl", "nlines", "last_start", "carry_start", "last_open", "finished"):
                assert got[f] == exp[f], (key, f, got[f], exp[f])
            assert ref.lines_of(text, got) == exp["lines"], key
            assert list(got["line_off"][:got["nlines"]]) == exp["starts"], key
            if got["last_open"]:
                assert got["line_off"][-1] == len(text) + 1, key                  # the sentinel
            if tabs and t0 < len(text):
                assert got["ntabs"] == exp["ntabs"] and list(got["tab_off"]) == exp["tab_off"], key
                assert list(got["tab0"]) == exp["tab0"] and list(got["has_nul"]) == exp["has_nul"], key


def test_model_on_the_largest_text():
    """too long for the loops above: the counts, and every line start behind a newline"""
    text = TEXTS["huge"]
    for t0, ok, lim in ref.combos("huge", text):
        got = ref.line_table(text, t0, ok, lim, True)
        assert got["nl"] == text.count(b"\n", t0) and got["ntabs"] == text.count(b"\t", t0)
        lo = got["line_off"][1:got["nlines"] + 1 - got["last_open"]].astype("int64")
        assert all(text[p - 1] == 10 for p in lo[:: max(1, len(lo) // 5000)])
        if lim is not None:
            assert got["finished"] == 1 and got["carry_start"] == lim and got["last_open"] == 0 and (got["line_off"][:got["nlines"]] < lim).all()


def test_cases_cover_what_they_claim():
    assert len(TEXTS["big"]) == ref.BIG and (len(TEXTS["huge"]) + ref.CHUNK - 1) // ref.CHUNK + 1 > 4096
    assert TEXTS["all_newlines"].count(b"\n") == 3 * ref.CHUNK
    assert max(ln.count(b"\t") for ln in TEXTS["tabs"].split(b"\n")) == 13
    c = ref.combos("at_4095_4096", TEXTS["at_4095_4096"])
    assert {t0 for t0, _, _ in c} >= {0, 1, 15, 16, 17, 4095, 4096, 4097, 8193, 8194}
