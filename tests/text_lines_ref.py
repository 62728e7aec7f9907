"""A model in plain Python / numpy of the line table the text readers share (csrc/dhts_text_lines.inc: line_table): bytes in, the result's
fields and the arrays out.  It restates the contract, not the kernels: one pass over the newline positions, no chunks and no ranks.

  line_table(text, t0, open_last_ok, lim, tabs) -> dict
    nl           newlines at or behind t0
    last_start   where the text behind the last of them starts (t0 when there is none)
    nlines       nl, plus one for an unterminated last line when open_last_ok, less the lines that start at or behind lim
    last_open    1 when the last of the nlines is that unterminated line
    carry_start  the text offset behind the table's lines
    finished     a line starts at or behind lim, or the carry does
    line_off     nlines + 1 starts: line i is text[line_off[i] : line_off[i + 1] - 1]; behind an open last line stands len(text) + 1
    ntabs, tab_off, tab0, has_nul (tabs=True): the tabs at or behind t0, their positions, the tabs in front of line_off[0 .. nlines], and per
                 line whether it holds a NUL
  A t0 at or behind the end of the text gives no table: every count is 0, carry_start and last_start are len(text), the arrays are empty.
"""
import numpy as np

NO_LIM = 0xffffffffffffffff
FIELDS = ("nl", "ntabs", "nlines", "last_start", "carry_start", "last_open", "finished")


def line_table(text, t0=0, open_last_ok=True, lim=None, tabs=False):
    ulen = len(text)
    lim = NO_LIM if lim is None else lim
    e32 = np.zeros(0, np.uint32)
    if t0 >= ulen:
        out = dict(nl=0, ntabs=0, nlines=0, last_start=ulen, carry_start=ulen, last_open=0, finished=0, line_off=e32)
        if tabs:
            out.update(tab_off=e32, tab0=e32, has_nul=e32)
        return out
    b = np.frombuffer(bytes(text), np.uint8)
    nlpos = t0 + np.flatnonzero(b[t0:] == 10)
    nl = int(nlpos.size)
    starts = np.concatenate(([t0], nlpos + 1)).astype(np.int64)             # starts[nl] = last_start
    last_start = int(starts[nl])
    nlines, last_open, carry_start, finished = nl, 0, last_start, 0
    if open_last_ok and last_start < ulen:
        starts = np.append(starts, ulen + 1)
        nlines, last_open, carry_start = nl + 1, 1, ulen
    if lim < ulen:
        first = int(np.searchsorted(starts[:nlines], lim, side="left"))     # first line that starts at or behind lim
        if first < nlines:
            nlines, last_open, carry_start, finished = first, 0, int(starts[first]), 1
        elif carry_start >= lim:
            finished = 1
    out = dict(nl=nl, ntabs=0, nlines=nlines, last_start=last_start, carry_start=carry_start, last_open=last_open, finished=finished,
               line_off=starts[:nlines + 1].astype(np.uint32))
    if tabs:
        tabpos = t0 + np.flatnonzero(b[t0:] == 9)
        nulpos = t0 + np.flatnonzero(b[t0:] == 0)
        # tabs in front of a line's start; the sentinel behind an open last line has every tab in front of it
        tab0 = np.searchsorted(tabpos, starts[:nlines + 1], side="left").astype(np.uint32)
        line_of_nul = np.searchsorted(starts[:nl + 1], nulpos, side="right") - 1        # by the text's own newlines, whatever is taken
        has_nul = np.zeros(nl + 1, np.uint32)
        has_nul[line_of_nul] = 1
        out.update(ntabs=int(tabpos.size), tab_off=tabpos.astype(np.uint32), tab0=tab0, has_nul=has_nul[:nlines])
    return out


def lines_of(text, tab):
    """the byte strings of the table's lines"""
    lo = tab["line_off"].astype(np.int64)
    return [bytes(text[lo[i]:lo[i + 1] - 1]) for i in range(tab["nlines"])]


# ---- the cases the model's self-test and the device test share ----------------------------------------------------------------------
CHUNK = 4096                      # one workgroup's bytes: 256 lanes x 16
BIG = 3 << 20                     # random short lines over 768 chunks
HUGE = (16 << 20) + CHUNK + 1     # more than 4096 chunks: the scan of the chunk counts takes a second part


def _random_lines(n, seed, tabs=False):
    """n bytes of printable text in lines of 0 .. 60 bytes (a third of them with tabs when asked), the last one open"""
    rng = np.random.default_rng(seed)
    b = rng.integers(0x21, 0x7f, size=n, dtype=np.uint8)
    ends = np.cumsum(rng.integers(1, 62, size=n // 20 + 2))
    b[ends[ends < n]] = 10
    if tabs:
        t = rng.integers(0, n, size=n // 40 + 1)
        b[t[b[t] != 10]] = 9
    return b.tobytes()


def texts():
    """name -> bytes, made once"""
    T = {}
    for n in (0, 1, 15, 16, 17, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
        T["none_%d" % n] = b"x" * n
        if n:
            T["first_%d" % n] = b"\n" + b"x" * (n - 1)
            T["last_%d" % n] = b"x" * (n - 1) + b"\n"
            T["rand_%d" % n] = _random_lines(n, n, tabs=True)
    def at(n, *pos):
        b = bytearray(b"y" * n)
        for p in pos:
            b[p] = 10
        return bytes(b)
    T["at_4095"] = at(2 * CHUNK + 1, CHUNK - 1)
    T["at_4096"] = at(2 * CHUNK + 1, CHUNK)
    T["at_4095_4096"] = at(2 * CHUNK + 1, CHUNK - 1, CHUNK)
    T["at_15"], T["at_16"], T["at_15_16"] = at(33, 15), at(33, 16), at(33, 15, 16)
    T["at_4111_4112"] = at(2 * CHUNK + 1, CHUNK + 15, CHUNK + 16)
    T["runs"] = b"ab\n\n\n\ncd\n\n" + b"\n" * 40 + b"e" * 30 + b"\n\n\nf"
    T["all_newlines"] = b"\n" * (3 * CHUNK)
    # the tab part: lines with 0, 1 and 13 tabs, a tab in front of a newline, a NUL in the first, the last and an open last line
    T["tabs"] = b"notab\n" + b"a\tb\n" + b"\t".join(b"f%d" % i for i in range(14)) + b"\n" + b"end\t\n" + b"\t\n" + b"\t\t\tq"
    T["nul_first"] = b"a\0b\tc\n" + b"d\te\n" * 5
    T["nul_last"] = b"d\te\n" * 5 + b"a\tb\0c\n"
    T["nul_open"] = b"d\te\n" * 5 + b"a\tb\0\tc"
    T["tabs_in_front"] = b"\t\t\0\t\tskipped\t\n" + b"x\ty\n" * 3 + b"z\t"
    T["big"] = _random_lines(BIG, 7, tabs=True)
    T["huge"] = _random_lines(HUGE, 8, tabs=True)
    return T


def combos(name, text):
    """(t0, open_last_ok, lim) for a text: every t0 the issue names that the text admits, a newline at t0 - 1 and at t0, both rules for the
    last line, and the cuts -- none, at a line start, one byte into a line, at last_start, behind the text, 0"""
    n = len(text)
    if name == "huge":
        mid = line_table(text)["line_off"]
        return [(0, True, None), (CHUNK + 1, False, int(mid[len(mid) // 2]))]
    t0s = {t for t in (0, 1, 15, 16, 17, CHUNK, CHUNK + 1, n, n + 1) if t <= n + 1}
    if name == "big":
        mid = line_table(text)["line_off"]
        return [(0, True, None), (0, False, None), (CHUNK + 1, True, int(mid[len(mid) // 3])), (17, False, int(mid[len(mid) // 2]) + 1)]
    p = text.find(b"\n")
    if p >= 0:
        t0s |= {p, p + 1}                                     # a newline at t0: an empty first line; at t0 - 1: it does not count
    q = text.rfind(b"\n")
    if q >= 0:
        t0s |= {q, q + 1}
    out = []
    for t0 in sorted(t0s):
        base = line_table(text, t0, True)
        lo = base["line_off"]
        lims = {None, 0, n + 5, base["last_start"]}
        if len(lo) > 1:
            k = len(lo) // 2
            lims |= {int(lo[k]), int(lo[k]) + 1, int(lo[1])}
        lims.discard(NO_LIM)
        for ok in (True, False):
            for lim in sorted(lims, key=lambda x: -1 if x is None else x):
                out.append((t0, ok, lim))
    return out
