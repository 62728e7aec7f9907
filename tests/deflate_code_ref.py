"""CPU restatement of the device DEFLATE encoder's own rules (duckhts_amd/csrc/bgzf_deflate.hip), test tooling only.

build_lengths restates dfl_build_lengths line for line: Shannon lengths capped at maxbits, the rank order, the fewer-than-two-symbols
rule, the lengthening loop for a code the cap over-subscribes, the completing loop.  table_words restates dfl_assign_codes (canonical
codes, bit-reversed, | length << 16); cl_sequence the code-length section (zero runs as 17 / 18, no 16); block_choice the size rule:
dynamic iff dyn_bits < fix_bits, stored iff ceil(best / 8) >= n + 5.

The completing loop here carries a guard the kernel does not: a full pass that changes nothing raises instead of spinning.  No count
vector goes to the device before this file has carried it through.
"""
import deflate_writer as W


class NoProgress(RuntimeError):
    pass


def shannon_lengths(cnt, maxbits):
    total = sum(cnt)
    lens = []
    for f in cnt:
        L = 0
        if f:
            L = 1
            while L < maxbits and (f << L) < total:
                L += 1
        lens.append(L)
    return lens


def build_lengths(cnt, maxbits, info=None, lengthen=True):
    """dfl_build_lengths(cnt, n = len(cnt), maxbits).  info (a dict) receives 'oversubscribed': whether the cap pushed the Kraft sum of
    the Shannon lengths above 1.  lengthen=False leaves the lengthening loop out (what a broken kernel would do; for the tests' own tests)."""
    n = len(cnt)
    used = sum(1 for f in cnt if f)
    lens = shannon_lengths(cnt, maxbits)
    order = sorted(range(n), key=lambda s: (-cnt[s], s))                 # rank by descending count, ties: lower symbol first
    if info is not None:
        info["oversubscribed"] = False
    if used < 2:
        a = next((s for s in range(n) if cnt[s]), n)
        lens = [0] * n
        if a == n:
            lens[0] = lens[1] = 1
        else:
            lens[a] = 1
            lens[1 if a == 0 else 0] = 1
        return lens
    one = 1 << maxbits
    K = sum(one >> l for l in lens if l)
    if info is not None:
        info["oversubscribed"] = K > one
    r = used - 1
    while lengthen and K > one and r >= 0:                               # lengthen the rarest short codes
        s = order[r]
        while K > one and lens[s] < maxbits:
            K -= one >> (lens[s] + 1)
            lens[s] += 1
        r -= 1
    while K < one:                                                       # complete the code: shorten, most frequent first, while it fits
        moved = False
        for r in range(used):
            if K >= one:
                break
            s = order[r]
            while lens[s] > 1 and K + (one >> lens[s]) <= one:
                K += one >> lens[s]
                lens[s] -= 1
                moved = True
        if not moved:
            raise NoProgress("the completing loop made a full pass without a change: K = %d of %d" % (K, one))
    return lens


def table_words(lens):
    """dfl_assign_codes: tab[s] = bit-reversed canonical code | length << 16 (0 for an unused symbol)"""
    codes = W.canonical(list(lens))
    return [(int(format(c, "0%db" % l)[::-1], 2) | (l << 16)) if l else 0 for c, l in zip(codes, lens)]


def cost(cnt, lens):
    return sum(f * l for f, l in zip(cnt, lens))


def trim(ll_lens, d_lens):
    """(hlit, hdist): the lengths sent, trailing zeros dropped down to 257 / 1"""
    hlit, hdist = 286, 30
    while hlit > 257 and ll_lens[hlit - 1] == 0:
        hlit -= 1
    while hdist > 1 and d_lens[hdist - 1] == 0:
        hdist -= 1
    return hlit, hdist


def cl_sequence(ll_lens, d_lens):
    """the code-length section of the kernel as (symbol, extra value) items: a zero run (it may cross from the literal/length into the
    distance lengths) of 11..138 as one 18, of 3..10 as one 17, shorter as plain zeros; a longer run starts over after 138; no 16"""
    hlit, hdist = trim(ll_lens, d_lens)
    seq = list(ll_lens[:hlit]) + list(d_lens[:hdist])
    items, i, tot = [], 0, hlit + hdist
    while i < tot:
        L = seq[i]
        if L == 0:
            r = 1
            while i + r < tot and r < 138 and seq[i + r] == 0:
                r += 1
            if r >= 11:
                items.append((18, r - 11)); i += r; continue
            if r >= 3:
                items.append((17, r - 3)); i += r; continue
        items.append((L, 0))
        i += 1
    return items


def token_counts(syms):
    """(literal/length counts[286], distance counts[30], extra bits) of a symbol list (ints, (length, distance)), end of block counted"""
    fl, fd, extra = [0] * 286, [0] * 30, 0
    for s in syms:
        if isinstance(s, int):
            fl[s] += 1
        else:
            lc, dc = W.length_code(s[0])[0], W.dist_code(s[1])[0]
            fl[lc] += 1
            fd[dc] += 1
            extra += W.LEN_EXTRA[lc - 257] + W.DIST_EXTRA[dc]
    fl[256] += 1
    return fl, fd, extra


def block_choice(syms, n):
    """the kernel's size rule for a block of n input bytes parsed into `syms`: a dict with dyn_bits, fix_bits, btype (0 stored, 1 fixed,
    2 dynamic), nbytes (the payload's size), and the dynamic header the kernel would build (ll_lens, d_lens, cl_lens, cl_items, hlit,
    hdist, hclen)"""
    fl, fd, extra = token_counts(syms)
    ll, dl = build_lengths(fl, 15), build_lengths(fd, 15)
    items = cl_sequence(ll, dl)
    fc = [0] * 19
    for s, _ in items:
        fc[s] += 1
    cl = build_lengths(fc, 7)
    hclen = 19
    while hclen > 4 and cl[W.CL_ORDER[hclen - 1]] == 0:
        hclen -= 1
    dyn = cost(fl, ll) + cost(fd, dl) + sum(fc[s] * (cl[s] + (3 if s == 17 else 7 if s == 18 else 0)) for s in range(19))
    dyn += 3 + 5 + 5 + 4 + 3 * hclen + extra
    fix = cost(fl, W.FIXED_LL[:286]) + 5 * sum(fd) + 3 + extra
    dynamic = dyn < fix
    best = dyn if dynamic else fix
    stored = (best + 7) // 8 >= n + 5
    hlit, hdist = trim(ll, dl)
    return dict(dyn_bits=dyn, fix_bits=fix, btype=0 if stored else 2 if dynamic else 1, nbytes=n + 5 if stored else (best + 7) // 8,
                ll_lens=ll, d_lens=dl, cl_lens=cl, cl_items=items, hlit=hlit, hdist=hdist, hclen=hclen)


# ---- count vectors -----------------------------------------------------------------------------------------------------------------
ALPHABETS = ((286, 15), (30, 15), (19, 7))
# the two vectors known to over-subscribe (the cap pushes the Kraft sum of the Shannon lengths above 1)
OVERSUB_LL = [20000, 10000, 5000, 2500, 1250, 625, 313, 157, 79, 40] + [1] * 36
OVERSUB_CL = [158, 79, 40, 20, 10] + [1] * 9


def _spread(vals, nsym, rnd):
    """the values on rnd-chosen symbols of an nsym alphabet, zeros elsewhere"""
    out = [0] * nsym
    for s, v in zip(rnd.sample(range(nsym), len(vals)), vals):
        out[s] = v
    return out


def ladder(total, rungs, ones):
    """ceil(total / 2^k) for k = 1..rungs, then `ones` ones: the shape of the two known over-subscribing vectors"""
    return [-(-total // (1 << k)) for k in range(1, rungs + 1)] + [1] * ones


def families(nsym, maxbits, seed=1951):
    """[(family name, count vector)] for one alphabet, deterministic.  Totals stay within what a block can make: 65,281 literal/length
    or distance symbols (0xff00 tokens and the end of block), 316 code-length items."""
    import random
    rnd = random.Random(seed * 1000 + nsym)
    cap = 316 if nsym == 19 else 65281
    out, seen = [], set()

    def add(name, vals, place=True):
        vals = list(vals)[:nsym]
        v = _spread(vals, nsym, rnd) if place else vals + [0] * (nsym - len(vals))
        if sum(v) > cap or tuple(v) in seen:
            return
        seen.add(tuple(v))
        out.append((name, v))

    for k in range(700):                                               # uniform small counts over a random number of symbols
        m = rnd.randint(2, nsym)
        hi = max(1, min(rnd.choice([1, 2, 3, 8, 30, 200]), cap // m))
        add("uniform", [rnd.randint(1, hi) for _ in range(m)])
    for k in range(700):                                               # heavy tails: count ~ cap / rank^a, cut to the total
        m = rnd.randint(2, nsym)
        a = rnd.choice([0.8, 1.0, 1.5, 2.0, 3.0])
        t = rnd.randint(m, cap)
        w = [1.0 / (r + 1) ** a for r in range(m)]
        sw = sum(w)
        add("heavy_tail", [max(1, int((t - m) * x / sw)) for x in w])
    for k in range(300):                                               # one giant count, everything else once
        m = rnd.randint(2, nsym)
        add("giant_and_ones", [rnd.randint(1, cap - (m - 1))] + [1] * (m - 1))
    for k in range(400):                                               # ladders of near powers of two (each count 2^j, 2^j - 1 or 2^j + 1)
        m = rnd.randint(2, min(nsym, 16 if cap > 316 else 8))
        top = rnd.randint(m - 1, 15 if cap > 316 else 7)
        v = [max(1, (1 << max(0, top - j)) + rnd.choice([-1, 0, 0, 1])) for j in range(m)]
        add("pow2_ladder", v + [1] * rnd.randint(0, nsym - m))
    fib = [1, 1]
    while fib[-1] + fib[-2] < cap:
        fib.append(fib[-1] + fib[-2])
    for k in range(200):                                               # Fibonacci counts: the deepest Huffman trees
        m = rnd.randint(2, min(nsym, len(fib)))
        v = fib[:m]
        while sum(v) > cap:
            v = v[:-1]
        add("fibonacci", v + [1] * rnd.randint(0, min(nsym - len(v), cap - sum(v))))
    for k in range(60):                                                # 0, 1 or 2 used symbols
        add("few_symbols", [rnd.randint(1, cap // 2) for _ in range(k % 3)])
    for c in [1, 2, 3, 7, cap // nsym]:                                # every symbol used, equal counts
        add("all_equal", [c] * nsym, place=False)
    # the cap over-subscribes: ladders ceil(T / 2^k) that take up almost all of the code space, and a tail of ones rarer than 2^-maxbits
    if nsym == 286:
        add("oversubscribed_known", OVERSUB_LL, place=False)
    if nsym == 19:
        add("oversubscribed_known", OVERSUB_CL, place=False)
    # (with T = ones << rungs the rungs take lengths 1..rungs, Kraft sum 1 - 2^-rungs, and the ones, capped at maxbits, more than 2^-rungs)
    pairs = [(r, o) for r in range(2, maxbits) for o in range((1 << (maxbits - r)) + 1, min(nsym - r, cap >> r) + 1)]
    for k in range(400):
        rungs, ones = rnd.choice(pairs)
        t = (ones << rungs) - rnd.choice([0, 0, 0, 1, 2, rnd.randint(0, ones)])
        add("ladder_and_ones", ladder(t, rungs, ones - rnd.choice([0, 0, 1])))
    return out
