"""lz_rounds_model.py file.bam [blocks] -- dependency rounds of bgzf_lz_resolve's 64-token batches on a real DEFLATE stream (CPU model):
rounds per batch under the kernel's cell policy, a cheaper 'first pending destination' policy and the exact byte-level bound.  The figures
behind DESIGN 5c (84 % of a batch's matches are ready in the first round)."""
import os, sys, struct, collections
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_stats as ds

def tokens_of(payload):
    """returns list of (lrun, mlen, dist) + trailing literals"""
    b = ds.Bits(payload); toks = []; run = 0
    while True:
        last = b.take(1); typ = b.take(2)
        if typ == 0:
            b.pos = (b.pos + 7) & ~7; ln = b.take(16); b.take(16); b.pos += 8 * ln; run += ln
        else:
            if typ == 1:
                ll = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8; dl = [5] * 32
            else:
                hl = b.take(5) + 257; hd = b.take(5) + 1; hc = b.take(4) + 4
                cl = [0] * 19
                for i in range(hc):
                    cl[[16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15][i]] = b.take(3)
                ct = ds.mkdec(cl); lens = []
                while len(lens) < hl + hd:
                    s, _ = ds.dec(b, ct)
                    if s < 16: lens.append(s)
                    elif s == 16: lens += [lens[-1]] * (3 + b.take(2))
                    elif s == 17: lens += [0] * (3 + b.take(3))
                    else: lens += [0] * (11 + b.take(7))
                ll, dl = lens[:hl], lens[hl:hl + hd]
            lt, dt = ds.mkdec(ll), ds.mkdec(dl)
            while True:
                s, L = ds.dec(b, lt)
                if s < 256: run += 1
                elif s == 256: break
                else:
                    j = s - 257; ln = ds.LBASE[j] + b.take(ds.LEXT[j])
                    d, L2 = ds.dec(b, dt); dist = ds.DBASE[d] + b.take(ds.DEXT[d])
                    while run >= 511: toks.append((511, 0, 0)); run -= 511
                    toks.append((run, ln, dist)); run = 0
        if last: break
    return toks, run

def load(path, maxb, skip):
    data = open(path, 'rb').read(); p = 0; n = 0; out = []
    while p + 18 <= len(data) and n < maxb + skip:
        bl = struct.unpack_from('<H', data, p + 16)[0] + 1
        if n >= skip and bl > 28: out.append(tokens_of(data[p + 18:p + bl - 8]))
        p += bl; n += 1
    return out

def simulate(toks, W, policy):
    """returns (steps, rounds, list of ready counts)"""
    outpos = 0; steps = 0; rounds = 0; nm = 0
    for t0 in range(0, len(toks), W):
        batch = toks[t0:t0 + W]; steps += 1
        # positions
        pos = outpos; items = []
        for (lr, ml, di) in batch:
            md = pos + lr; items.append((md, ml, di)); pos = md + ml
        tot = pos - outpos
        pend = [i for i, (md, ml, di) in enumerate(items) if ml > 0]
        nm += len(pend)
        sh = 4
        while (tot >> sh) > 63: sh += 1
        while pend:
            rounds += 1
            ready = []
            if policy == 'cell':
                owed = 0
                for i in pend:
                    md, ml, di = items[i]; ms = md - di; sp = min(ml, di)
                    lo = (md - outpos) >> sh; hi = (md - outpos + ml - 1) >> sh
                    dmask = ((1 << (hi + 1)) - 1) & ~((1 << lo) - 1)
                    smask = 0
                    if ms + sp > outpos:
                        slo = (max(ms, outpos) - outpos) >> sh; shi = (ms + sp - 1 - outpos) >> sh
                        smask = ((1 << (shi + 1)) - 1) & ~((1 << slo) - 1)
                    if smask & owed == 0: ready.append(i)
                    owed |= dmask
            elif policy == 'first':
                fmd = items[pend[0]][0]
                for k, i in enumerate(pend):
                    md, ml, di = items[i]; ms = md - di; sp = min(ml, di)
                    if k == 0 or ms + sp <= fmd: ready.append(i)
            elif policy == 'exact':
                owed = []
                for i in pend:
                    md, ml, di = items[i]; ms = md - di; sp = min(ml, di)
                    if not any(ms < e and ms + sp > s for (s, e) in owed): ready.append(i)
                    owed.append((md, md + ml))
            rs = set(ready); pend = [i for i in pend if i not in rs]
        outpos = pos
    return steps, rounds, nm

RING, SPAN, SEQ_T = 4096, 1536, 6          # B_RING_LOG2, BR_SPAN, B_SEQ_T of bgzf_inflate.hip

def kernel_model(toks, ncell, sh0, seq_t=SEQ_T):
    """lz_block's lane-parallel batches as the kernel runs them: far-big matches placed first, rounds of windowed copies behind the cell
    test (ncell cells of at least 2^sh0 bytes), the rest replayed as soon as seq_t or fewer are pending or a round copied nothing.
    Returns a Counter: batches, oversized, matches, rounds, ready[r] (copied by round r), replayed, replay_wait (replayed matches that a
    windowed copy could have taken: they only waited), and the literal pass's classes per batch."""
    c = collections.Counter(); outpos = 0
    for t0 in range(0, len(toks), 64):
        batch = toks[t0:t0 + 64]
        tot = sum(lr + ml for lr, ml, _ in batch); lit = sum(lr for lr, _, _ in batch)
        if tot > SPAN or lit > 1024:
            c['oversized'] += 1; outpos += tot; continue
        c['batches'] += 1
        bend = outpos + tot; rlo = max(bend - RING, 0); pos = outpos; lanes = []
        n8 = nwin = nexact = nexact4 = 0
        for lr, ml, di in batch:
            md = pos + lr
            # the literal pass: runs of 8..32 bytes (four windows), a short run in front of a match (one 8-byte window when run + match
            # reach 8 bytes, else one 4-byte window: both end inside the lane's own match), the exact 4 / 2 / 1 classes for the rest
            if 8 <= lr <= 32: n8 += 1
            elif 1 <= lr < 8 and ml > 0 and lr + ml >= 8: nwin += 1
            elif 1 <= lr < 8:
                nexact += 1; nexact4 += ml > 0
            if ml > 0:
                ms = md - di; far = ms < rlo; rs, rd = ms % RING, md % RING
                wcopy = ml <= 32 and rd + ml <= RING and (far or (rs + ml <= RING and (di >= ml or di == 1)))
                if not (far and not wcopy): lanes.append((md, ml, ms, min(ml, di), far, wcopy))
                c['matches'] += 1; c['farbig'] += far and not wcopy
            pos = md + ml
        c['lit_has_8plus'] += n8 > 0; c['lit_has_exact'] += nexact > 0; c['lit_has_exact_without_4window'] += nexact > nexact4
        c['runs_8plus'] += n8; c['runs_window8'] += nwin; c['runs_exact'] += nexact; c['runs_exact_match_behind'] += nexact4
        sh = sh0
        while (tot >> sh) > ncell - 1: sh += 1
        pend = lanes; r = 0
        while pend:
            if r and len(pend) <= seq_t: break
            r += 1; c['rounds'] += 1; owed = 0; keep = []; nready = 0
            for md, ml, ms, sp, far, wcopy in pend:
                lo, hi = (md - outpos) >> sh, (md - outpos + ml - 1) >> sh
                smask = 0
                if not far and ms + sp > outpos:
                    slo, shi = (max(ms, outpos) - outpos) >> sh, (ms + sp - 1 - outpos) >> sh
                    smask = ((1 << (shi + 1)) - 1) & ~((1 << slo) - 1)
                if wcopy and smask & owed == 0: nready += 1
                else: keep.append((md, ml, ms, sp, far, wcopy))
                owed |= ((1 << (hi + 1)) - 1) & ~((1 << lo) - 1)
            c['ready%d' % min(r, 4)] += nready; pend = keep
            if nready == 0: break
        c['replayed'] += len(pend); c['replay_wait'] += sum(1 for x in pend if x[5])
        outpos = bend
    return c

def load_synth(nrec):
    """bench-shaped blocks (duckhts_amd.synth.bam_segment from the middle of the bench's file, host code only)"""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from duckhts_amd import synth
    body, _ = synth.bam_segment(nrec, seed=42, total_n=4_000_000, rec0=2_000_000, with_header=False, with_eof=False)
    data = body.tobytes(); p = 0; out = []
    while p + 18 <= len(data):
        bl = struct.unpack_from('<H', data, p + 16)[0] + 1
        if bl > 28: out.append(tokens_of(data[p + 18:p + bl - 8]))
        p += bl
    return out

def report_kernel(blocks):
    for name, ncell, sh0 in (('64 cells of >= 16 bytes (the kernel)', 64, 4), ('128 cells of >= 8 bytes', 128, 3)):
        c = collections.Counter()
        for toks, tail in blocks: c += kernel_model(toks, ncell, sh0)
        B, M = c['batches'], c['matches'] - c['farbig']
        print(f"{name}: blocks {len(blocks)} batches {B} oversized {c['oversized']} pending matches/batch {M / B:.1f} far-big {c['farbig'] / B:.2f}")
        print(f"  rounds/batch {c['rounds'] / B:.3f}  ready in round 1 / 2 / 3 / 4+: " + ' / '.join(f"{100 * c['ready%d' % r] / M:.1f} %" for r in (1, 2, 3, 4))
              + f"  replayed {100 * c['replayed'] / M:.1f} % = {c['replayed'] / B:.2f} per batch ({c['replay_wait'] / B:.2f} of them only waited)")
    print(f"literal pass, per batch: runs of 8..32 bytes {c['runs_8plus'] / B:.2f} (in {100 * c['lit_has_8plus'] / B:.1f} % of the batches), "
          f"1..7 bytes with run + match >= 8 {c['runs_window8'] / B:.2f}, other runs of 1..7 bytes {c['runs_exact'] / B:.2f} "
          f"({c['runs_exact_match_behind'] / B:.2f} with a match behind); batches with such a run {100 * c['lit_has_exact'] / B:.1f} %, "
          f"with one that has no match behind {100 * c['lit_has_exact_without_4window'] / B:.1f} %")

if __name__ == '__main__':
    if sys.argv[1] == '--synth':             # lz_rounds_model.py --synth [records]: the kernel's policy on bench-shaped data
        report_kernel(load_synth(int(sys.argv[2]) if len(sys.argv) > 2 else 60_000))
        sys.exit(0)
    blocks = load(sys.argv[1], int(sys.argv[2]), 3)
    for W in (64, 128):
        for pol in ('cell', 'first', 'exact'):
            S = R = M = 0
            for toks, tail in blocks:
                s, r, m = simulate(toks, W, pol); S += s; R += r; M += m
            print(f"W={W} {pol:6s}: blocks {len(blocks)} steps/blk {S/len(blocks):.1f} rounds/blk {R/len(blocks):.1f} rounds/step {R/S:.2f} matches/blk {M/len(blocks):.0f}")
