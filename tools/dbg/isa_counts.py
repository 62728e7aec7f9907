"""isa_counts.py FILE.s KERNEL [--loop-with PATTERN] [--dump OUT.s] -- static instruction counts of one kernel in a gfx950 device assembly
listing (hipcc ... --cuda-device-only -S): instructions, SALU, saveexec groups, branches, flat_ / ds_ / global_ / scratch_ accesses and the
s_waitcnt forms in front of stores.  --loop-with PATTERN [--without PATTERN] [--pick N]: count also the loops (a backward branch to a
label) whose body matches the first regular expression and not the second, largest first, and one of them in full; --dump writes that
loop (or the kernel without --loop-with) to a file."""
import re
import sys


def kernel_text(path, name):
    lines = open(path).read().split("\n")
    beg = next(i for i, l in enumerate(lines) if l.split(";")[0].strip() == name + ":")
    end = next(i for i in range(beg, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[beg + 1:end]


def is_instr(l):
    s = l.split(";")[0].strip()
    return bool(s) and not s.startswith((".", "//")) and not s.endswith(":")


def counts(body):
    ins = [l.strip().split(";")[0].strip() for l in body if is_instr(l)]
    op = [i.split()[0] for i in ins]
    c = {"instructions": len(op),
         "SALU (s_*, without s_waitcnt / s_nop / branches)": sum(o.startswith("s_") and not o.startswith(("s_waitcnt", "s_nop", "s_cbranch", "s_branch", "s_barrier", "s_endpgm", "s_load", "s_buffer_load")) for o in op),
         "VALU (v_*)": sum(o.startswith("v_") for o in op),
         "saveexec groups": sum("saveexec" in o for o in op),
         "branches": sum(o.startswith(("s_cbranch", "s_branch")) for o in op),
         "flat_": sum(o.startswith("flat_") for o in op),
         "ds_": sum(o.startswith("ds_") for o in op),
         "global_load": sum(o.startswith("global_load") for o in op),
         "global_store / atomic": sum(o.startswith(("global_store", "global_atomic")) for o in op),
         "scratch_": sum(o.startswith("scratch_") for o in op),
         "s_waitcnt": sum(o == "s_waitcnt" for o in op)}
    # the wait that stands in front of each global store (the last s_waitcnt before it, within 12 instructions)
    waits = {}
    for i, o in enumerate(op):
        if o.startswith("global_store"):
            w = next((ins[j] for j in range(i - 1, max(i - 12, -1), -1) if op[j] == "s_waitcnt"), "(none near)")
            waits[w] = waits.get(w, 0) + 1
    return c, waits


def loops(body):
    """(start, end) line ranges of backward branches"""
    lab = {l.split(";")[0].strip()[:-1]: i for i, l in enumerate(body) if l.split(";")[0].strip().endswith(":")}
    out = []
    for i, l in enumerate(body):
        m = re.match(r"\s*s_cbranch_\w+\s+(\S+)|\s*s_branch\s+(\S+)", l)
        if m:
            t = m.group(1) or m.group(2)
            if t in lab and lab[t] < i:
                out.append((lab[t], i))
    return out


def main():
    path, name = sys.argv[1], sys.argv[2]
    pat = sys.argv[sys.argv.index("--loop-with") + 1] if "--loop-with" in sys.argv else None
    dump = sys.argv[sys.argv.index("--dump") + 1] if "--dump" in sys.argv else None
    body = kernel_text(path, name)
    sel = body
    print(f"== {name}: whole kernel")
    c, w = counts(body)
    for k, v in c.items():
        print(f"  {k:52s} {v}")
    print("  waits in front of global stores:", w)
    if pat:
        cand = [(a, b) for a, b in loops(body) if any(re.search(pat, l) for l in body[a:b + 1])]
        # of these, the loops without a match of --without (e.g. 'global_|s_barrier': a walk out of LDS, not the row loop around it), largest first;
        # --pick N chooses one (default: the largest)
        wo = sys.argv[sys.argv.index("--without") + 1] if "--without" in sys.argv else None
        cand = sorted(((a, b) for a, b in cand if not (wo and any(re.search(wo, l) for l in body[a:b + 1]))), key=lambda r: r[0] - r[1])
        if not cand:
            print(f"  no loop contains /{pat}/ without /{wo}/")
            return
        for i, (a, b) in enumerate(cand[:8]):
            print(f"  loop {i}: kernel lines {a}..{b}, {counts(body[a:b + 1])[0]['instructions']} instructions")
        pick = int(sys.argv[sys.argv.index("--pick") + 1]) if "--pick" in sys.argv else 0
        a, b = cand[pick]
        sel = body[a:b + 1]
        print(f"== {name}: loop {pick} of the loops containing /{pat}/ and not /{wo}/ (lines {a}..{b} of the kernel)")
        c, w = counts(sel)
        for k, v in c.items():
            print(f"  {k:52s} {v}")
        print("  waits in front of global stores:", w)
    if dump:
        open(dump, "w").write("\n".join(sel) + "\n")


if __name__ == "__main__":
    main()
