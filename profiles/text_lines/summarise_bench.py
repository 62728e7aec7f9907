"""One line per measured leg: the parent's two runs, the change's two runs, and whether each run of the change lies inside the parent's two
(margin: the parent's own spread on that visit).  usage: summarise_bench.py <dir with <tool>_<tree>_<run>.log>"""
import json
import os
import sys

KEYS = ("warm_s", "ms_per_scan", "build_wall_s_run1", "warm_query_s", "ms_per_step", "line_table_ms")
d = sys.argv[1]
legs = {}
for f in sorted(os.listdir(d)):
    tool, tree, run = f[:-4].rsplit("_", 2)
    n = 0
    for ln in open(os.path.join(d, f)):
        if not ln.startswith("{"):
            continue
        j = json.loads(ln)
        for k in KEYS:
            if k in j:
                what = j.get("columns") or j.get("form") or (j.get("query", "")[:40] + " thr=%s res=%s" % (j.get("DHTS_THREADS"), j.get("file_resident")) if "query" in j else "")
                legs.setdefault((tool, n, k, what), {}).setdefault(tree, []).append(j[k])
                n += 1
for (tool, n, k, what), v in sorted(legs.items()):
    p, c = v.get("parent", []), v.get("change", [])
    lo, hi = min(p), max(p)
    out = [x for x in c if x < lo or x > hi]
    verdict = "inside" if not out else "; ".join("%g is %s the parent's runs by %.3g" % (x, "below" if x < lo else "above", lo - x if x < lo else x - hi) for x in out)
    print("%-8s %-18s %-52s parent %s  change %s  %s" % (tool, k, what[:52], p, c, verdict))
