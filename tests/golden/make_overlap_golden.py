"""Golden vectors for the interval overlap join: seeded intervals against the reads of range.bam, expected pairs produced by the
REFERENCE's own cgranges (oracle/_ref/libcgranges.so, compiled from the reference tree's third_party/cgranges by oracle/Makefile).
  overlap_range_bam.json        400 intervals (tests/test_oracle.py, tests/test_gpu_bam.py)
  overlap_cgranges_cases.json   1, 7 and 2000 random intervals; targets.bed moved onto the reads (the same two tests)
Run from the repo root where the reference tree is readable (make -C oracle REF=<reference tree>): python tests/golden/make_overlap_golden.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import orc  # noqa: E402
import region_oracle as ro  # noqa: E402

LIB = os.path.join(ROOT, "oracle", "_ref", "libcgranges.so")
t = orc.bam_read(open(os.path.join(GOLDEN, "range.bam"), "rb").read())
names = [bytes(x).decode() for x in t["ref_names"]]
q = []
for i in range(t["n_rows"]):
    ti, st = int(t["tid"][i]), int(t["POS"][i]) - 1
    q.append((names[ti] if ti >= 0 else "*", st, ro.endpos(st, int(t["FLAG"][i]), t["CIGAR"][i])))

rng = np.random.default_rng(3)
n = 400
tid = rng.integers(0, len(names), n).astype(np.int32)
beg = rng.integers(0, int(max(t["POS"])) + 200, n).astype(np.int64)
end = beg + rng.choice([0, 1, 5, 50, 500, 5000], n)
ref = ro.cgranges_overlap(LIB, names, tid, beg, end, q)
json.dump({"tid": tid.tolist(), "beg": beg.tolist(), "end": end.tolist(), "queries": q, "overlaps": [x.tolist() for x in ref]},
          open(os.path.join(GOLDEN, "overlap_range_bam.json"), "w"))
print("rows", len(ref), "pairs", sum(len(x) for x in ref))

# random intervals: 1, 7 and 2000 of them, lengths from empty to longer than the reads' span
rng = np.random.default_rng(11)
cases = []
for n in (1, 7, 2000):
    tid = rng.integers(0, len(names), n).astype(np.int32)
    beg = rng.integers(0, 30000, n).astype(np.int64)
    end = beg + rng.choice([0, 1, 2, 30, 700, 20000], n)
    ref = ro.cgranges_overlap(LIB, names, tid, beg, end, q)
    cases.append({"tid": tid.tolist(), "beg": beg.tolist(), "end": end.tolist(), "overlaps": [x.tolist() for x in ref]})
    print("random", n, "pairs", sum(len(x) for x in ref))
# targets.bed moved onto the reads: 1 kb further along, each 100 times as long (read_bed's rows as the join's intervals)
bed = open(os.path.join(GOLDEN, "targets.bed"), "rb").read()
moved = b"".join(b"\t".join([f[0], b"%d" % (int(f[1]) * 100 + 1000), b"%d" % (int(f[2]) * 100 + 1000)] + f[3:]) + b"\n"
                 for f in (ln.split(b"\t") for ln in bed.splitlines() if ln))
tid, beg, end = ro.bed_join_intervals(ro.bed_rows(moved), t["ref_names"])
ref = ro.cgranges_overlap(LIB, names, tid, beg, end, q)
print("moved targets.bed pairs", sum(len(x) for x in ref))
json.dump({"random_intervals": cases, "moved_targets_bed": [x.tolist() for x in ref]},
          open(os.path.join(GOLDEN, "overlap_cgranges_cases.json"), "w"))
