"""time_tile_scan.py -- device time of the tile pass (scan kernel + two repair rounds + finalize, the library's "tiles" timer) per batch, for
DHTS_TILE_SCAN=wave and =lanes at 256, 1,024, 4,096 and 24,576 BGZF blocks per batch, on 4 M records of the bench data (19,813 blocks).
The repair rounds and the finalize pass are the same in both, so the difference is the scan kernel's.  The two kernels alternate, five
scans each per size (the library reads the variable per batch); the spread is the range of the five.  This is where TILE_SCAN_LANES_MIN
(dhts_bam_scan.inc) comes from: the smallest size from which the lane kernel wins by more than the wave kernel's own spread."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import duckhts_amd  # noqa: E402
from duckhts_amd import synth  # noqa: E402

head, _ = synth.bam_segment(0, seed=42, total_n=4_000_000, with_header=True, with_eof=False)
body, st = synth.bam_segment(4_000_000, seed=42, total_n=4_000_000, with_header=False, with_eof=False)
tail = np.frombuffer(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"), dtype=np.uint8)
ctx = duckhts_amd.Context(0)
ctx.open_tiled(head, body, 1, tail)
nb = ctx.bgzf_index(); ctx.bam_open()


def scan(mb):
    ctx.rewind(); rows = 0
    while True:
        b = ctx.next_batch(mb)
        rows += b.n_rows
        if b.status != 0:
            return rows


ctx.set_timing(True)
for mb in (256, 1024, 4096, 24576):
    t = {"wave": [], "lanes": []}
    for rep in range(6):
        for mode in ("wave", "lanes"):
            os.environ["DHTS_TILE_SCAN"] = mode
            ctx.reset_times()
            rows = scan(mb)
            v = ctx.kernel_times()["tiles"]
            if rep:                                              # the first scan of each kind warms up
                t[mode].append(v[0] / max(v[1], 1))
    w, l = t["wave"], t["lanes"]
    print(f"{mb:6d} blocks per batch ({nb} blocks, {rows} rows, about {mb * 65280 // 8192} tiles per batch): tile pass ms per batch  "
          f"wave avg {sum(w) / 5:.4f} min {min(w):.4f} max {max(w):.4f} (spread {max(w) - min(w):.4f})   "
          f"lanes avg {sum(l) / 5:.4f} min {min(l):.4f} max {max(l):.4f}   wave - lanes {sum(w) / 5 - sum(l) / 5:+.4f}", flush=True)
ctx.close()
