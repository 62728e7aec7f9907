"""The batch pipeline of read_bam and read_bcf (duckhts_amd/csrc/duckdb_pipeline.h) raced on the CPU: tools/hostsim/sim_pipeline.cpp includes
nothing but that header, runs fake producer threads that publish batches of numbered rows (1, 2047, 2048, 2049 and 5000 rows, three slots per
source, ten batches per source so that slots recycle) and worker threads that consume them through next_rows and the chunk loop.  Built once
with ThreadSanitizer and once with AddressSanitizer + UBSan, each run as a process of its own.  The cases, each in the overlapped and in the
serial form of the read-back:
  complete_ordered        1 and 3 sources, 1 worker: every row once, source after source, every chunk full except the last
  parallel                1 and 3 sources, 3 and 4 workers: every row once, no chunk above 2048 rows
  unclean_end_first_source  the rows before the unclean end, nothing of the later sources, no error
  producer_error / two_errors_first_wins  the consumer returns the error; of two failing sources the first message stays
  cancel_in_take_slot     the consumer takes one chunk and tears down while the producer waits for a free slot; teardown returns, every
                          producer is joined and every context destroyed before an arena is freed (ASan would see a late write)
  every case              a batch is seen by a consumer only after the fetch_wait of its copy slot and the landed step; the last pending batch
                          is delivered
A check of the host threading code, not a product path."""
import os
import platform
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "hostsim", "sim_pipeline.cpp")
CASES = {"complete_ordered": 4, "parallel": 8, "unclean_end_first_source": 2, "producer_error": 2, "two_errors_first_wins": 2, "cancel_in_take_slot": 2,
         "eight_batches_three_sources": 2}


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_pipeline_raced_under_sanitizers(tmp_path, sanitizer):
    exe = str(tmp_path / "sim_pipeline")
    b = subprocess.run(["g++", "-std=c++17", "-pthread", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=" + sanitizer, SRC, "-o", exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    cmd = [exe]
    for _ in range(3):                                             # the interleavings differ from run to run
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)
        if r.returncode != 0 and "ThreadSanitizer: unexpected memory mapping" in r.stderr and cmd == [exe]:
            # the runtime of this g++ cannot place its shadow under the kernel's address randomisation and stops before main: run this one
            # process without randomisation; where that is not possible either, ThreadSanitizer cannot run on this machine at all
            if shutil.which("setarch"):
                cmd = ["setarch", platform.machine(), "-R", exe]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)
            if r.returncode != 0 and ("unexpected memory mapping" in r.stderr or "setarch" in r.stderr):
                pytest.skip("ThreadSanitizer's runtime cannot start on this machine: " + r.stderr.strip()[-200:])
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        assert r.stderr.strip() == "", r.stderr[-3000:]                # both sanitizers report nothing
        lines = [l for l in r.stdout.splitlines() if l.startswith("case ")]
        assert "FAIL" not in r.stdout and r.stdout.splitlines()[-1] == "ALL OK: %d cases, 0 failed" % sum(CASES.values()), r.stdout[-3000:]
        assert {n: sum(1 for l in lines if l.split()[1] == n) for n in CASES} == CASES
        assert all(l.endswith(": ok") and " early 0/0 arenas 0 contexts 0" in l for l in lines)
        ordered = [l for l in lines if l.split()[1] == "complete_ordered" and " sources 3 " in l]
        assert len(ordered) == 2 and all(" rows 66870 of 66870 chunks 33 " in l for l in ordered)      # 3 x 22290 rows = 32 full chunks and one of 1334
        assert all(" rows 2048 of " in l and "cancelled-in-take 1 " in l for l in lines if l.split()[1] == "cancel_in_take_slot")
