#!/bin/bash
# Host build of bam_tile_scan_lanes' per-lane function (tile_scan_lane: line loads, prefilter, rec_check_t<GSrc> three deep, light walk)
# under ASAN/UBSAN: its text and the record helpers it calls are cut out of bam_records.hip and bam_tiles_lds.hip at build time (nothing is
# duplicated in the tree) and compared tile by tile with a plain serial model on exact-size images of the stream.
#   tools/hostsim/run_scan.sh [-r N] [-t] stream.bin [[-t] more.bin ...]   (a stream: BAM records one behind the other; -t: a non-final batch;
#                                                                          -r N: N references for the files that follow, default 2)
set -euo pipefail
here="$(cd "$(dirname "$0")" && pwd)"; root="$(cd "$here/../.." && pwd)"
gen="$here/_gen"; mkdir -p "$gen"
rec="$root/duckhts_amd/csrc/bam_records.hip"; til="$root/duckhts_amd/csrc/bam_tiles_lds.hip"
cut_out() {   # file, first line (regular expression), line behind the last one (regular expression)
  local a b
  a=$(grep -n "$2" "$1" | head -1 | cut -d: -f1); b=$(grep -n "$3" "$1" | head -1 | cut -d: -f1)
  [ -n "$a" ] && [ -n "$b" ] && [ "$a" -lt "$b" ] || { echo "run_scan.sh: markers not found in $1" >&2; exit 2; }
  sed -n "${a},$((b - 1))p" "$1"
}
{
  cut_out "$rec" '^#define REC_OK 0$' '^// A shard that starts mid-stream:'
  cut_out "$til" '^#ifndef TL_TILE$' '^// flags in res\[14\]'
  cut_out "$til" '^struct GSrc {$' '^// One hop of the record chain:'
  cut_out "$til" '^#define LS_LINE 128u$' '^// the kernel: lane i of the grid takes tile 1 + i'
} > "$gen/scan_extract.inc"
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I"$gen" -o "$gen/sim_scan" "$here/sim_scan.cpp"
"$gen/sim_scan" "$@"
