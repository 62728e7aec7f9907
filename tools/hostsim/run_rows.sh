#!/bin/bash
# Host build of the record helpers of the row passes (aux_size .. rec_check_t with the 64-bit HBM accessor and the 32-bit window accessor)
# under ASAN/UBSAN: the helper text is cut out of bam_records.hip and bam_tiles_lds.hip at build time (nothing is duplicated in the
# tree) and compared record by record with a plain serial model on exact-size images of the stream and of each tile's staged window.
#   tools/hostsim/run_rows.sh stream.bin [more.bin ...]      (a stream: BAM records one behind the other)
set -euo pipefail
here="$(cd "$(dirname "$0")" && pwd)"; root="$(cd "$here/../.." && pwd)"
gen="$here/_gen"; mkdir -p "$gen"
rec="$root/duckhts_amd/csrc/bam_records.hip"; til="$root/duckhts_amd/csrc/bam_tiles_lds.hip"
cut_out() {   # file, first line (regular expression), line behind the last one (regular expression)
  local a b
  a=$(grep -n "$2" "$1" | head -1 | cut -d: -f1); b=$(grep -n "$3" "$1" | head -1 | cut -d: -f1)
  [ -n "$a" ] && [ -n "$b" ] && [ "$a" -lt "$b" ] || { echo "run_rows.sh: markers not found in $1" >&2; exit 2; }
  sed -n "${a},$((b - 1))p" "$1"
}
{
  cut_out "$rec" '^#define REC_OK 0$' '^// (the bam_read1 checks themselves live in bam_tiles_lds.hip'
  cut_out "$til" '^#ifndef TL_TILE$' '^// flags in res\[14\]'
  cut_out "$til" '^struct GSrc {$' '^// One hop of the record chain:'
} > "$gen/rows_extract.inc"
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I"$gen" -o "$gen/sim_rows" "$here/sim_rows.cpp"
"$gen/sim_rows" "$@"
