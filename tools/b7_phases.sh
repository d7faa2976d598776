#!/bin/bash
# Pipeline-7 K4 phase timing: one tuning build per phase with bin_sort_v7 compiled to return
# after it (-DSHD_B7_STOP = 1 load, 2 look-back, 3 grouping, 4 sorts; 0 = the whole kernel), and
# the kernel stats of 10 C5 rounds on each.  A stopped build's output is wrong by design; only its
# kernel times are read.  Build on the build machine, run on the GPU:
#   tools/b7_phases.sh build     libraries into ablibs/libshd_b7stop<k>.so
#   tools/b7_phases.sh           traces into bench_out/b7stop<k>, bin_sort_v7's line of each
set -e
cd "$(dirname "$0")/.."
stops=${B7_STOPS:-0 1 2 3 4}
if [ "$1" = build ]; then
  mkdir -p ablibs
  for k in $stops; do tools/build_variant.sh ablibs/libshd_b7stop$k.so -DSHD_B7_STOP=$k; done
  exit 0
fi
mkdir -p bench_out
for k in $stops; do
  SHD_ACCEL_LIB=$PWD/ablibs/libshd_b7stop$k.so timeout -k 10 120 rocprofv3 --kernel-trace --stats \
    --output-format csv -d bench_out/b7stop$k -o run -- python3 tools/relay_only.py 10 > bench_out/b7stop$k.log 2>&1 || exit 3
  grep -h "bin_sort" bench_out/b7stop$k/run_kernel_stats.csv | cut -d, -f1-4 | sed "s/^/stop=$k /"
done
