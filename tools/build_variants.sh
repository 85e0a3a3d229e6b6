#!/bin/bash
# Build libstl variants for same-box A/B runs: tools/build_variants.sh NAME "FLAGS" [NAME "FLAGS" ...]
# Output build/ab/NAME.so, from the product's own source list (stellard_amd/build.py build_product);
# load one with STL_LIB_PATH.
set -e
cd "$(dirname "$0")/.."
pids=()
while [ $# -ge 2 ]; do
  n=$1; f=$2; shift 2
  ( python3 -c 'import sys; from stellard_amd.build import build_product
build_product(extra_flags=sys.argv[2].split(), variant=sys.argv[1])' "$n" "$f" && echo "built $n" ) &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
