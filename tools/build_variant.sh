#!/bin/bash
# Builds a variant of the library for same-box A/B timing (tools/ab_bench.sh, tools/ab_long.sh):
#   tools/build_variant.sh <name> [-DFLAG ...]   ->   decodingustools_amd/lib/libcallable_hip_<name>.so
# from the product's own source list (decodingustools_amd.build.SOURCES)
set -e
cd "$(dirname "$0")/.."
name=$1; shift
mapfile -t SRC < <(python -c "from decodingustools_amd.build import SOURCES; print('\n'.join(SOURCES))")
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Wall -Wno-unused-function "$@" \
  "${SRC[@]}" -lz -ldl \
  -o decodingustools_amd/lib/libcallable_hip_$name.so 2>&1 | grep -E "error|spill" || true
ls -la decodingustools_amd/lib/libcallable_hip_$name.so
