#!/bin/bash
# AddressSanitizer + UBSan over the host-only planning layer of the index build (rkmh_amd/csrc/rk_index_plan.hpp) as a stand-alone
# program: hash-space table with its overflow chains and value forms, first-level filter, build_kpost, compound values, group filter and
# the exact maps of narrow and wide k-mers, each read back with the documented probe; the refusals but "postings overflow" (2^30 posting words).  The layer includes rk_device.hpp
# for its __host__ __device__ helpers, so hipcc compiles it; only the host half runs.  Host code only, no GPU needed.
# Usage: bash tools/asan_index/run.sh
set -e
HERE=$(cd "$(dirname "$0")" && pwd); ROOT=$(cd "$HERE/../.." && pwd); W=${TMPDIR:-/tmp}/rk_asan_index; mkdir -p $W
${HIPCC:-/opt/rocm/bin/hipcc} --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -Xarch_host -fno-omit-frame-pointer -I$ROOT/rkmh_amd/csrc -x hip $HERE/main.cpp -o $W/index_asan
$W/index_asan 2> $W/err.txt || { cat $W/err.txt; exit 1; }
echo "sanitizer output: $(wc -c < $W/err.txt) bytes"
