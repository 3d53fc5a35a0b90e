#!/bin/bash
# AddressSanitizer + UBSan over the weighted-comparison functions of rk_scaled_host.cpp (rk_compare_scaled_abund_host,
# rk_abund_row_sums_host, rk_angular_similarity) as a stand-alone program: the hand-checked vectors of tests/golden/wdist_kat.json (on 1
# and 4 threads, mirrored, against themselves), seeded random CSR sets against a set-algebra loop, every refusal.  Host code only, no
# GPU needed.
# Usage: bash tools/asan_wdist/run.sh
set -e
HERE=$(cd "$(dirname "$0")" && pwd); ROOT=$(cd "$HERE/../.." && pwd); W=${TMPDIR:-/tmp}/rk_asan_wdist; mkdir -p $W
g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$ROOT/include $HERE/main.cpp $ROOT/rkmh_amd/csrc/rk_scaled_host.cpp -o $W/wdist_asan
python3 - $ROOT/tests/golden/wdist_kat.json > $W/vectors.txt <<'PY'
import json, sys
def side(pieces):
    out = []
    for p in pieces:
        out.extend(range(p[1], p[2], p[3]) if isinstance(p, list) else [p])
    return out
def abund(pieces):
    out = []
    for p in pieces:
        out.extend([p[1]] * p[2] if isinstance(p, list) else [p])
    return out
for v in json.load(open(sys.argv[1])):
    if v["kind"] == "pair":
        a, aw, b, bw = side(v["a"]), abund(v["aw"]), side(v["b"]), abund(v["bw"])
        print("P", *(v["want"] + v["sums_a"] + v["sums_b"] + [len(a)] + a + aw + [len(b)] + b + bw))
    else:
        print("S", v["dot"], v["sumsq_a"], v["sumsq_b"], repr(float(v["cosine"])), repr(float(v["angular"])))
PY
$W/wdist_asan $W/vectors.txt 2> $W/err.txt || { cat $W/err.txt; exit 1; }
echo "sanitizer output: $(wc -c < $W/err.txt) bytes"
