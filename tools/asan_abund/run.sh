#!/bin/bash
# AddressSanitizer + UBSan over the abundance functions of rk_scaled_host.cpp (rk_merge_scaled_abund, rk_gather_scaled_abund_host) as a
# stand-alone program: the hand-checked vectors of tests/golden/abund_kat.json (gather on 1 and 4 threads), seeded random sets against
# plain loops, every refusal.  Host code only, no GPU needed.
# Usage: bash tools/asan_abund/run.sh
set -e
HERE=$(cd "$(dirname "$0")" && pwd); ROOT=$(cd "$HERE/../.." && pwd); W=${TMPDIR:-/tmp}/rk_asan_abund; mkdir -p $W
g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$ROOT/include $HERE/main.cpp $ROOT/rkmh_amd/csrc/rk_scaled_host.cpp -o $W/abund_asan
python3 - $ROOT/tests/golden/abund_kat.json > $W/vectors.txt <<'PY'
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
    if v["kind"] == "gather":
        q, a, refs = side(v["q"]), abund(v["abund"]), [side(r) for r in v["refs"]]
        row = ["G", v["min_shared"], v["max_rounds"] or len(refs), len(v["want"])] + [x for w in v["want"] for x in w] + v["wunique"] + [len(q)] + q + a + [len(refs)]
        for r in refs:
            row += [len(r)] + r
    else:
        row = ["M", (1 << 64) - 1 if v["max_hash"] is None else v["max_hash"], len(v["parts"])]
        for p in v["parts"]:
            row += [len(p["v"])] + p["v"] + p["a"]
        row += [len(v["want_v"])] + v["want_v"] + v["want_a"]
    print(*row)
PY
$W/abund_asan $W/vectors.txt 2> $W/err.txt || { cat $W/err.txt; exit 1; }
echo "sanitizer output: $(wc -c < $W/err.txt) bytes"
