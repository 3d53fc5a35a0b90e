#!/bin/bash
# AddressSanitizer + UBSan over the host form of search (rk_scaled_host.cpp: rk_search_scaled_host, rk_search_min_count) as a
# stand-alone program: the hand-checked vectors of tests/golden/search_kat.json on 1 and 4 threads, seeded random sets against a plain
# loop, the threshold rule against its definition, every refusal.  Host code only, no GPU needed.
# Usage: bash tools/asan_search/run.sh
set -e
HERE=$(cd "$(dirname "$0")" && pwd); ROOT=$(cd "$HERE/../.." && pwd); W=${TMPDIR:-/tmp}/rk_asan_search; mkdir -p $W
g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$ROOT/include $HERE/main.cpp $ROOT/rkmh_amd/csrc/rk_scaled_host.cpp -o $W/search_asan
python3 - $ROOT/tests/golden/search_kat.json > $W/vectors.txt <<'PY'
import json, sys
def side(pieces):
    out = []
    for p in pieces:
        out.extend(range(p[1], p[2], p[3]) if isinstance(p, list) else [p])
    return out
for v in json.load(open(sys.argv[1])):
    queries, refs = [side(q) for q in v["queries"]], [side(r) for r in v["refs"]]
    row = [v["min_shared"], int(v["q_min"] is not None), len(v["want"])] + [x for w in v["want"] for x in w] + [len(queries)] + (v["q_min"] or [])
    for q in queries:
        row += [len(q)] + q
    row += [len(refs)]
    for r in refs:
        row += [len(r)] + r
    print(*row)
PY
$W/search_asan $W/vectors.txt 2> $W/err.txt || { cat $W/err.txt; exit 1; }
echo "sanitizer output: $(wc -c < $W/err.txt) bytes"
