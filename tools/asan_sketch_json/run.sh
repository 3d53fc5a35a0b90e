#!/bin/bash
# AddressSanitizer + UBSan over the reader of sketch files (rkmh_sketch_json.cpp: load_sketch_json) as a stand-alone program: the files
# the refusal tests of tests/test_scaled_cpu.py and tests/test_abund_cpu.py make (good and bad), a bottom-s file, a scaled file and one
# with abundances cut after every byte, the empty file.
# Host code only, no GPU needed.
# Usage: bash tools/asan_sketch_json/run.sh
set -e
HERE=$(cd "$(dirname "$0")" && pwd); ROOT=$(cd "$HERE/../.." && pwd); W=${TMPDIR:-/tmp}/rk_asan_sketch_json; rm -rf $W; mkdir -p $W/in
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$ROOT/include -I$ROOT/rkmh_amd/csrc $HERE/main.cpp $ROOT/rkmh_amd/csrc/rkmh_sketch_json.cpp $ROOT/rkmh_amd/csrc/rk_scaled_host.cpp -pthread -o $W/sketch_json_asan
python3 - $W/in <<'PY'
import json, os, sys
W = sys.argv[1]
MAX = lambda s: (2 ** 64 - 1) // s
def sketch_file(name, scaled=None, hashes=(3, 9, 20), length=None, max_hash=None, per_object_scaled=None, kmer="16", abund=None, abund_in=(0, 1)):   # tests/test_scaled_cpu.py::_sketch_file; abund: tests/test_abund_cpu.py::_abund_file
    doc = []
    for i in range(2):
        d = {"alphabet": "ATGC", "canonical": "true", "hashBits": 64, "hashPolicy": "fold=swap32,windows=len-k,zero=count,mask=lt,freqmax=incl,seed=42",
             "hashSeed": 42, "hashType": "MurmurHash3_x64_128", "kmer": kmer, "name": "s%d" % i, "preserveCase": "false", "seqLen": 100,
             "sketches": {"comment": "", "hashes": list(hashes), "length": len(hashes) if length is None else length, "name": "s%d" % i}}
        if abund is not None and i in abund_in:
            d["sketches"]["abundances"] = abund
        s = per_object_scaled[i] if per_object_scaled else scaled
        if s:
            d["scaled"], d["maxHash"] = s, MAX(s) if max_hash is None else max_hash
        doc.append(d)
    text = json.dumps(doc, separators=(",", ":"), sort_keys=True)
    open(os.path.join(W, name + ".json"), "w").write(text)
    return text
scaled = sketch_file("sc10", scaled=10)
bottom = sketch_file("bottom", length=4)
sketch_file("sc100", scaled=100)
sketch_file("k21", scaled=10, kmer="21")
sketch_file("mixed", per_object_scaled=[10, 100])
sketch_file("half", per_object_scaled=[10, 0])
sketch_file("unsorted", scaled=10, hashes=(9, 3, 20))
sketch_file("repeat", scaled=10, hashes=(3, 9, 9))
sketch_file("zero", scaled=10, hashes=(0, 3, 9))
sketch_file("above", scaled=10, hashes=(3, 9, MAX(10) + 1))
sketch_file("wrongmax", scaled=10, max_hash=12345)
with_abund = sketch_file("abund", scaled=10, abund=[1, 7, 4294967295])
for i, bad in enumerate(([1, 2], [1, 2, 3, 4], [], [1, 0, 3], [1, 4294967296, 3], [1, 18446744073709551616, 3], [1, -2, 3], [1, 2.5, 3], [1, "x", 3], 7)):
    sketch_file("abund_bad%d" % i, scaled=10, abund=bad)
sketch_file("abund_half0", scaled=10, abund=[1, 1, 1], abund_in=(1,))
sketch_file("abund_half1", scaled=10, abund=[1, 1, 1], abund_in=(0,))
sketch_file("abund_bottom", length=4, abund=[1, 1, 1])
for tag, text in (("cut_scaled", scaled), ("cut_bottom", bottom), ("cut_abund", with_abund)):
    for n in range(len(text)):                       # n = 0: the empty file
        open(os.path.join(W, "%s_%04d.json" % (tag, n)), "w").write(text[:n])
PY
$W/sketch_json_asan $W/in/*.json > $W/out.txt 2> $W/err.txt || { cat $W/err.txt; exit 1; }
echo "$(wc -l < $W/out.txt) loads, $(grep -c "	ok	" $W/out.txt) ok; sanitizer output: $(wc -c < $W/err.txt) bytes"
