"""Generates tests/golden/lexmin_kat.json: known-answer vectors for the `sourmash` hashing rule (canon=lexmin): MurmurHash3_x64_128,
seed 42, of whichever of a k-mer and its reverse complement is the smaller upper-case string.

As in gen_murmur3_kat.py the murmur is independent of this repository: the public-domain Appleby source that scikit-learn
vendors (<site-packages>/sklearn/utils/src/MurmurHash3.cpp), compiled in a temp dir; the strand is chosen here with Python's
bytes comparison.  The vectors pin the preset by the published rule plus an independent murmur -- not by a run of sourmash
itself.  Run: python tests/golden/gen_lexmin_kat.py
"""
import json, os, random, subprocess, tempfile
import sklearn

src_dir = os.path.join(os.path.dirname(sklearn.__file__), "utils", "src")
drv = r'''
#include "MurmurHash3.h"
#include <cstdio>
#include <cstring>
#include <cstdint>
int main(int argc, char** argv){
  char line[4096];
  while (fgets(line, sizeof line, stdin)) {
    int n = (int)strcspn(line, "\r\n");
    uint64_t out[2]; MurmurHash3_x64_128(line, n, 42, out);
    printf("%llu %llu\n", (unsigned long long)out[0], (unsigned long long)out[1]);
  }
  return 0; }
'''
COMP = {65: 84, 84: 65, 67: 71, 71: 67}


def rc(s):
    return bytes(COMP[c] for c in reversed(s))


rng = random.Random(20261016)
kmers = []
for k in list(range(8, 33)) + [40, 64]:
    kmers.append(bytes(rng.choice(b"ACGT") for _ in range(k)))
    kmers.append(bytes(rng.choice(b"ACGT") for _ in range(k)))
    if k % 2 == 0:  # a palindrome: its own reverse complement
        half = bytes(rng.choice(b"ACGT") for _ in range(k // 2))
        kmers.append(half + rc(half))
    # The latest place where the two strands can differ FIRST is the middle: base i of the reverse complement is the complement
    # of base k - 1 - i, so strands that agree on the first half agree everywhere (no k-mer differs first at its last base).
    # These k-mers agree with their reverse complement on every base before the middle one (odd k) or the middle pair (even k).
    half = bytes(rng.choice(b"ACGT") for _ in range((k - 1) // 2))
    if k % 2:
        mid = bytes([rng.choice(b"ACGT")])          # odd k: the middle base is never its own complement
        kmers.append(half + mid + rc(half))
    else:
        a = rng.choice(b"ACGT")
        b = rng.choice([c for c in b"ACGT" if c != COMP[a]])
        kmers.append(half + bytes([a, b]) + rc(half))
with tempfile.TemporaryDirectory() as td:
    open(os.path.join(td, "drv.cpp"), "w").write(drv)
    exe = os.path.join(td, "kat")
    subprocess.check_call(["g++", "-O1", "-I", src_dir, os.path.join(td, "drv.cpp"), os.path.join(src_dir, "MurmurHash3.cpp"), "-o", exe])
    strands = [min(km, rc(km)) for km in kmers]
    out = subprocess.check_output([exe], input=b"".join(s + b"\n" for s in strands)).split()
vec = [{"kmer": km.decode(), "k": len(km), "lexmin_strand": s.decode(), "h1": int(out[2 * i]), "h2": int(out[2 * i + 1])}
       for i, (km, s) in enumerate(zip(kmers, strands))]
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lexmin_kat.json")
json.dump({"source": "sklearn/utils/src/MurmurHash3.cpp (Appleby, public domain), sklearn " + sklearn.__version__ + "; seed 42",
           "vectors": vec}, open(path, "w"), indent=0)
print("wrote", path, len(vec), "palindromes", sum(v["kmer"] == rc(v["kmer"].encode()).decode() for v in vec),
      "forward is lexmin", sum(v["kmer"] == v["lexmin_strand"] for v in vec))
