"""Inputs of the dedup=distinct tests (tests/test_gpu_dedup.py) and their non-vacuity conditions, which tests/test_policy_dedup_cpu.py
checks on the model without a GPU.  Sizes are the smallest at which each branch of the device code can go wrong: S = 16 for raw
hash arrays (the in-LDS sorter's smallest buffer P = 64, its largest 16 384, the multi-block select above that and above 2^18),
S = 64 for sequences (references longer than next_pow2(S) windows take the block pre-select)."""
import numpy as np

import dedup_model as dm
import sourmash_model as sm

S_RAW = 16
P_MIN = 64                   # smallest sort buffer of k_sort_intersect (next_pow2 from 64 up)
SORT_MAX_P = 16384           # largest in-LDS sort (rk_kernels.hpp): longer arrays are selected from by several blocks
PRESEL_SIDE = 1024
BIG = 262145                 # beyond the block pre-select's 2^18
S_SEQ = 64
ROW_K = (16, 18, 24)
SPECS = (("sourmash", dm.SOURMASH), ("dedup=distinct", dm.DISTINCT_DEFAULT))
SET_WINDOWS = 2048           # capacity of the kernel's per-read set of distinct hashes (DEDUP_MAX_SLOTS / 2, rk_classify.hip)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _u(a):
    return np.asarray(a, dtype=np.uint64)


def raw_arrays():
    """name -> (hashes, S)"""
    rng = np.random.default_rng(5)
    S = S_RAW
    out = {}
    for n in (0, 1, S - 1, S, S + 1, P_MIN, P_MIN + 1, SORT_MAX_P, SORT_MAX_P + 1):
        out["n=%d few values" % n] = (_u(rng.integers(0, 40, n)), S)             # zeros and heavy duplicates
        out["n=%d 64-bit values" % n] = (rng.integers(1, 2**63, n, dtype=np.uint64) * _u(2) + _u(1), S)
    out["all equal"] = (_u([7] * 100), S)
    out["all equal, selected from"] = (_u([7] * (SORT_MAX_P + 5)), S)
    out["zeros and duplicates"] = (_u([0, 9, 0, 3, 3, 3, 0, 9, 1, 0, 1] * 9), S)
    low = list(range(1, S))                                                      # S - 1 distinct values below the S-th
    for copies in (1, 2, 40):
        for n in (300, SORT_MAX_P + 300):
            h = low * 3 + [1000] * copies + rng.integers(2000, 2**40, n - 3 * len(low) - copies).tolist()
            out["the S-th distinct value %d times, n=%d" % (copies, n)] = (rng.permutation(_u(h)), S)
    for n in (4 * P_MIN, 4 * SORT_MAX_P):
        out["fewer than S distinct among %d" % n] = (_u(rng.choice(_u([11, 5, 2**50, 77, 3, 2**63 + 5, 0]), n)), S)
    top = _u(0xABCDE12345678) << _u(12)
    for n in (500, SORT_MAX_P + 500):
        out["top 52 bits shared, n=%d" % n] = (top | _u(rng.integers(0, 4096, n)), S)
        out["top 52 bits shared, few values, n=%d" % n] = (top | _u(rng.integers(0, 12, n)), S)
    n = SORT_MAX_P + 4000
    below = rng.integers(1, 2**40, S - 3).tolist()
    rest = (rng.integers(2**62, 2**63, n - 5000 - len(below), dtype=np.uint64)).tolist()
    out["threshold bucket is one value repeated"] = (rng.permutation(_u(below + [2**61 + 12345] * 5000 + rest)), S)
    bucket = (_u(0x5A5) << _u(52)) | _u(rng.integers(0, 2**52, 3000))             # > PRESEL_SIDE values in one top-12-bit bucket
    bucket = np.concatenate([bucket, bucket[:1500]])                              # ... half of them twice
    rest = rng.integers(2**63, 2**64 - 1, n - len(bucket) - 4, dtype=np.uint64)
    out["threshold bucket larger than PRESEL_SIDE"] = (rng.permutation(np.concatenate([_u([1, 2, 3, 3]), bucket, rest])), S)
    vals = rng.integers(1, 2**63, 3 * S, dtype=np.uint64)
    out["262145 hashes from 3S distinct values"] = (vals[rng.integers(0, 3 * S, BIG)], S)
    out["262145 hashes from S-1 distinct values"] = (vals[rng.integers(0, S - 1, BIG)], S)
    return out


def raw_conditions(arrays):
    """what the arrays must show for the tests to mean something (on the model)"""
    differ = sum(dm.bottom_distinct(h, S).tolist() != sm.bottom(h, S).tolist() for h, S in arrays.values())
    assert 2 * differ >= len(arrays), differ                                   # the multiset rule answers most of them differently
    h, S = arrays["threshold bucket is one value repeated"]
    sk = dm.bottom_distinct(h, S)
    assert len(sk) == S and int((h == sk[S - 3]).sum()) == 5000                 # the repeated value is inside the sketch, once
    h, S = arrays["threshold bucket larger than PRESEL_SIDE"]
    sk = dm.bottom_distinct(h, S)
    assert (sk[3:] >> _u(52) == _u(0x5A5)).all() and len(np.unique(h[(h >> _u(52)) == _u(0x5A5)])) > PRESEL_SIDE
    h, S = arrays["262145 hashes from S-1 distinct values"]
    assert len(dm.bottom_distinct(h, S)) == S - 1 and len(sm.bottom(h, S)) == S
    h, S = arrays["262145 hashes from 3S distinct values"]
    assert len(dm.bottom_distinct(h, S)) == S and len(np.unique(sm.bottom(h, S))) < S
    for name, (h, S) in arrays.items():
        if "64-bit values" in name:
            assert dm.bottom_distinct(h, S).tolist() == sm.bottom(h, S).tolist(), name      # no repeats: both rules agree


def filter_counter(h, slots=10007):
    """a depth table that removes the smallest non-zero value of h through the range filter [1, 1], and nothing else"""
    nz = np.unique(h[h != 0])
    counter = np.ones(slots, dtype=np.int32)
    if len(nz):
        counter[int(nz[0] % _u(slots))] = 5
    return counter


def rand(rng, n):
    return bytes(rng.choice(ACGT, n).tolist())


def references():
    """twelve random 150-base references, the tandem repeat ACGTT x 400, and one that contains reference 0 twice"""
    rng = np.random.default_rng(21)
    refs = [rand(rng, 150) for _ in range(12)]
    refs.append(b"ACGTT" * 400)
    refs.append(rand(rng, 40) + refs[0] + rand(rng, 25) + refs[0] + rand(rng, 30))
    return refs


def reads(k, pol):
    """about eighty reads for k-mer size k under the window rule of pol; returns (reads, kinds)"""
    rng = np.random.default_rng(100 + k)
    refs = references()
    extra = k if pol["drop_last"] else k - 1              # read length = windows + extra
    tail = b"A" if pol["drop_last"] else b""              # (windows=len-k: a k-mer at the very end starts no window)
    sk = dm.sketch_refs(refs, [k], S_SEQ, pol)
    out, kinds = [], []

    def add(kind, r):
        out.append(r); kinds.append(kind)

    for i in range(16):                                   # drawn from the references, no repeat, at most S windows
        j = i % 12
        p = int(rng.integers(0, 150 - (40 + extra)))
        add("drawn", refs[j][p:p + 40 + extra])
    for i in range(14):                                   # a k-mer that IS a sketch hash, twice (at most S windows)
        j = i % 12
        h = sm.window_hashes(refs[j], k, pol)
        at = np.nonzero(np.isin(h, sk[j]))[0]
        p = int(at[int(rng.integers(0, len(at)))])
        km = refs[j][p:p + k]
        q = int(rng.integers(0, 150 - (10 + extra)))
        add("sketch k-mer repeated", km + b"T" + refs[j][q:q + 10 + extra] + km + tail)
    for i in range(12):                                   # a k-mer of no sketch, twice: only field 3 moves
        j = i % 12
        x = rand(rng, k)
        q = int(rng.integers(0, 150 - (15 + extra)))
        add("foreign k-mer repeated", x + refs[j][q:q + 14 + extra] + x + tail)
    for i in range(10):                                   # tandem copies of the repeat reference's unit, then a piece of another reference
        j = i % 12
        q = int(rng.integers(0, 150 - (30 + extra)))
        add("tandem + piece", b"ACGTT" * ((k + 24) // 5 + i % 4) + refs[j][q:q + 30 + extra])   # ~25 windows of the repeat
    for i in range(6):
        add("tandem", (b"ACGTT" * 40)[i:i + 30 + extra])
    # k-mers of reference 0 that the reference containing it twice sketches twice, each twice in the read: the multiset rule
    # scores the container 2 per k-mer and reference 0 one, the set rule ties them and the first index wins
    h0 = sm.window_hashes(refs[0], k, pol)
    v13, c13 = np.unique(sm.bottom(sm.window_hashes(refs[13], k, pol), S_SEQ), return_counts=True)
    at = np.nonzero(np.isin(h0, v13[c13 >= 2]))[0]
    for i in range(6):
        ps = rng.choice(at, 3, replace=False)
        add("doubled in the container", b"".join(refs[0][int(p):int(p) + k] * 2 for p in ps) + tail)
    for i in range(6):                                    # N runs between repeated pieces
        j = i % 12
        piece = refs[j][10:10 + k + 6]
        add("N runs", piece + b"N" * (1 + i) + piece + b"NN" + rand(rng, k + 3))
    for w in (0, 1):                                      # lengths 0, k - 1, k and one window exactly
        add("edge", b"") if w == 0 else add("edge", refs[1][:k - 1])
    add("edge", refs[2][:k]); add("edge", refs[3][:extra + 1])
    for w in (255, 256, 257):                             # 8- | 16-bit counter fields: low complexity (answered by the kernel) and random (general path)
        unit = rand(rng, 11)
        add("windows %d tandem" % w, (unit * 40)[:w + extra])
        add("windows %d random" % w, rand(rng, w + extra))
    for i in range(6):                                    # more windows than S, fewer distinct hashes than S
        unit = rand(rng, 7 + i)
        add("long, few distinct", (unit * 40)[:S_SEQ + 20 + 10 * i + extra])
    return out, kinds


def pack(seqs, pad=64):
    b = np.frombuffer(b"".join(seqs) + b"\0" * pad, dtype=np.uint8).copy()
    o = np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)
    return b, o


def max_repeat(read, k, pol):
    h = sm.window_hashes(read, k, pol)
    h = h[h != 0]
    return int(np.unique(h, return_counts=True)[1].max()) if len(h) else 0


def flag_allowed(read, k, pol):
    """May the fused kernel hand this read back?  Only when its DISTINCT hashes exceed the sketch (bottom-S selection: the general
    path, as for the multiset rule), or it has more windows than the kernel's set of distinct hashes holds."""
    h = sm.window_hashes(read, k, pol)
    return len(np.unique(h[h != 0])) > S_SEQ or len(h) > SET_WINDOWS


def row_conditions(k, pol):
    """(reads, kinds, distinct rows, multiset rows) after the non-vacuity checks"""
    refs = references()
    rd, kinds = reads(k, pol)
    assert 70 <= len(rd) <= 90
    want = dm.classify(rd, dm.sketch_refs(refs, [k], S_SEQ, pol), [k], S_SEQ, pol)
    multi = sm.classify(rd, sm.sketch_refs(refs, [k], S_SEQ, pol), [k], S_SEQ, pol)
    differ = (want != multi).any(axis=1)
    assert 3 * int(differ.sum()) >= len(rd), int(differ.sum())                  # at least a third of the rows
    for f in range(4):
        assert (want[:, f] != multi[:, f]).any(), f                            # every field somewhere
    only3 = [i for i, kd in enumerate(kinds) if kd == "foreign k-mer repeated"]
    assert all((want[i, :3] == multi[i, :3]).all() and want[i, 3] < multi[i, 3] for i in only3)
    nwin = [len(sm.window_hashes(r, k, pol)) for r in rd]
    assert {0, 1, 255, 256, 257} <= set(nwin)
    # reads the kernel itself must answer: at most 256 windows (and, with more, few distinct hashes), nothing repeated more than 30 times
    must = [i for i, r in enumerate(rd) if not flag_allowed(r, k, pol)]
    assert sum(1 for i in must if nwin[i] > S_SEQ) >= 8                          # ... among them reads with more windows than S
    assert any(kinds[i] == "windows 256 tandem" for i in must) and any(kinds[i] == "windows 257 tandem" for i in must)
    assert 4 * len(must) >= 3 * len(rd)
    return rd, kinds, want, multi
