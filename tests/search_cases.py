"""Inputs the search tests share (tests/test_search_cpu.py, tests/test_gpu_search.py): the hand-checked vectors, seeded random
collections with the model's hits, collections laid out around the edges of a reference block, and posting lists of chosen lengths --
computed once per process and left unchanged."""
import functools
import json
import os

import numpy as np

import scaled_cases as sc
import search_model as sem

NREFS = (1, 9, 65, 1100)     # one reference; a few; more than one wave's span of counters in use; many
NQS = (1, 9, 65)             # the first nq queries of a case are a case of their own: their hits are the hits whose query is below nq
REF_BLOCK = 8192             # include/rkmh_amd.h: RK_SEARCH_REF_BLOCK (asserted equal to the binding's by the tests)


def _side(pieces):
    a = sc._expand(pieces)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def kat():
    """-> tuple of dict(name, refs, queries, min_shared, q_min, want): rows uint64 arrays, want int32 [n, 3]"""
    doc = json.load(open(os.path.join(sc.GOLDEN, "search_kat.json")))
    out = []
    for v in doc:
        want = np.asarray(v["want"], dtype=np.int32).reshape(len(v["want"]), 3)
        want.setflags(write=False)
        out.append(dict(name=v["name"], refs=tuple(_side(r) for r in v["refs"]), queries=tuple(_side(q) for q in v["queries"]),
                        min_shared=int(v["min_shared"]), q_min=v["q_min"], want=want))
    return tuple(out)


def first_queries(hits, nq):
    return hits[hits[:, 0] < nq]


@functools.lru_cache(maxsize=None)
def random_case(nref):
    """-> dict(refs, queries, want1, cut, want_cut, q_min, want_qmin): nref rows with lengths from scaled_cases.LENGTHS, the first one
    the 70 000 row, 65 queries drawn from the same pool (the first of 1 000 values); want1: the hits at min_shared = 1; cut: the median
    of their counts, a threshold with pairs on both sides; q_min: a threshold of its own per query, some below `cut`, some above"""
    rng = np.random.default_rng(2000 + nref)
    pl = sc.pool(rng, 100000)
    refs = sc.random_sets(rng, nref, pl, first=sc.LONG_ROW)
    queries = sc.random_sets(rng, max(NQS), pl, first=1000)
    for a in refs + queries:
        a.setflags(write=False)
    want1 = sem.search(refs, queries)
    cut = max(2, int(np.median(want1[:, 2])))
    q_min = rng.integers(1, 2 * cut + 1, size=len(queries)).astype(np.int32)
    out = dict(refs=tuple(refs), queries=tuple(queries), want1=want1, cut=cut, want_cut=want1[want1[:, 2] >= cut], q_min=q_min,
               want_qmin=want1[want1[:, 2] >= np.maximum(q_min, 2)[want1[:, 0]]])
    for k in ("want1", "want_cut", "q_min", "want_qmin"):
        out[k].setflags(write=False)
    return out


BLOCK_EDGE_NREFS = (REF_BLOCK - 1, REF_BLOCK, REF_BLOCK + 1, 2 * REF_BLOCK + 1)


@functools.lru_cache(maxsize=None)
def block_edges(nref):
    """-> dict(refs, queries, edge): nref rows of 1 to 3 values from a few hundred distinct ones.  Every row holds EVERY (so its posting
    list has nref entries and spans every block); the first and the last reference of every block hold EDGE_A and EDGE_B and nothing
    else; the other rows hold up to two values of a pool of 300.  Queries: [EVERY]; [EDGE_A, EDGE_B] (2 shared with the edge rows alone);
    60 pool values and EVERY; the same plus the edge values."""
    rng = np.random.default_rng(3000 + nref)
    every, edge_a, edge_b = np.uint64(1 << 40), np.uint64(5), np.uint64((1 << 64) - 2)
    pl = np.unique(rng.integers(1 << 20, 1 << 63, size=300, dtype=np.uint64))
    edge = sorted(set(x for b in range(0, nref, REF_BLOCK) for x in (b, min(b + REF_BLOCK - 1, nref - 1))))
    extra = rng.integers(0, 3, size=nref)
    refs = [np.unique(np.concatenate([[every], rng.choice(pl, size=int(extra[r]), replace=False)]).astype(np.uint64)) for r in range(nref)]
    for r in edge:
        refs[r] = np.unique(np.array([every, edge_a, edge_b], dtype=np.uint64))
    some = np.sort(rng.choice(pl, size=60, replace=False))
    queries = [np.array([every], dtype=np.uint64), np.unique(np.array([edge_a, edge_b], dtype=np.uint64)),
               np.unique(np.concatenate([some, [every]]).astype(np.uint64)), np.unique(np.concatenate([some, [every, edge_a, edge_b]]).astype(np.uint64))]
    for a in refs + queries:
        a.setflags(write=False)
    assert all(1 <= len(r) <= 3 for r in refs) and len(np.unique(np.concatenate(refs))) <= 303
    return dict(refs=tuple(refs), queries=tuple(queries), edge=tuple(edge))


POSTING_LENGTHS = (63, 64, 65, 129)


@functools.lru_cache(maxsize=None)
def posting_lists(length):
    """-> dict(refs, queries): 300 references inside one block; the value LONG is held by `length` of them (a run that starts at
    reference 100), the value SHORT by 3, every reference holds one value of its own; queries: [LONG], [SHORT, LONG], [LONG, one own value]"""
    long_v, short_v = np.uint64(1 << 50), np.uint64(77)
    refs = []
    for r in range(300):
        row = [np.uint64(1000 + r)]
        if 100 <= r < 100 + length:
            row.append(long_v)
        if r in (0, 150, 299):
            row.append(short_v)
        a = np.unique(np.array(row, dtype=np.uint64))
        a.setflags(write=False)
        refs.append(a)
    queries = [np.array([long_v], dtype=np.uint64), np.unique(np.array([short_v, long_v], dtype=np.uint64)),
               np.unique(np.array([long_v, 1000 + 120], dtype=np.uint64))]
    return dict(refs=tuple(refs), queries=tuple(queries))


KEY_TOTALS = (1, 63, 64, 65, 1023, 1024, 1025, 2049)   # entries of the sorted value array the index's keys are compacted from
KEY_EDGES = (64, 1024)                                  # where a wave's 64 elements and a workgroup's 1 024 end in that compaction


@functools.lru_cache(maxsize=None)
def key_edges(total):
    """-> dict(refs, nkeys, longest, runs): five references whose values, concatenated and sorted, are `total` entries laid out around
    KEY_EDGES.  The first value and the last one are each held by two references (entries 0, 1 and total - 2, total - 1; at total = 1
    they are one entry).  At every edge e a value held by three references stands at entries e - 2, e - 1, e wherever these lie
    between the two pairs (total >= e + 3); at total = e + 1 the last value's pair itself lies across the edge, and below that the
    edge is not reached.  Every other value is held by one reference.  The value of multiplicity m that is the i-th distinct one is
    held by references i % 5 ... (i + m - 1) % 5; the last value is 2^64 - 1.  runs: entry where a repeated value begins -> its length."""
    runs = {} if total < 2 else {0: 2, total - 2: 2}
    for e in KEY_EDGES:
        if total >= e + 3:
            runs[e - 2] = 3
    mult, t = [], 0
    while t < total:
        mult.append(runs.get(t, 1))
        t += mult[-1]
    assert t == total
    values = (np.arange(1, len(mult) + 1, dtype=np.uint64) << np.uint64(20)) + np.uint64(3)
    values[-1] = np.uint64((1 << 64) - 1)
    rows = [[] for _ in range(5)]
    for i, (v, m) in enumerate(zip(values, mult)):
        for j in range(m):
            rows[(i + j) % 5].append(v)
    refs = tuple(np.array(r, dtype=np.uint64) for r in rows)
    for a in refs:
        a.setflags(write=False)
    return dict(refs=refs, nkeys=len(mult), longest=max(mult), runs=runs)
