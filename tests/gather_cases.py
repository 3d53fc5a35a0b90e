"""Inputs the gather tests share (tests/test_gather_cpu.py, tests/test_gather_gpu.py): the hand-checked vectors and seeded random
cases with the model's rows -- computed once per process and left unchanged."""
import functools
import json
import os

import numpy as np

import gather_model as gm
import scaled_cases as sc

NREFS = (1, 9, 65, 1100)      # one reference; a few; more than one wave of candidates per workgroup; more than one 1 024-wide pick stride


def _side(pieces):
    a = sc._expand(pieces)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def kat():
    """-> tuple of dict(name, q, refs, min_shared, max_rounds, want): q and refs uint64 arrays, want int32 [n, 4]"""
    doc = json.load(open(os.path.join(sc.GOLDEN, "gather_kat.json")))
    out = []
    for v in doc:
        want = np.asarray(v["want"], dtype=np.int32).reshape(len(v["want"]), 4)
        want.setflags(write=False)
        out.append(dict(name=v["name"], q=_side(v["q"]), refs=tuple(_side(r) for r in v["refs"]), min_shared=int(v["min_shared"]),
                        max_rounds=v["max_rounds"], want=want))
    return tuple(out)


def foreign(rng, n, known):
    """n distinct values that `known` does not hold"""
    f = np.unique(rng.integers(1, 1 << 64, size=n + n // 8 + 8, dtype=np.uint64, endpoint=False))
    return rng.permutation(f[~np.isin(f, known)])[:n]


def query_of(rng, rows, pl, size=None):
    """the union of the rows plus as many foreign values (or foreign values up to `size` in all)"""
    u = np.unique(np.concatenate([np.zeros(0, np.uint64)] + list(rows)))
    q = np.unique(np.concatenate([u, foreign(rng, len(u) if size is None else size - len(u), pl)]))
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def random_case(nref):
    """-> (q, refs, want): lengths from scaled_cases.LENGTHS, the query made of the five longest rows and as many foreign values"""
    rng = np.random.default_rng(1000 + nref)
    pl = sc.pool(rng, 6000)
    refs = sc.random_sets(rng, nref, pl, first=1000)
    longest = sorted(range(nref), key=lambda i: -len(refs[i]))[:5]
    q = query_of(rng, [refs[i] for i in longest], pl)
    want = gm.gather(q, refs)
    want.setflags(write=False)
    return q, tuple(refs), want


@functools.lru_cache(maxsize=None)
def staircase(n):
    """n disjoint references of strictly decreasing sizes, listed smallest first, and a query that holds them all plus foreign values:
    the model picks exactly n of them, from the last index down.  n = 0: one reference the query shares nothing with."""
    rng = np.random.default_rng(50 + n)
    m = max(n, 1)
    vals = np.sort(foreign(rng, (m + 3) * m, np.zeros(0, np.uint64)))
    refs, at = [], 0
    for i in range(m):                                        # sizes 3 + 1, 3 + 2, ...
        refs.append(vals[at:at + 4 + i])
        at += 4 + i
    q = query_of(rng, refs if n else [], vals)
    return q, tuple(refs)
