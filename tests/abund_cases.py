"""Inputs the abundance tests share (tests/test_abund_cpu.py, tests/test_gpu_abund.py): the hand-checked vectors, abundances for the
random CSR sets of gather_cases, sequences whose k-mers repeat, and the model's sketches of the bundled files -- computed once per
process and left unchanged."""
import functools
import json
import os

import numpy as np

import abund_model as am
import gather_cases as gc
import scaled_cases as sc
import scaled_model as scm
import sourmash_model as sm


def _abund(pieces):
    """abundances as written: numbers and ["rep", value, count] pieces"""
    out = []
    for p in pieces:
        if isinstance(p, list):
            assert p[0] == "rep"
            out.extend([p[1]] * p[2])
        else:
            out.append(p)
    assert all(1 <= x <= am.SAT for x in out)
    a = np.asarray(out, dtype=np.uint32)
    a.setflags(write=False)
    return a


def _values(v):
    a = np.asarray(v, dtype=np.uint64)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _doc():
    return json.load(open(os.path.join(sc.GOLDEN, "abund_kat.json")))


@functools.lru_cache(maxsize=None)
def gather_kat():
    """-> tuple of dict(name, q, abund, refs, min_shared, max_rounds, want int32 [n, 4], wunique uint64 [n], wtotal, left)"""
    out = []
    for v in _doc():
        if v["kind"] != "gather":
            continue
        want = np.asarray(v["want"], dtype=np.int32).reshape(len(v["want"]), 4)
        want.setflags(write=False)
        out.append(dict(name=v["name"], q=gc._side(v["q"]), abund=_abund(v["abund"]), refs=tuple(gc._side(r) for r in v["refs"]),
                        min_shared=int(v["min_shared"]), max_rounds=v["max_rounds"], want=want, wunique=_values(v["wunique"]),
                        wtotal=int(v["wtotal"]), left=int(v["left"])))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def merge_kat():
    """-> tuple of dict(name, parts: tuple of (values, abund), max_hash, want_v, want_a)"""
    out = []
    for v in _doc():
        if v["kind"] != "merge":
            continue
        parts = tuple((_values(p["v"]), np.asarray(p["a"], dtype=np.uint32)) for p in v["parts"])
        out.append(dict(name=v["name"], parts=parts, max_hash=am.FULL if v["max_hash"] is None else int(v["max_hash"]), want_v=_values(v["want_v"]),
                        want_a=np.asarray(v["want_a"], dtype=np.uint32)))
    return tuple(out)


def csr(parts):
    """list of (values, abund) -> (values, abund, offsets)"""
    v, off = scm.csr([p[0] for p in parts])
    a = np.concatenate([np.zeros(0, np.uint32)] + [np.asarray(p[1], dtype=np.uint32) for p in parts])
    return v, np.ascontiguousarray(a, dtype=np.uint32), off


def abundances(rng, n, heavy=0.1):
    """n abundances: mostly 1, a tenth between 2 and 500, and one of 2^32 - 1 when there is room"""
    a = np.ones(n, dtype=np.uint32)
    pick = rng.random(n) < heavy
    a[pick] = rng.integers(2, 501, size=int(pick.sum()), dtype=np.uint32)
    if n > 3:
        a[int(rng.integers(0, n))] = am.SAT
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def random_case(nref):
    """gather_cases.random_case(nref) with abundances -> (q, abund, refs, rows, wunique uint64, left)"""
    q, refs, want = gc.random_case(nref)
    a = abundances(np.random.default_rng(2000 + nref), len(q))
    rows, wu, left = am.gather_weighted(q, a, refs)
    assert (rows == want).all()
    return q, a, refs, want, _values(wu), left


@functools.lru_cache(maxsize=None)
def staircase(n):
    q, refs = gc.staircase(n)
    return q, abundances(np.random.default_rng(3000 + n), len(q), heavy=0.5), refs


@functools.lru_cache(maxsize=None)
def list_of(n, seed=0):
    """a query of 2 n + 5 values, a reference that holds n of them, scattered, and one that holds up to 3 others (and is listed
    first): the first pick's hit list has n entries, and from n = 2 on its weight passes 2^32 -> (q, abund, refs)"""
    rng = np.random.default_rng(4000 + n + seed)
    vals = np.sort(gc.foreign(rng, 2 * n + 5, np.zeros(0, np.uint64)))
    idx = rng.permutation(len(vals))
    big = np.sort(vals[idx[:n]])
    few = np.sort(vals[idx[n:n + min(n - 1, 3)]])
    q = _values(vals)
    a = np.array(abundances(rng, len(q), heavy=0.3))
    if n >= 2:                                                # the first and the last hit of the long list weigh 2^32 - 1: a 64-bit sum
        a[np.searchsorted(vals, big[[0, -1]])] = am.SAT
    a.setflags(write=False)
    return q, a, (few, big)


# ---- sequences whose k-mers repeat ----
REPEATS = ((1, 2), (3, 64), (5, 65), (7, 300), (100, 11))


def repeated_unit(L, m, k, seed=0):
    """a unit of L random bases written until it holds L * m windows of k bases (len - k + 1 of them): at most L distinct k-mers"""
    rng = np.random.default_rng(5000 + 13 * L + m + seed)
    unit = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=L)])
    n = L * m + k - 1
    return (unit * (n // L + 1))[:n]


# ---- the bundled sample against the bundled references ----
@functools.lru_cache(maxsize=None)
def z1_query(scaled):
    """the reads of z1.fq.gz as ONE query at k = 16 under the default policy -> (values, abund)"""
    seqs, _ = sc._seqs("z1.fq.gz")
    mh = scm.max_hash(scaled)
    v, a = am.merge([am.sketch(s, [16], sm.DEFAULT, mh) for s in seqs], mh)
    v.setflags(write=False)
    a.setflags(write=False)
    return v, a
