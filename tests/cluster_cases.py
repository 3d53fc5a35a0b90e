"""Inputs the cluster tests share (tests/test_cluster_cpu.py, tests/test_gpu_cluster.py): the hand-checked vectors, graphs given as
hits (paths, the zigzag path, stars, a complete graph), and collections of sketches in families for the self-search -- computed once
per process and left unchanged.  What each case claims about itself is shown by tests/test_cluster_cpu.py."""
import functools
import json
import os

import numpy as np

import cluster_model as clm
import scaled_cases as sc
import search_model as sem

REF_BLOCK = 8192   # include/rkmh_amd.h: RK_SEARCH_REF_BLOCK
PATH_N = 4097      # more nodes than one workgroup's lanes, no multiple of anything


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _case(name, lens, hits, measure=clm.JACCARD, ppm=0, **more):
    hits = np.asarray(hits, dtype=np.int32).reshape(-1, 3)
    lens = np.asarray(lens, dtype=np.uint64)
    _ro(hits, lens)
    return dict(name=name, lens=lens, hits=hits, measure=measure, ppm=ppm, **more)


@functools.lru_cache(maxsize=None)
def kat():
    """-> tuple of dict(name, lens, hits, measure, ppm, want)"""
    doc = json.load(open(os.path.join(sc.GOLDEN, "cluster_kat.json")))
    return tuple(_case(v["name"], v["lens"], v["hits"], int(v["measure"]), int(v["ppm"]), want=_ro(np.asarray(v["want"], dtype=np.int32))) for v in doc)


def _path_hits(ids, shared):
    """one hit per edge of the path that visits `ids` in order, the direction alternating"""
    a, b = np.asarray(ids[:-1]), np.asarray(ids[1:])
    flip = (np.arange(len(a)) % 2).astype(bool)
    return np.stack([np.where(flip, b, a), np.where(flip, a, b), np.full(len(a), shared)], axis=1)


def zigzag_ids(m):
    """the ids along a path of m positions: odd positions carry the low ids 0 .. m // 2 - 1 in order, even positions the high ones"""
    low = m // 2
    return np.array([(p - 1) // 2 if p % 2 else low + p // 2 for p in range(m)], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def graphs():
    """-> tuple of cases given as hits; every sketch has 8 values and every link shares 4 (jaccard 4 / 12) unless the case says otherwise"""
    rng = np.random.default_rng(77)
    out = [_case("n = 1", [5], []), _case("no hits", [3, 4, 5, 6, 7], []),
           _case("self hits only", [3, 4, 5, 6], [[i, i, 3 + i] for i in range(4)])]
    n = PATH_N
    out.append(_case("path in index order", [8] * n, _path_hits(np.arange(n), 4), ppm=300000))
    perm = rng.permutation(n)
    out.append(_case("path under a random permutation", [8] * n, _path_hits(perm, 4), ppm=300000, ids=_ro(perm)))
    zz = zigzag_ids(n)
    out.append(_case("zigzag path", [8] * n, _path_hits(zz, 4), ppm=300000, ids=_ro(zz)))
    m = 300
    out.append(_case("star whose centre is the highest id", [8] * m, [[m - 1, i, 4] if i % 2 else [i, m - 1, 4] for i in range(m - 1)], ppm=300000))
    # two stars of identical sets (100 values; node 15 holds 200), centres 0 and 10, and the bridge 5 -- 15 with 60 shared:
    # jaccard 60 / 240 is under 0.4, max containment 60 / 100 is over it; the link 10 -- 15 passes both (100 / 200, 100 / 100)
    lens = [100] * 20
    lens[15] = 200
    star = [[0, i, 100] for i in range(1, 10)] + [[i, 10, 100] for i in range(11, 20)] + [[5, 15, 60]]
    out.append(_case("two stars and a bridge, jaccard", lens, star, clm.JACCARD, 400000))
    out.append(_case("two stars and a bridge, max containment", lens, star, clm.MAX_CONTAINMENT, 400000))
    # a complete graph on 1 500 nodes, both directions of every pair: 2 248 500 hits, more than one launch's lanes; 500 singletons after it
    k, n2 = 1500, 2000
    i, j = np.nonzero(~np.eye(k, dtype=bool))
    out.append(_case("complete graph and singletons", [8] * n2, np.stack([i, j, np.full(len(i), 4)], axis=1), ppm=300000))
    # hits that name -1, n and 2^31 - 1, on either side, mixed into a random graph's
    n3 = 500
    good = np.stack([rng.integers(0, n3, 400), rng.integers(0, n3, 400), np.full(400, 4)], axis=1)
    bad = np.stack([rng.choice([-1, n3, (1 << 31) - 1], 300), rng.integers(0, n3, 300), np.full(300, 8)], axis=1)
    bad[::2] = bad[::2][:, [1, 0, 2]]
    mixed = np.concatenate([good, bad])[rng.permutation(700)]
    out.append(_case("bad indices mixed in", [8] * n3, mixed, ppm=300000, good=_ro(good)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def clamped():
    """offsets that overshoot nvalues: rows of 10, 10, 10, 10 values with 25 behind the pointer are rows of 10, 10, 5, 0.  At 450000
    the hit (1, 2, 5) links only with the clamped length (5 / 10, not 5 / 15), (2, 3, 1) in neither reading (1 / 4, 1 / 19)."""
    c = _case("clamped lengths", [10, 10, 5, 0], [[0, 1, 8], [1, 2, 5], [2, 3, 1]], ppm=450000, nvalues=25)
    c["offsets"] = _ro(np.array([0, 10, 20, 30, 40], dtype=np.uint64))
    c["lens_as_given"] = _ro(np.array([10, 10, 10, 10], dtype=np.uint64))
    return c


@functools.lru_cache(maxsize=None)
def want(name):
    """the labels of a graph case: the numpy model's (shown equal to the plain-Python one and to the vectors by tests/test_cluster_cpu.py)"""
    c = by_name(name)
    return _ro(clm.propagate(c["hits"], c["lens"], c["measure"], c["ppm"]))


def by_name(name):
    for c in kat() + graphs() + (clamped(),):
        if c["name"] == name:
            return c
    raise KeyError(name)


# ---- collections for the self-search ----
THRESHOLDS = (0, 200000, 800000, 1000000)
NFAMILIES, NSKETCHES = 40, 1100


@functools.lru_cache(maxsize=None)
def families():
    """-> dict(sketches, family, hits): 1 100 sketches in 40 families.  A family has a base of 60 to 130 pool values; a member keeps
    each with a probability of its own between 0.3 and 1 and adds up to 6 values of its own; every seventh member is a pure subset of
    the base, every eleventh the whole base (so identical sets and subsets exist), and every family's base holds one value of the next
    family's (so at threshold 0 families chain).  Five sketches are empty.  hits: search_model's, every sketch against every sketch."""
    rng = np.random.default_rng(4040)
    pl = sc.pool(rng, 40000)
    pl = pl[rng.permutation(len(pl))]
    bases, at = [], 0
    for f in range(NFAMILIES):
        m = int(rng.integers(60, 131))
        bases.append(pl[at:at + m])
        at += m
    for f in range(NFAMILIES - 1):
        bases[f] = np.concatenate([bases[f], bases[f + 1][:1]])
    fam = rng.integers(0, NFAMILIES, NSKETCHES)
    sketches = []
    for i in range(NSKETCHES):
        b = bases[int(fam[i])]
        if i % 11 == 0:
            s = b
        else:
            s = b[rng.random(len(b)) < rng.uniform(0.3, 1.0)]
            if i % 7:
                own = int(rng.integers(0, 7))
                s = np.concatenate([s, pl[at:at + own]])
                at += own
        if i % 223 == 5:
            s = s[:0]
        sketches.append(_ro(np.unique(s.astype(np.uint64))))
    hits = sem.search_by_rows(sketches, sketches)
    return dict(sketches=tuple(sketches), family=_ro(fam), hits=_ro(hits), lens=_ro(np.array([len(s) for s in sketches], dtype=np.uint64)))


@functools.lru_cache(maxsize=None)
def families_want(measure, ppm, min_shared=1):
    f = families()
    h = f["hits"]
    return _ro(clm.propagate(h[h[:, 2] >= min_shared], f["lens"], measure, ppm))


@functools.lru_cache(maxsize=None)
def block_edge():
    """-> dict(sketches, hits, want): RK_SEARCH_REF_BLOCK + 1 sketches, so the last one is alone in the second reference block.  Every
    sketch holds EVERY; sketches 0, REF_BLOCK - 1 and REF_BLOCK (the edges of the blocks) hold two edge values and nothing else; sketch
    r of the others holds the value of its group r % 500 and one value of its own.  hits and want: at min_shared = 2, threshold 0."""
    n = REF_BLOCK + 1
    every, e1, e2 = 1 << 40, 5, (1 << 64) - 2
    edge = (0, REF_BLOCK - 1, REF_BLOCK)
    sk = [np.array(sorted([every, e1, e2] if r in edge else [every, 1000 + r % 500, (1 << 41) + r]), dtype=np.uint64) for r in range(n)]
    for s in sk:
        s.setflags(write=False)
    hits = sem.search_by_rows(sk, sk, 2)
    lens = np.full(n, 3, dtype=np.uint64)
    return dict(sketches=tuple(sk), hits=_ro(hits), lens=_ro(lens), edge=edge, want=_ro(clm.propagate(hits, lens, clm.JACCARD, 0)))
