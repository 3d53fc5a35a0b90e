"""Inputs the multigather tests share (tests/test_multigather_cpu.py, tests/test_multigather_gpu.py): batches of queries over the
collections of gather_cases, search_cases and abund_cases, and the expected answer query by query -- from tests/gather_model.py, or,
for the collections of thousands of references, from rk_gather_scaled_host (itself held to the model by tests/test_gather_cpu.py).
Computed once per process and left unchanged."""
import functools

import numpy as np

import abund_cases as ac
import abund_model as am
import gather_cases as gc
import gather_model as gm
import scaled_cases as sc
import scaled_model as scm
import search_cases as sec

EMPTY = np.zeros(0, dtype=np.uint64)
EMPTY.setflags(write=False)
STAIRS = (0, 1, 15, 16, 17, 33)          # picks of the staircase queries of one batch: around RK_GATHER_BATCH = 16 and two groups of it
MAX_ROUNDS = (1, 16, 17, None)


def _ro(a):
    a = np.asarray(a, dtype=np.uint64)
    a.setflags(write=False)
    return a


def answer(refs, queries, min_shared=1, max_rounds=None, abunds=None, host=False):
    """-> (rows int32 [n, 4], row_offsets uint64 [nq + 1], wunique uint64 [n] or None): gather query by query, laid end to end.
    host: rk_gather_scaled_host / rk_gather_scaled_abund_host instead of the Python model"""
    rows, off, wu = [], [0], []
    if host:
        from rkmh_amd import api
        rv, ro = scm.csr(refs)
    for i, q in enumerate(queries):
        if host and abunds is not None:
            r, w = api.gather_scaled_abund_host(q, abunds[i], rv, ro, min_shared=min_shared, max_rounds=max_rounds)
            wu.extend(int(x) for x in w)
        elif host:
            r = api.gather_scaled_host(q, rv, ro, min_shared=min_shared, max_rounds=max_rounds)
        elif abunds is not None:
            r, w, _ = am.gather_weighted(q, abunds[i], refs, min_shared, max_rounds)
            wu.extend(w)
        else:
            r = gm.gather(q, refs, min_shared, max_rounds)
        rows.append(np.asarray(r, dtype=np.int32).reshape(len(r), 4))
        off.append(off[-1] + len(r))
    rows = np.concatenate(rows) if rows else np.zeros((0, 4), np.int32)
    return rows, np.asarray(off, dtype=np.uint64), (np.asarray(wu, dtype=np.uint64) if abunds is not None else None)


def cut(ans, max_rounds):
    """the answer at a smaller max_rounds: the first max_rounds rows of every query (a greedy run cut short is its own beginning;
    shown against the model itself by tests/test_multigather_cpu.py)"""
    rows, off, wu = ans
    if max_rounds is None:
        return ans
    keep = np.concatenate([np.arange(int(off[i]), min(int(off[i + 1]), int(off[i]) + max_rounds)) for i in range(len(off) - 1)] + [np.zeros(0, np.int64)]).astype(np.int64)
    n = np.minimum(np.diff(off.astype(np.int64)), max_rounds)
    return rows[keep], np.concatenate([[0], np.cumsum(n)]).astype(np.uint64), (None if wu is None else wu[keep])


def blocks(ans):
    """the answer as one (rows, wunique) pair per query"""
    rows, off, wu = ans
    return [(rows[int(off[i]):int(off[i + 1])], None if wu is None else wu[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def median_count(ans):
    """a min_shared with rows on both sides of it: the median of the unique counts at min_shared = 1 (at least 2)"""
    return max(2, int(np.median(ans[0][:, 1]))) if len(ans[0]) else 2


@functools.lru_cache(maxsize=None)
def kat_batches():
    """every vector of gather_kat.json as a batch of [Q] and of [Q, empty, Q] -> tuple of dict(name, refs, queries, min_shared, max_rounds, want)"""
    out = []
    for v in gc.kat():
        for queries in ((v["q"],), (v["q"], EMPTY, v["q"])):
            z = np.zeros((0, 4), np.int32)
            rows = np.concatenate([v["want"]] + ([z, v["want"]] if len(queries) == 3 else []))
            off = np.cumsum([0] + [len(v["want"]) if len(q) else 0 for q in queries]).astype(np.uint64)
            out.append(dict(name="%s x %d" % (v["name"], len(queries)), refs=v["refs"], queries=queries, min_shared=v["min_shared"], max_rounds=v["max_rounds"],
                            want=(rows, off, None)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def random_batch(nref):
    """gather_cases.random_case(nref) as a batch: its query; an empty one; one of foreign values alone (no candidate); the union of two
    other references plus foreign values; the first query again; every second value of it -> dict(refs, queries, abunds)"""
    q, refs, _ = gc.random_case(nref)
    rng = np.random.default_rng(7000 + nref)
    known = np.unique(np.concatenate(list(refs) + [q]))
    two = gc.query_of(rng, [refs[i % nref] for i in (1, 2)], known)
    queries = (q, EMPTY, _ro(np.sort(gc.foreign(rng, 100, known))), two, q, _ro(q[::2]))
    abunds = tuple(ac.abundances(np.random.default_rng(7100 + nref + i), len(x)) for i, x in enumerate(queries))
    return dict(refs=refs, queries=queries, abunds=abunds)


@functools.lru_cache(maxsize=None)
def staircases():
    """the staircases of STAIRS side by side: one collection that holds the references of all of them (they share nothing), one query
    per staircase -- it finishes after that many picks -- and an empty query -> dict(refs, queries, picks)"""
    refs, queries = [], []
    for n in STAIRS:
        q, r = gc.staircase(n)
        refs.extend(r)
        queries.append(q)
    allv = np.concatenate(refs)
    assert len(np.unique(allv)) == len(allv), "two staircases share a value"
    queries.append(EMPTY)
    return dict(refs=tuple(refs), queries=tuple(queries), picks=STAIRS + (0,))


@functools.lru_cache(maxsize=None)
def ties():
    """-> dict(refs, queries, later): references 0 and 1 identical, 2, 3 and 4 identical (the lowest index wins); 5, 6, 7: counts 6, 5, 4
    against the last query, and 3, 3 once reference 5 is picked -- equal counts that arise in the second round only"""
    a = np.arange(101, 111, dtype=np.uint64)
    b = np.arange(201, 208, dtype=np.uint64)
    r5 = np.array([1, 2, 3, 4, 5, 6], dtype=np.uint64)
    r6 = np.array([5, 6, 11, 12, 13], dtype=np.uint64)
    r7 = np.array([1, 21, 22, 23], dtype=np.uint64)
    refs = tuple(_ro(x) for x in (a, a, b, b, b, r5, r6, r7))
    later = _ro(np.unique(np.concatenate([r5, r6, r7, [900, 901]]).astype(np.uint64)))
    queries = (_ro(np.concatenate([a, [500, 501]]).astype(np.uint64)), _ro(b), later, _ro(np.unique(np.concatenate([a, b, later]))))
    return dict(refs=refs, queries=queries, later=2)


@functools.lru_cache(maxsize=None)
def block_edges(nref):
    """nref references of 1 to 3 values, as search_cases.block_edges lays them out: every row holds EVERY (a posting list of nref
    entries that spans every block of the search); the first and the last reference of every block hold two values of their own
    besides; the other rows hold up to two values of a pool of 300.  Queries: all edge values, EVERY and 40 pool values (every edge
    reference is picked); EVERY alone; the edge values alone -> dict(refs, queries, edge)"""
    rng = np.random.default_rng(8000 + nref)
    every = np.uint64(1 << 40)
    pl = np.unique(rng.integers(1 << 41, 1 << 63, size=300, dtype=np.uint64))
    edge = sorted(set(x for b in range(0, nref, sec.REF_BLOCK) for x in (b, min(b + sec.REF_BLOCK - 1, nref - 1))))
    extra = rng.integers(0, 3, size=nref)
    refs = [np.unique(np.concatenate([[every], rng.choice(pl, size=int(extra[r]), replace=False)]).astype(np.uint64)) for r in range(nref)]
    own = []
    for j, r in enumerate(edge):
        mine = np.array([10 + 2 * j, 11 + 2 * j], dtype=np.uint64)
        own.append(mine)
        refs[r] = np.unique(np.concatenate([[every], mine]).astype(np.uint64))
    own = np.concatenate(own)
    some = np.sort(rng.choice(pl, size=40, replace=False))
    queries = (np.unique(np.concatenate([own, [every], some]).astype(np.uint64)), np.array([every], dtype=np.uint64), np.unique(own))
    assert all(1 <= len(r) <= 3 for r in refs)
    return dict(refs=tuple(_ro(r) for r in refs), queries=tuple(_ro(q) for q in queries), edge=tuple(edge))


@functools.lru_cache(maxsize=None)
def many_queries():
    """65 queries of 0 ... 4 097 values (the lengths of scaled_cases.LENGTHS, over and over) against the 65 references of
    gather_cases.random_case(65): values of the references' pool and as many foreign ones -> dict(refs, queries)"""
    _, refs, _ = gc.random_case(65)
    rng = np.random.default_rng(9000)
    pl = np.unique(np.concatenate(refs))
    queries = []
    for i in range(65):
        m = sc.LENGTHS[i % len(sc.LENGTHS)]
        mine = rng.choice(pl, size=min(m - m // 2, len(pl)), replace=False)
        queries.append(_ro(np.unique(np.concatenate([mine, gc.foreign(rng, m // 2, pl)]).astype(np.uint64))))
    assert sorted(set(len(q) for q in queries))[0] == 0 and max(len(q) for q in queries) == 4097
    return dict(refs=refs, queries=tuple(queries))
