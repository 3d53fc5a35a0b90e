"""Search (rk_search_scaled, `rkmh manysearch`) in pure Python and numpy, from the definitions in include/rkmh_amd.h, "SEARCH" -- it
calls neither the library nor the oracle.

  search          the hits of query sketches against reference sketches: np.intersect1d per pair, threshold, sort -> int32 [n, 3]
  search_by_rows  the same hits from one np.isin per query over the concatenated references (for collections of many thousands of
                  rows; shown equal to search() by tests/test_search_cpu.py)
  min_count       the smallest t with t / length >= x in Python doubles: the count --min-containment asks of a query
  search_text     the lines of `rkmh manysearch`
Pinned by tests/golden/search_kat.json."""
import numpy as np

import scaled_model as scm


def thresholds(nq, min_shared=1, q_min=None):
    assert min_shared >= 1 and (q_min is None or (len(q_min) == nq and all(int(t) >= 1 for t in q_min)))
    return [min_shared if q_min is None else max(min_shared, int(q_min[i])) for i in range(nq)]


def _rows(hits):
    return np.asarray(hits, dtype=np.int32).reshape(len(hits), 3)


def search(refs, queries, min_shared=1, q_min=None):
    thr = thresholds(len(queries), min_shared, q_min)
    hits = []
    for i, q in enumerate(queries):
        for j, r in enumerate(refs):
            n = int(np.intersect1d(np.asarray(q, dtype=np.uint64), np.asarray(r, dtype=np.uint64), assume_unique=True).size)
            if n >= thr[i]:
                hits.append((i, j, n))
    return _rows(sorted(hits))


def search_by_rows(refs, queries, min_shared=1, q_min=None):
    thr = thresholds(len(queries), min_shared, q_min)
    values, off = scm.csr(refs)
    row = np.repeat(np.arange(len(refs)), np.diff(off.astype(np.int64)))
    hits = []
    for i, q in enumerate(queries):
        n = np.bincount(row[np.isin(values, np.asarray(q, dtype=np.uint64))], minlength=len(refs))
        for j in np.flatnonzero(n >= thr[i]):
            hits.append((i, int(j), int(n[j])))
    return _rows(hits)


def min_count(x, length):
    assert 0.0 <= x <= 1.0 and length >= 0
    if length == 0:
        return 0
    t = 0
    while float(t) / float(length) < x:
        t += 1
    return t


def search_text(ref_names, refs, query_names, queries, k, min_shared=1, min_containment=0.0):
    q_min = [max(1, min_count(min_containment, len(q))) for q in queries]
    return "".join(scm.dist_line(ref_names[j], query_names[i], n, len(queries[i]), len(refs[j]), k)
                   for i, j, n in search(refs, queries, min_shared, q_min).tolist())
