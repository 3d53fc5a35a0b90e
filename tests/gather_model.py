"""Gather (rk_gather_scaled, rk_gather_scaled_device, rk_gather_scaled_host, `rkmh gather`) in pure Python and numpy, from the
definitions in include/rkmh_amd.h, "GATHER" -- it calls neither the library nor the oracle.

  gather          the rows (ref, unique, total, remaining) of the greedy decomposition of one query into reference sets
  gather_line     one line of `rkmh gather`;  gather_text: all lines of a run, query by query
Pinned by tests/golden/gather_kat.json."""
import numpy as np


def gather(q, refs, min_shared=1, max_rounds=None):
    """q: ascending distinct non-zero uint64; refs: list of such arrays -> int32 [n, 4]"""
    q = np.asarray(q, dtype=np.uint64)
    max_rounds = len(refs) if max_rounds is None else max_rounds
    assert min_shared >= 1 and max_rounds >= 1
    hits = []                                                # per reference: the indices of the query values it holds
    for r in refs:
        r = np.asarray(r, dtype=np.uint64)
        at = np.searchsorted(q, r)
        ok = at < len(q)
        ok[ok] = q[at[ok]] == r[ok]
        hits.append(at[ok])
    alive = np.ones(len(q), dtype=bool)
    rows = []
    while len(rows) < max_rounds:
        count = [int(alive[h].sum()) for h in hits]
        best = int(np.argmax(count)) if count else 0          # the first of the largest: the lowest reference index
        if not count or count[best] < min_shared:
            break
        alive[hits[best]] = False
        rows.append((best, count[best], len(hits[best]), int(alive.sum())))
    return np.asarray(rows, dtype=np.int32).reshape(len(rows), 4)


def gather_line(query, rank, ref, unique, total, lq, lr, remaining):
    return "%s\t%d\t%s\t%d/%d\t%d/%d\t%d/%d\t%d\n" % (query, rank, ref, unique, lq, total, lq, total, lr, remaining)


def gather_text(query_names, queries, ref_names, refs, min_shared=1, max_rounds=None):
    out = []
    for qn, q in zip(query_names, queries):
        for t, (r, u, tot, rem) in enumerate(gather(q, refs, min_shared, max_rounds).tolist()):
            out.append(gather_line(qn, t + 1, ref_names[r], u, tot, len(q), len(refs[r]), rem))
    return "".join(out)
