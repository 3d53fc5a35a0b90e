"""Abundance sketches and weighted gather (rk_sketch_scaled_abund_batch, rk_merge_scaled_abund, rk_gather_scaled_abund and its _device
and _host forms, `rkmh sketch --scaled <n> --abund`, `rkmh gather --abund`) in pure Python and numpy, from the definitions in
include/rkmh_amd.h, "ABUNDANCE" -- it calls neither the library nor the oracle.

  sketch           (values, abund): the scaled sketch of a sequence and the number of windows behind every value
  merge            the union of (values, abund) pairs cut at a max_hash, abundances summed and saturating at 2^32 - 1
  gather_weighted  gather_model.gather's rows and, per row, the summed abundances of the query values the pick removes
  gather_line      one line of `rkmh gather --abund`;  gather_text: all lines of a run, query by query
Pinned by tests/golden/abund_kat.json."""
import numpy as np

import gather_model as gm
import sourmash_model as sm

FULL = (1 << 64) - 1
SAT = (1 << 32) - 1


def sketch(seq, ks, pol, mh):
    h = np.asarray(sm.calc_hashes(seq, ks, pol), dtype=np.uint64)
    v, a = np.unique(h[(h != 0) & (h <= np.uint64(mh))], return_counts=True)
    return v.astype(np.uint64), np.minimum(a, SAT).astype(np.uint32)


def merge(parts, mh=FULL):
    """parts: list of (values, abund)"""
    tot = {}
    for v, a in parts:
        assert len(v) == len(a)
        for x, n in zip(np.asarray(v, dtype=np.uint64).tolist(), np.asarray(a, dtype=np.uint32).tolist()):
            if 0 < x <= mh:
                tot[x] = min(tot.get(x, 0) + n, SAT)
    keys = sorted(tot)
    return np.asarray(keys, dtype=np.uint64), np.asarray([tot[x] for x in keys], dtype=np.uint32)


def downsample(v, a, mh):
    keep = np.asarray(v, dtype=np.uint64) <= np.uint64(mh)
    return np.asarray(v, dtype=np.uint64)[keep], np.asarray(a, dtype=np.uint32)[keep]


def gather_weighted(q, abund, refs, min_shared=1, max_rounds=None):
    """-> (rows int32 [n, 4], wunique: list of n Python ints, left: the abundances of the values still alive at the end, summed)"""
    q = np.asarray(q, dtype=np.uint64)
    abund = [int(x) for x in np.asarray(abund, dtype=np.uint32).tolist()]
    assert len(abund) == len(q)
    rows = gm.gather(q, refs, min_shared, max_rounds)
    alive = [True] * len(q)
    at = {int(x): i for i, x in enumerate(q.tolist())}
    wunique = []
    for r in rows[:, 0].tolist():
        w = 0
        for x in np.asarray(refs[r], dtype=np.uint64).tolist():
            i = at.get(int(x))
            if i is not None and alive[i]:
                w += abund[i]
                alive[i] = False
        wunique.append(w)
    return rows, wunique, sum(a for a, al in zip(abund, alive) if al)


def gather_line(query, rank, ref, unique, total, lq, lr, remaining, wunique, wtotal):
    return gm.gather_line(query, rank, ref, unique, total, lq, lr, remaining)[:-1] + "\t%d/%d\t%.6g\n" % (wunique, wtotal, wunique / unique)


def gather_text(query_names, queries, ref_names, refs, min_shared=1, max_rounds=None):
    """queries: list of (values, abund)"""
    out = []
    for qn, (q, a) in zip(query_names, queries):
        rows, wu, _ = gather_weighted(q, a, refs, min_shared, max_rounds)
        wtotal = int(np.asarray(a, dtype=np.uint64).sum())
        for t, (r, u, tot, rem) in enumerate(rows.tolist()):
            out.append(gather_line(qn, t + 1, ref_names[r], u, tot, len(q), len(refs[r]), rem, wu[t], wtotal))
    return "".join(out)
