"""Shared inputs of the bottom-sample tests (include/rkmh_amd.h "BOTTOM SAMPLES"): reads as bytes from seeded numpy generators (most
are tests/sample_cases.py's), and the synthetic (values, counts) sets the cut is tested on, each with the place its cut was built to
fall at.  What the cases hold -- enough cuts, a candidate that qualifies late, a count that alone fills the sketch, the cut places --
is shown on the model by tests/test_bottom_cpu.py; tests/test_gpu_bottom.py relies on it."""
import functools

import numpy as np

import sample_cases as sc

KEEP_BLK = 1024               # rk_sets.hpp: entries per workgroup of k_cut_weights / k_cut_find
MAX_SKETCH = 16384            # RK_MAX_SKETCH
SAT = (1 << 32) - 1
K = sc.K
POLICIES = sc.POLICIES        # name -> the hashing side of the preset
DISTINCT = {"default": False, "mash": False, "sourmash": True}   # the preset's dedup rule
FOLD_S = 64                   # the sketch size of the fold test: small, so that the 43 feeds of 7 reads bring many cuts
FOLD_BATCH = sc.FOLD_BATCH
FOLD_CAPS = sc.FOLD_CAPS


def reads300():
    """sample_cases.reads300: every tenth read is a copy of an earlier one -- at min_copies = 2 the values of such a pair qualify only
    with the batch that brings the copy"""
    return sc.reads300()


@functools.lru_cache(maxsize=None)
def twice():
    """120 reads and the same 120 in another order: every value has at least two copies, the second in a later feed"""
    reads = list(sc.reads300()[:120])
    rng = np.random.default_rng(31)
    return tuple(reads), tuple(reads[i] for i in rng.permutation(len(reads)))


@functools.lru_cache(maxsize=None)
def many_short(n=5000, length=24):
    """more reads in one batch than a bottom sample takes before its first cut (4 096): the batch goes in as sub-batches"""
    rng = np.random.default_rng(32)
    return tuple(sc.rand_read(rng, length) for _ in range(n))


# ---- synthetic sets for the cut.  values: ascending, distinct, non-zero.
def values(n):
    return np.arange(1, n + 1, dtype=np.uint64) * np.uint64(7) + np.uint64(3)


def crossing_at(P, n, distinct, m, seed):
    """(counts, S): a set of n entries whose cut falls at entry P - 1 (cut_len P).  About half of the entries in front of it do not
    qualify (m > 1) or weigh what their count says (multiset)."""
    rng = np.random.default_rng(seed)
    c = rng.integers(m, m + 3, size=n).astype(np.uint32)
    if m > 1:
        c[rng.random(n) < 0.5] = m - 1
    c[P - 1] = m + 1
    before = c[:P - 1].astype(np.int64)
    w = np.where(before < m, 0, 1 if distinct else before)
    S = int(w.sum()) + (1 if distinct else int(rng.integers(1, m + 2)))   # reached inside entry P - 1's own weight
    return c, S


CUT_PLACES = (63, 64, 65, 255, 256, 257, KEEP_BLK - 1, KEEP_BLK, KEEP_BLK + 1)


@functools.lru_cache(maxsize=None)
def cut_cases():
    """name -> (counts, S, m, distinct, the cut_len it was built for; 0: no cut).  The values are values(len(counts))."""
    out = {}
    ones = lambda n: np.ones(n, dtype=np.uint32)
    out["n=1"] = (ones(1), 1, 1, True, 1)
    out["n=1, S=2: no cut"] = (ones(1), 2, 1, False, 0)
    out["S=1"] = (ones(10), 1, 1, False, 1)
    out["S=1, m=2"] = (np.array([1, 1, 2, 1, 5], np.uint32), 1, 2, True, 3)
    for i, P in enumerate(CUT_PLACES):
        for distinct in (True, False):
            for m in (1, 2):
                c, S = crossing_at(P, P + 100, distinct, m, 100 + i)
                out["place %d %s m=%d" % (P, "distinct" if distinct else "multiset", m)] = (c, S, m, distinct, P)
    c, S = crossing_at(700, 700, True, 2, 7)
    out["the very last entry"] = (c, S, 2, True, 700)
    c, S = crossing_at(2 * KEEP_BLK, 2 * KEEP_BLK, False, 1, 8)
    out["the very last entry, multiset, at a block end"] = (c, S, 1, False, 2 * KEEP_BLK)
    out["stops at S - 1"] = (ones(1500), 1501, 1, True, 0)
    out["stops at S - 1, multiset"] = (np.full(1500, 2, np.uint32), 3001, 1, False, 0)
    out["nothing qualifies"] = (ones(3000), 1, 2, True, 0)
    c = np.concatenate([np.full(10, 2, np.uint32), ones(3000), np.full(50, 2, np.uint32)])
    out["3 000 unqualified entries in front of the crossing"] = (c, 12, 2, True, 3012)
    out["one count >= S"] = (np.array([1, 1, 50000, 1], np.uint32), 100, 1, False, 3)
    out["exactly S at a block's last entry"] = (np.full(2 * KEEP_BLK, 2, np.uint32), 2 * KEEP_BLK, 1, False, KEEP_BLK)
    sat = np.array([5, SAT, 7, SAT], np.uint32)
    out["saturated, distinct, m = 2^32 - 1"] = (sat, 2, SAT, True, 4)
    out["saturated, multiset, S = 16 384"] = (sat, MAX_SKETCH, SAT, False, 2)
    return out


@functools.lru_cache(maxsize=None)
def wide_case():
    """n = 1 024 * KEEP_BLK + 5: k_scan_blocks takes two block sums per thread; 16 380 qualifying entries lie 64 apart, the last five
    entries qualify too, and at S = 16 384 (distinct, m = 2) the crossing is the fourth of those five: in the last block"""
    n = 1024 * KEEP_BLK + 5
    c = np.ones(n, dtype=np.uint32)
    c[np.arange(16380) * 64] = 2
    c[n - 5:] = 3
    return c, MAX_SKETCH, 2, True, n - 1
