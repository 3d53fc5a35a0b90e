"""Sketch comparison (rk_compare_sketches, `rkmh dist`) in pure Python and numpy, from the statement of the four counts in
include/rkmh_amd.h -- it calls neither the library nor the oracle.  A sketch is a row of S uint64, ascending, the first `len` of them
its values, zeros behind; a zero is never a value.  D(x) = np.unique of the values.

  values          the values of a row: x[:len] without zeros
  pair_counts     (shared, shared_distinct, common, denom) of one pair
  all_pairs       int32 [na, nb, 4] of every pair of two sets of rows, lengths clamped to [0, S] as the device clamps them
  mash_distance   (jaccard, distance) from common, denom and k
  distance_text   the distance as `rkmh dist` prints it
Pinned by tests/golden/pairs_kat.json."""
import math

import numpy as np

import sourmash_model as sm


def values(row, n=None):
    x = np.asarray(row, dtype=np.uint64)
    if n is not None:
        x = x[:n]
    return x[x != 0]


def pair_counts(a, b, S):
    """a, b: the VALUES of two sketches (values()).  shared: the two-pointer merge `stream` counts with (both sides advance on
    equality: the sum over values of min of the multiplicities); shared_distinct: |D(a) & D(b)|; U: the S smallest of D(a) | D(b);
    common: |U & D(a) & D(b)|; denom: |U|."""
    a, b = values(a), values(b)
    shared = sm.intersection_size(a.tolist(), b.tolist())
    da, db = np.unique(a), np.unique(b)
    both = np.intersect1d(da, db, assume_unique=True)
    U = np.union1d(da, db)[:S]
    common = np.intersect1d(U, both, assume_unique=True).size
    return shared, int(both.size), int(common), int(U.size)


def all_pairs(A, alens, B=None, blens=None, S=None):
    A = np.asarray(A, dtype=np.uint64)
    if B is None:
        B, blens = A, alens
    B = np.asarray(B, dtype=np.uint64)
    if S is None:
        S = A.shape[1]
    va = [values(A[i], min(max(int(alens[i]), 0), S)) for i in range(len(alens))]
    vb = [values(B[j], min(max(int(blens[j]), 0), S)) for j in range(len(blens))]
    out = np.zeros((len(va), len(vb), 4), dtype=np.int32)
    for i, x in enumerate(va):
        for j, y in enumerate(vb):
            out[i, j] = pair_counts(x, y, S)
    return out


def mash_distance(common, denom, k):
    j = common / denom if denom else 0.0
    if common == 0:
        return j, 1.0
    d = -math.log(2.0 * j / (1.0 + j)) / k
    return j, min(1.0, d) if d > 0.0 else 0.0


def distance_text(d):
    return "%.6g" % d


def rows(sketches, S):
    """list of value lists -> (uint64 [n, S] zero padded, int32 lens)"""
    sk = np.zeros((len(sketches), S), dtype=np.uint64)
    ln = np.zeros(len(sketches), dtype=np.int32)
    for i, v in enumerate(sketches):
        assert len(v) <= S
        sk[i, :len(v)] = np.asarray(v, dtype=np.uint64)
        ln[i] = len(v)
    return sk, ln
