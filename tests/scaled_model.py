"""Scaled (FracMinHash) sketches (rk_sketch_scaled_batch, rk_compare_scaled, `rkmh sketch --scaled`, `rkmh dist --scaled`) in pure
Python and numpy, from the definitions in include/rkmh_amd.h, "SCALED SKETCHES" -- it calls neither the library nor the oracle.

  max_hash        floor((2^64 - 1) / scaled)
  sketch          the ascending distinct window hashes 0 < h <= max_hash of a sequence, pooled over the k-mer sizes
  shared          |A & B| of two sketches;  all_shared: int32 [na, nb] of every pair
  merge           the ascending distinct union of sketches cut at a max_hash;  downsample: one sketch at a larger `scaled`
  distance        (jaccard, distance) from shared, |A|, |B| and k
  dist_line       one line of `rkmh dist --scaled`;  dist_text: all lines of a run, query-major
  csr / rows      list of arrays <-> (values, offsets)
Pinned by tests/golden/scaled_kat.json."""
import math

import numpy as np

import sourmash_model as sm

FULL = (1 << 64) - 1


def max_hash(scaled):
    assert scaled >= 1
    return FULL // scaled


def sketch(seq, ks, pol, mh):
    h = np.asarray(sm.calc_hashes(seq, ks, pol), dtype=np.uint64)
    return np.unique(h[(h != 0) & (h <= np.uint64(mh))])


def shared(a, b):
    return int(np.intersect1d(np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)).size)


def all_shared(A, B=None):
    B = A if B is None else B
    out = np.zeros((len(A), len(B)), dtype=np.int32)
    for i, x in enumerate(A):
        for j, y in enumerate(B):
            out[i, j] = shared(x, y)
    return out


def merge(sketches, mh=FULL):
    v = np.concatenate([np.asarray(s, dtype=np.uint64) for s in sketches]) if len(sketches) else np.zeros(0, dtype=np.uint64)
    return np.unique(v[(v != 0) & (v <= np.uint64(mh))])


def downsample(s, scaled):
    s = np.asarray(s, dtype=np.uint64)
    return s[s <= np.uint64(max_hash(scaled))]


def distance(sh, la, lb, k):
    union = la + lb - sh
    j = sh / union if union else 0.0
    if sh == 0:
        return j, 1.0
    d = -math.log(2.0 * j / (1.0 + j)) / k
    return j, min(1.0, d) if d > 0.0 else 0.0


def dist_line(ref, query, sh, lq, lr, k):
    return "%s\t%s\t%.6g\t%d/%d\t%d/%d\t%d/%d\n" % (ref, query, distance(sh, lq, lr, k)[1], sh, lq + lr - sh, sh, lq, sh, lr)


def dist_text(ref_names, refs, query_names, queries, k, max_dist=None):
    """one line per (query, reference), query by query; max_dist: only the pairs at or below it"""
    out = []
    for qn, q in zip(query_names, queries):
        for rn, r in zip(ref_names, refs):
            sh = shared(q, r)
            if max_dist is not None and distance(sh, len(q), len(r), k)[1] > max_dist:
                continue
            out.append(dist_line(rn, qn, sh, len(q), len(r), k))
    return "".join(out)


def csr(sketches):
    off = np.zeros(len(sketches) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in sketches], dtype=np.uint64)
    v = np.concatenate([np.asarray(s, dtype=np.uint64) for s in sketches]) if len(sketches) else np.zeros(0, dtype=np.uint64)
    return np.ascontiguousarray(v, dtype=np.uint64), off


def rows(values, offsets):
    return [np.asarray(values[int(offsets[i]):int(offsets[i + 1])], dtype=np.uint64) for i in range(len(offsets) - 1)]
