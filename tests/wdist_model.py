"""Weighted comparison of abundance sketches (rk_compare_scaled_abund and its _device and _host forms, rk_abund_row_sums*,
rk_angular_similarity, `rkmh dist --abund`) in pure Python and numpy with Python integers, from the definitions in include/rkmh_amd.h,
"WEIGHTED COMPARISON" -- it calls neither the library nor the oracle.

  pair            (shared, dot, wa_in, wb_in) of two (values, abund) sketches; dot saturates at 2^64 - 1
  all_pairs       uint64 [na, nb, 4] of every pair
  row_sums        (sum, sumsq) of one sketch's abundances; sumsq saturates at 2^64 - 1;  all_row_sums: uint64 [n, 2]
  similarity      (cosine, angular) from dot and the two sumsq
  dist_line       one line of `rkmh dist --abund`;  dist_text: all lines of a run, query-major
  mirror          a pair's four fields with the sides swapped
Pinned by tests/golden/wdist_kat.json."""
import math

import numpy as np

import scaled_model as scm

U64 = (1 << 64) - 1
SAT = (1 << 32) - 1


def _ints(x):
    return [int(t) for t in np.asarray(x).tolist()]


def _table(a):
    """(values, abund) -> {value: abundance}"""
    t = dict(zip(_ints(a[0]), _ints(a[1])))
    assert len(t) == len(a[0]) == len(a[1]) and 0 not in t and all(1 <= w <= SAT for w in t.values())
    return t


def _pair(wa, wb):
    few, many = (wa, wb) if len(wa) <= len(wb) else (wb, wa)
    both = [x for x in few if x in many]
    return len(both), min(sum(wa[x] * wb[x] for x in both), U64), sum(wa[x] for x in both), sum(wb[x] for x in both)


def pair(a, b):
    """a, b: (values, abund)"""
    return _pair(_table(a), _table(b))


def mirror(fields):
    return fields[0], fields[1], fields[3], fields[2]


def all_pairs(A, B=None):
    B = A if B is None else B
    out = np.zeros((len(A), len(B), 4), dtype=np.uint64)
    tb = [_table(y) for y in B]
    for i, x in enumerate(A):
        tx = _table(x)
        for j, ty in enumerate(tb):
            out[i, j] = np.array(_pair(tx, ty), dtype=np.uint64)
    return out


def row_sums(abund):
    w = _ints(abund)
    return sum(w), min(sum(x * x for x in w), U64)


def all_row_sums(A):
    """A: list of (values, abund), or of abundance arrays"""
    return np.array([row_sums(x[1] if isinstance(x, tuple) else x) for x in A], dtype=np.uint64).reshape(len(A), 2)


def similarity(dot, sumsq_a, sumsq_b):
    if sumsq_a == 0 or sumsq_b == 0:
        assert dot == 0
        return 0.0, 0.0
    c = float(dot) / math.sqrt(float(sumsq_a) * float(sumsq_b))
    c = min(c, 1.0)
    return c, 1.0 - 2.0 * math.acos(c) / math.pi


def dist_line(ref, query, fields, lq, lr, sums_q, sums_r, k):
    """fields: pair(query, reference); lq, lr: the two lengths; sums_q, sums_r: row_sums of the two"""
    sh, dot, wq, wr = fields
    ang = similarity(dot, sums_q[1], sums_r[1])[1]
    return scm.dist_line(ref, query, sh, lq, lr, k)[:-1] + "\t%.6g\t%d/%d\t%d/%d\n" % (ang, wq, sums_q[0], wr, sums_r[0])


def dist_text(ref_names, refs, query_names, queries, k, max_dist=None):
    """one line per (query, reference), query by query; max_dist: only the pairs whose DISTANCE column is at or below it"""
    out = []
    tr, sr = [_table(r) for r in refs], [row_sums(r[1]) for r in refs]
    for qn, q in zip(query_names, queries):
        tq, sq = _table(q), row_sums(q[1])
        for rn, r, t, s in zip(ref_names, refs, tr, sr):
            f = _pair(tq, t)
            if max_dist is not None and scm.distance(f[0], len(tq), len(t), k)[1] > max_dist:
                continue
            out.append(dist_line(rn, qn, f, len(tq), len(t), sq, s, k))
    return "".join(out)


def csr(A):
    """list of (values, abund) -> (values uint64, abund uint32, offsets uint64)"""
    v, off = scm.csr([x[0] for x in A])
    a = np.concatenate([np.zeros(0, np.uint32)] + [np.asarray(x[1], dtype=np.uint32) for x in A])
    return v, np.ascontiguousarray(a, dtype=np.uint32), off
