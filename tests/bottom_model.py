"""Bottom samples (rk_sample_create_bottom, rk_sample_finish_bottom, rk_bottom_cut, `rkmh sketch -g -s <S> --min-copies <m>`) in pure
Python and numpy, from the definition in include/rkmh_amd.h, "BOTTOM SAMPLES" -- it calls neither the library nor the oracle.

  counted     the distinct non-zero window hashes of a read set and their multiplicities (abund_model.sketch / merge at FULL)
  emit        the sketch of a counted set: the values with at least m copies, once each (distinct) or once per copy (multiset), the first S
  direct      the definition: emit(counted(reads))
  weights     what every entry of a counted set weighs in a cut
  cut         (j* + 1, values[j*]) of a counted set, (0, 0) when the weights stay below S
  Stream      the accumulator as plain Python: a threshold that only comes down, every value at or below it with its exact count
  row         a sketch as rk_sample_finish_bottom gives it: (uint64 [S] zero padded, length)"""
import numpy as np

import abund_model as am
import sourmash_model as sm

FULL = am.FULL
SAT = am.SAT


def counted(reads, ks, pol):
    return am.merge([am.sketch(r, list(ks), pol, FULL) for r in reads], FULL)


def emit(values, counts, S, m, distinct):
    out = []
    for v, c in zip(np.asarray(values, dtype=np.uint64).tolist(), np.asarray(counts, dtype=np.uint32).tolist()):
        if c < m:
            continue
        out += [v] * (1 if distinct else min(c, S - len(out)))
        if len(out) >= S:
            break
    return out[:S]


def direct(reads, ks, pol, S, m=1, distinct=False):
    return emit(*counted(reads, ks, pol), S, m, distinct)


def weights(counts, S, m, distinct):
    c = np.asarray(counts, dtype=np.uint64)
    return np.where(c < m, 0, 1 if distinct else np.minimum(c, S)).astype(np.uint64)


def cut(values, counts, S, m, distinct):
    run = np.cumsum(weights(counts, S, m, distinct), dtype=np.uint64)
    j = int(np.searchsorted(run, np.uint64(S), side="left"))      # the first inclusive sum that reaches S
    if j >= len(run):
        return 0, 0
    return j + 1, int(np.asarray(values, dtype=np.uint64)[j])


def row(sketch, S):
    r = np.zeros(S, dtype=np.uint64)
    r[:len(sketch)] = np.asarray(sketch, dtype=np.uint64)
    return r, len(sketch)


def read_hashes(read, ks, pol):
    h = sm.calc_hashes(read, list(ks), pol)
    return h[h != 0].tolist()


class Stream:
    """Feeds are lists of window hashes; when a cut happens is the caller's business (cut_now), the result must not depend on it."""

    def __init__(self, S, m=1, distinct=False):
        self.S, self.m, self.distinct = S, m, distinct
        self.T = FULL
        self.res = {}                # every value <= T seen so far -> its count
        self.cuts = 0
        self.thresholds = [FULL]     # T after every cut_now
        self.spared = []             # at each cut that lowered T: the values below the new T that did not qualify yet

    def feed(self, hashes):
        for h in hashes:
            if 0 < h <= self.T:
                self.res[h] = min(self.res.get(h, 0) + 1, SAT)

    def sorted(self):
        v = sorted(self.res)
        return np.asarray(v, dtype=np.uint64), np.asarray([self.res[x] for x in v], dtype=np.uint32)

    def cut_now(self):
        v, c = self.sorted()
        n, t = cut(v, c, self.S, self.m, self.distinct)
        if n:
            self.T = t
            self.res = {x: k for x, k in self.res.items() if x <= t}
            self.cuts += 1
            self.spared.append({x for x, k in self.res.items() if k < self.m})
        self.thresholds.append(self.T)
        return n

    def finish(self):
        self.cut_now()
        return emit(*self.sorted(), self.S, self.m, self.distinct)
