"""The sketch rule dedup=distinct (policy U6) in pure Python and numpy, on top of tests/sourmash_model.py: a sketch is the S
smallest DISTINCT non-zero hashes of a sequence (after mask_by_frequency / the frequency range filter), an intersection is a set
intersection, row field 3 is the length of the read's sketch.  Hashing, argmax / diff and the depth counters are sourmash_model's.
Pinned by tests/golden/dedup_kat.json and by the rule that on inputs without repeated values it equals sourmash_model.bottom."""
import numpy as np

import sourmash_model as sm

SOURMASH = dict(sm.LEXMIN)                       # the hashing side of the `sourmash` preset: mash + canon=lexmin
DISTINCT_DEFAULT = dict(sm.DEFAULT)              # dedup=distinct alone


def bottom_distinct(h, S: int) -> np.ndarray:
    u = np.unique(np.asarray(h, dtype=np.uint64))            # sorted, each value once
    return u[u != 0][:S]


def frequency_filter(h, counter, fmin: int, fmax: int, incl=True) -> np.ndarray:
    """minhashes_frequency_filter's keep rule: a non-zero hash stays when its slot's count lies in [fmin, fmax] (freqmax=incl)."""
    h = np.asarray(h, dtype=np.uint64)
    c = counter[(h % np.uint64(len(counter))).astype(np.int64)]
    keep = (c >= fmin) & ((c <= fmax) if incl else (c < fmax))
    return np.where(keep, h, np.uint64(0))


def sketch_refs(ref_seqs, ks, S, pol):
    return [bottom_distinct(sm.calc_hashes(r, ks, pol), S) for r in ref_seqs]


def read_sketch(read, ks, S, pol, counter=None, min_occ=0):
    h = sm.calc_hashes(read, ks, pol)
    if counter is not None:
        h = sm.mask_by_frequency(h, counter, min_occ, pol)
    return bottom_distinct(h, S)


def classify(read_seqs, ref_sketches, ks, S, pol, counter=None, min_occ=0, bound=None):
    """Rows (ref, shared, diff, len(sketch(read))): shared[r] = |sketch(read) & sketch(ref_r)|; first index wins (sm.argmax_diff);
    bound: rk_set_min_num_bound's cap on field 3."""
    post = {}
    for j, sk in enumerate(ref_sketches):
        for v in np.unique(sk).tolist():
            post.setdefault(v, []).append(j)
    rows = np.zeros((len(read_seqs), 4), dtype=np.int32)
    for i, r in enumerate(read_seqs):
        mins = read_sketch(r, ks, S, pol, counter, min_occ)
        shared = [0] * len(ref_sketches)
        for v in mins.tolist():
            for j in post.get(v, ()):
                shared[j] += 1
        mi, ms, d = sm.argmax_diff(shared)
        n = len(mins)
        rows[i] = (mi, ms, d, n if bound is None or bound < 0 else min(n, bound))
    return rows
