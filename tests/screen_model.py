"""Screen (rk_screen_*, rk_screen_rows_host, `rkmh screen`) in pure Python and numpy, from the definition in include/rkmh_amd.h, "SCREEN"
-- it calls neither the library nor the oracle.

  counted    the distinct non-zero window hashes of a read set and their multiplicities as Python ints, NOT clamped
             (abund_model.sketch / merge at FULL; exact while no single count reaches 2^32)
  collapse   the distinct values of a row, ascending
  rows       (rows, counted dict, m) -> [[shared, median, wshared, wmedian]] by the definition: presence on the clamped count,
             lower median, owner by the cross-multiplied ratio with the lowest index among equals
  identity   (shared / len)^(1 / k), 0 and 1 at the ends
  line       one line of `rkmh screen`
Pinned by tests/golden/screen_kat.json."""
import numpy as np

import abund_model as am

FULL = am.FULL
SAT = am.SAT


def counted(reads, ks, pol):
    """-> dict value -> multiplicity over all reads"""
    v, a = am.merge([am.sketch(r, list(ks), pol, FULL) for r in reads], FULL)
    return dict(zip((int(x) for x in v.tolist()), (int(x) for x in a.tolist())))


def collapse(row):
    return sorted(set(int(x) for x in row))


def lower_median(cs):
    return sorted(cs)[(len(cs) - 1) // 2] if cs else 0


def rows(ref_rows, counts, m=1):
    """ref_rows: list of sequences of ints (ascending, repeats allowed); counts: dict value -> multiplicity (any size)"""
    R = [collapse(r) for r in ref_rows]
    rep = {v: min(int(c), SAT) for v, c in counts.items()}
    present = {v for v, c in rep.items() if c >= m}
    shared = [sum(1 for v in r if v in present) for r in R]
    posting = {}
    for i, r in enumerate(R):
        for v in r:
            posting.setdefault(v, []).append(i)
    owner = {}
    for v in present:
        best = None
        for a in posting.get(v, []):     # ascending reference index: a strict improvement only, so the lowest index wins a tie
            if best is None or shared[a] * len(R[best]) > shared[best] * len(R[a]):
                best = a
        if best is not None:
            owner[v] = best
    out = []
    for i, r in enumerate(R):
        cs = [rep[v] for v in r if v in present]
        ws = [rep[v] for v in r if v in present and owner[v] == i]
        out.append([len(cs), lower_median(cs), len(ws), lower_median(ws)])
    return out


def present_keys(ref_rows, counts, m=1):
    keys = set()
    for r in ref_rows:
        keys.update(int(x) for x in r)
    return sum(1 for v in keys if min(int(counts.get(v, 0)), SAT) >= m)


def key_counts(ref_rows, counts):
    """what rk_screen_counts gives: (keys ascending, raw counts)"""
    keys = sorted({int(x) for r in ref_rows for x in r})
    return keys, [int(counts.get(v, 0)) for v in keys]


def identity(shared, length, k):
    if shared == 0 or length == 0:
        return 0.0
    if shared == length:
        return 1.0
    return (shared / length) ** (1.0 / k)


def line(shared, length, median, k, ref, path):
    return "%.6g\t%d/%d\t%d\t%s\t%s\n" % (identity(shared, length, k), shared, length, median, ref, path)


def to_csr(ref_rows):
    off = np.zeros(len(ref_rows) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in ref_rows], dtype=np.uint64)
    vals = np.asarray([int(x) for r in ref_rows for x in r], dtype=np.uint64)
    return vals, off
