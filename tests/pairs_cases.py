"""Inputs the sketch-comparison tests share (tests/test_pairs_cpu.py, tests/test_gpu_pairs.py): the hand-checked vectors, random
sketches with planted overlaps and repeats, and model sketches of the bundled panel with the model's answer for them -- computed
once per process and left unchanged."""
import functools
import json
import os

import numpy as np

import dedup_model as dm
import pairs_model as pm
import sourmash_model as sm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DATA = os.path.join(GOLDEN, "data")


@functools.lru_cache(maxsize=None)
def kat():
    return json.load(open(os.path.join(GOLDEN, "pairs_kat.json")))


# ---- random sketches ----
def random_sketches(rng, n, S):
    """n rows of S: values drawn WITH replacement (planted repeats) from a pool of 2 S + 3 values that all rows share (planted
    overlaps), spread over the whole 64-bit range; the first and the last row are full, the other lengths from {0, 1, S - 1, S} and
    uniform."""
    pool = rng.integers(1, 1 << 64, size=2 * S + 3, dtype=np.uint64, endpoint=False)
    pool[0] = np.uint64((1 << 64) - 1)
    sk = np.zeros((n, S), dtype=np.uint64)
    ln = np.zeros(n, dtype=np.int32)
    edge = [0, 1, S - 1, S]
    for i in range(n):
        ln[i] = S if i in (0, n - 1) else edge[int(rng.integers(0, 4))] if rng.random() < 0.5 else int(rng.integers(0, S + 1))
        sk[i, :ln[i]] = np.sort(rng.choice(pool, size=int(ln[i]), replace=True))
    return sk, ln


# every sketch size at which the tile geometry changes (rk_pairs.hip, pairs_geometry): 16 x 16 tiles (<= 631), 10 x 10 (1000), `b` in
# global memory under 4 (4096), 2 (8192, 8193) and 1 (16384) staged rows of `a`; counts that are no multiple of any tile and that
# span several tiles on either side, (9, 3) and (5, 3) several tiles of `a` where `b` stays in global memory -- the small ones only
# where the model's merge is long
TILE_CASES = {
    1: [(1, 1), (1, 9), (7, 8), (9, 65), (65, 3)],
    2: [(1, 1), (1, 9), (7, 8), (9, 65), (65, 3)],
    63: [(1, 1), (1, 9), (7, 8), (9, 65), (65, 3)],
    64: [(1, 1), (1, 9), (7, 8), (9, 65), (65, 3)],
    65: [(1, 1), (1, 9), (7, 8), (9, 65), (65, 3)],
    1000: [(1, 1), (1, 9), (7, 8), (9, 65), (65, 3)],
    4096: [(1, 1), (1, 9), (7, 8), (9, 65), (9, 3)],
    8192: [(1, 1), (1, 9), (7, 8), (9, 3)],
    8193: [(1, 1), (1, 9), (7, 8), (3, 129)],
    16384: [(1, 1), (1, 9), (1, 257), (5, 3)],
}


# ---- the bundled panel ----
def _seqs(path, first=None):
    from rkmh_amd import api   # the host parser only (checked against the kseq grammar by tests/test_abi_cpu.py)
    r = api.parse_files([os.path.join(DATA, path)])
    seqs = [bytes(r["bases"][int(r["offsets"][i]):int(r["offsets"][i + 1])]) for i in range(r["nseq"])]
    names = r["names"]
    return (seqs, names) if first is None else (seqs[:first], names[:first])


# name -> (file, first n records, policy text, model policy, distinct, k).  40 of the panel's 182 references: the model answers
# their 1 600 ordered pairs in about a second per setting
PANEL = {
    "default-k12": ("all_pave_ref.fa.gz", 40, "default", sm.DEFAULT, False, 12),
    "mash-k16": ("all_pave_ref.fa.gz", 40, "mash", sm.MASH, False, 16),
    "sourmash-k21": ("all_pave_ref.fa.gz", 40, "sourmash", dm.SOURMASH, True, 21),
    "zika-k16": ("zika.refs.fa.gz", None, "default", sm.DEFAULT, False, 16),
}
PANEL_S = 1000


@functools.lru_cache(maxsize=None)
def panel(name):
    """-> dict(seqs, names, spec, k, sk, ln, out): the model's sketches of the case as rows, and the model's answer for all pairs"""
    path, first, spec, pol, distinct, k = PANEL[name]
    seqs, names = _seqs(path, first)
    sketches = (dm.sketch_refs if distinct else sm.sketch_refs)(seqs, [k], PANEL_S, pol)
    sk, ln = pm.rows([s.tolist() for s in sketches], PANEL_S)
    out = pm.all_pairs(sk, ln)
    for a in (sk, ln, out):
        a.setflags(write=False)
    return dict(seqs=seqs, names=names, spec=spec, k=k, distinct=distinct, sk=sk, ln=ln, out=out)


def unordered(out):
    """rows of the pairs i < j"""
    return out[np.triu_indices(out.shape[0], 1)]
