"""Inputs the scaled-sketch tests share (tests/test_scaled_cpu.py, tests/test_gpu_scaled.py): the hand-checked vectors, random CSR
sets drawn from a shared pool, and model sketches of the bundled panels -- computed once per process and left unchanged."""
import functools
import json
import os

import numpy as np

import dedup_model as dm
import scaled_model as scm
import sourmash_model as sm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DATA = os.path.join(GOLDEN, "data")


def _expand(pieces):
    """a side of a vector: a list of values and of ["range", start, stop, step] pieces, ascending as written"""
    out = []
    for p in pieces:
        if isinstance(p, list):
            assert p[0] == "range"
            out.extend(range(p[1], p[2], p[3]))
        else:
            out.append(p)
    assert all(0 < x < (1 << 64) for x in out) and all(x < y for x, y in zip(out, out[1:])), "a vector's side ascends strictly"
    return np.asarray(out, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def kat():
    """-> tuple of dict(name, a, b, want): a, b uint64 arrays"""
    doc = json.load(open(os.path.join(GOLDEN, "scaled_kat.json")))
    out = []
    for v in doc:
        a, b = _expand(v["a"]), _expand(v["b"])
        a.setflags(write=False)
        b.setflags(write=False)
        out.append(dict(name=v["name"], a=a, b=b, want=int(v["want"])))
    return tuple(out)


# ---- random CSR sets ----
LENGTHS = [0, 1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 1000, 4097]
SHAPES = [(1, 1), (1, 9), (7, 8), (9, 65), (65, 3)]
LONG_ROW = 70000


def pool(rng, n):
    """n distinct values over the whole 64-bit range, 2^64 - 1 among them"""
    p = np.unique(rng.integers(1, 1 << 64, size=n + n // 8, dtype=np.uint64, endpoint=False))[:n]
    p = rng.permutation(p)
    p[0] = np.uint64(scm.FULL)
    return np.unique(p)


def random_sets(rng, n, pl, lengths=LENGTHS, first=None):
    """n ascending distinct sets drawn from the pool pl; lengths from `lengths`, the first one `first` values when given"""
    out = []
    for i in range(n):
        m = first if (i == 0 and first is not None) else int(lengths[int(rng.integers(0, len(lengths)))])
        out.append(np.sort(rng.choice(pl, size=min(m, len(pl)), replace=False)))
    return out


# ---- the bundled panels ----
def _seqs(path, first=None):
    from rkmh_amd import api   # the host parser only (checked against the kseq grammar by tests/test_abi_cpu.py)
    r = api.parse_files([os.path.join(DATA, path)])
    seqs = [bytes(r["bases"][int(r["offsets"][i]):int(r["offsets"][i + 1])]) for i in range(r["nseq"])]
    names = r["names"]
    return (seqs, names) if first is None else (seqs[:first], names[:first])


# name -> (file, first n records, policy text, model policy, k-mer sizes)
PANEL = {
    "default-k12": ("all_pave_ref.fa.gz", 40, "default", sm.DEFAULT, (12,)),
    "mash-k16": ("all_pave_ref.fa.gz", 40, "mash", sm.MASH, (16,)),
    "sourmash-k21": ("all_pave_ref.fa.gz", 40, "sourmash", dm.SOURMASH, (21,)),
    "default-k12-k16": ("all_pave_ref.fa.gz", 40, "default", sm.DEFAULT, (12, 16)),
    "zika-k16": ("zika.refs.fa.gz", None, "default", sm.DEFAULT, (16,)),
}
SCALED = (1, 2, 10, 100, 1000)


@functools.lru_cache(maxsize=None)
def panel(name):
    """-> dict(seqs, names, spec, pol, ks, full): full[i] = the model's sketch of record i at scaled 1 (every other scaled is a prefix
    of it: sketches()), hashes = the non-zero window hashes before repeats are dropped"""
    path, first, spec, pol, ks = PANEL[name]
    seqs, names = _seqs(path, first)
    full, nonzero = [], 0
    for s in seqs:
        h = np.asarray(sm.calc_hashes(s, list(ks), pol), dtype=np.uint64)
        nonzero += int((h != 0).sum())
        u = np.unique(h[h != 0])
        u.setflags(write=False)
        full.append(u)
    return dict(seqs=seqs, names=names, spec=spec, pol=pol, ks=list(ks), full=tuple(full), nonzero=nonzero)


@functools.lru_cache(maxsize=None)
def sketches(name, scaled):
    return tuple(scm.downsample(f, scaled) for f in panel(name)["full"])


@functools.lru_cache(maxsize=None)
def panel_shared(name, scaled):
    out = scm.all_shared(sketches(name, scaled))
    out.setflags(write=False)
    return out


def unordered(out):
    return out[np.triu_indices(out.shape[0], 1)]
