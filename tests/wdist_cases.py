"""Inputs the weighted-comparison tests share (tests/test_wdist_cpu.py, tests/test_gpu_wdist.py): the hand-checked vectors, random CSR
sets with abundances, and the model's abundance sketches of the bundled files -- computed once per process and left unchanged."""
import functools
import json
import os

import numpy as np

import abund_cases as ac
import abund_model as am
import dedup_model as dm
import scaled_cases as sc
import scaled_model as scm
import sourmash_model as sm
import wdist_model as wm

WEIGHTS = (1, 2, 255, 65535, (1 << 32) - 1)          # what the random sets draw their abundances from


@functools.lru_cache(maxsize=None)
def _doc():
    return json.load(open(os.path.join(sc.GOLDEN, "wdist_kat.json")))


def _frozen(x):
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def pair_kat():
    """-> tuple of dict(name, a: (values, abund), b: (values, abund), want: 4 ints, sums_a, sums_b: 2 ints each)"""
    out = []
    for v in _doc():
        if v["kind"] != "pair":
            continue
        a = (_frozen(sc._expand(v["a"])), _frozen(np.array(ac._abund(v["aw"]))))
        b = (_frozen(sc._expand(v["b"])), _frozen(np.array(ac._abund(v["bw"]))))
        assert len(a[0]) == len(a[1]) and len(b[0]) == len(b[1]), v["name"]
        out.append(dict(name=v["name"], a=a, b=b, want=tuple(int(x) for x in v["want"]), sums_a=tuple(int(x) for x in v["sums_a"]),
                        sums_b=tuple(int(x) for x in v["sums_b"])))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def sim_kat():
    return tuple(v for v in _doc() if v["kind"] == "sim")


def weights(rng, n):
    return _frozen(np.array(WEIGHTS, dtype=np.uint32)[rng.integers(0, len(WEIGHTS), size=n)])


def with_weights(rng, sets):
    return [(_frozen(np.array(s, dtype=np.uint64)), weights(rng, len(s))) for s in sets]


@functools.lru_cache(maxsize=None)
def random_case(na, nb, long_row=False, self_form=False):
    """na x nb sets drawn from one pool (row lengths from scaled_cases.LENGTHS; long_row: the first of `a` holds 70 000 values), each with
    abundances from WEIGHTS -> (A, B, want uint64 [na, nb, 4]); self_form: B is A"""
    rng = np.random.default_rng(7000 + 131 * na + nb + (1 if long_row else 0))
    pl = sc.pool(rng, 100000 if long_row else 6000)
    A = with_weights(rng, sc.random_sets(rng, na, pl, first=sc.LONG_ROW if long_row else None))
    B = A if self_form else with_weights(rng, sc.random_sets(rng, nb, pl))
    return A, B, _frozen(wm.all_pairs(A, B))


# ---- the bundled files under the two policies: name -> (file, first n records, policy text, model policy, k) ----
FILES = {
    ("pave", "default"): ("all_pave_ref.fa.gz", 40, "default", sm.DEFAULT, 12),
    ("pave", "sourmash"): ("all_pave_ref.fa.gz", 40, "sourmash", dm.SOURMASH, 21),
    ("zika", "default"): ("zika.refs.fa.gz", None, "default", sm.DEFAULT, 16),
    ("zika", "sourmash"): ("zika.refs.fa.gz", None, "sourmash", dm.SOURMASH, 21),
}


@functools.lru_cache(maxsize=None)
def file_full(key):
    """-> dict(path, names, seqs, spec, k, full): full[i] = the model's abundance sketch of record i at scaled 1"""
    path, first, spec, pol, k = FILES[key]
    seqs, names = sc._seqs(path, first)
    full = tuple(tuple(_frozen(x) for x in am.sketch(s, [k], pol, am.FULL)) for s in seqs)
    return dict(path=os.path.join(sc.DATA, path), first=first, names=[n.decode() for n in names], seqs=seqs, spec=spec, k=k, full=full)


@functools.lru_cache(maxsize=None)
def file_sketches(key, scaled):
    mh = scm.max_hash(scaled)
    return tuple(tuple(_frozen(x) for x in am.downsample(v, a, mh)) for v, a in file_full(key)["full"])
