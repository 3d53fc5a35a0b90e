"""Gather without a GPU: the model (tests/gather_model.py) against the hand-checked vectors, rk_gather_scaled_host against the model
on the vectors and on random CSR sets, the invariants of include/rkmh_amd.h "GATHER", what the binding refuses, and the help text
and every refusal of `rkmh gather` (all made before a context exists)."""
import json
import os
import subprocess

import numpy as np
import pytest

import gather_cases as gc
import gather_model as gm
import scaled_cases as sc
import scaled_model as scm
from rkmh_amd import api
from test_scaled_cpu import DEFAULT_POLICY, _sketch_file


def _same(got, want, what):
    assert got.dtype == np.int32 and got.shape == want.shape and (got == want).all(), (what, got.tolist()[:4], want.tolist()[:4])


# ---- the model against the vectors ----
def test_there_are_enough_vectors():
    names = [v["name"] for v in gc.kat()]
    assert len(names) >= 16 and len(set(names)) == len(names)
    assert any(len(v["q"]) == 0 for v in gc.kat()) and any(any(len(r) == 0 for r in v["refs"]) for v in gc.kat())
    assert any(v["min_shared"] > 1 for v in gc.kat()) and any(v["max_rounds"] is not None for v in gc.kat())
    assert any(len(v["q"]) and int(v["q"][-1]) == scm.FULL for v in gc.kat())


@pytest.mark.parametrize("i", range(len(gc.kat())))
def test_model_matches_hand_checked_vectors(i):
    v = gc.kat()[i]
    _same(gm.gather(v["q"], v["refs"], v["min_shared"], v["max_rounds"]), v["want"], v["name"])


# ---- rk_gather_scaled_host against the model ----
def _host(q, refs, min_shared=1, max_rounds=None, threads=1):
    rv, ro = scm.csr(refs)
    return api.gather_scaled_host(q, rv, ro, min_shared=min_shared, max_rounds=max_rounds, threads=threads)


@pytest.mark.parametrize("i", range(len(gc.kat())))
def test_host_entry_matches_hand_checked_vectors(i):
    v = gc.kat()[i]
    for threads in (1, 4):
        _same(_host(v["q"], v["refs"], v["min_shared"], v["max_rounds"], threads), v["want"], (v["name"], threads))


def _invariants(rows, q, refs, min_shared, what):
    u = rows[:, 1]
    assert (np.diff(u) <= 0).all(), (what, "unique increases")
    assert len(set(rows[:, 0].tolist())) == len(rows), (what, "a reference is picked twice")
    assert (u >= min_shared).all() and (rows[:, 2] >= u).all()
    for r, _, tot, _ in rows.tolist():
        assert tot == scm.shared(q, refs[r]) >= min_shared, (what, r)
    if len(rows):
        assert len(q) - int(u.sum()) == rows[-1, 3], (what, "remaining")
        assert (rows[:, 3] == len(q) - np.cumsum(u)).all()


@pytest.mark.parametrize("nref", gc.NREFS)
def test_host_entry_on_random_sets(nref):
    q, refs, want = gc.random_case(nref)
    assert len(want) >= min(3, nref), len(want)              # not vacuous (one reference gives one row at most)
    _invariants(want, q, refs, 1, ("model", nref))
    for threads in (1, 16):
        _same(_host(q, refs, threads=threads), want, (nref, threads))
    for min_shared, max_rounds in ((1, 2), (50, None), (int(want[-1, 1]) + 1, None), (1, 10 ** 6)):
        w = gm.gather(q, refs, min_shared, max_rounds)
        _invariants(w, q, refs, min_shared, (nref, min_shared, max_rounds))
        _same(_host(q, refs, min_shared, max_rounds, threads=3), w, (nref, min_shared, max_rounds))
    assert len(gm.gather(q, refs, int(want[-1, 1]) + 1)) < len(want)         # min_shared just above the last row cuts it off


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 33])
def test_host_entry_on_staircases(n):
    q, refs = gc.staircase(n)
    want = gm.gather(q, refs)
    assert len(want) == n and want[:, 0].tolist() == list(range(len(refs) - 1, -1, -1))[:n]
    _same(_host(q, refs), want, n)


# ---- the binding and the C entry refuse ----
def test_binding_refusals():
    q = np.arange(1, 9, dtype=np.uint64)
    rv, ro = np.arange(1, 7, dtype=np.uint64), np.array([0, 3, 6], dtype=np.uint64)
    assert api.RK_GATHER_BATCH == 16
    assert api.gather_scaled_host(q, rv, ro).tolist() == [[0, 3, 3, 5], [1, 3, 3, 2]]
    with pytest.raises(ValueError):
        api.gather_scaled_host(q, rv, np.array([0, 3, 9], dtype=np.uint64))      # offsets past the values: refused by the binding

    class NoContext(api.Context):
        def __init__(self):
            pass

        def __del__(self):
            pass
    with pytest.raises(ValueError):
        NoContext().gather_scaled(q, rv, np.array([0, 3, 9], dtype=np.uint64))   # before a context is needed
    for bad in (dict(q=q[::-1].copy()), dict(q=np.array([1, 1, 2], dtype=np.uint64)), dict(q=np.array([0, 1], dtype=np.uint64)),
                dict(ro=np.array([0, 5, 3], dtype=np.uint64)), dict(ro=np.array([0], dtype=np.uint64)), dict(min_shared=0), dict(max_rounds=0),
                dict(min_shared=-3), dict(max_rounds=-1)):
        a = dict(q=q, rv=rv, ro=ro, min_shared=1, max_rounds=None)
        a.update(bad)
        with pytest.raises(api.RkmhError) as e:
            api.gather_scaled_host(a["q"], a["rv"], a["ro"], min_shared=a["min_shared"], max_rounds=a["max_rounds"])
        assert e.value.code == -1, bad
    lib = api.load_library()
    n = api.C.c_int(0)
    out = np.zeros(8, np.int32)
    assert lib.rk_gather_scaled_host(None, 3, None, None, 1, 1, 1, 1, None, None) == -1
    assert lib.rk_gather_scaled_host(api._p(q, api.C.c_uint64), 1 << 31, api._p(rv, api.C.c_uint64), api._p(ro, api.C.c_uint64), 2, 1, 1, 1,
                                     api._p(out, api.C.c_int32), api.C.byref(n)) == -5


# ---- the command, as far as it goes without a GPU ----
def _run(root, *args):
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    return subprocess.run([os.path.join(root, "bin", "rkmh")] + list(args), capture_output=True, env=env)


def test_help_text(root):
    r = _run(root, "gather")
    assert r.returncode == 1 and r.stdout == b""
    for word in (b"rkmh gather", b"--scaled", b"--min-shared", b"--max-rounds", b"-R", b"-Q", b"-g", b"--hash-policy"):
        assert word in r.stderr, word
    assert b"gather" in _run(root).stderr


def _refused(r, *words):
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"rkmh gather: "), r.stderr[-300:]
    for w in words:
        assert w.encode() in r.stderr, (w, r.stderr[-300:])


def test_gather_refusals(root, tmp_path):
    fa = tmp_path / "x.fa"
    fa.write_text(">x\nACGTACGTACGTACGTACGTACGT\n")
    fa = str(fa)
    sc10 = _sketch_file(tmp_path / "sc10.json", scaled=10)
    sc100 = _sketch_file(tmp_path / "sc100.json", scaled=100)
    bottom = _sketch_file(tmp_path / "bottom.json", length=4)
    ok = ["--scaled", "10", "-k", "16"]
    _refused(_run(root, "gather", "-f", fa, *ok), "references")                              # no references
    _refused(_run(root, "gather", "-r", fa, "-R", sc10, "-f", fa, *ok), "references")         # both kinds
    _refused(_run(root, "gather", "-r", fa, *ok), "queries")                                 # no queries
    _refused(_run(root, "gather", "-r", fa, "-f", fa, "-Q", sc10, *ok), "queries")
    _refused(_run(root, "gather", "-r", fa, "-f", fa, "-s", "100", *ok), "-s")
    _refused(_run(root, "gather", "-r", fa, "-f", fa, "-s", "100", "-k", "16"), "-s")
    _refused(_run(root, "gather", "-R", bottom, "-f", fa, *ok), "bottom")
    _refused(_run(root, "gather", "-R", sc10, "-Q", bottom), "bottom")
    for bad in ("0", "x", "-2", "3x", ""):
        _refused(_run(root, "gather", "-r", fa, "-f", fa, "--min-shared", bad, *ok), "--min-shared")
        _refused(_run(root, "gather", "-r", fa, "-f", fa, "--max-rounds", bad, *ok), "--max-rounds")
    _refused(_run(root, "gather", "-r", fa, "-f", fa, "--scaled", "0", "-k", "16"), "--scaled")
    _refused(_run(root, "gather", "-r", fa, "-f", fa, "--scaled", "ten"), "--scaled")
    _refused(_run(root, "gather", "-r", fa, "-f", fa, "--scaled", "10", "-k", "16", "-k", "21"), "one k-mer size")
    _refused(_run(root, "gather", "-r", fa, "-f", fa, "-k", "16"), "--scaled")                # nothing says at which scaled
    _refused(_run(root, "gather", "-R", sc100, "-f", fa, "--scaled", "10"), "scaled = 100")   # cannot be made finer
    _refused(_run(root, "gather", "-R", sc10, "-Q", sc100, "--scaled", "50"), "scaled = 100")
    _refused(_run(root, "gather", "-R", sc10, "-f", fa, "--hash-policy", "mash"), "--hash-policy")     # policy disagreement
    _refused(_run(root, "gather", "-R", sc10, "-f", fa, "-k", "21"), "k = 16")               # k disagreement with -k
    doc = json.load(open(sc10))
    for d in doc:
        d["kmer"] = "21"
    k21 = tmp_path / "k21.json"
    k21.write_text(json.dumps(doc, separators=(",", ":"), sort_keys=True))
    _refused(_run(root, "gather", "-R", sc10, "-Q", str(k21)), "k = 21")                     # and between files
    _refused(_run(root, "gather", "-g", "-R", sc10, "-f", fa), "-g")
    mixed = _sketch_file(tmp_path / "mixed.json", per_object_scaled=[10, 100])
    _refused(_run(root, "gather", "-R", mixed, "-f", fa), "disagree in scaled")
    assert DEFAULT_POLICY in open(sc10).read()
