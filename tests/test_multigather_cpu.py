"""Multigather without a GPU: rk_multigather_scaled_host against tests/gather_model.py query by query, what the shared inputs
(tests/multigather_cases.py) exercise shown on the model's output, every refusal of the bindings, and `rkmh multigather` as far as
it goes before a context exists."""
import os
import subprocess

import numpy as np
import pytest

import abund_cases as ac
import gather_cases as gc
import gather_model as gm
import multigather_cases as mc
import scaled_model as scm
from rkmh_amd import api
from test_scaled_cpu import _sketch_file


def _same(got, want, what):
    rows, off, wu = got
    wrows, woff, wwu = want
    assert rows.dtype == np.int32 and rows.shape == wrows.shape and (rows == wrows).all(), (what, rows.tolist()[:4], wrows.tolist()[:4])
    assert off.dtype == np.uint64 and off.tolist() == woff.tolist(), (what, off.tolist()[:8], woff.tolist()[:8])
    if wwu is None:
        assert wu is None, what
    else:
        assert wu is not None and wu.dtype == np.uint64 and wu.tolist() == wwu.tolist(), (what, wu.tolist()[:4], wwu.tolist()[:4])


def _host(refs, queries, abunds=None, **kw):
    rv, ro = scm.csr(refs)
    qv, qo = scm.csr(queries)
    qa = None if abunds is None else np.concatenate([np.zeros(0, np.uint32)] + [np.asarray(a, np.uint32) for a in abunds])
    return api.multigather_scaled_host(rv, ro, qv, qo, q_abund=qa, **kw)


def _sweep(refs, queries, what, abunds=None):
    """min_shared 1 and the median count; max_rounds 1, 16, 17 and None; 1 and 4 threads"""
    full = mc.answer(refs, queries, abunds=abunds)
    for ms in (1, mc.median_count(full)):
        want = full if ms == 1 else mc.answer(refs, queries, ms, abunds=abunds)
        for mr in mc.MAX_ROUNDS:
            for threads in (1, 4):
                _same(_host(refs, queries, abunds, min_shared=ms, max_rounds=mr, threads=threads), mc.cut(want, mr), (what, ms, mr, threads))
    return full


def test_a_cut_run_is_the_beginning_of_the_full_run():
    """what multigather_cases.cut relies on, against the model itself"""
    s = mc.staircases()
    b = mc.random_batch(9)
    for refs, queries in ((s["refs"], s["queries"]), (b["refs"], b["queries"])):
        full = mc.answer(refs, queries)
        for mr in (1, 16, 17):
            _same(mc.cut(full, mr), mc.answer(refs, queries, 1, mr), mr)


def test_hand_checked_vectors():
    for v in mc.kat_batches():
        got = _host(v["refs"], v["queries"], min_shared=v["min_shared"], max_rounds=v["max_rounds"])
        _same(got, v["want"], v["name"])
        _same(got, mc.answer(v["refs"], v["queries"], v["min_shared"], v["max_rounds"]), (v["name"], "model"))
        _sweep(v["refs"], v["queries"], v["name"])


@pytest.mark.parametrize("nref", gc.NREFS)
def test_random_sets(nref):
    b = mc.random_batch(nref)
    full = _sweep(b["refs"], b["queries"], nref)
    per = mc.blocks(full)
    assert len(per[1][0]) == 0 and len(per[2][0]) == 0                      # the empty query and the one without a candidate: no row
    assert (per[0][0] == per[4][0]).all() and (per[0][0] == gc.random_case(nref)[2]).all()
    if nref > 1:
        assert max(len(p[0]) for p in per) >= 2


def test_staircases_and_ties():
    s = mc.staircases()
    full = _sweep(s["refs"], s["queries"], "staircases")
    assert np.diff(full[1].astype(np.int64)).tolist() == list(s["picks"])   # 0, 1, 15, 16, 17 and 33 rows, and none for the empty query
    t = mc.ties()
    full = _sweep(t["refs"], t["queries"], "ties")
    per = [p[0] for p in mc.blocks(full)]
    assert per[0][:, 0].tolist() == [0] and per[1][:, 0].tolist() == [2]     # identical references: the lowest index, and the others never
    later = per[t["later"]]
    assert later[:, 0].tolist() == [5, 6, 7] and later[1, 1] == later[2, 1] == 3   # a tie that the first pick made


def test_many_queries_and_their_order():
    m = mc.many_queries()
    refs, queries = m["refs"], m["queries"]
    want = mc.answer(refs, queries)
    rows = np.diff(want[1].astype(np.int64))
    assert (rows == 0).any() and (rows >= 2).any()
    _same(_host(refs, queries, threads=4), want, "65 queries")
    perm = np.random.default_rng(3).permutation(len(queries))
    got = mc.blocks(_host(refs, [queries[i] for i in perm], threads=3))
    per = mc.blocks(want)
    for at, i in enumerate(perm):                                             # permuting the queries permutes the row blocks
        assert (got[at][0] == per[i][0]).all(), (at, i)


@pytest.mark.parametrize("nref", (9, 65))
def test_abundances(nref):
    b = mc.random_batch(nref)
    refs, queries, abunds = b["refs"], b["queries"], b["abunds"]
    want = mc.answer(refs, queries, abunds=abunds)
    _same(want, mc.answer(refs, queries, abunds=abunds, host=True), "the per-query host entry and the model")
    for ms, mr, threads in ((1, None, 1), (1, 2, 4), (mc.median_count(want), None, 4)):
        w = mc.cut(want, mr) if ms == 1 else mc.answer(refs, queries, ms, mr, abunds=abunds)
        _same(_host(refs, queries, abunds, min_shared=ms, max_rounds=mr, threads=threads), w, (nref, ms, mr))
    assert len(want[0]) and (want[2] != want[0][:, 1]).any()                 # the weights say something the counts do not
    ones = tuple(np.ones(len(q), np.uint32) for q in queries)
    got = _host(refs, queries, ones)
    assert (got[2] == got[0][:, 1].astype(np.uint64)).all()                  # all abundances 1: wunique = unique
    _same((got[0], got[1], None), mc.answer(refs, queries), "the rows do not depend on the abundances")
    for v in ac.gather_kat():
        got = _host(v["refs"], (v["q"], mc.EMPTY, v["q"]), (v["abund"], np.zeros(0, np.uint32), v["abund"]), min_shared=v["min_shared"], max_rounds=v["max_rounds"])
        assert got[0].tolist() == v["want"].tolist() * 2 and got[2].tolist() == v["wunique"].tolist() * 2, v["name"]


# ---- the bindings and the C entries refuse ----
def test_binding_refusals():
    rv, ro = np.arange(1, 7, dtype=np.uint64), np.array([0, 3, 6], dtype=np.uint64)
    qv, qo = np.array([2, 3, 4, 9], dtype=np.uint64), np.array([0, 3, 4], dtype=np.uint64)
    rows, off, wu = api.multigather_scaled_host(rv, ro, qv, qo)
    assert rows.tolist() == [[0, 2, 2, 1], [1, 1, 1, 0]] and off.tolist() == [0, 2, 2] and wu is None
    with pytest.raises(ValueError):
        api.multigather_scaled_host(rv, np.array([0, 3, 9], dtype=np.uint64), qv, qo)      # offsets past the values: refused by the binding
    with pytest.raises(ValueError):
        api.multigather_scaled_host(rv, ro, qv, np.array([0, 3, 5], dtype=np.uint64))
    with pytest.raises(ValueError):
        api.multigather_scaled_host(rv, ro, qv, qo, q_abund=[1, 2, 3])                    # three abundances for four values

    class NoContext(api.Context):
        def __init__(self):
            self._lib = api.load_library()

        def __del__(self):
            pass
    idx = api.ScaledIndex(NoContext(), api.C.c_void_p())
    with pytest.raises(ValueError):
        idx.multigather(qv, np.array([0, 3, 5], dtype=np.uint64))                          # before a context is needed
    with pytest.raises(ValueError):
        idx.multigather(qv, qo, q_abund=[1])
    for bad in (dict(ro=np.array([0, 5, 3], dtype=np.uint64)), dict(qo=np.array([0, 4, 2], dtype=np.uint64)), dict(ro=np.array([0], dtype=np.uint64)),
                dict(qo=np.array([0], dtype=np.uint64)), dict(min_shared=0), dict(min_shared=-3), dict(max_rounds=0), dict(max_rounds=-1),
                dict(qv=np.array([2, 3, 3, 9], dtype=np.uint64)), dict(qv=np.array([4, 3, 2, 9], dtype=np.uint64)), dict(qv=np.array([0, 3, 4, 9], dtype=np.uint64)),
                dict(qa=[1, 1, 0, 1])):
        a = dict(ro=ro, qv=qv, qo=qo, min_shared=1, max_rounds=None, qa=None)
        a.update(bad)
        with pytest.raises(api.RkmhError) as e:
            api.multigather_scaled_host(rv, a["ro"], a["qv"], a["qo"], q_abund=a["qa"], min_shared=a["min_shared"], max_rounds=a["max_rounds"])
        assert e.value.code == -1, bad
    # a value that repeats across two rows is no repeat: [2, 3] and [3, 9]
    assert api.multigather_scaled_host(rv, ro, np.array([2, 3, 3, 9], dtype=np.uint64), np.array([0, 2, 4], dtype=np.uint64))[1].tolist() == [0, 1, 2]
    lib = api.load_library()
    out, w, n = api._i32p(), api._u64p(), api.C.c_uint64()
    u64 = api.C.c_uint64
    off = np.zeros(3, np.uint64)
    assert lib.rk_multigather_scaled_host(None, None, 1, None, None, None, 1, 1, 1, 1, None, None, None, None) == -1
    args = (api._p(rv, u64), api._p(ro, u64), 2, api._p(qv, u64), None, api._p(qo, u64), 2)
    tail = (api.C.byref(out), api.C.byref(w), api._p(off, u64), api.C.byref(n))
    assert lib.rk_multigather_scaled_host(*args[:2], 1 << 31, *args[3:], 1, 1, 1, *tail) == -5        # before the offsets are read
    assert lib.rk_multigather_scaled_host(*args[:6], 1 << 31, 1, 1, 1, *tail) == -5
    assert lib.rk_multigather_scaled_host(*args, 1, 1, 1, api.C.byref(out), api.C.byref(w), None, api.C.byref(n)) == -1
    ab = np.ones(4, np.uint32)
    assert lib.rk_multigather_scaled_host(*args[:4], api._p(ab, api.C.c_uint32), *args[5:], 1, 1, 1, api.C.byref(out), None, api._p(off, u64), api.C.byref(n)) == -1
    # the entries that need a context and an index refuse missing ones
    assert lib.rk_multigather_scaled(None, None, api._p(qv, u64), None, api._p(qo, u64), 2, 1, 1, *tail) == -1
    assert lib.rk_multigather_scaled_device(None, None, 8, None, 8, 2, 4, 1, 1, 8, None, 1, 8, api.C.byref(n), None) == -1


# ---- the command, as far as it goes without a GPU ----
def _run(root, *args):
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    return subprocess.run([os.path.join(root, "bin", "rkmh")] + list(args), capture_output=True, env=env)


def test_help_text(root):
    r = _run(root, "multigather")
    assert r.returncode == 1 and r.stdout == b""
    for word in (b"rkmh multigather", b"--scaled", b"--min-shared", b"--max-rounds", b"--abund", b"-R", b"-Q", b"-g", b"--hash-policy", b"inverted index"):
        assert word in r.stderr, word
    assert b"multigather" in _run(root).stderr
    assert b"multigather" not in _run(root, "gather").stderr                # gather's own text is as it was


def _refused(r, *words):
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"rkmh multigather: "), r.stderr[-300:]
    for w in words:
        assert w.encode() in r.stderr, (w, r.stderr[-300:])


def test_multigather_refusals(root, tmp_path):
    fa = tmp_path / "x.fa"
    fa.write_text(">x\nACGTACGTACGTACGTACGTACGT\n")
    fa = str(fa)
    sc10 = _sketch_file(tmp_path / "sc10.json", scaled=10)
    sc100 = _sketch_file(tmp_path / "sc100.json", scaled=100)
    bottom = _sketch_file(tmp_path / "bottom.json", length=4)
    ok = ["--scaled", "10", "-k", "16"]
    cmd = "multigather"
    _refused(_run(root, cmd, "-f", fa, *ok), "references")                              # no references
    _refused(_run(root, cmd, "-r", fa, "-R", sc10, "-f", fa, *ok), "references")         # both kinds
    _refused(_run(root, cmd, "-r", fa, *ok), "queries")                                 # no queries
    _refused(_run(root, cmd, "-r", fa, "-f", fa, "-Q", sc10, *ok), "queries")
    _refused(_run(root, cmd, "-r", fa, "-f", fa, "-s", "100", *ok), "-s")
    _refused(_run(root, cmd, "-r", fa, "-f", fa, "-s", "100", "-k", "16"), "-s")
    _refused(_run(root, cmd, "-R", bottom, "-f", fa, *ok), "bottom")
    _refused(_run(root, cmd, "-R", sc10, "-Q", bottom), "bottom")
    for bad in ("0", "x", "-2", "3x", ""):
        _refused(_run(root, cmd, "-r", fa, "-f", fa, "--min-shared", bad, *ok), "--min-shared")
        _refused(_run(root, cmd, "-r", fa, "-f", fa, "--max-rounds", bad, *ok), "--max-rounds")
    _refused(_run(root, cmd, "-r", fa, "-f", fa, "--scaled", "0", "-k", "16"), "--scaled")
    _refused(_run(root, cmd, "-r", fa, "-f", fa, "--scaled", "ten"), "--scaled")
    _refused(_run(root, cmd, "-r", fa, "-f", fa, "--scaled", "10", "-k", "16", "-k", "21"), "one k-mer size")
    _refused(_run(root, cmd, "-r", fa, "-f", fa, "-k", "16"), "--scaled")                # nothing says at which scaled
    _refused(_run(root, cmd, "-R", sc100, "-f", fa, "--scaled", "10"), "scaled = 100")   # cannot be made finer
    _refused(_run(root, cmd, "-R", sc10, "-Q", sc100, "--scaled", "50"), "scaled = 100")
    _refused(_run(root, cmd, "-R", sc10, "-f", fa, "--hash-policy", "mash"), "--hash-policy")
    _refused(_run(root, cmd, "-R", sc10, "-f", fa, "-k", "21"), "k = 16")
    _refused(_run(root, cmd, "-g", "-R", sc10, "-Q", sc10), "-g")
    _refused(_run(root, cmd, "-R", sc10, "-Q", sc10, "--abund"), "abund")                # -Q sketches without abundances
    # gather refuses the same runs in its own name
    r = _run(root, "gather", "-r", fa, *ok)
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"rkmh gather: ")
