"""Search without a GPU: the model (tests/search_model.py) against the hand-checked vectors, rk_search_scaled_host against the model
on the vectors and on random collections, the rule behind --min-containment, what the bindings refuse, and the help text and every
refusal of `rkmh manysearch` (all made before a context exists)."""
import os
import subprocess

import numpy as np
import pytest

import scaled_model as scm
import search_cases as sec
import search_model as sem
from rkmh_amd import api
from test_scaled_cpu import _sketch_file


def _same(got, want, what):
    assert got.dtype == np.int32 and got.shape == want.shape and (got == want).all(), (what, got.tolist()[:4], want.tolist()[:4])


def _host(refs, queries, min_shared=1, q_min=None, threads=1):
    rv, ro = scm.csr(refs)
    qv, qo = scm.csr(queries)
    return api.search_scaled_host(rv, ro, qv, qo, min_shared=min_shared, q_min=q_min, threads=threads)


# ---- the model against the vectors ----
def test_there_are_enough_vectors():
    kat = sec.kat()
    names = [v["name"] for v in kat]
    assert len(names) >= 20 and len(set(names)) == len(names)
    assert any(any(len(q) == 0 for q in v["queries"]) for v in kat) and any(any(len(r) == 0 for r in v["refs"]) for v in kat)
    assert any(v["q_min"] is not None and len(set(v["q_min"])) > 1 for v in kat) and any(v["min_shared"] > 1 for v in kat)
    assert any(len(v["want"]) == len(v["refs"]) > 2 and len(v["queries"]) == 1 for v in kat)            # a value held by every reference
    assert any(len(v["refs"]) > 1 and all(np.array_equal(r, v["refs"][0]) for r in v["refs"]) for v in kat)               # identical rows
    by_inputs = {}
    for v in kat:                                                      # one pair at thresholds equal to, below and above its count
        by_inputs.setdefault((tuple(map(bytes, v["refs"])), tuple(map(bytes, v["queries"]))), []).append(v)
    assert any(len(vs) >= 3 and {len(v["want"]) for v in vs} == {0, 1} for vs in by_inputs.values())


@pytest.mark.parametrize("i", range(len(sec.kat())))
def test_model_matches_hand_checked_vectors(i):
    v = sec.kat()[i]
    _same(sem.search(v["refs"], v["queries"], v["min_shared"], v["q_min"]), v["want"], v["name"])
    _same(sem.search_by_rows(v["refs"], v["queries"], v["min_shared"], v["q_min"]), v["want"], (v["name"], "by rows"))


# ---- rk_search_scaled_host against the model ----
@pytest.mark.parametrize("i", range(len(sec.kat())))
def test_host_entry_matches_hand_checked_vectors(i):
    v = sec.kat()[i]
    for threads in (1, 4):
        _same(_host(v["refs"], v["queries"], v["min_shared"], v["q_min"], threads), v["want"], (v["name"], threads))


@pytest.mark.parametrize("nref", sec.NREFS)
def test_host_entry_on_random_sets(nref):
    c = sec.random_case(nref)
    refs, queries, want1 = c["refs"], c["queries"], c["want1"]
    npairs = nref * len(queries)
    # not vacuous: hits and non-hits; pairs below, at and above the cut; q_min decides some pairs either way
    assert 0 < len(want1) < npairs and (want1[:, 2] >= 1).all()
    assert 0 < len(c["want_cut"]) < len(want1)
    assert 0 < len(c["want_qmin"]) < len(want1)
    assert sorted(map(tuple, want1[:, :2].tolist())) == list(map(tuple, want1[:, :2].tolist()))
    if nref <= 65:
        _same(sem.search_by_rows(refs, queries), want1, (nref, "the two forms of the model"))
    for threads in (1, 4):
        _same(_host(refs, queries, threads=threads), want1, (nref, threads))
        _same(_host(refs, queries, min_shared=c["cut"], threads=threads), c["want_cut"], (nref, threads, "cut"))
        _same(_host(refs, queries, min_shared=2, q_min=c["q_min"], threads=threads), c["want_qmin"], (nref, threads, "q_min"))
    for nq in sec.NQS:
        _same(_host(refs, queries[:nq], threads=3), sec.first_queries(want1, nq), (nref, nq))


def test_model_forms_agree_around_a_block_edge():
    c = sec.block_edges(sec.REF_BLOCK + 1)
    near = list(range(0, 40)) + list(range(sec.REF_BLOCK - 40, sec.REF_BLOCK + 1))
    refs = [c["refs"][r] for r in near]
    for ms in (1, 2):
        _same(sem.search_by_rows(refs, c["queries"], ms), sem.search(refs, c["queries"], ms), ms)
        _same(_host(refs, c["queries"], ms, threads=2), sem.search(refs, c["queries"], ms), (ms, "host"))


# ---- the rule behind --min-containment ----
@pytest.mark.parametrize("x", [0.1, 0.5, 0.7, 1.0])
def test_min_count_rule(x):
    for n in range(1, 21):
        want = next(t for t in range(0, n + 1) if float(t) / float(n) >= x)         # the definition, in Python doubles
        assert api.search_min_count(x, n) == want == sem.min_count(x, n), (x, n)
        assert want >= 1 and (want - 1) / n < x
    assert api.search_min_count(x, 0) == 0 and api.search_min_count(0.0, 7) == 0


def test_min_count_refusals():
    for bad in (-0.1, 1.0000001, float("nan"), float("inf")):
        with pytest.raises(api.RkmhError) as e:
            api.search_min_count(bad, 5)
        assert e.value.code == -1
    with pytest.raises(api.RkmhError) as e:
        api.search_min_count(0.5, 1 << 31)
    assert e.value.code == -5


# ---- the bindings and the C entry refuse ----
def test_binding_refusals():
    assert api.RK_SEARCH_REF_BLOCK == sec.REF_BLOCK == 8192
    rv, ro = np.arange(1, 7, dtype=np.uint64), np.array([0, 3, 6], dtype=np.uint64)
    qv, qo = np.array([2, 3, 4, 9], dtype=np.uint64), np.array([0, 3, 4], dtype=np.uint64)
    assert api.search_scaled_host(rv, ro, qv, qo).tolist() == [[0, 0, 2], [0, 1, 1]]
    with pytest.raises(ValueError):
        api.search_scaled_host(rv, np.array([0, 3, 9], dtype=np.uint64), qv, qo)       # offsets past the values: refused by the binding
    with pytest.raises(ValueError):
        api.search_scaled_host(rv, ro, qv, np.array([0, 3, 5], dtype=np.uint64))
    with pytest.raises(ValueError):
        api.search_scaled_host(rv, ro, qv, qo, q_min=[1])                             # one threshold for two queries

    class NoContext(api.Context):
        def __init__(self):
            self._lib = api.load_library()

        def __del__(self):
            pass
    with pytest.raises(ValueError):
        NoContext().scaled_index(rv, np.array([0, 3, 9], dtype=np.uint64))            # before a context is needed
    idx = api.ScaledIndex(NoContext(), api.C.c_void_p())
    with pytest.raises(ValueError):
        idx.search(qv, np.array([0, 3, 5], dtype=np.uint64))
    with pytest.raises(ValueError):
        idx.search(qv, qo, q_min=[1, 2, 3])
    for bad in (dict(ro=np.array([0, 5, 3], dtype=np.uint64)), dict(qo=np.array([0, 4, 2], dtype=np.uint64)), dict(ro=np.array([0], dtype=np.uint64)),
                dict(qo=np.array([0], dtype=np.uint64)), dict(min_shared=0), dict(min_shared=-3), dict(q_min=[1, 0]), dict(q_min=[-2, 5])):
        a = dict(ro=ro, qo=qo, min_shared=1, q_min=None)
        a.update(bad)
        with pytest.raises(api.RkmhError) as e:
            api.search_scaled_host(rv, a["ro"], qv, a["qo"], min_shared=a["min_shared"], q_min=a["q_min"])
        assert e.value.code == -1, bad
    lib = api.load_library()
    out, n = api._i32p(), api.C.c_uint64()
    u64 = api.C.c_uint64
    assert lib.rk_search_scaled_host(None, None, 1, None, None, 1, 1, None, 1, None, None) == -1
    args = (api._p(rv, u64), api._p(ro, u64), 2, api._p(qv, u64), api._p(qo, u64), 2)
    assert lib.rk_search_scaled_host(*args[:2], 1 << 31, *args[3:], 1, None, 1, api.C.byref(out), api.C.byref(n)) == -5   # before the offsets are read
    assert lib.rk_search_scaled_host(*args[:5], 1 << 31, 1, None, 1, api.C.byref(out), api.C.byref(n)) == -5
    assert lib.rk_search_scaled_host(*args, 1, None, 1, api.C.byref(out), None) == -1
    # the entries that need a context refuse a missing one, and an index refuses a NULL handle
    assert lib.rk_scaled_index_create(None, api._p(rv, u64), api._p(ro, u64), 2, api.C.byref(api.C.c_void_p())) == -1
    assert lib.rk_search_scaled(None, None, api._p(qv, u64), api._p(qo, u64), 2, 1, None, api.C.byref(out), api.C.byref(n)) == -1
    assert lib.rk_scaled_index_stats(None, None) == -1
    lib.rk_scaled_index_destroy(None)


# ---- the command, as far as it goes without a GPU ----
def _run(root, *args):
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    return subprocess.run([os.path.join(root, "bin", "rkmh")] + list(args), capture_output=True, env=env)


def test_help_text(root):
    r = _run(root, "manysearch")
    assert r.returncode == 1 and r.stdout == b""
    for word in (b"rkmh manysearch", b"--scaled", b"--min-shared", b"--min-containment", b"-R", b"-Q", b"-g", b"--hash-policy", b"inverted index"):
        assert word in r.stderr, word
    assert b"manysearch" in _run(root).stderr


def _refused(r, *words):
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"rkmh manysearch: "), r.stderr[-300:]
    for w in words:
        assert w.encode() in r.stderr, (w, r.stderr[-300:])


def test_manysearch_refusals(root, tmp_path):
    fa = tmp_path / "x.fa"
    fa.write_text(">x\nACGTACGTACGTACGTACGTACGT\n")
    fa = str(fa)
    sc10 = _sketch_file(tmp_path / "sc10.json", scaled=10)
    sc100 = _sketch_file(tmp_path / "sc100.json", scaled=100)
    bottom = _sketch_file(tmp_path / "bottom.json", length=4)
    ok = ["--scaled", "10", "-k", "16"]
    _refused(_run(root, "manysearch", "-f", fa, *ok), "references")                              # no references
    _refused(_run(root, "manysearch", "-r", fa, "-R", sc10, "-f", fa, *ok), "references")         # both kinds
    _refused(_run(root, "manysearch", "-r", fa, "-f", fa, "-Q", sc10, *ok), "queries")
    _refused(_run(root, "manysearch", "-r", fa, "-f", fa, "-s", "100", *ok), "-s")
    _refused(_run(root, "manysearch", "-r", fa, "-f", fa, "-s", "100", "-k", "16"), "-s")
    _refused(_run(root, "manysearch", "-R", bottom, "-f", fa, *ok), "bottom")
    _refused(_run(root, "manysearch", "-R", sc10, "-Q", bottom), "bottom")
    _refused(_run(root, "manysearch", "-r", fa, "-f", fa, "--abund", *ok), "--abund")
    _refused(_run(root, "manysearch", "-R", sc10, "--abund"), "--abund")
    for bad in ("0", "x", "-2", "3x", ""):
        _refused(_run(root, "manysearch", "-r", fa, "-f", fa, "--min-shared", bad, *ok), "--min-shared")
    for bad in ("-0.1", "1.5", "x", "0.5x", "", "nan", "inf"):
        _refused(_run(root, "manysearch", "-r", fa, "-f", fa, "--min-containment", bad, *ok), "--min-containment")
    _refused(_run(root, "manysearch", "-r", fa, "-f", fa, "--scaled", "0", "-k", "16"), "--scaled")
    _refused(_run(root, "manysearch", "-r", fa, "-f", fa, "--scaled", "ten"), "--scaled")
    _refused(_run(root, "manysearch", "-r", fa, "-f", fa, "--scaled", "10", "-k", "16", "-k", "21"), "one k-mer size")
    _refused(_run(root, "manysearch", "-r", fa, "-f", fa, "-k", "16"), "--scaled")                # nothing says at which scaled
    _refused(_run(root, "manysearch", "-R", sc100, "-f", fa, "--scaled", "10"), "scaled = 100")   # cannot be made finer
    _refused(_run(root, "manysearch", "-R", sc10, "-Q", sc100, "--scaled", "50"), "scaled = 100")
    _refused(_run(root, "manysearch", "-R", sc10, "-f", fa, "--hash-policy", "mash"), "--hash-policy")
    _refused(_run(root, "manysearch", "-R", sc10, "-f", fa, "-k", "21"), "k = 16")
    _refused(_run(root, "manysearch", "-g", "-R", sc10, "-Q", sc10), "-g")
    mixed = _sketch_file(tmp_path / "mixed.json", per_object_scaled=[10, 100])
    _refused(_run(root, "manysearch", "-R", mixed, "-f", fa), "disagree in scaled")


@pytest.mark.parametrize("total", sec.KEY_TOTALS)
def test_key_edge_cases_lie_where_they_say(total):
    """the layout of search_cases.key_edges, read back from the sorted concatenation alone"""
    c = sec.key_edges(total)
    refs = c["refs"]
    assert all((np.diff(r.astype(object)) > 0).all() for r in refs)                  # rows ascend and hold no value twice
    flat = np.sort(np.concatenate(refs))
    assert len(flat) == total
    values, first, count = np.unique(flat, return_index=True, return_counts=True)
    assert len(values) == c["nkeys"] and count.max() == c["longest"] == min(total, 2 + (total >= 67))
    assert {int(f): int(n) for f, n in zip(first, count) if n > 1} == c["runs"]
    if total > 1:
        assert count[0] == 2 and count[-1] == 2                                       # the first and the last value: two references each
    for e in sec.KEY_EDGES:                                                           # a repeated value lies across every edge that is reached
        across = [(int(f), int(n)) for f, n in zip(first, count) if f < e < f + n]
        assert across == ([(e - 2, 3)] if total >= e + 3 else [(e - 1, 2)] if total == e + 1 else []), (total, e)
    want = sem.search(refs, refs)
    assert len(want) >= sum(len(r) > 0 for r in refs)                                 # every reference with a value finds itself
    _same(_host(refs, refs, threads=2), want, total)
    _same(_host(refs, refs, min_shared=2, threads=2), sem.search(refs, refs, 2), (total, 2))
