"""Abundances without a GPU: the model (tests/abund_model.py) against the hand-checked vectors, rk_merge_scaled_abund and
rk_gather_scaled_abund_host against the model, the invariants of include/rkmh_amd.h "ABUNDANCE", what the entries and the binding
refuse, the help texts, every refusal of `sketch --abund` and `gather --abund` (all made before a context exists), the JSON reader's
refusals, and what the bundled sample gives in the model: the floors the GPU tests rest on."""
import json
import os
import subprocess

import numpy as np
import pytest

import abund_cases as ac
import abund_model as am
import gather_cases as gc
import gather_model as gm
import scaled_cases as sc
import scaled_model as scm
from rkmh_amd import api
from test_scaled_cpu import DEFAULT_POLICY

C = api.C


def _same_rows(got, want, what):
    assert got.dtype == np.int32 and got.shape == want.shape and (got == want).all(), (what, got.tolist()[:4], want.tolist()[:4])


def _same_w(got, want, what):
    assert got.dtype == np.uint64 and got.tolist() == [int(x) for x in want], (what, got.tolist()[:4], list(want)[:4])


# ---- the model against the vectors ----
def test_there_are_enough_vectors():
    g, m = ac.gather_kat(), ac.merge_kat()
    names = [v["name"] for v in g + m]
    assert len(g) >= 14 and len(m) >= 10 and len(set(names)) == len(names)
    assert any(len(v["q"]) == 0 for v in g) and any(v["min_shared"] > 1 for v in g) and any(v["max_rounds"] is not None for v in g)
    assert any(v["left"] > 0 for v in g) and any(max(v["wunique"].tolist() + [0]) > (1 << 33) for v in g)
    assert any((v["abund"] == 1).all() and len(v["q"]) for v in g)
    assert any(len(set(v["want"][:, 1].tolist())) < len(v["want"]) for v in g)                              # a tie
    assert any(int(v["want"][t, 1]) < int(v["want"][t, 2]) for v in g for t in range(len(v["want"])))       # values removed by an earlier pick
    assert any(int(v["want_a"].max(initial=0)) == am.SAT and sum(int(p[1].sum()) for p in v["parts"]) > (1 << 32) for v in m)
    assert any(v["max_hash"] != am.FULL for v in m) and any(len(v["parts"]) == 0 for v in m)


@pytest.mark.parametrize("i", range(len(ac.gather_kat())))
def test_model_gather_matches_hand_checked_vectors(i):
    v = ac.gather_kat()[i]
    rows, wu, left = am.gather_weighted(v["q"], v["abund"], v["refs"], v["min_shared"], v["max_rounds"])
    _same_rows(rows, v["want"], v["name"])
    assert wu == v["wunique"].tolist() and left == v["left"], (v["name"], wu, left)
    assert int(v["abund"].astype(np.uint64).sum()) == v["wtotal"] == sum(wu) + left
    _same_rows(gm.gather(v["q"], v["refs"], v["min_shared"], v["max_rounds"]), v["want"], (v["name"], "the rows are the plain ones"))


@pytest.mark.parametrize("i", range(len(ac.merge_kat())))
def test_model_merge_matches_hand_checked_vectors(i):
    v = ac.merge_kat()[i]
    gv, ga = am.merge(v["parts"], v["max_hash"])
    assert gv.tolist() == v["want_v"].tolist() and ga.tolist() == v["want_a"].tolist(), v["name"]
    assert gv.tolist() == scm.merge([p[0] for p in v["parts"]], v["max_hash"]).tolist()


def test_model_lines():
    assert am.gather_line("q", 1, "r", 510, 600, 21888, 1000, 21378, 1309, 25527) == "q\t1\tr\t510/21888\t600/21888\t600/1000\t21378\t1309/25527\t2.56667\n"
    assert am.gather_line("q", 2, "r", 3, 3, 3, 3, 0, 3, 3).endswith("\t3/3\t1\n")


# ---- rk_merge_scaled_abund ----
def _merge(parts, mh=am.FULL):
    v, a, off = ac.csr(parts)
    return api.merge_scaled_abund(v, a, off, mh)


@pytest.mark.parametrize("i", range(len(ac.merge_kat())))
def test_merge_entry_matches_hand_checked_vectors(i):
    v = ac.merge_kat()[i]
    gv, ga = _merge(v["parts"], v["max_hash"])
    assert gv.dtype == np.uint64 and ga.dtype == np.uint32
    assert gv.tolist() == v["want_v"].tolist() and ga.tolist() == v["want_a"].tolist(), v["name"]


@pytest.mark.parametrize("n", [1, 2, 17])
def test_merge_entry_on_random_parts(n):
    rng = np.random.default_rng(70 + n)
    pl = sc.pool(rng, 3000)
    parts = [(s, ac.abundances(rng, len(s))) for s in sc.random_sets(rng, n, pl, first=1000)]
    for mh in (am.FULL, int(np.sort(pl)[len(pl) // 3])):
        wv, wa = am.merge(parts, mh)
        gv, ga = _merge(parts, mh)
        assert gv.tolist() == wv.tolist() and ga.tolist() == wa.tolist(), (n, mh)
        assert gv.tolist() == api.merge_scaled(*scm.csr([p[0] for p in parts]), mh).tolist()          # the values of the plain merge
        assert (ga >= 1).all() and len(gv) > 100
        if n == 1 and mh != am.FULL:                                                                       # a cut is a prefix of both arrays
            full_v, full_a = _merge(parts)
            assert gv.tolist() == full_v[:len(gv)].tolist() and ga.tolist() == full_a[:len(ga)].tolist() and len(gv) < len(full_v)
    if n == 17:
        assert int(am.merge(parts)[1].max()) == am.SAT and sum(int((p[1] == am.SAT).sum()) for p in parts) >= 2              # saturation is reached by sums as well
        many = [(np.array([5], np.uint64), np.array([1 << 31], np.uint32))] * 17
        gv, ga = _merge(many)
        assert gv.tolist() == [5] and ga.tolist() == [am.SAT]


def test_merge_entry_refusals():
    lib = api.load_library()
    v, a, off = np.array([1, 2, 3], np.uint64), np.array([1, 1, 1], np.uint32), np.array([0, 2, 3], np.uint64)
    out, oa, n = api._u64p(), api._u32p(), C.c_uint64()
    pv, pa, po = api._p(v, C.c_uint64), api._p(a, C.c_uint32), api._p(off, C.c_uint64)
    assert lib.rk_merge_scaled_abund(pv, pa, po, 2, am.FULL, C.byref(out), C.byref(oa), C.byref(n)) == 0 and n.value == 3
    lib.rk_free(out)
    lib.rk_free(oa)
    assert lib.rk_merge_scaled_abund(pv, None, po, 2, am.FULL, C.byref(out), C.byref(oa), C.byref(n)) == -1      # NULL abundances
    assert lib.rk_merge_scaled_abund(None, pa, po, 2, am.FULL, C.byref(out), C.byref(oa), C.byref(n)) == -1
    assert lib.rk_merge_scaled_abund(pv, pa, None, 2, am.FULL, C.byref(out), C.byref(oa), C.byref(n)) == -1
    assert lib.rk_merge_scaled_abund(pv, pa, po, -1, am.FULL, C.byref(out), C.byref(oa), C.byref(n)) == -1
    assert lib.rk_merge_scaled_abund(pv, pa, po, 2, am.FULL, None, C.byref(oa), C.byref(n)) == -1
    assert lib.rk_merge_scaled_abund(pv, pa, po, 2, am.FULL, C.byref(out), None, C.byref(n)) == -1
    assert lib.rk_merge_scaled_abund(pv, pa, po, 2, am.FULL, C.byref(out), C.byref(oa), None) == -1
    with pytest.raises(api.RkmhError) as e:
        api.merge_scaled_abund(v, np.array([1, 0, 1], np.uint32), off)                                          # an abundance of 0
    assert e.value.code == -1 and "abundance 0" in str(e.value)
    with pytest.raises(api.RkmhError):
        api.merge_scaled_abund(v, a, np.array([0, 3, 2], np.uint64))                                            # offsets that decrease
    with pytest.raises(ValueError):
        api.merge_scaled_abund(v, a[:2], off)                                                                   # the binding: lengths differ
    with pytest.raises(ValueError):
        api.merge_scaled_abund(v, a, np.array([0, 2, 4], np.uint64))


# ---- rk_gather_scaled_abund_host ----
def _host(q, a, refs, min_shared=1, max_rounds=None, threads=1):
    rv, ro = scm.csr(refs)
    return api.gather_scaled_abund_host(q, a, rv, ro, min_shared=min_shared, max_rounds=max_rounds, threads=threads)


def _plain(q, refs, min_shared=1, max_rounds=None):
    rv, ro = scm.csr(refs)
    return api.gather_scaled_host(q, rv, ro, min_shared=min_shared, max_rounds=max_rounds)


@pytest.mark.parametrize("i", range(len(ac.gather_kat())))
def test_host_entry_matches_hand_checked_vectors(i):
    v = ac.gather_kat()[i]
    for threads in (1, 4):
        rows, wu = _host(v["q"], v["abund"], v["refs"], v["min_shared"], v["max_rounds"], threads)
        _same_rows(rows, v["want"], (v["name"], threads))
        _same_w(wu, v["wunique"], (v["name"], threads))


def _invariants(q, a, refs, rows, wu, what):
    wtotal = int(np.asarray(a, dtype=np.uint64).sum())
    alive = np.ones(len(q), dtype=bool)
    for r in rows[:, 0].tolist():
        alive[np.isin(q, refs[r])] = False
    left = int(np.asarray(a, dtype=np.uint64)[alive].sum())
    assert sum(int(x) for x in wu) + left == wtotal, what
    assert all(int(w) >= int(u) for w, u in zip(wu, rows[:, 1].tolist())), (what, "every abundance is at least 1")
    ones = np.ones(len(q), dtype=np.uint32)
    r1, w1 = _host(q, ones, refs, max_rounds=max(len(rows), 1))
    assert w1.tolist() == r1[:, 1].tolist() and (r1[:len(rows)] == rows).all(), (what, "abundances of 1: wunique = unique")


@pytest.mark.parametrize("nref", gc.NREFS)
def test_host_entry_on_random_sets(nref):
    q, a, refs, want, wunique, left = ac.random_case(nref)
    assert len(want) >= min(3, nref) and int(a.max()) == am.SAT and int((a > 1).sum()) > 50
    assert any(int(w) > int(u) for w, u in zip(wunique.tolist(), want[:, 1].tolist()))                        # the weights matter
    for threads in (1, 4):
        rows, wu = _host(q, a, refs, threads=threads)
        _same_rows(rows, want, (nref, threads))
        _same_rows(rows, _plain(q, refs), (nref, "the plain entry's rows"))
        _same_w(wu, wunique, (nref, threads))
    _invariants(q, a, refs, want, wunique.tolist(), nref)
    for min_shared, max_rounds in ((1, 2), (50, None), (int(want[-1, 1]) + 1, None), (1, 10 ** 6)):
        wr, ww, _ = am.gather_weighted(q, a, refs, min_shared, max_rounds)
        rows, wu = _host(q, a, refs, min_shared, max_rounds, threads=3)
        _same_rows(rows, wr, (nref, min_shared, max_rounds))
        _same_rows(rows, _plain(q, refs, min_shared, max_rounds), (nref, min_shared, max_rounds, "plain"))
        _same_w(wu, ww, (nref, min_shared, max_rounds))


@pytest.mark.parametrize("n", [0, 1, 16, 17, 33])
def test_host_entry_on_staircases(n):
    q, a, refs = ac.staircase(n)
    rows, wu, left = am.gather_weighted(q, a, refs)
    assert len(rows) == n
    got, gw = _host(q, a, refs, threads=4)
    _same_rows(got, rows, n)
    _same_w(gw, wu, n)
    if n == 33:
        cut, cw, _ = am.gather_weighted(q, a, refs, 1, 20)
        got, gw = _host(q, a, refs, max_rounds=20)
        assert len(got) == 20
        _same_rows(got, cut, "max_rounds cuts 33")
        _same_w(gw, cw, "max_rounds cuts 33")


def test_gather_entry_refusals():
    lib = api.load_library()
    q, a = np.arange(1, 9, dtype=np.uint64), np.arange(1, 9, dtype=np.uint32)
    rv, ro = np.arange(1, 7, dtype=np.uint64), np.array([0, 3, 6], dtype=np.uint64)
    rows, wu = api.gather_scaled_abund_host(q, a, rv, ro)
    assert rows.tolist() == [[0, 3, 3, 5], [1, 3, 3, 2]] and wu.tolist() == [6, 15]
    # what the plain host entry refuses, this one refuses
    for bad in (dict(q=q[::-1].copy()), dict(q=np.array([1, 1, 2, 3, 4, 5, 6, 7], dtype=np.uint64)), dict(q=np.arange(0, 8, dtype=np.uint64)),
                dict(ro=np.array([0, 5, 3], dtype=np.uint64)), dict(ro=np.array([0], dtype=np.uint64)), dict(min_shared=0), dict(max_rounds=0),
                dict(min_shared=-3), dict(max_rounds=-1), dict(a=np.array([1, 2, 3, 0, 5, 6, 7, 8], dtype=np.uint32))):
        k = dict(q=q, a=a, ro=ro, min_shared=1, max_rounds=None)
        k.update(bad)
        with pytest.raises(api.RkmhError) as e:
            api.gather_scaled_abund_host(k["q"], k["a"], rv, k["ro"], min_shared=k["min_shared"], max_rounds=k["max_rounds"])
        assert e.value.code == -1, bad
    n = C.c_int(0)
    out, w = np.zeros(8, np.int32), np.zeros(2, np.uint64)
    pq, pa, prv, pro = api._p(q, C.c_uint64), api._p(a, C.c_uint32), api._p(rv, C.c_uint64), api._p(ro, C.c_uint64)
    po, pw = api._p(out, C.c_int32), api._p(w, C.c_uint64)
    assert lib.rk_gather_scaled_abund_host(pq, pa, 8, prv, pro, 2, 1, 2, 1, po, pw, C.byref(n)) == 0 and n.value == 2 and w.tolist() == [6, 15]
    assert lib.rk_gather_scaled_abund_host(pq, None, 8, prv, pro, 2, 1, 2, 1, po, pw, C.byref(n)) == -1        # NULL abundances of a query that has values
    assert lib.rk_gather_scaled_abund_host(pq, pa, 8, prv, pro, 2, 1, 2, 1, po, None, C.byref(n)) == -1        # NULL wunique
    assert lib.rk_gather_scaled_abund_host(None, None, 0, prv, pro, 2, 1, 2, 1, po, pw, C.byref(n)) == 0 and n.value == 0   # an empty query needs neither
    assert lib.rk_gather_scaled_abund_host(pq, pa, 1 << 31, prv, pro, 2, 1, 1, 1, po, pw, C.byref(n)) == -5
    assert lib.rk_gather_scaled_abund_host(pq, pa, 8, prv, pro, 2, 1, 2, 1, None, pw, C.byref(n)) == -1
    # the entry that needs a context makes its own checks of q_abund and wunique first, then refuses the missing context
    assert lib.rk_gather_scaled_abund(None, pq, None, 8, prv, pro, 2, 1, 2, po, pw, C.byref(n)) == -1
    assert lib.rk_gather_scaled_abund(None, pq, pa, 8, prv, pro, 2, 1, 2, po, None, C.byref(n)) == -1
    assert lib.rk_gather_scaled_abund(None, pq, pa, 8, prv, pro, 2, 1, 2, po, pw, C.byref(n)) == -1
    assert lib.rk_gather_scaled_abund_device(None, 8, None, 8, 8, 8, 2, 6, 1, 2, 8, 8, C.byref(n), None) == -1
    assert lib.rk_gather_scaled_abund_device(None, 8, 8, 8, 8, 8, 2, 6, 1, 2, 8, None, C.byref(n), None) == -1


def test_binding_refusals():
    q, a = np.arange(1, 9, dtype=np.uint64), np.arange(1, 9, dtype=np.uint32)
    rv, ro = np.arange(1, 7, dtype=np.uint64), np.array([0, 3, 6], dtype=np.uint64)

    class NoContext(api.Context):
        def __init__(self):
            pass

        def __del__(self):
            pass
    for short in (a[:7], np.zeros(0, np.uint32), np.ones(9, np.uint32), np.ones((8, 1), np.uint32)):
        with pytest.raises(ValueError):
            api.gather_scaled_abund_host(q, short, rv, ro)
        with pytest.raises(ValueError):
            NoContext().gather_scaled_abund(q, short, rv, ro)                      # before a context is needed
    with pytest.raises(ValueError):
        api.gather_scaled_abund_host(q, a, rv, np.array([0, 3, 9], dtype=np.uint64))
    for name in ("sketch_scaled_abund_batch", "gather_scaled_abund", "gather_scaled_abund_device"):
        assert callable(getattr(api.Context, name))


# ---- the commands, as far as they go without a GPU ----
def _run(root, *args):
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    return subprocess.run([os.path.join(root, "bin", "rkmh")] + list(args), capture_output=True, env=env)


def test_help_texts(root):
    r = _run(root, "gather")
    assert r.returncode == 1 and r.stdout == b""
    for word in (b"--abund", b"wunique/wtotal", b"mean", b"wunique / unique", b"sketch --scaled <m> --abund"):
        assert word in r.stderr, word
    r = _run(root, "sketch")
    assert r.returncode == 1 and r.stdout == b""
    for word in (b"--abund", b"abundances", b"--scaled"):
        assert word in r.stderr, word


def _abund_file(path, abund="same", scaled=10, hashes=(3, 9, 20), n=2, drop_in=None):
    """a file of n scaled sketches; abund: a list for every object's "abundances", "same": ones, None: no key"""
    doc = []
    for i in range(n):
        h = [int(x) for x in hashes]
        sk = {"comment": "", "hashes": h, "length": len(h), "name": "s%d" % i}
        if abund is not None and i != drop_in:
            sk["abundances"] = [1] * len(h) if isinstance(abund, str) else abund
        doc.append({"alphabet": "ATGC", "canonical": "true", "hashBits": 64, "hashPolicy": DEFAULT_POLICY, "hashSeed": 42, "hashType": "MurmurHash3_x64_128",
                    "kmer": "16", "maxHash": scm.max_hash(scaled), "name": "s%d" % i, "preserveCase": "false", "scaled": scaled, "seqLen": 100, "sketches": sk})
    path.write_text(json.dumps(doc, separators=(",", ":"), sort_keys=True))
    return str(path)


def _refused(r, command, *words):
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"rkmh " + command + b": "), r.stderr[-300:]
    for w in words:
        assert w.encode() in r.stderr, (w, r.stderr[-300:])


def test_sketch_abund_refusals(root, tmp_path):
    fa = tmp_path / "x.fa"
    fa.write_text(">x\nACGTACGTACGTACGTACGTACGT\n")
    for extra in ([], ["-s", "100"], ["-g"], ["-k", "16"]):
        r = _run(root, "sketch", "--abund", "-f", str(fa), "-k", "16", *extra)
        assert r.returncode == 1 and r.stdout == b"" and b"rkmh sketch: --abund" in r.stderr and b"--scaled" in r.stderr, (extra, r.stderr[-300:])
    r = _run(root, "sketch", "--abund", "--scaled", "0", "-f", str(fa), "-k", "16")
    assert r.returncode == 1 and r.stdout == b"" and b"--scaled takes" in r.stderr


def test_gather_abund_refusals_and_the_json_reader(root, tmp_path):
    fa = tmp_path / "x.fa"
    fa.write_text(">x\nACGTACGTACGTACGTACGTACGT\n")
    fa = str(fa)
    refs = _abund_file(tmp_path / "refs.json", None)
    good = _abund_file(tmp_path / "good.json", [1, 7, 4294967295])
    # -Q files without abundances
    plain = _abund_file(tmp_path / "plain.json", None)
    _refused(_run(root, "gather", "--abund", "-R", refs, "-Q", plain), b"gather", "plain.json", "holds no abundances", "sketch --scaled")
    _refused(_run(root, "gather", "--abund", "-R", refs, "-Q", good, "-Q", plain), b"gather", "plain.json", "holds no abundances")
    _refused(_run(root, "gather", "--abund", "-r", fa, "-Q", plain, "--scaled", "10"), b"gather", "holds no abundances")
    # what gather refuses, it refuses with --abund as well
    _refused(_run(root, "gather", "--abund", "-R", refs, "-f", fa, "-Q", good), b"gather", "queries")
    _refused(_run(root, "gather", "--abund", "-R", refs), b"gather", "queries")
    _refused(_run(root, "gather", "--abund", "-f", fa, "--scaled", "10"), b"gather", "references")
    _refused(_run(root, "gather", "--abund", "-r", fa, "-f", fa, "-s", "100"), b"gather", "-s")
    _refused(_run(root, "gather", "--abund", "-R", refs, "-Q", good, "--scaled", "5"), b"gather", "scaled = 10")
    # the reader: a length that differs from "hashes", entries outside 1 .. 2^32 - 1, things that are no numbers, a file that disagrees in itself
    for i, bad in enumerate(([1, 2], [1, 2, 3, 4], [], [1, 0, 3], [1, 4294967296, 3], [1, 18446744073709551616, 3], [1, -2, 3], [1, 2.5, 3], [1, "x", 3], 7)):
        f = _abund_file(tmp_path / ("bad%d.json" % i), bad)
        _refused(_run(root, "gather", "--abund", "-R", refs, "-Q", f), b"gather", "bad%d.json" % i, "abundances", "2^32 - 1")
        _refused(_run(root, "gather", "-R", refs, "-Q", f), b"gather", "bad%d.json" % i, "abundances")      # a malformed file is refused by every reader
        _refused(_run(root, "dist", "-R", refs, "-Q", f), b"dist", "bad%d.json" % i, "abundances")
    half = _abund_file(tmp_path / "half.json", "same", drop_in=1)
    _refused(_run(root, "gather", "--abund", "-R", refs, "-Q", half), b"gather", "half.json", "disagree")
    half0 = _abund_file(tmp_path / "half0.json", "same", drop_in=0)
    _refused(_run(root, "gather", "--abund", "-R", refs, "-Q", half0), b"gather", "half0.json", "disagree")


# ---- what the bundled sample gives in the model: the floors of the GPU tests ----
@pytest.mark.parametrize("scaled,nvalues,windows,above1,largest,nrows,first", [(10, 21888, 25527, 2020, 10, 17, (28, 510, 1309)),
                                                                               (100, 2296, 2658, None, None, 7, (None, 57, 140))])
def test_bundled_sample_in_the_model(scaled, nvalues, windows, above1, largest, nrows, first):
    v, a = ac.z1_query(scaled)
    assert len(v) == nvalues and int(a.sum()) == windows
    if above1 is not None:
        assert int((a > 1).sum()) == above1 and int(a.max()) == largest
    assert int((a > 1).sum()) > 0
    refs = sc.sketches("zika-k16", scaled)
    rows, wu, left = am.gather_weighted(v, a, refs)
    assert len(rows) == nrows and int(rows[0, 1]) == first[1] and wu[0] == first[2]
    if first[0] is not None:
        assert int(rows[0, 0]) == first[0]
    assert sum(wu) + left == windows
    v10, a10 = ac.z1_query(10)
    dv, da = am.downsample(v10, a10, scm.max_hash(scaled))                  # cutting the finer sketch gives the coarser one
    assert dv.tolist() == v.tolist() and da.tolist() == a.tolist()
