"""Weighted comparison without a GPU: tests/wdist_model.py against the hand-checked vectors, the host entries
(rk_compare_scaled_abund_host, rk_abund_row_sums_host, rk_angular_similarity) against the model, every refusal of the entries, the
bindings and `rkmh dist --abund`, and what the bundled files give in the model -- the floors of tests/test_gpu_wdist.py."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import scaled_cases as sc
import scaled_model as scm
import wdist_cases as wc
import wdist_model as wm
from rkmh_amd import api

U64, SAT = wm.U64, wm.SAT


# ---- the model against the vectors ----
def test_there_are_enough_vectors():
    kat = wc.pair_kat()
    assert len(kat) >= 20 and len(wc.sim_kat()) >= 6
    names = " | ".join(v["name"] for v in kat)
    for word in ("empty", "disjoint", "identical", "first of both", "last of both", "first of a and the last of b", "last of a and the first of b",
                 "b shorter than a", "dot saturates", "sumsq of a saturates"):
        assert word in names, word
    assert any(v["want"][1] == U64 for v in kat) and any(v["sums_a"][1] == U64 for v in kat)


def test_model_against_vectors():
    for v in wc.pair_kat():
        assert wm.pair(v["a"], v["b"]) == v["want"], v["name"]
        assert wm.pair(v["b"], v["a"]) == wm.mirror(v["want"]), v["name"]
        assert wm.row_sums(v["a"][1]) == v["sums_a"] and wm.row_sums(v["b"][1]) == v["sums_b"], v["name"]
        both = wm.all_pairs([v["a"], v["b"]])
        assert tuple(both[0, 1].tolist()) == v["want"] and tuple(both[1, 0].tolist()) == wm.mirror(v["want"])
        assert tuple(both[0, 0].tolist()) == (len(v["a"][0]), v["sums_a"][1], v["sums_a"][0], v["sums_a"][0]), v["name"]
    for v in wc.sim_kat():
        c, a = wm.similarity(v["dot"], v["sumsq_a"], v["sumsq_b"])
        assert c == v["cosine"] and abs(a - v["angular"]) <= 1e-15, v["name"]
        if v["angular"] in (0.0, 1.0):
            assert a == v["angular"], v["name"]


def test_model_line():
    q = (np.array([3, 6], np.uint64), np.array([10, 20], np.uint32))
    r = (np.array([2, 3, 4, 6, 9], np.uint64), np.array([1, 5, 1, 7, 1], np.uint32))
    line = wm.dist_text(["ref"], [r], ["query"], [q], 16)
    cos = 190 / math.sqrt(500.0 * 77.0)
    assert line == scm.dist_line("ref", "query", 2, 2, 5, 16)[:-1] + "\t%.6g\t30/30\t12/15\n" % (1 - 2 * math.acos(cos) / math.pi)
    assert line.count("\t") == 8 and line.split("\t")[:6] == scm.dist_line("ref", "query", 2, 2, 5, 16)[:-1].split("\t")
    assert wm.dist_text(["ref"], [r], ["query"], [q], 16, max_dist=0.0) == "" and wm.dist_text(["ref"], [r], ["query"], [q], 16, max_dist=1.0) == line


# ---- the host entries against the model ----
def _host_pairs(A, B, threads=1, self_form=False):
    av, aw, ao = wm.csr(A)
    if self_form:
        return api.compare_scaled_abund_host(av, aw, ao, threads=threads)
    bv, bw, bo = wm.csr(B)
    return api.compare_scaled_abund_host(av, aw, ao, bv, bw, bo, threads=threads)


def _host_sums(A):
    _, w, off = wm.csr(A)
    return api.abund_row_sums_host(w, off)


def _same(got, want, what):
    assert got.dtype == np.uint64 and got.shape == want.shape and (got == want).all(), (what, got.reshape(-1, got.shape[-1])[:3].tolist(), want.reshape(-1, want.shape[-1])[:3].tolist())


@pytest.mark.parametrize("threads", [1, 2, 16])
def test_host_entries_on_the_vectors(threads):
    kat = wc.pair_kat()
    for v in kat:
        _same(_host_pairs([v["a"]], [v["b"]], threads), np.array([[v["want"]]], dtype=np.uint64), v["name"])
        _same(_host_pairs([v["b"]], [v["a"]], threads), np.array([[wm.mirror(v["want"])]], dtype=np.uint64), (v["name"], "mirror"))
        _same(_host_sums([v["a"], v["b"]]), np.array([v["sums_a"], v["sums_b"]], dtype=np.uint64), v["name"])
    rows = [v["a"] for v in kat] + [v["b"] for v in kat]                      # every row against every row, itself among them
    want = wm.all_pairs(rows)
    _same(_host_pairs(rows, rows, threads), want, "all vectors")
    _same(_host_pairs(rows, None, threads, self_form=True), want, "all vectors, self form")


@pytest.mark.parametrize("threads", [1, 2, 16])
@pytest.mark.parametrize("shape", [(1, 1), (7, 8), (9, 65), (65, 3)])
def test_host_entries_on_random_sets(shape, threads):
    A, B, want = wc.random_case(*shape)
    assert int((want[:, :, 0] > 0).sum()) > 0 or shape == (1, 1)
    _same(_host_pairs(A, B, threads), want, shape)
    _same(_host_sums(A), wm.all_row_sums(A), shape)
    _same(_host_sums(B), wm.all_row_sums(B), shape)


def test_host_entries_long_row_and_self_form():
    A, B, want = wc.random_case(3, 5, long_row=True)
    assert len(A[0][0]) == sc.LONG_ROW and int(want[0, :, 0].max()) > 100 and int((want[:, :, 1] == U64).sum()) > 0     # a dot that saturates
    _same(_host_pairs(A, B, 16), want, "long row")
    A, _, want = wc.random_case(9, 9, self_form=True)
    _same(_host_pairs(A, None, 2, self_form=True), want, "self form")
    _same(_host_pairs(A, A, 2), want, "the same sets as two sides")


def test_the_three_consequences():
    A, B, want = wc.random_case(7, 8)
    ones = lambda S: [(v, np.ones(len(v), np.uint32)) for v, _ in S]
    plain = scm.all_shared([v for v, _ in A], [v for v, _ in B]).astype(np.uint64)
    got = _host_pairs(ones(A), ones(B))
    for f in range(4):                                                          # all abundances 1: every field is `shared`
        assert (got[:, :, f] == plain).all(), f
    assert (want[:, :, 0] == plain).all()                                       # field 0 never depends on the abundances
    back = _host_pairs(B, A)                                                    # swapping the sides swaps fields 2 and 3
    assert (back.transpose(1, 0, 2)[:, :, [0, 1, 3, 2]] == want).all() and (want[:, :, 2] != want[:, :, 3]).any()
    own = _host_pairs(A, None, self_form=True)                                  # a sketch against itself
    sums = _host_sums(A)
    for i, (v, _) in enumerate(A):
        assert own[i, i].tolist() == [len(v), int(sums[i, 1]), int(sums[i, 0]), int(sums[i, 0])], i


# ---- the angular similarity ----
def _triples():
    out = [(v["dot"], v["sumsq_a"], v["sumsq_b"]) for v in wc.sim_kat()]
    for shape in ((7, 8), (9, 65)):
        A, B, want = wc.random_case(*shape)
        sa, sb = wm.all_row_sums(A), wm.all_row_sums(B)
        out += [(int(want[i, j, 1]), int(sa[i, 1]), int(sb[j, 1])) for i in range(len(A)) for j in range(len(B))]
    for v in wc.pair_kat():
        out.append((v["want"][1], v["sums_a"][1], v["sums_b"][1]))
    out += [(1, 1, U64), (U64 - 1, U64, U64 - 1), ((1 << 53) + 1, (1 << 53) + 1, (1 << 53) + 3), (3, 5, 7), (10 ** 18, 10 ** 18 + 1, 10 ** 18 + 2)]
    return out


def test_angular_similarity_against_the_model():
    t = _triples()
    assert len(t) > 600 and sum(1 for d, a, b in t if 0 < d < U64) > 50
    between = 0
    for dot, sa, sb in t:
        c, a = api.angular_similarity(dot, sa, sb)
        wc_, wa_ = wm.similarity(dot, sa, sb)
        assert c == wc_, (dot, sa, sb, c, wc_)                                 # bit-equal: the same IEEE operations in the same order
        assert abs(a - wa_) <= 1e-15, (dot, sa, sb, a, wa_)                     # both call the same libm: one last-place difference at the most
        assert 0.0 <= c <= 1.0 and 0.0 <= a <= 1.0
        between += 0.0 < a < 1.0
    assert between > 50


def test_a_sketch_against_itself_is_exactly_one():
    for s in ((1 << 53) + 1, (1 << 53) + 3, (1 << 60) + 12345, (1 << 63) + 1, U64 - 1, U64, 3, 14, 10 ** 18 + 7):
        assert api.angular_similarity(s, s, s) == (1.0, 1.0), s
        assert wm.similarity(s, s, s) == (1.0, 1.0), s
    big = (np.array([5, 9], np.uint64), np.array([SAT, SAT - 1], np.uint32))    # (2^32 - 1)^2 + (2^32 - 2)^2 > 2^64: sumsq and dot saturate alike
    own = _host_pairs([big], None, self_form=True)[0, 0]
    sums = _host_sums([big])[0]
    assert int(own[1]) == int(sums[1]) == U64 > (1 << 53)
    assert api.angular_similarity(int(own[1]), int(sums[1]), int(sums[1])) == (1.0, 1.0)
    mid = (np.array([5, 9], np.uint64), np.array([1 << 27, (1 << 27) + 1], np.uint32))     # sumsq = 2^55 + 2^28 + 1: above 2^53, not saturated, odd
    own, sums = _host_pairs([mid], None, self_form=True)[0, 0], _host_sums([mid])[0]
    assert int(own[1]) == int(sums[1]) == (1 << 55) + (1 << 28) + 1
    assert api.angular_similarity(int(own[1]), int(sums[1]), int(sums[1])) == (1.0, 1.0)


def test_angular_similarity_edges():
    lib = api.load_library()
    assert api.angular_similarity(0, 0, 0) == (0.0, 0.0) and api.angular_similarity(0, 0, 9) == (0.0, 0.0) and api.angular_similarity(0, 9, 0) == (0.0, 0.0)
    for bad in ((1, 0, 5), (1, 5, 0), (U64, 0, 0)):
        with pytest.raises(api.RkmhError) as e:
            api.angular_similarity(*bad)
        assert e.value.code == -1, bad
    c, a = C.c_double(-1), C.c_double(-1)
    assert lib.rk_angular_similarity(1, 2, 2, None, C.byref(a)) == 0 and abs(a.value - 1 / 3) <= 1e-15          # either pointer may be NULL
    assert lib.rk_angular_similarity(1, 2, 2, C.byref(c), None) == 0 and c.value == 0.5
    assert lib.rk_angular_similarity(1, 2, 2, None, None) == 0


# ---- refusals of the entries and the bindings ----
def test_entry_refusals():
    lib = api.load_library()
    v, w = np.array([1, 2, 3, 4], np.uint64), np.array([1, 2, 3, 4], np.uint32)
    off, down, wide = np.array([0, 2, 4], np.uint64), np.array([0, 3, 1], np.uint64), np.array([0, 1 << 31, 1 << 31], np.uint64)
    w0 = np.array([1, 2, 0, 4], np.uint32)
    out = np.zeros(16, np.uint64)
    pv, pw, po, pd, pwide, pw0, pout = (api._p(x, t) for x, t in ((v, C.c_uint64), (w, C.c_uint32), (off, C.c_uint64), (down, C.c_uint64), (wide, C.c_uint64),
                                                                   (w0, C.c_uint32), (out, C.c_uint64)))
    host = lib.rk_compare_scaled_abund_host
    assert host(pv, pw, po, 2, pv, pw, po, 2, 1, pout) == 0 and out[:4].tolist() == [2, 5, 3, 3] and out[4:8].tolist() == [0, 0, 0, 0]
    for args in ((pv, None, po, 2, pv, pw, po, 2, 1, pout), (pv, pw, po, 2, pv, None, po, 2, 1, pout),            # NULL abundances where there are values
                 (None, pw, po, 2, pv, pw, po, 2, 1, pout), (pv, pw, None, 2, pv, pw, po, 2, 1, pout), (pv, pw, po, 2, pv, pw, None, 2, 1, pout),
                 (pv, pw, po, 2, pv, pw, po, 2, 1, None), (pv, pw, po, 0, pv, pw, po, 2, 1, pout), (pv, pw, po, 2, pv, pw, po, -1, 1, pout),
                 (pv, pw, pd, 2, pv, pw, po, 2, 1, pout), (pv, pw, po, 2, pv, pw, pd, 2, 1, pout),                  # offsets that decrease
                 (pv, pw, pwide, 2, pv, pw, po, 2, 1, pout),                                                       # a row of 2^31 values
                 (pv, pw0, po, 2, pv, pw, po, 2, 1, pout), (pv, pw, po, 2, pv, pw0, po, 2, 1, pout)):              # an abundance of 0
        assert host(*args) == -1, args
    empty = np.zeros(3, np.uint64)
    assert host(None, None, api._p(empty, C.c_uint64), 2, pv, pw, po, 2, 0, pout) == 0 and not out[:16].any()      # empty sketches need no arrays
    sums = lib.rk_abund_row_sums_host
    o2 = np.zeros(4, np.uint64)
    p2 = api._p(o2, C.c_uint64)
    assert sums(pw, po, 2, p2) == 0 and o2.tolist() == [3, 5, 7, 25]
    for args in ((None, po, 2, p2), (pw, None, 2, p2), (pw, po, 2, None), (pw, po, 0, p2), (pw, pd, 2, p2), (pw, pwide, 2, p2), (pw0, po, 2, p2)):
        assert sums(*args) == -1, args
    # the entries that need a context refuse a missing one like everything else, before anything is launched
    assert lib.rk_compare_scaled_abund(None, pv, pw, po, 2, pv, pw, po, 2, 0, pout) == -1
    assert lib.rk_compare_scaled_abund_device(None, 8, 8, 8, 2, 4, 8, 8, 8, 2, 4, 0, 8, None) == -1
    assert lib.rk_abund_row_sums(None, pw, po, 2, p2) == -1
    assert lib.rk_abund_row_sums_device(None, 8, 8, 2, 4, 8, None) == -1


def test_binding_refusals():
    v, w = np.arange(1, 9, dtype=np.uint64), np.arange(1, 9, dtype=np.uint32)
    off = np.array([0, 3, 8], dtype=np.uint64)

    class NoContext(api.Context):
        def __init__(self):
            pass

        def __del__(self):
            pass
    for short in (w[:7], np.zeros(0, np.uint32), np.ones(9, np.uint32), np.ones((8, 1), np.uint32)):
        for call in (lambda: api.compare_scaled_abund_host(v, short, off), lambda: api.compare_scaled_abund_host(v, w, off, v, short, off),
                     lambda: NoContext().compare_scaled_abund(v, short, off), lambda: NoContext().compare_scaled_abund(v, w, off, v, short, off)):
            with pytest.raises(ValueError):
                call()                                                         # before a context is needed
    past = np.array([0, 3, 9], dtype=np.uint64)
    for call in (lambda: api.compare_scaled_abund_host(v, w, past), lambda: api.compare_scaled_abund_host(v, w, off, v, w, past),
                 lambda: NoContext().compare_scaled_abund(v, w, past), lambda: api.abund_row_sums_host(w, past), lambda: NoContext().abund_row_sums(w, past),
                 lambda: api.compare_scaled_abund_host(v, w, off, None, w, off)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(api.RkmhError):
        api.compare_scaled_abund_host(v, np.zeros(8, np.uint32), off)
    for name in ("compare_scaled_abund", "compare_scaled_abund_device", "abund_row_sums", "abund_row_sums_device"):
        assert callable(getattr(api.Context, name))


# ---- the command, as far as it goes without a GPU ----
def _run(root, *args):
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    return subprocess.run([os.path.join(root, "bin", "rkmh")] + list(args), capture_output=True, env=env)


def test_help_texts(root):
    r = _run(root, "dist")
    assert r.returncode == 1 and r.stdout == b""
    for word in (b"--abund", b"angular", b"wq_in/wq_total", b"wr_in/wr_total", b"acos", b"sketch --scaled <m> --abund", b"-d still filters on the distance"):
        assert word in r.stderr, word
    r = _run(root, "sketch")
    assert r.returncode == 1 and r.stdout == b"" and b"`rkmh gather --abund -Q` and `rkmh dist --abund -R / -Q` need them, every other reader ignores them" in r.stderr


DEFAULT_POLICY = "fold=swap32,windows=len-k,zero=count,mask=lt,freqmax=incl,seed=42"


def _file(path, abund=None, scaled=10, hashes=(3, 9, 20), n=2):
    """a file of n sketches; scaled: None for bottom-s ones; abund: every object's "abundances", None: no key"""
    doc = []
    for i in range(n):
        h = [int(x) for x in hashes]
        sk = {"comment": "", "hashes": h, "length": len(h) if scaled else 4, "name": "s%d" % i}
        if abund is not None:
            sk["abundances"] = abund
        d = {"alphabet": "ATGC", "canonical": "true", "hashBits": 64, "hashPolicy": DEFAULT_POLICY, "hashSeed": 42, "hashType": "MurmurHash3_x64_128",
             "kmer": "16", "name": "s%d" % i, "preserveCase": "false", "seqLen": 100, "sketches": sk}
        if scaled:
            d.update(scaled=scaled, maxHash=scm.max_hash(scaled))
        doc.append(d)
    path.write_text(json.dumps(doc, separators=(",", ":"), sort_keys=True))
    return str(path)


def _refused(r, *words):
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"rkmh dist: "), r.stderr[-300:]
    for w in words:
        assert w.encode() in r.stderr, (w, r.stderr[-300:])


def test_dist_abund_refusals(root, tmp_path):
    fa = tmp_path / "x.fa"
    fa.write_text(">x\nACGTACGTACGTACGTACGTACGT\n")
    fa = str(fa)
    good = _file(tmp_path / "good.json", [1, 7, 4294967295])
    plain = _file(tmp_path / "plain.json")
    bottom = _file(tmp_path / "bottom.json", scaled=None)
    how = "rkmh sketch --scaled <n> --abund"
    # with -s, whatever else is given
    _refused(_run(root, "dist", "--abund", "-s", "100", "-r", fa), "--abund", "-s")
    _refused(_run(root, "dist", "--abund", "-s", "4", "-R", bottom), "--abund", "-s")
    # a run that is not scaled at all
    _refused(_run(root, "dist", "--abund", "-r", fa), "--abund", "--scaled")
    _refused(_run(root, "dist", "--abund", "-r", fa, "-f", fa, "-k", "16"), "--abund", "--scaled")
    # bottom-s files
    _refused(_run(root, "dist", "--abund", "-R", bottom), "bottom.json", "bottom-s", how)
    _refused(_run(root, "dist", "--abund", "-R", good, "-Q", bottom), "bottom.json", "bottom-s")
    _refused(_run(root, "dist", "--abund", "--scaled", "10", "-r", fa, "-Q", bottom), "bottom.json", "bottom-s")
    # -R or -Q files without abundances: the message names the file and how to make one
    _refused(_run(root, "dist", "--abund", "-R", plain), "plain.json", "holds no abundances", how)
    _refused(_run(root, "dist", "--abund", "-R", plain, "-Q", good), "plain.json", "holds no abundances", how)
    _refused(_run(root, "dist", "--abund", "-R", good, "-Q", plain), "plain.json", "holds no abundances", how)
    _refused(_run(root, "dist", "--abund", "-R", good, "-R", plain), "plain.json", "holds no abundances", how)
    _refused(_run(root, "dist", "--abund", "--scaled", "10", "-r", fa, "-Q", plain), "plain.json", "holds no abundances", how)
    # what dist refuses, it refuses with --abund as well
    _refused(_run(root, "dist", "--abund", "--scaled", "0", "-r", fa), "--scaled")
    _refused(_run(root, "dist", "--abund", "--scaled", "5", "-R", good), "scaled = 10")
    _refused(_run(root, "dist", "--abund", "-R", good, "-r", fa), "references")
    _refused(_run(root, "dist", "--abund", "-R", good, "-Q", good, "-f", fa), "queries")
    _refused(_run(root, "dist", "--abund", "-g", "-R", good), "-g")
    _refused(_run(root, "dist", "--abund", "-R", _file(tmp_path / "zero.json", [1, 0, 3])), "zero.json", "abundances")
    # and gather's wording for its own refusal is what it was
    r = _run(root, "gather", "--abund", "-R", good, "-Q", plain)
    assert r.returncode == 1 and r.stdout == b"" and b"--abund needs query sketches of `rkmh sketch --scaled <n> --abund`" in r.stderr


# ---- what the bundled files give in the model: the floors of the GPU tests ----
# (policy file, scaled) -> sketches, values in all, sketches with an abundance above 1, ordered pairs of different sketches that share a value
# and both hold an abundance above 1, ordered pairs of different sketches with dot != shared
FLOORS = {
    (('pave', 'default'), 10): (40, 58771, 39, 1480, 432),
    (('pave', 'default'), 100): (40, 6245, 18, 228, 138),
    (('pave', 'sourmash'), 10): (40, 30873, 10, 34, 30),
    (('pave', 'sourmash'), 100): (40, 3041, 1, 0, 0),
    (('zika', 'default'), 10): (60, 118119, 1, 0, 118),
    (('zika', 'default'), 100): (60, 10938, 1, 0, 2),
    (('zika', 'sourmash'), 10): (60, 63556, 1, 0, 116),
    (('zika', 'sourmash'), 100): (60, 7421, 1, 0, 2),
}


@pytest.mark.parametrize("key,scaled", [(k, s) for k in sorted(wc.FILES) for s in (10, 100)])
def test_bundled_files_in_the_model(key, scaled):
    A = wc.file_sketches(key, scaled)
    want = wm.all_pairs(A)
    n = len(A)
    off = ~np.eye(n, dtype=bool)
    heavy = np.array([int((a > 1).sum()) > 0 for _, a in A])
    both_heavy = int(((want[:, :, 0] > 0) & off & heavy[:, None] & heavy[None, :]).sum())
    weighted = int(((want[:, :, 1] != want[:, :, 0]) & off).sum())
    figures = (n, sum(len(v) for v, _ in A), int(heavy.sum()), both_heavy, weighted)
    assert figures == FLOORS[(key, scaled)], figures


def test_the_floors_are_not_vacuous():
    """the command's GPU tests compare these files: pairs in which both sides carry an abundance above 1 and share a value, and pairs
    whose dot differs from shared, exist under both policies and in both files (the zika records repeat few k-mers: one sketch there
    holds an abundance above 1, so its weighted pairs are that sketch's)"""
    assert sum(f[3] for f in FLOORS.values()) >= 1 and sum(f[4] for f in FLOORS.values()) >= 1
    for name in ("pave", "zika"):
        for pol in ("default", "sourmash"):
            assert FLOORS[((name, pol), 10)][4] >= 30, (name, pol)
    assert FLOORS[(("pave", "default"), 10)][3] >= 1000 and FLOORS[(("pave", "sourmash"), 10)][3] >= 30
