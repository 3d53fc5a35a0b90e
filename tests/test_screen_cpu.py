"""Screen without a GPU (include/rkmh_amd.h "SCREEN"): the pure-Python model (tests/screen_model.py), the hand-checked vectors
(tests/golden/screen_kat.json) and the library's host code (rk_screen_rows_host, rk_screen_identity) agree; the invariants the header
states hold on random small inputs; every host refusal and every refusal of `rkmh screen` is a sentence; and the shared inputs
(tests/screen_cases.py) hold what tests/test_gpu_screen.py relies on."""
import json
import os
import subprocess

import numpy as np
import pytest

import screen_cases as cs
import screen_model as scm
import sourmash_model as sm
from rkmh_amd import api


@pytest.fixture(scope="module")
def vectors(golden_dir):
    return json.load(open(os.path.join(golden_dir, "screen_kat.json")))["vectors"]


def _host(rows, counts, m):
    v, off = scm.to_csr(rows)
    cv, cc = cs.counted_arrays(counts)
    return api.screen_rows_host(v, off, cv, cc, m).tolist()


def test_vectors_model_and_host_code(vectors):
    names = {v["name"] for v in vectors}
    assert len(vectors) >= 12 and len(names) == len(vectors)
    for v in vectors:
        counts = dict(zip(v["values"], v["counts"]))
        assert scm.rows(v["rows"], counts, v["m"]) == v["out4"], v["name"]
        assert _host(v["rows"], counts, v["m"]) == v["out4"], v["name"]
    # what the vectors are there to pin
    by = {v["name"]: v for v in vectors}
    assert by["even_shared_lower_median"]["out4"][0][0] % 2 == 0 and by["odd_shared"]["out4"][0][0] % 2 == 1
    assert max(by["saturated_counts"]["counts"]) > scm.SAT and by["saturated_counts"]["out4"][0][1] == scm.SAT
    assert by["identical_references"]["rows"][0] == by["identical_references"]["rows"][1]
    assert by["empty_counted_set"]["values"] == []


@pytest.mark.parametrize("seed", range(12))
def test_invariants_on_random_inputs(seed):
    rows, counts = cs.random_pair(seed)
    for m in (1, 2, 3):
        out = scm.rows(rows, counts, m)
        assert _host(rows, counts, m) == out, (seed, m)
        assert all(r[2] <= r[0] for r in out)
        assert sum(r[2] for r in out) == scm.present_keys(rows, counts, m)
        lens = [len(scm.collapse(r)) for r in rows]
        ratios = [(out[i][0] / lens[i]) if lens[i] else 0.0 for i in range(len(rows))]
        best = max(range(len(rows)), key=lambda i: (ratios[i], -i))
        if out[best][0]:
            assert out[best][2] == out[best][0] and out[best][3] == out[best][1], (seed, m, best)
        # feeding twice doubles every count: at 2 m the doubled set gives the rows of the single one at m, medians doubled
        twice = scm.rows(rows, {v: 2 * c for v, c in counts.items()}, 2 * m)
        assert [[r[0], 2 * r[1], r[2], 2 * r[3]] for r in out] == twice
    # a reference given twice: the second copy owns nothing
    dup = scm.rows(rows + [rows[0]], counts, 1)
    assert dup[-1][0] == dup[0][0] and dup[-1][2] == 0 and _host(rows + [rows[0]], counts, 1) == dup


@pytest.mark.parametrize("seed", range(4))
def test_disjoint_rows_own_what_they_share(seed):
    rows, counts = cs.random_pair(100 + seed, disjoint=True)
    out = scm.rows(rows, counts, 1)
    assert all(r[0] == r[2] and r[1] == r[3] for r in out) and _host(rows, counts, 1) == out


def test_identity():
    assert api.screen_identity(0, 1000, 21) == 0.0 == scm.identity(0, 1000, 21)
    assert api.screen_identity(1000, 1000, 21) == 1.0 == scm.identity(1000, 1000, 21)
    assert api.screen_identity(0, 0, 21) == 0.0
    for shared, length, k in ((1, 1000, 21), (999, 1000, 21), (500, 1000, 16), (3, 7, 1), (12345, 16384, 31)):
        got, want = api.screen_identity(shared, length, k), scm.identity(shared, length, k)
        assert abs(got - want) <= 4 * np.finfo(np.float64).eps * want and 0.0 < got < 1.0, (shared, length, k)
    for bad in ((2, 1, 21), (1, 2, 0)):
        with pytest.raises(api.RkmhError):
            api.screen_identity(*bad)


def test_host_side_refusals():
    lib = api.load_library()
    import ctypes as C
    v, off = scm.to_csr([[1, 2, 3], [2, 5]])
    cv, cc = cs.counted_arrays({2: 1, 5: 2})
    assert api.screen_rows_host(v, off, cv, cc, 1).tolist() == [[1, 1, 0, 0], [2, 1, 2, 1]]
    out = np.zeros(8, np.uint32)
    p = api._p

    def rc(values=v, offsets=off, nref=2, c_values=cv, c_counts=cc, nc=2, m=1, o=out):
        return lib.rk_screen_rows_host(None if values is None else p(values, C.c_uint64), None if offsets is None else p(offsets, C.c_uint64), nref,
                                       None if c_values is None else p(c_values, C.c_uint64), None if c_counts is None else p(c_counts, C.c_uint64), nc,
                                       C.c_uint64(m), None if o is None else p(o, C.c_uint32))

    assert rc() == 0
    ARG, LIMIT = -1, -5                                                      # RK_ERR_ARG, RK_ERR_LIMIT
    assert rc(nref=1 << 31) == LIMIT and b"2^31-1" in lib.rk_last_error()    # (refused before any offset is read)
    for kw, word in ((dict(offsets=None), b"bad arguments"), (dict(o=None), b"bad arguments"), (dict(values=None), b"bad arguments"),
                     (dict(c_values=None), b"bad arguments"), (dict(c_counts=None), b"bad arguments"), (dict(nref=0), b"at least one"),
                     (dict(m=0), b"min_copies"), (dict(m=1 << 32), b"min_copies"),
                     (dict(offsets=np.asarray([0, 3, 2], np.uint64)), b"decrease"),
                     (dict(values=np.asarray([1, 3, 2, 2, 5], np.uint64)), b"descends"),
                     (dict(values=np.asarray([0, 2, 3, 2, 5], np.uint64)), b"is 0"),
                     (dict(c_values=np.asarray([5, 2], np.uint64)), b"does not ascend"),
                     (dict(c_values=np.asarray([2, 2], np.uint64)), b"does not ascend"),
                     (dict(c_values=np.asarray([0, 2], np.uint64)), b"is 0")):
        assert rc(**kw) == ARG and word in lib.rk_last_error(), (kw, lib.rk_last_error())
    # an empty counted set and empty rows are inputs like any other
    assert rc(c_values=None, c_counts=None, nc=0) == 0 and out.tolist() == [0] * 8
    assert api.screen_rows_host(np.zeros(0, np.uint64), np.zeros(3, np.uint64), cv, cc, 1).tolist() == [[0, 0, 0, 0]] * 2


def test_cli_refuses_before_a_context_exists(root, data_dir):
    """every refusal of `rkmh screen` is a sentence and a non-zero exit; this runs where there is no GPU, so none of them needed one"""
    fa = os.path.join(data_dir, "all_pave_ref.fa.gz")
    fq = os.path.join(data_dir, "minION25.fq.gz")
    base = [os.path.join(root, "bin", "rkmh"), "screen", "-r", fa, "-f", fq, "-k", "21", "-s", "1000"]
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    for extra, word in ((["-k", "31"], "one k-mer size"), (["--scaled", "100"], "rkmh gather"), (["--abund"], "--abund"),
                        (["--min-copies", "0"], "--min-copies"), (["--min-copies", "4294967296"], "--min-copies"), (["--min-copies", "two"], "--min-copies"),
                        (["--min-identity", "1.5"], "--min-identity"), (["--min-identity", "-0.1"], "--min-identity"), (["--min-identity", "x"], "--min-identity"),
                        (["--min-shared", "0"], "--min-shared"), (["-s", "0"], "sketch size"), (["-R", "x.json"], "one of the two"), (["-Q", "x.json"], "-Q")):
        r = subprocess.run(base + extra, capture_output=True, env=env)
        err = r.stderr.decode()
        assert r.returncode != 0 and r.stdout == b"" and err.startswith("rkmh screen: ") and word in err, (extra, err)
    r = subprocess.run(base[:4] + ["-k", "21"], capture_output=True, env=env)
    assert r.returncode != 0 and r.stdout == b"" and r.stderr.decode().startswith("rkmh screen: no read files")
    r = subprocess.run(base[:2] + ["-R", "x.json", "-g", "-f", fq], capture_output=True, env=env)
    assert r.returncode != 0 and r.stderr.decode().startswith("rkmh screen: -g says")
    r = subprocess.run(base[:2], capture_output=True, env=env)
    assert r.returncode != 0 and b"rkmh screen (-r" in r.stderr
    assert b"  screen " in subprocess.run(base[:1], capture_output=True, env=env).stderr


def test_shared_cases_have_what_they_claim():
    W, K = cs.W, cs.K
    assert [len(cs.single_read(t)[0]) for t in cs.TOTALS] == [1, K - 1, K, W - 1, W, W + 1, 3 * W + 5]
    reads = cs.edge_batch()
    st = cs.starts(reads).tolist()
    rel = {s % W for s in st[1:-1]} | {(s - W) % W - W for s in st[1:-1] if s % W == W - 1}
    assert {0, 1}.issubset(rel) and any(s % W == W - 1 for s in st)          # a read boundary on, one behind and one before a tile edge
    assert any(len(r) == 1 for r in reads) and any(len(r) < K for r in reads) and any(b"N" in r for r in reads)
    assert st[-1] % W == 5 + (st[-1 - 1] % W) or st[-1] > 3 * W
    assert (cs.many_tiles_R() * cs.block_bases() + W - 1) // W > cs.GRID_CAP
    h = cs.hashes(cs.homopolymers(3), (K,), sm.DEFAULT)
    assert len(set(h)) == 1 and len(h) == 3 * (60 - K)
    rng = np.random.default_rng(1)
    rows = cs.rows_from(h + [5, 9], rng, 3, 4, repeats=True)
    assert all(r == sorted(r) for r in rows) and any(len(r) != len(set(r)) for r in rows)
