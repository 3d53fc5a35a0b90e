"""CPU-only: cluster's definitions (include/rkmh_amd.h, "CLUSTER").  The two models of tests/cluster_model.py agree with each other,
with the hand-checked vectors and with the library's host code (rk_cluster_hits_host, rk_cluster_members); the labels do not depend
on how the hits are given; every host-side refusal; and every shared case of tests/cluster_cases.py has what it claims."""
import ctypes as C

import numpy as np
import pytest

import cluster_cases as cc
import cluster_model as clm
from rkmh_amd import api


def _all_cases():
    return cc.kat() + cc.graphs() + (cc.clamped(),)


def _host(c, hits=None):
    return api.cluster_hits_host(c["hits"] if hits is None else hits, c["lens"], c["measure"], c["ppm"])


def _same(got, want, what):
    assert got.dtype == np.int32 and got.shape == want.shape and (got == want).all(), (what, got.tolist()[:8], want.tolist()[:8])


def _well_formed(lab):
    assert (lab[lab] == lab).all() and (lab <= np.arange(len(lab))).all()


def test_vectors_models_and_host_code():
    for v in cc.kat():
        for got in (clm.union_find(v["hits"], v["lens"], v["measure"], v["ppm"]), clm.propagate(v["hits"], v["lens"], v["measure"], v["ppm"]), _host(v)):
            _same(got, v["want"], v["name"])
    on = [v for v in cc.kat() if "exactly on the threshold" in v["name"]]
    assert len(on) == 2 and {v["measure"] for v in on} == {0, 1}
    for v in on:                                             # the boundary pairs sit exactly on the threshold
        (i, j, s), ln = v["hits"][0].tolist(), v["lens"].tolist()
        denom = ln[i] + ln[j] - s if v["measure"] == clm.JACCARD else min(ln[i], ln[j])
        assert s * 1000000 == v["ppm"] * denom and v["want"].tolist() == [0, 0]
    under = [v for v in cc.kat() if "one shared hash fewer" in v["name"]]
    assert [(u["lens"].tolist(), int(u["hits"][0][2]) + 1, u["measure"]) for u in under] == [(v["lens"].tolist(), int(v["hits"][0][2]), v["measure"]) for v in on]
    assert all(u["want"].tolist() == [0, 1] for u in under)


@pytest.mark.parametrize("name", [c["name"] for c in cc.graphs() + (cc.clamped(),)])
def test_models_and_host_code_agree(name):
    c = cc.by_name(name)
    want = cc.want(name)
    _well_formed(want)
    _same(clm.union_find(c["hits"], c["lens"], c["measure"], c["ppm"]), want, (name, "the two models"))
    _same(_host(c), want, (name, "host code"))


def test_families_models_and_host_code_agree():
    f = cc.families()
    counts = {}
    for measure in (clm.JACCARD, clm.MAX_CONTAINMENT):
        for ppm in cc.THRESHOLDS:
            want = cc.families_want(measure, ppm)
            _well_formed(want)
            _same(clm.union_find(f["hits"], f["lens"], measure, ppm), want, (measure, ppm, "the two models"))
            _same(api.cluster_hits_host(f["hits"], f["lens"], measure, ppm), want, (measure, ppm, "host code"))
            counts[measure, ppm] = len(np.unique(want))
    n = cc.NSKETCHES
    # what the collection claims: at 0 the families chain (a few clusters beside the empty sketches), higher thresholds split them,
    # at 1 000 000 identical sets (jaccard) and subsets (max containment) still link
    for measure in (clm.JACCARD, clm.MAX_CONTAINMENT):
        c = [counts[measure, p] for p in cc.THRESHOLDS]
        assert c == sorted(c) and c[0] < cc.NFAMILIES and c[0] < c[1] < c[2] < c[3] < n, c
    assert counts[clm.MAX_CONTAINMENT, 1000000] < counts[clm.JACCARD, 1000000]
    assert int((f["lens"] == 0).sum()) == 5
    assert (f["hits"][:, 0] != f["hits"][:, 1]).sum() > 20000     # many related members: the hit list is what is large
    at0 = cc.families_want(clm.JACCARD, 0)
    assert (at0[f["lens"] == 0] == np.flatnonzero(f["lens"] == 0)).all()     # an empty sketch matches nothing, itself included


def test_labels_do_not_depend_on_how_the_hits_are_given():
    rng = np.random.default_rng(5)
    f = cc.families()
    for c in list(cc.graphs()) + [dict(name="families", hits=f["hits"], lens=f["lens"], measure=clm.JACCARD, ppm=200000)]:
        h = c["hits"]
        if len(h) == 0:
            continue
        want = _host(c)
        _same(_host(c, h[rng.permutation(len(h))]), want, (c["name"], "order"))
        _same(_host(c, h[::-1]), want, (c["name"], "reversed"))
        _same(_host(c, np.concatenate([h, h[: len(h) // 2 + 1], h])), want, (c["name"], "duplicated"))
        _same(_host(c, h[:, [1, 0, 2]]), want, (c["name"], "every hit turned round"))
        both = np.concatenate([h, h[:, [1, 0, 2]]])
        one = both[both[:, 0] <= both[:, 1]]                                  # one direction of every pair
        _same(_host(c, one), want, (c["name"], "one direction"))
    h = f["hits"]
    assert len(h[h[:, 0] < h[:, 1]]) * 2 + int((h[:, 0] == h[:, 1]).sum()) == len(h)   # the self-search gives both directions


def test_members_and_representatives():
    rng = np.random.default_rng(6)
    f = cc.families()
    cases = [(cc.families_want(clm.JACCARD, 200000), f["lens"]), (cc.want("two stars and a bridge, jaccard"), cc.by_name("two stars and a bridge, jaccard")["lens"]),
             (np.zeros(1, np.int32), np.array([7], np.uint64)), (np.arange(9, dtype=np.int32), np.full(9, 3, np.uint64))]
    # equal lengths inside a cluster: the lowest index is the representative; and a later, strictly longer member wins
    cases.append((np.array([0, 0, 2, 0, 2, 2], np.int32), np.array([5, 9, 4, 9, 4, 4], np.uint64)))
    lab = cc.families_want(clm.JACCARD, 0)
    cases.append((lab, rng.integers(1, 4, len(lab)).astype(np.uint64)))       # few distinct lengths: ties in every cluster
    for lab, lens in cases:
        got = api.cluster_members(lab, lens)
        want = clm.members(lab, lens)
        for g, w, what in zip(got, want, ("cl_off", "members", "rep")):
            _same(g, w, what)
    off, mem, rep = api.cluster_members(cases[4][0], cases[4][1])
    assert off.tolist() == [0, 3, 6] and mem.tolist() == [0, 1, 3, 2, 4, 5] and rep.tolist() == [1, 2]
    names = ["s%d" % i for i in range(6)]
    assert clm.cluster_text(names, cases[4][1], cases[4][0]) == ("0\t3\ts1\ts0\t5\n0\t3\ts1\ts1\t9\n0\t3\ts1\ts3\t9\n"
                                                                  "1\t3\ts2\ts2\t4\n1\t3\ts2\ts4\t4\n1\t3\ts2\ts5\t4\n")
    assert clm.cluster_text(names, cases[4][1], cases[4][0], True) == "0\t3\ts1\t9\n1\t3\ts2\t4\n"


def test_host_side_refusals():
    lens = np.array([3, 3, 3], np.uint64)
    hits = np.array([[0, 1, 2]], np.int32)
    for bad, code in ((dict(measure=2), -1), (dict(measure=-1), -1), (dict(min_ppm=1000001), -1)):
        a = dict(measure=0, min_ppm=0)
        a.update(bad)
        with pytest.raises(api.RkmhError) as e:
            api.cluster_hits_host(hits, lens, **a)
        assert e.value.code == code, bad
    with pytest.raises(api.RkmhError) as e:
        api.cluster_hits_host(hits, np.array([3, 1 << 31, 3], np.uint64))
    assert e.value.code in (-1, -5)
    assert api.cluster_hits_host(hits, np.array([3, (1 << 31) - 1, 3], np.uint64)).tolist() == [0, 0, 2]
    lib = api.load_library()
    lab = np.zeros(3, np.int32)
    p = lambda a, t: api._p(a, t)
    assert lib.rk_cluster_hits_host(p(hits, C.c_int32), 1, p(lens, C.c_uint64), 0, 0, 0, p(lab, C.c_int32)) == -1
    assert lib.rk_cluster_hits_host(p(hits, C.c_int32), 1, p(lens, C.c_uint64), 1 << 31, 0, 0, p(lab, C.c_int32)) == -5
    assert lib.rk_cluster_hits_host(None, 1, p(lens, C.c_uint64), 3, 0, 0, p(lab, C.c_int32)) == -1
    assert lib.rk_cluster_hits_host(p(hits, C.c_int32), 1, None, 3, 0, 0, p(lab, C.c_int32)) == -1
    assert lib.rk_cluster_hits_host(p(hits, C.c_int32), 1, p(lens, C.c_uint64), 3, 0, 0, None) == -1
    assert lib.rk_cluster_hits_host(None, 0, p(lens, C.c_uint64), 3, 0, 0, p(lab, C.c_int32)) == 0 and lab.tolist() == [0, 1, 2]
    # labels that are not the smallest index of their cluster
    for bad in ([0, 2, 2], [1, 1, 2], [0, 0, 1], [0, -1, 2], [0, 1, 3]):
        with pytest.raises(api.RkmhError) as e:
            api.cluster_members(np.array(bad, np.int32), lens)
        assert e.value.code == -1, bad
    ncl = C.c_int64()
    good = np.array([0, 0, 2], np.int32)
    a3, a4 = np.zeros(3, np.int32), np.zeros(4, np.int32)
    assert lib.rk_cluster_members(p(good, C.c_int32), p(lens, C.c_uint64), 0, C.byref(ncl), p(a4, C.c_int32), p(a3, C.c_int32), p(a3, C.c_int32)) == -1
    assert lib.rk_cluster_members(p(good, C.c_int32), None, 3, C.byref(ncl), p(a4, C.c_int32), p(a3, C.c_int32), p(a3, C.c_int32)) == -1
    assert lib.rk_cluster_members(p(good, C.c_int32), p(lens, C.c_uint64), 3, None, p(a4, C.c_int32), p(a3, C.c_int32), p(a3, C.c_int32)) == -1


def test_shared_cases_have_what_they_claim():
    g = {c["name"]: c for c in cc.graphs()}
    n = cc.PATH_N
    for name in ("path in index order", "path under a random permutation", "zigzag path"):
        c = g[name]
        assert len(c["hits"]) == n - 1 and (cc.want(name) == 0).all()                          # one component, a tree
        deg = np.bincount(c["hits"][:, :2].ravel(), minlength=n)
        assert sorted(np.bincount(deg).tolist()) == [0, 2, n - 2]                              # a path: two ends, the rest of degree 2
    assert (np.abs(g["path in index order"]["hits"][:, 0] - g["path in index order"]["hits"][:, 1]) == 1).all()
    # the zigzag: every link joins a high id and a low one, so in round 1 (every node its own root) no low id is ever the larger end
    # of a link and stays a root; the low ids are not adjacent, and there are many of them: a second changing round is needed
    zz = g["zigzag path"]
    low = n // 2
    a, b = zz["hits"][:, 0], zz["hits"][:, 1]
    assert ((a < low) != (b < low)).all()
    ids = zz["ids"]
    assert (ids[1::2] == np.arange(low)).all() and (ids[0::2] >= low).all() and sorted(ids.tolist()) == list(range(n))
    first = np.arange(n)
    np.minimum.at(first, np.maximum(a, b), np.minimum(a, b))                                   # what round 1's atomicMin leaves
    assert (first[:low] == np.arange(low)).all() and (first[low:] < low).all()
    st = g["star whose centre is the highest id"]
    m = len(st["lens"])
    assert ((st["hits"][:, 0] == m - 1) | (st["hits"][:, 1] == m - 1)).all() and (cc.want(st["name"]) == 0).all()
    j, mc = cc.want("two stars and a bridge, jaccard"), cc.want("two stars and a bridge, max containment")
    assert j.tolist() == [0] * 10 + [10] * 10 and mc.tolist() == [0] * 20
    cg = g["complete graph and singletons"]
    assert len(cg["hits"]) == 1500 * 1499 > 2048 * 256 * 4 and cc.want(cg["name"]).tolist() == [0] * 1500 + list(range(1500, 2000))
    bad = g["bad indices mixed in"]
    h = bad["hits"]
    out = (h[:, 0] < 0) | (h[:, 0] >= 500) | (h[:, 1] < 0) | (h[:, 1] >= 500)
    assert out.sum() == 300 and {-1, 500, (1 << 31) - 1} <= set(h[out][:, :2].ravel().tolist())
    _same(clm.propagate(bad["good"], bad["lens"], bad["measure"], bad["ppm"]), cc.want(bad["name"]), "without the bad hits")
    assert 1 < len(np.unique(cc.want(bad["name"]))) < 500
    cl = cc.clamped()
    assert cc.want(cl["name"]).tolist() == [0, 0, 0, 3]
    _same(clm.propagate(cl["hits"], cl["lens_as_given"], cl["measure"], cl["ppm"]), np.array([0, 0, 2, 3], np.int32), "unclamped lengths differ")
    off = np.minimum(cl["offsets"], np.uint64(cl["nvalues"]))
    assert (np.diff(off.astype(np.int64)) == cl["lens"].astype(np.int64)).all()


def test_block_edge_collection():
    b = cc.block_edge()
    n = cc.REF_BLOCK + 1
    assert api.RK_SEARCH_REF_BLOCK == cc.REF_BLOCK and len(b["sketches"]) == n
    w = b["want"]
    _same(api.cluster_hits_host(b["hits"], b["lens"]), w, "host code")
    assert w[cc.REF_BLOCK - 1] == 0 and w[cc.REF_BLOCK] == 0                                   # a cluster across the edge of the reference blocks
    assert len(np.unique(w)) == 501 and w[501] == 1 and w[1 + 500 * 16] == 1


def test_cli_refuses_before_a_context_exists(root, data_dir):
    """every refusal of `rkmh cluster` is a sentence and a non-zero exit; this runs where there is no GPU, so none of them needed one"""
    import os
    import subprocess
    fa = os.path.join(data_dir, "all_pave_ref.fa.gz")
    base = [os.path.join(root, "bin", "rkmh"), "cluster", "-r", fa, "-k", "21", "--scaled", "100"]
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    for extra, word in ((["-f", fa], "-f / -Q"), (["-Q", "x.json"], "-f / -Q"), (["-s", "100"], "bottom-s"), (["--abund"], "--abund"),
                        (["--min-jaccard", "1.5"], "decimal"), (["--min-jaccard", "0.1234567"], "decimal"), (["--min-jaccard", "1e-3"], "decimal"),
                        (["--min-jaccard", "-0.1"], "decimal"), (["--min-max-containment", "abc"], "decimal"), (["--min-jaccard", ""], "decimal"),
                        (["--min-jaccard", "1.000001"], "decimal"), (["--min-jaccard", "2"], "decimal"), (["--min-jaccard", "0x1"], "decimal"),
                        (["--min-jaccard", "0.5", "--min-max-containment", "0.5"], "give one of the two"),
                        (["--min-shared", "0"], "--min-shared"), (["--scaled", "0"], "--scaled"), (["-R", "x.json"], "one of the two"), (["-k", "31"], "one k-mer size")):
        r = subprocess.run(base + extra, capture_output=True, env=env)
        err = r.stderr.decode()
        assert r.returncode != 0 and r.stdout == b"" and err.startswith("rkmh cluster: ") and word in err, (extra, err)
    r = subprocess.run(base[:2] + ["-k", "21", "--scaled", "100"], capture_output=True, env=env)
    assert r.returncode != 0 and r.stderr.decode().startswith("rkmh cluster: the collection comes from")
    r = subprocess.run(base[:2] + ["-R", "x.json", "-g"], capture_output=True, env=env)
    assert r.returncode != 0 and r.stderr.decode().startswith("rkmh cluster: -g says")


def test_ppm_of_a_decimal():
    assert [clm.ppm(t) for t in ("0", "1", "0.95", ".5", "1.000000", "0.000001", "0.")] == [0, 1000000, 950000, 500000, 1000000, 1, 0]
