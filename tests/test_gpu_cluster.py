"""Cluster on the GPU: the hook and compress kernels of rk_cluster.hip through rk_cluster_hits, rk_cluster_hits_device and the
self-search rk_cluster_scaled / rk_cluster_scaled_device, against tests/cluster_model.py label for label, and `rkmh cluster` on the
182 HPV references against the model's lines.  What the shared inputs exercise is shown on the model's output by
tests/test_cluster_cpu.py."""
import os
import subprocess

import numpy as np
import pytest

import cluster_cases as cc
import cluster_model as clm
import scaled_model as scm
import search_model as sem

pytestmark = pytest.mark.gpu

GUARD = 64        # int32 guard words on each side of the labels


def _up(x, dtype=np.uint64):
    import torch
    x = np.array(x, dtype=dtype)                             # (a writable copy: the shared inputs are read-only)
    x = x if x.size else np.zeros(3, dtype=dtype)
    return torch.from_numpy(x.view(np.int64 if dtype == np.uint64 else dtype)).cuda()


def _same(got, want, what):
    assert got.dtype == np.int32 and got.shape == want.shape and (got == want).all(), (what, np.flatnonzero(got != want)[:8].tolist() if got.shape == want.shape else got.shape)


def _guarded(n, call):
    """runs call(pointer to n int32 between guard words) -> (its result, the n labels)"""
    import torch
    d = torch.full((GUARD + n + GUARD,), -7, dtype=torch.int32, device="cuda")
    r = call(d.data_ptr() + 4 * GUARD)
    torch.cuda.synchronize()
    out = d.cpu().numpy()
    assert (out[:GUARD] == -7).all() and (out[GUARD + n:] == -7).all(), "written outside the labels"
    return r, out[GUARD:GUARD + n].copy()


def _hits_device(ctx, c, offsets=None, nvalues=None):
    """the resident-hits entry on torch's arrays and stream -> (rounds, labels)"""
    import torch
    n = len(c["lens"])
    off = np.concatenate([[0], np.cumsum(c["lens"].astype(np.uint64))]).astype(np.uint64) if offsets is None else offsets
    d_hits, d_off = _up(c["hits"], np.int32), _up(off)
    return _guarded(n, lambda p: ctx.cluster_hits_device(d_hits.data_ptr(), len(c["hits"]), d_off.data_ptr(), n, int(off[-1]) if nvalues is None else nvalues, p,
                                                        c["measure"], c["ppm"], stream=torch.cuda.current_stream().cuda_stream))


def _graph(ctx, name):
    c, want = cc.by_name(name), cc.want(name)
    _same(ctx.cluster_hits(c["hits"], c["lens"], c["measure"], c["ppm"]), want, (name, "host arrays"))
    rounds, lab = _hits_device(ctx, c)
    _same(lab, want, (name, "resident hits"))
    return rounds


def test_hand_checked_vectors(ctx):
    for v in cc.kat():
        _same(ctx.cluster_hits(v["hits"], v["lens"], v["measure"], v["ppm"]), v["want"], (v["name"], "host arrays"))
        _same(_hits_device(ctx, v)[1], v["want"], (v["name"], "resident hits"))


@pytest.mark.parametrize("name", [c["name"] for c in cc.graphs()])
def test_graphs(ctx, name):
    rounds = _graph(ctx, name)
    c = cc.by_name(name)
    linking = len(clm.links_np(c["hits"], c["lens"], c["measure"], c["ppm"]))
    if len(c["hits"]) == 0:
        assert rounds == 0                                   # nothing to hook: no launch
    elif linking == 0:
        assert rounds == 1                                   # one look, nothing changed
    else:
        assert rounds >= 2                                   # a changing round is followed by another look
    if name == "zigzag path":
        assert rounds >= 3                                   # two changing rounds (tests/test_cluster_cpu.py shows why) and the last look


def test_lengths_are_clamped_on_the_device(ctx):
    c = cc.clamped()
    _, lab = _hits_device(ctx, c, offsets=c["offsets"], nvalues=c["nvalues"])
    _same(lab, cc.want(c["name"]), "offsets beyond nvalues")
    _, lab = _hits_device(ctx, c, offsets=c["offsets"], nvalues=40)
    _same(lab, np.array([0, 0, 2, 3], np.int32), "all the values behind the pointer")
    down = np.array([20, 10, 20, 30, 40], dtype=np.uint64)   # offsets that decrease: row 0 is empty
    _, lab = _hits_device(ctx, c, offsets=down, nvalues=40)
    _same(lab, clm.propagate(c["hits"], [0, 10, 10, 10], c["measure"], c["ppm"]), "decreasing offsets")


def _index(ctx, sketches):
    rv, ro = scm.csr(sketches)
    return ctx.scaled_index(rv, ro), rv, ro


def _self_device(idx, rv, ro, **kw):
    import torch
    d_v, d_o = _up(rv), _up(ro)
    n = len(ro) - 1
    return _guarded(n, lambda p: idx.cluster_device(d_v.data_ptr(), d_o.data_ptr(), n, len(rv), p, stream=torch.cuda.current_stream().cuda_stream, **kw))[1]


def test_families_through_the_self_search(ctx):
    f = cc.families()
    idx, rv, ro = _index(ctx, f["sketches"])
    for measure in (clm.JACCARD, clm.MAX_CONTAINMENT):
        for ppm in cc.THRESHOLDS:
            want = cc.families_want(measure, ppm)
            _same(idx.cluster(rv, ro, measure=measure, min_ppm=ppm), want, (measure, ppm, "host arrays"))
            _same(_self_device(idx, rv, ro, measure=measure, min_ppm=ppm), want, (measure, ppm, "resident arrays"))
            _same(ctx.cluster_hits(f["hits"], f["lens"], measure, ppm), want, (measure, ppm, "the model's hits"))
    want3 = cc.families_want(clm.JACCARD, 0, 3)
    assert len(np.unique(want3)) > len(np.unique(cc.families_want(clm.JACCARD, 0)))          # the one value that chains two families no longer links
    _same(idx.cluster(rv, ro, min_shared=3), want3, "min_shared = 3")
    idx.close()


@pytest.mark.parametrize("hit_cap", [1, 7, 12345, 0])
def test_hit_cap(ctx, hit_cap):
    """blocks halved down to single queries, and a query's hits in pieces below its own hit count: the same labels"""
    f = cc.families()
    per_query = np.bincount(f["hits"][:, 0], minlength=cc.NSKETCHES)
    assert per_query.max() > 7 and len(f["hits"]) > 12345 > per_query.max()
    idx, rv, ro = _index(ctx, f["sketches"])
    want = cc.families_want(clm.MAX_CONTAINMENT, 800000)
    _same(idx.cluster(rv, ro, measure=clm.MAX_CONTAINMENT, min_ppm=800000, hit_cap=hit_cap), want, (hit_cap, "host arrays"))
    if hit_cap != 1:
        _same(_self_device(idx, rv, ro, measure=clm.MAX_CONTAINMENT, min_ppm=800000, hit_cap=hit_cap), want, (hit_cap, "resident arrays"))
    idx.close()


def test_block_edges_of_the_search(ctx):
    b = cc.block_edge()
    idx, rv, ro = _index(ctx, b["sketches"])
    assert idx.stats()["nref"] == cc.REF_BLOCK + 1
    _same(idx.cluster(rv, ro, min_shared=2), b["want"], "host arrays")
    _same(_self_device(idx, rv, ro, min_shared=2, hit_cap=1000), b["want"], "resident arrays, blocks of 1 000 hits")
    _same(idx.cluster(rv, ro, min_shared=1), np.zeros(cc.REF_BLOCK + 1, np.int32), "everything shares one value")
    idx.close()


def test_reuse(ctx):
    f = cc.families()
    idx, rv, ro = _index(ctx, f["sketches"])
    a = idx.cluster(rv, ro, min_ppm=200000)
    b = idx.cluster(rv, ro, measure=clm.MAX_CONTAINMENT, min_ppm=1000000, hit_cap=50)
    _same(a, cc.families_want(clm.JACCARD, 200000), "first call")
    _same(b, cc.families_want(clm.MAX_CONTAINMENT, 1000000), "second call")
    q = f["sketches"][:20]
    qv, qo = scm.csr(q)
    h = f["hits"]
    _same(idx.search(qv, qo), h[h[:, 0] < 20], "a search after two clusterings")
    _same(idx.cluster(rv, ro, min_ppm=200000), a, "and a clustering after the search")
    idx.close()


def test_entry_refusals(ctx):
    import rkmh_amd
    from rkmh_amd import api
    C = api.C
    f = cc.families()
    sk = f["sketches"][:6]
    idx, rv, ro = _index(ctx, sk)
    lib, h = ctx._lib, ctx._h
    r = C.c_uint32()
    for n, measure, ppm, code in ((0, 0, 0, -1), (-1, 0, 0, -1), (1 << 31, 0, 0, -5), (4, 2, 0, -1), (4, -1, 0, -1), (4, 0, 1000001, -1)):
        assert lib.rk_cluster_hits_device(h, 8, 1, 8, n, 1, measure, ppm, 8, C.byref(r), None) == code       # before anything is read
    assert lib.rk_cluster_hits_device(h, None, 1, 8, 4, 1, 0, 0, 8, None, None) == -1
    assert lib.rk_cluster_hits_device(h, 8, 1, None, 4, 1, 0, 0, 8, None, None) == -1
    assert lib.rk_cluster_hits_device(h, 8, 1, 8, 4, 1, 0, 0, None, None, None) == -1
    assert lib.rk_cluster_hits_device(None, 8, 1, 8, 4, 1, 0, 0, 8, None, None) == -1
    for nref, ms, measure, ppm, code in ((0, 1, 0, 0, -1), (1 << 31, 1, 0, 0, -5), (6, 0, 0, 0, -1), (6, 1, 3, 0, -1), (6, 1, 0, 1000001, -1), (5, 1, 0, 0, -1)):
        assert lib.rk_cluster_scaled_device(h, idx._h, 8, 8, nref, 1, ms, measure, ppm, 0, 8, None) == code
    assert lib.rk_cluster_scaled_device(h, None, 8, 8, 6, 1, 1, 0, 0, 0, 8, None) == -1
    assert lib.rk_cluster_scaled_device(h, idx._h, 8, None, 6, 1, 1, 0, 0, 0, 8, None) == -1
    assert lib.rk_cluster_scaled_device(h, idx._h, 8, 8, 6, 1, 1, 0, 0, 0, None, None) == -1
    for bad in (dict(min_shared=0), dict(measure=2), dict(min_ppm=1000001)):
        with pytest.raises(api.RkmhError) as e:
            idx.cluster(rv, ro, **bad)
        assert e.value.code == -1, bad
    lab = np.zeros(6, np.int32)
    down = np.array(ro, dtype=np.uint64)
    down[2], down[3] = down[3], down[2]
    assert down[3] < down[2]
    assert lib.rk_cluster_scaled(h, idx._h, api._p(rv, C.c_uint64), api._p(down, C.c_uint64), 6, 1, 0, 0, 0, api._p(lab, C.c_int32)) == -1   # offsets that decrease
    with pytest.raises(api.RkmhError):
        ctx.cluster_hits(np.array([[0, 1, 1]], np.int32), np.array([3, 1 << 31], np.uint64))             # a length of 2^31
    other = rkmh_amd.Context(0)
    assert other._lib.rk_cluster_scaled(other._h, idx._h, api._p(rv, C.c_uint64), api._p(ro, C.c_uint64), 6, 1, 0, 0, 0, api._p(lab, C.c_int32)) == -1   # an index of another context
    other.close()
    h6 = f["hits"]
    h6 = h6[(h6[:, 0] < 6) & (h6[:, 1] < 6)]
    _same(idx.cluster(rv, ro), clm.propagate(h6, f["lens"][:6]), "and the index still works")
    idx.close()


# ---- the command ----
def _run(root, *args, ok=True):
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    r = subprocess.run([os.path.join(root, "bin", "rkmh")] + list(args), capture_output=True, env=env)
    assert (r.returncode == 0) == ok, (args, r.stderr[-400:])
    return r.stdout.decode() if ok else r.stderr.decode()


# (flag, x, clusters of the 182 references at k = 21, scaled 100: the model's, chosen between one cluster and 182 singletons)
CLI_THRESHOLDS = (("--min-jaccard", "0.02", 122), ("--min-max-containment", "0.05", 138))


def test_cli_on_the_hpv_references(root, data_dir, tmp_path):
    import json
    fa = os.path.join(data_dir, "all_pave_ref.fa.gz")
    opts = ["-k", "21", "--scaled", "100", "--hash-policy", "sourmash"]
    rj = str(tmp_path / "refs.json")
    _run(root, "sketch", "-f", fa, "-o", rj, *opts)
    doc = json.load(open(rj))
    names = [d["name"] for d in doc]
    sk = [np.array(d["sketches"]["hashes"], dtype=np.uint64) for d in doc]
    assert len(names) == 182 and all(d["scaled"] == 100 and d["kmer"] == "21" for d in doc) and all((s[1:] > s[:-1]).all() for s in sk)
    lens = np.array([len(s) for s in sk], dtype=np.uint64)
    hits = sem.search_by_rows(sk, sk)
    for flag, x, ncl in CLI_THRESHOLDS:
        lab = clm.union_find(hits, lens, clm.JACCARD if flag == "--min-jaccard" else clm.MAX_CONTAINMENT, clm.ppm(x))
        assert len(np.unique(lab)) == ncl and 1 < ncl < 182
        want = clm.cluster_text(names, lens, lab)
        got = _run(root, "cluster", "-r", fa, flag, x, *opts)
        assert got == want
        assert _run(root, "cluster", "-R", rj, flag, x, "--hash-policy", "sourmash") == got         # scaled and k come from the file
        reps = _run(root, "cluster", "-r", fa, flag, x, "--representatives", *opts)
        assert reps == clm.cluster_text(names, lens, lab, True)
        full = [ln.split("\t") for ln in got.splitlines()]
        own = {(c, s, r): ln for c, s, r, m, ln in full if m == r}                                 # the representative's own line
        assert [ln.split("\t") for ln in reps.splitlines()] == [[c, s, r, own[c, s, r]] for c, s, r in sorted(own, key=lambda t: int(t[0]))]
    # the default: --min-jaccard 0; and --min-shared
    lab0 = clm.union_find(hits, lens)
    assert len(np.unique(lab0)) == 19
    assert _run(root, "cluster", "-r", fa, *opts) == clm.cluster_text(names, lens, lab0)
    lab5 = clm.union_find(hits[hits[:, 2] >= 5], lens)
    assert len(np.unique(lab5)) == 149
    assert _run(root, "cluster", "-r", fa, "--min-shared", "5", *opts) == clm.cluster_text(names, lens, lab5)
