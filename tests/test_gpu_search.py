"""Search on the GPU: the index build and k_search_block of rk_search.hip through both entries (rk_search_scaled,
rk_search_scaled_device) and `rkmh manysearch`, against tests/search_model.py hit for hit, against the dense rk_compare_scaled on the
same inputs, and against `rkmh dist --scaled` byte for byte.  What the shared inputs exercise is shown on the model's output by
tests/test_search_cpu.py."""
import os
import subprocess

import numpy as np
import pytest

import scaled_cases as sc
import scaled_model as scm
import search_cases as sec
import search_model as sem

pytestmark = pytest.mark.gpu

GUARD = 96        # int32 guard words on each side of the hits: a multiple of 3, so the hits keep their alignment


def _up(x, dtype=np.uint64):
    import torch
    x = np.array(x, dtype=dtype)                             # (a writable copy: the shared inputs are read-only)
    x = x if len(x) else np.zeros(1, dtype=dtype)
    return torch.from_numpy(x.view(np.int64 if dtype == np.uint64 else dtype)).cuda()


def _device(idx, queries, min_shared=1, q_min=None, cap=None, q_nvalues=None, qo=None):
    """the resident-input entry on torch's arrays and stream, guard words on both sides of the hits -> (total, the hits written)"""
    import torch
    qv, off = scm.csr(queries)
    off = off if qo is None else qo
    nq = len(off) - 1
    d_qv, d_qo = _up(qv), _up(off)
    d_qm = None if q_min is None else _up(q_min, np.int32)
    if cap is None:                                          # a first call sizes the answer, as a caller would
        cap = idx.search_device(d_qv.data_ptr(), d_qo.data_ptr(), nq, len(qv) if q_nvalues is None else q_nvalues, 0, 0, min_shared=min_shared,
                                d_q_min_ptr=None if d_qm is None else d_qm.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    d_hits = torch.full((GUARD + cap * 3 + GUARD,), -7, dtype=torch.int32, device="cuda")
    total = idx.search_device(d_qv.data_ptr(), d_qo.data_ptr(), nq, len(qv) if q_nvalues is None else q_nvalues, d_hits.data_ptr() + 4 * GUARD, cap,
                              min_shared=min_shared, d_q_min_ptr=None if d_qm is None else d_qm.data_ptr(),
                              stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_hits.cpu().numpy()
    n = min(total, cap)
    assert (out[:GUARD] == -7).all() and (out[GUARD + 3 * n:] == -7).all(), "written outside the hits"
    return total, out[GUARD:GUARD + 3 * n].reshape(n, 3)


def _same(got, want, what):
    assert got.dtype == np.int32 and got.shape == want.shape and (got == want).all(), (what, got.tolist()[:4], want.tolist()[:4])


def _both_entries(idx, queries, want, what, min_shared=1, q_min=None):
    qv, qo = scm.csr(queries)
    _same(idx.search(qv, qo, min_shared=min_shared, q_min=q_min), want, (what, "host entry"))
    total, hits = _device(idx, queries, min_shared, q_min)
    assert total == len(want), (what, total, len(want))
    _same(hits, want, (what, "device entry"))


def _index(ctx, refs):
    rv, ro = scm.csr(refs)
    return ctx.scaled_index(rv, ro)


def _dense_hits(ctx, refs, queries):
    """the non-zero entries of the dense comparison, row-major: what search(min_shared=1) must equal"""
    rv, ro = scm.csr(refs)
    qv, qo = scm.csr(queries)
    d = ctx.compare_scaled(qv, qo, rv, ro)
    i, j = np.nonzero(d)
    return np.stack([i, j, d[i, j]], axis=1).astype(np.int32), d


def test_hand_checked_vectors_both_entries(ctx):
    for v in sec.kat():
        idx = _index(ctx, v["refs"])
        s = idx.stats()
        assert s["nref"] == len(v["refs"]) and s["npost"] == sum(len(r) for r in v["refs"])
        assert s["nkeys"] == len(np.unique(np.concatenate([np.zeros(0, np.uint64)] + list(v["refs"]))))
        _both_entries(idx, v["queries"], v["want"], v["name"], v["min_shared"], v["q_min"])
        idx.close()


@pytest.mark.parametrize("nref", sec.NREFS)
def test_random_sets(ctx, nref):
    c = sec.random_case(nref)
    idx = _index(ctx, c["refs"])
    s = idx.stats()
    assert s["nref"] == nref and s["npost"] == sum(len(r) for r in c["refs"]) and s["longest_posting"] >= 1
    dense, d = _dense_hits(ctx, c["refs"], c["queries"])
    assert (d == 0).any() and (d > 0).any()
    _same(dense, c["want1"], (nref, "the dense path and the model"))
    for nq in sec.NQS:
        q = c["queries"][:nq]
        _both_entries(idx, q, sec.first_queries(c["want1"], nq), (nref, nq))
        _both_entries(idx, q, sec.first_queries(c["want_cut"], nq), (nref, nq, "cut"), min_shared=c["cut"])
        _both_entries(idx, q, sec.first_queries(c["want_qmin"], nq), (nref, nq, "q_min"), min_shared=2, q_min=c["q_min"][:nq])
    idx.close()


@pytest.mark.parametrize("nref", sec.BLOCK_EDGE_NREFS)
def test_block_edges(ctx, nref):
    from rkmh_amd import api
    assert api.RK_SEARCH_REF_BLOCK == sec.REF_BLOCK
    c = sec.block_edges(nref)
    refs, queries, edge = c["refs"], c["queries"], c["edge"]
    idx = _index(ctx, refs)
    s = idx.stats()
    assert s["nref"] == nref and s["longest_posting"] == nref and 100 < s["nkeys"] <= 303
    assert 0 in edge and nref - 1 in edge and len(edge) == 2 * ((nref + sec.REF_BLOCK - 1) // sec.REF_BLOCK) - (nref % sec.REF_BLOCK == 1)
    dense, _ = _dense_hits(ctx, refs, queries)
    want1 = sem.search_by_rows(refs, queries)
    _same(dense, want1, (nref, "the dense path and the model"))
    assert (want1[want1[:, 0] == 0][:, 1] == np.arange(nref)).all()                       # the value every reference holds: a hit everywhere
    want2 = sem.search_by_rows(refs, queries, 2)
    assert want2[want2[:, 0] == 1][:, 1].tolist() == list(edge)                             # the edge values: the first and last row of every block
    want3 = sem.search_by_rows(refs, queries, 3)
    assert set(edge) <= set(want3[want3[:, 0] == 3][:, 1].tolist()) and 0 < len(want3) < len(want2) < len(want1)
    _both_entries(idx, queries, want1, (nref, 1))
    _both_entries(idx, queries, want2, (nref, 2), min_shared=2)
    _both_entries(idx, queries, want3, (nref, 3), min_shared=3)
    _both_entries(idx, queries, sem.search_by_rows(refs, queries, 1, [1, 2, 3, 2]), (nref, "q_min"), q_min=[1, 2, 3, 2])
    idx.close()


@pytest.mark.parametrize("length", sec.POSTING_LENGTHS)
def test_posting_lists_around_the_whole_wave_walk(ctx, length):
    c = sec.posting_lists(length)
    idx = _index(ctx, c["refs"])
    s = idx.stats()
    assert s["longest_posting"] == length and s["nref"] == 300 and s["nkeys"] == 302      # the stats prove the length that was built
    for ms in (1, 2):
        want = sem.search(c["refs"], c["queries"], ms)
        assert len(want) >= (length if ms == 1 else 1)
        _both_entries(idx, c["queries"], want, (length, ms), min_shared=ms)
    idx.close()


@pytest.mark.parametrize("total", sec.KEY_TOTALS)
def test_keys_around_the_edges_of_the_compaction(ctx, total):
    """the index's keys come out of the compaction that scaled sketches are kept with: repeated values across the end of a wave's and
    of a workgroup's elements, at the first and at the last entry (the layout is proved by tests/test_search_cpu.py)"""
    c = sec.key_edges(total)
    idx = _index(ctx, c["refs"])
    s = idx.stats()
    assert s["nref"] == 5 and s["npost"] == total and s["nkeys"] == c["nkeys"] and s["longest_posting"] == c["longest"]
    for ms in (1, 2):
        _both_entries(idx, c["refs"], sem.search(c["refs"], c["refs"], ms), (total, ms), min_shared=ms)
    idx.close()


def test_equal_to_the_dense_path_on_the_panel(ctx):
    sk = sc.sketches("sourmash-k21", 10)                                                    # the 40 panel records
    assert len(sk) == 40
    dense, d = _dense_hits(ctx, sk, sk)
    assert (d == 0).any() and (d[~np.eye(40, dtype=bool)] > 0).any()                         # sharing and non-sharing pairs
    _same(dense, sem.search(sk, sk), "the dense path and the model")
    idx = _index(ctx, sk)
    _both_entries(idx, sk, dense, "panel")
    _both_entries(idx, sk, dense[dense[:, 2] >= 5], "panel, 5", min_shared=5)
    idx.close()


def test_capacity(ctx):
    c = sec.random_case(65)
    want = sec.first_queries(c["want1"], 9)
    total = len(want)
    assert total > 3
    idx = _index(ctx, c["refs"])
    for cap in (0, 1, total - 1, total, total + 5):
        n, hits = _device(idx, c["queries"][:9], cap=cap)                                  # (the guard words and the tail are checked in there)
        assert n == total
        _same(hits, want[:min(cap, total)], ("cap", cap))
    idx.close()


def test_rows_are_clamped_on_the_device(ctx):
    import torch
    rng = np.random.default_rng(9)
    pl = sc.pool(rng, 3000)
    A = sc.random_sets(rng, 4, pl, lengths=[65, 129, 1000])
    Q = sc.random_sets(rng, 3, pl, lengths=[129, 1000])
    rv, ro = scm.csr(A)
    qv, qo = scm.csr(Q)
    # fewer reference values behind the pointer than the offsets say: row 2 is cut short, row 3 lies outside altogether
    n = int(ro[2]) + 10
    d_rv, d_ro = _up(rv), _up(ro)
    idx = ctx.scaled_index_device(d_rv.data_ptr(), d_ro.data_ptr(), 4, n, stream=torch.cuda.current_stream().cuda_stream)
    assert idx.stats()["npost"] == n
    cut = [A[0], A[1], A[2][:10], A[3][:0]]
    _both_entries(idx, Q, sem.search(cut, Q), "fewer reference values")
    idx.close()
    down = np.array([ro[1], ro[0], ro[1], ro[2]], dtype=np.uint64)                           # offsets that decrease: an empty row
    d_down = _up(down)
    idx = ctx.scaled_index_device(d_rv.data_ptr(), d_down.data_ptr(), 3, len(rv), stream=torch.cuda.current_stream().cuda_stream)
    total, hits = _device(idx, Q)
    want = sem.search([A[0][:0], A[0], A[1]], Q)
    assert total == len(want)
    _same(hits, want, "decreasing reference offsets")
    idx.close()
    # the same on the query side
    idx = _index(ctx, A)
    m = int(qo[1]) + 7
    total, hits = _device(idx, Q, q_nvalues=m)
    want = sem.search(A, [Q[0], Q[1][:7], Q[2][:0]])
    assert total == len(want)
    _same(hits, want, "fewer query values")
    total, hits = _device(idx, Q, qo=np.array([qo[1], qo[0], qo[1]], dtype=np.uint64))
    want = sem.search(A, [Q[0][:0], Q[0]])
    assert total == len(want)
    _same(hits, want, "decreasing query offsets")
    with pytest.raises(ValueError):
        ctx.scaled_index(rv[:n], ro)                                                         # offsets past the values: refused by the bindings
    with pytest.raises(ValueError):
        idx.search(qv[:m], qo)
    idx.close()


def test_reuse(ctx):
    import rkmh_amd
    a, b = sec.random_case(9), sec.random_case(65)
    ia, ib = _index(ctx, a["refs"]), _index(ctx, b["refs"])                                  # two indexes live on one context
    small = [v for v in sec.kat() if v["name"] == "q_min differs per query"][0]
    isml = _index(ctx, small["refs"])
    for _ in range(2):
        _both_entries(ia, a["queries"], a["want1"], "a")
        _both_entries(ib, b["queries"][:9], sec.first_queries(b["want_cut"], 9), "b, cut", min_shared=b["cut"])
        _both_entries(isml, small["queries"], small["want"], "small after large", small["min_shared"], small["q_min"])   # no stale counts or hits
        _both_entries(ia, a["queries"][:1], sec.first_queries(a["want1"], 1), "a, fewer queries than before")
    ib.close()
    ib.close()                                                                               # a second close does nothing
    _both_entries(ia, a["queries"], a["want1"], "a after b is closed")
    other = rkmh_amd.Context(0)
    from rkmh_amd import api
    qv, qo = scm.csr(a["queries"])
    n, out = api.C.c_uint64(), api._i32p()
    assert other._lib.rk_search_scaled(other._h, ia._h, api._p(qv, api.C.c_uint64), api._p(qo, api.C.c_uint64), len(qo) - 1, 1, None,
                                       api.C.byref(out), api.C.byref(n)) == -1              # an index is used with its own context only
    io = _index(other, a["refs"])
    other.close()
    io.close()                                                                               # an index may outlive its context
    ia.close()
    isml.close()
    dense, _ = _dense_hits(ctx, a["refs"], a["queries"])                                     # and the context works on
    _same(dense, a["want1"], "the context after its indexes are closed")


def test_entry_refusals(ctx):
    from rkmh_amd import api
    v = [x for x in sec.kat() if x["name"] == "q_min differs per query"][0]
    idx = _index(ctx, v["refs"])
    qv, qo = scm.csr(v["queries"])
    for bad in (dict(qo=np.array([0, 6, 3, 8], dtype=np.uint64)), dict(min_shared=0), dict(min_shared=-1), dict(q_min=[1, 0, 1])):
        a = dict(qo=qo, min_shared=1, q_min=None)
        a.update(bad)
        with pytest.raises(api.RkmhError) as e:
            idx.search(qv, a["qo"], min_shared=a["min_shared"], q_min=a["q_min"])
        assert e.value.code == -1, bad
    lib, h = ctx._lib, ctx._h
    n = api.C.c_uint64()
    for nq, ms, code in ((0, 1, -1), (1, 0, -1), (1 << 31, 1, -5)):
        assert lib.rk_search_scaled_device(h, idx._h, 8, 8, nq, 1, ms, None, 8, 1, api.C.byref(n), None) == code   # before anything is read
    assert lib.rk_search_scaled_device(h, idx._h, 8, None, 1, 1, 1, None, 8, 1, api.C.byref(n), None) == -1
    assert lib.rk_search_scaled_device(h, idx._h, 8, 8, 1, 1, 1, None, None, 1, api.C.byref(n), None) == -1
    hh = api.C.c_void_p()
    for nref, code in ((0, -1), (1 << 31, -5)):
        assert lib.rk_scaled_index_create_device(h, 8, 8, nref, 1, None, api.C.byref(hh)) == code
    assert lib.rk_scaled_index_create_device(h, 8, None, 1, 1, None, api.C.byref(hh)) == -1
    assert lib.rk_scaled_index_create_device(h, 8, 8, 1, 1 << 32, None, api.C.byref(hh)) == -5
    _both_entries(idx, v["queries"], v["want"], "and the index still works", v["min_shared"], v["q_min"])
    idx.close()


# ---- the command ----
def _run(root, *args):
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    r = subprocess.run([os.path.join(root, "bin", "rkmh")] + list(args), capture_output=True, env=env)
    assert r.returncode == 0, (args, r.stderr[-400:])
    return r.stdout.decode()


def _column(line, i):
    return int(line.split("\t")[i].split("/")[0]), int(line.split("\t")[i].split("/")[1])


def test_cli_on_the_panel(root, tmp_path):
    p = sc.panel("sourmash-k21")
    fa = tmp_path / "panel.fa"
    fa.write_bytes(b"".join(b">" + n + b"\n" + s + b"\n" for n, s in zip(p["names"], p["seqs"])))
    fa = str(fa)
    opts = ["--scaled", "10", "-k", "21", "--hash-policy", "sourmash"]
    dist = _run(root, "dist", "-r", fa, "-f", fa, *opts).splitlines(keepends=True)
    assert len(dist) == 40 * 40
    shared = [_column(ln, 3)[0] for ln in dist]
    want = "".join(ln for ln, s in zip(dist, shared) if s > 0)
    assert 40 < len(want.splitlines()) < 1600
    names = [n.decode() for n in p["names"]]
    sk = sc.sketches("sourmash-k21", 10)
    assert want == sem.search_text(names, sk, names, sk, 21)                                 # the model's lines, and dist's own
    assert _run(root, "manysearch", "-r", fa, "-f", fa, *opts) == want
    assert _run(root, "manysearch", "-r", fa, *opts) == want                                 # the self form
    want5 = "".join(ln for ln, s in zip(dist, shared) if s >= 5)
    assert 0 < len(want5) < len(want)
    assert _run(root, "manysearch", "-r", fa, "-f", fa, "--min-shared", "5", *opts) == want5
    half = "".join(ln for ln, s in zip(dist, shared) if s >= max(1, sem.min_count(0.5, _column(ln, 4)[1])))
    assert 40 <= len(half.splitlines()) < len(want.splitlines())
    assert _run(root, "manysearch", "-r", fa, "-f", fa, "--min-containment", "0.5", *opts) == half
    both = "".join(ln for ln, s in zip(dist, shared) if s >= max(5, sem.min_count(0.02, _column(ln, 4)[1])))
    assert _run(root, "manysearch", "-r", fa, "-f", fa, "--min-containment", "0.02", "--min-shared", "5", *opts) == both
    # -R / -Q round trips through `rkmh sketch --scaled`
    rj = str(tmp_path / "r.json")
    _run(root, "sketch", "-f", fa, "-o", rj, *opts)
    assert _run(root, "manysearch", "-R", rj, "-Q", rj, "--hash-policy", "sourmash") == want  # scaled and k come from the files
    assert _run(root, "manysearch", "-R", rj, "--hash-policy", "sourmash") == want
    assert _run(root, "manysearch", "-R", rj, "-f", fa, "--hash-policy", "sourmash", "--min-shared", "5") == want5
