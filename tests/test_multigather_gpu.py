"""Multigather on the GPU: the kernels of rk_multigather.hip through both entries (rk_multigather_scaled, rk_multigather_scaled_device)
against tests/gather_model.py and the existing gather entries query by query, and `rkmh multigather` against `rkmh gather` byte for
byte.  What the shared inputs exercise is shown on the model's output by tests/test_multigather_cpu.py."""
import os
import subprocess

import numpy as np
import pytest

import abund_cases as ac
import abund_model as am
import gather_cases as gc
import multigather_cases as mc
import scaled_cases as sc
import scaled_model as scm
import search_cases as sec

pytestmark = pytest.mark.gpu

GUARD = 64


def _up(x, dtype=np.uint64):
    import torch
    x = np.array(x, dtype=dtype)                                 # (a writable copy: the shared inputs are read-only)
    x = x if len(x) else np.zeros(1, dtype=dtype)
    return torch.from_numpy(x.view(np.int64 if dtype == np.uint64 else np.int32)).cuda()


def _device(idx, queries, abunds=None, min_shared=1, max_rounds=None, cap=None, q_nvalues=None, qo=None):
    """the resident-input entry on torch's arrays and stream, guard words on both sides of the rows, of wunique and of the row offsets
    -> (total, the rows written, row_offsets, wunique written or None)"""
    import torch
    qv, off = scm.csr(queries)
    qo = off if qo is None else qo
    nq = len(qo) - 1
    d_qv, d_qo = _up(qv), _up(qo)
    d_qa = None if abunds is None else _up(np.concatenate([np.zeros(0, np.uint32)] + [np.asarray(a, np.uint32) for a in abunds]), np.uint32)
    st = torch.cuda.current_stream().cuda_stream
    nv = len(qv) if q_nvalues is None else q_nvalues
    d_off = torch.full((GUARD + nq + 1 + GUARD,), -7, dtype=torch.int64, device="cuda")
    if cap is None:                                              # room for exactly the rows there are: asked for with room for none
        cap = idx.multigather_device(d_qv.data_ptr(), d_qo.data_ptr(), nq, nv, 0, d_off.data_ptr() + 8 * GUARD, 0, d_q_abund_ptr=None if d_qa is None else d_qa.data_ptr(),
                                     min_shared=min_shared, max_rounds=max_rounds, stream=st)
    d_out = torch.full((GUARD + cap * 4 + GUARD,), -7, dtype=torch.int32, device="cuda")
    d_wu = torch.full((GUARD + cap + GUARD,), -7, dtype=torch.int64, device="cuda")
    n = idx.multigather_device(d_qv.data_ptr(), d_qo.data_ptr(), nq, nv, d_out.data_ptr() + 4 * GUARD, d_off.data_ptr() + 8 * GUARD, cap,
                               d_q_abund_ptr=None if d_qa is None else d_qa.data_ptr(), d_wunique_ptr=d_wu.data_ptr() + 8 * GUARD,
                               min_shared=min_shared, max_rounds=max_rounds, stream=st)
    torch.cuda.synchronize()
    out, wu, ro = d_out.cpu().numpy(), d_wu.cpu().numpy(), d_off.cpu().numpy()
    w = min(n, cap)
    assert (out[:GUARD] == -7).all() and (out[GUARD + 4 * w:] == -7).all(), "written outside the rows"
    assert (ro[:GUARD] == -7).all() and (ro[GUARD + nq + 1:] == -7).all(), "written outside the row offsets"
    if abunds is None:
        assert (wu == -7).all(), "wunique written by a plain call"
    else:
        assert (wu[:GUARD] == -7).all() and (wu[GUARD + w:] == -7).all(), "written outside wunique"
    ro = ro[GUARD:GUARD + nq + 1].view(np.uint64).copy()
    assert ro[0] == 0 and ro[-1] == n and (np.diff(ro.astype(np.int64)) >= 0).all()
    return n, out[GUARD:GUARD + 4 * w].reshape(w, 4).copy(), ro, (None if abunds is None else wu[GUARD:GUARD + w].view(np.uint64).copy())


def _same(got, want, what):
    rows, off, wu = got
    wrows, woff, wwu = want
    assert rows.dtype == np.int32 and rows.shape == wrows.shape and (rows == wrows).all(), (what, rows.tolist()[:4], wrows.tolist()[:4])
    assert off.dtype == np.uint64 and off.tolist() == woff.tolist(), (what, off.tolist()[:8], woff.tolist()[:8])
    if wwu is None:
        assert wu is None, what
    else:
        assert wu is not None and wu.dtype == np.uint64 and wu.tolist() == wwu.tolist(), (what, wu.tolist()[:4], wwu.tolist()[:4])


def _host_entry(idx, queries, abunds=None, **kw):
    qv, qo = scm.csr(queries)
    qa = None if abunds is None else np.concatenate([np.zeros(0, np.uint32)] + [np.asarray(a, np.uint32) for a in abunds])
    return idx.multigather(qv, qo, q_abund=qa, **kw)


def _both_entries(idx, queries, want, what, abunds=None, min_shared=1, max_rounds=None):
    _same(_host_entry(idx, queries, abunds, min_shared=min_shared, max_rounds=max_rounds), want, (what, "host entry"))
    n, rows, ro, wu = _device(idx, queries, abunds, min_shared, max_rounds)
    assert n == len(want[0])
    _same((rows, ro, wu), want, (what, "device entry"))


def _index(ctx, refs):
    rv, ro = scm.csr(refs)
    return ctx.scaled_index(rv, ro)


def test_hand_checked_vectors_both_entries(ctx):
    for v in mc.kat_batches():
        idx = _index(ctx, v["refs"])
        _both_entries(idx, v["queries"], v["want"], v["name"], min_shared=v["min_shared"], max_rounds=v["max_rounds"])
        idx.close()


@pytest.mark.parametrize("nref", gc.NREFS)
def test_random_sets(ctx, nref):
    b = mc.random_batch(nref)
    refs, queries = b["refs"], b["queries"]
    idx = _index(ctx, refs)
    full = mc.answer(refs, queries)
    _both_entries(idx, queries, full, nref)
    ms = mc.median_count(full)
    _both_entries(idx, queries, mc.answer(refs, queries, ms), (nref, "min_shared", ms), min_shared=ms)
    _both_entries(idx, queries, mc.cut(full, 2), (nref, "max_rounds 2"), max_rounds=2)
    idx.close()


def test_equal_to_gather_on_the_same_resident_arrays(ctx):
    import torch
    b = mc.random_batch(65)
    refs, queries = b["refs"], b["queries"]
    rv, ro = scm.csr(refs)
    d_rv, d_ro = _up(rv), _up(ro)
    st = torch.cuda.current_stream().cuda_stream
    idx = ctx.scaled_index_device(d_rv.data_ptr(), d_ro.data_ptr(), len(refs), len(rv), stream=st)
    n, rows, off, _ = _device(idx, queries, min_shared=3)
    d_out = torch.full((len(refs), 4), -1, dtype=torch.int32, device="cuda")
    for i, q in enumerate(queries):
        d_q = _up(q)
        m = ctx.gather_scaled_device(d_q.data_ptr(), len(q), d_rv.data_ptr(), d_ro.data_ptr(), len(refs), len(rv), d_out.data_ptr(), min_shared=3, stream=st)
        torch.cuda.synchronize()
        mine = rows[int(off[i]):int(off[i + 1])]
        assert m == len(mine) and (d_out.cpu().numpy()[:m] == mine).all(), i
    idx.close()


def test_round_groups_and_finished_queries(ctx):
    from rkmh_amd import api
    assert api.RK_GATHER_BATCH == 16
    s = mc.staircases()
    refs, queries = s["refs"], s["queries"]
    idx = _index(ctx, refs)
    full = mc.answer(refs, queries)
    assert np.diff(full[1].astype(np.int64)).tolist() == [0, 1, 15, 16, 17, 33, 0]
    _both_entries(idx, queries, full, "staircases")                          # the queries that finish early stay as written while the 33 goes on
    for mr in (1, 16, 17):
        want = mc.answer(refs, queries, 1, mr)
        assert int(np.diff(want[1].astype(np.int64))[5]) == mr
        _both_entries(idx, queries, want, ("staircases cut", mr), max_rounds=mr)
    idx.close()


def test_ties(ctx):
    t = mc.ties()
    idx = _index(ctx, t["refs"])
    want = mc.answer(t["refs"], t["queries"])
    later = mc.blocks(want)[t["later"]][0]
    assert later[:, 0].tolist() == [5, 6, 7] and later[1, 1] == later[2, 1]
    _both_entries(idx, t["queries"], want, "ties")
    idx.close()


@pytest.mark.parametrize("nref", sec.BLOCK_EDGE_NREFS)
def test_block_edges(ctx, nref):
    c = mc.block_edges(nref)
    refs, queries = c["refs"], c["queries"]
    idx = _index(ctx, refs)
    assert idx.stats()["longest_posting"] == nref                             # one value held by every reference: its list spans every block
    want = mc.answer(refs, queries, host=True)
    picked = set(mc.blocks(want)[0][0][:, 0].tolist())
    assert set(c["edge"]) <= picked and len(picked) > len(c["edge"])          # the first and the last reference of every block are picked
    first = mc.blocks(want)[0][0]
    assert int(first[0, 1]) == 3 and (first[1:, 1] <= 2).all()                # the first pick takes EVERY out: every candidate's count falls
    _both_entries(idx, queries, want, nref)
    idx.close()


@pytest.mark.parametrize("length", sec.POSTING_LENGTHS)
def test_posting_lists_around_the_whole_wave_walk(ctx, length):
    c = sec.posting_lists(length)
    refs = c["refs"]
    idx = _index(ctx, refs)
    assert idx.stats()["longest_posting"] == length
    own = np.array([1000 + r for r in (100, 101, 150, 299)], dtype=np.uint64)  # the values of their own of four references, and LONG and SHORT
    queries = tuple(c["queries"]) + (np.unique(np.concatenate([own, c["queries"][1]])),)
    want = mc.answer(refs, queries)
    last = mc.blocks(want)[3][0]
    assert last[0].tolist()[:2] == [150, 3] and len(last) >= 4                 # reference 150 holds its own value, SHORT and LONG; LONG then leaves every list
    _both_entries(idx, queries, want, length)
    idx.close()


def test_many_queries_their_order_and_repeats(ctx):
    m = mc.many_queries()
    refs, queries = m["refs"], m["queries"]
    idx = _index(ctx, refs)
    want = mc.answer(refs, queries, host=True)
    _both_entries(idx, queries, want, "65 queries of 0 ... 4097 values")
    per = mc.blocks(want)
    perm = np.random.default_rng(3).permutation(len(queries))
    n, rows, off, _ = _device(idx, [queries[i] for i in perm])
    for at, i in enumerate(perm):
        assert (rows[int(off[at]):int(off[at + 1])] == per[i][0]).all(), (at, i)
    twice = (queries[13], queries[27], queries[13])
    got = mc.blocks(_host_entry(idx, twice))
    assert len(got[0][0]) >= 2 and (got[0][0] == got[2][0]).all() and (got[0][0] == per[13][0]).all()
    first = _device(idx, queries)
    again = _device(idx, queries)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first[1:3], again[1:3]))   # two runs: identical bytes
    idx.close()


def test_capacity(ctx):
    b = mc.random_batch(65)
    want = mc.answer(b["refs"], b["queries"], abunds=b["abunds"])
    total = len(want[0])
    assert total > 3
    idx = _index(ctx, b["refs"])
    for cap in (0, 1, total - 1, total, total + 5):
        n, rows, ro, wu = _device(idx, b["queries"], b["abunds"], cap=cap)     # (the guard words and the tails are checked in there)
        w = min(cap, total)
        assert n == total and ro.tolist() == want[1].tolist()                   # row_offsets is complete whatever the room
        assert (rows == want[0][:w]).all() and wu.tolist() == want[2][:w].tolist(), cap
    idx.close()


def test_rows_are_clamped_and_refusals(ctx):
    import rkmh_amd
    from rkmh_amd import api
    b = mc.random_batch(9)
    refs, Q = b["refs"], [b["queries"][i] for i in (0, 3, 5)]
    idx = _index(ctx, refs)
    qv, qo = scm.csr(Q)
    m = int(qo[1]) + 7                                                        # fewer values behind the pointer than the offsets say
    n, rows, ro, _ = _device(idx, Q, q_nvalues=m)
    _same((rows, ro, None), mc.answer(refs, [Q[0], Q[1][:7], Q[2][:0]]), "fewer query values")
    n, rows, ro, _ = _device(idx, Q, qo=np.array([qo[1], qo[0], qo[1], qo[2]], dtype=np.uint64))   # offsets that decrease: an empty row
    _same((rows, ro, None), mc.answer(refs, [Q[0][:0], Q[0], Q[1]]), "decreasing query offsets")
    with pytest.raises(ValueError):
        idx.multigather(qv[:m], qo)                                           # offsets past the values: refused by the bindings
    for bad in (dict(qo=np.array([qo[1], qo[0], qo[1], qo[2]], dtype=np.uint64)), dict(min_shared=0), dict(max_rounds=0), dict(max_rounds=-1),
                dict(qv=qv[::-1].copy()), dict(qa=np.zeros(len(qv), np.uint32))):
        a = dict(qv=qv, qo=qo, min_shared=1, max_rounds=None, qa=None)
        a.update(bad)
        with pytest.raises(api.RkmhError) as e:
            idx.multigather(a["qv"], a["qo"], q_abund=a["qa"], min_shared=a["min_shared"], max_rounds=a["max_rounds"])
        assert e.value.code == -1, bad
    lib, h = ctx._lib, ctx._h
    k = api.C.c_uint64()
    for nq, ms, mr, code in ((0, 1, 1, -1), (1, 0, 1, -1), (1, 1, 0, -1), (1 << 31, 1, 1, -5), (1 << 24, 1, 1, -5)):
        assert lib.rk_multigather_scaled_device(h, idx._h, 8, None, 8, nq, 1, ms, mr, 8, None, 1, 8, api.C.byref(k), None) == code   # before anything is read
    assert lib.rk_multigather_scaled_device(h, idx._h, 8, None, None, 1, 1, 1, 1, 8, None, 1, 8, api.C.byref(k), None) == -1
    assert lib.rk_multigather_scaled_device(h, idx._h, 8, None, 8, 1, 1, 1, 1, 8, None, 1, None, api.C.byref(k), None) == -1
    assert lib.rk_multigather_scaled_device(h, idx._h, 8, None, 8, 1, 1, 1, 1, None, None, 1, 8, api.C.byref(k), None) == -1
    assert lib.rk_multigather_scaled_device(h, idx._h, 8, 8, 8, 1, 1, 1, 1, 8, None, 1, 8, api.C.byref(k), None) == -1          # abundances and no wunique
    other = rkmh_amd.Context(0)
    off = np.zeros(len(qo), np.uint64)
    out, w = api._i32p(), api._u64p()
    assert other._lib.rk_multigather_scaled(other._h, idx._h, api._p(qv, api.C.c_uint64), None, api._p(qo, api.C.c_uint64), len(qo) - 1, 1, 1,
                                            api.C.byref(out), api.C.byref(w), api._p(off, api.C.c_uint64), api.C.byref(k)) == -1   # an index of another context
    other.close()
    _both_entries(idx, Q, mc.answer(refs, Q), "and the index still works")
    idx.close()


def test_an_index_serves_searches_and_multigathers_in_turn(ctx):
    import search_model as sem
    b = mc.random_batch(65)
    refs, queries = b["refs"], b["queries"]
    idx = _index(ctx, refs)
    qv, qo = scm.csr(queries)
    hits = sem.search(refs, queries)
    assert (idx.search(qv, qo) == hits).all()
    _both_entries(idx, queries[:2], mc.answer(refs, queries[:2]), "two queries after a search of six")
    assert (idx.search(qv, qo, min_shared=2) == hits[hits[:, 2] >= 2]).all()
    _both_entries(idx, queries, mc.answer(refs, queries), "six after two")
    one, oo = scm.csr(queries[3:4])
    assert (idx.search(one, oo) == sem.search(refs, queries[3:4])).all()
    idx.close()


@pytest.mark.parametrize("nref", (9, 65))
def test_abundances(ctx, nref):
    b = mc.random_batch(nref)
    refs, queries, abunds = b["refs"], b["queries"], b["abunds"]
    idx = _index(ctx, refs)
    want = mc.answer(refs, queries, abunds=abunds, host=True)
    assert max(int(a.max()) for a in abunds if len(a)) == am.SAT              # abundances of 2^32 - 1
    _both_entries(idx, queries, want, nref, abunds=abunds)
    q, a, two = ac.list_of(130)                                               # a first pick of 130 values, two of them 2^32 - 1: a sum past 32 bits
    lidx = _index(ctx, two)
    lwant = mc.answer(two, (q, q), abunds=(a, a), host=True)
    assert int(lwant[2][0]) > 2 * am.SAT - 2 and lwant[0][0].tolist()[:2] == [1, 130]
    _both_entries(lidx, (q, q), lwant, "list of 130", abunds=(a, a))
    lidx.close()
    _both_entries(idx, queries, mc.answer(refs, queries, 2, 3, abunds=abunds, host=True), (nref, 2, 3), abunds=abunds, min_shared=2, max_rounds=3)
    ones = tuple(np.ones(len(q), np.uint32) for q in queries)
    rows, off, wu = _host_entry(idx, queries, ones)
    assert (wu == rows[:, 1].astype(np.uint64)).all()                         # all abundances 1: wunique = unique
    rows, off, wu = _host_entry(idx, queries, abunds)
    for i, (q, a) in enumerate(zip(queries, abunds)):                         # sum(wunique) + the abundances left alive = wtotal
        mine = rows[int(off[i]):int(off[i + 1])]
        gone = np.zeros(len(q), bool)
        for r in mine[:, 0].tolist():
            gone |= np.isin(q, refs[r])
        assert int(wu[int(off[i]):int(off[i + 1])].sum()) + int(a[~gone].astype(np.uint64).sum()) == int(np.asarray(a, np.uint64).sum()), i
    for v in ac.gather_kat():
        small = _index(ctx, v["refs"])
        got = _host_entry(small, (v["q"], v["q"]), (v["abund"], v["abund"]), min_shared=v["min_shared"], max_rounds=v["max_rounds"] or None)
        assert got[0].tolist() == v["want"].tolist() * 2 and got[2].tolist() == v["wunique"].tolist() * 2, v["name"]
        small.close()
    idx.close()


# ---- the command: the bytes of `rkmh gather` ----
def _run(root, *args):
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    r = subprocess.run([os.path.join(root, "bin", "rkmh")] + list(args), capture_output=True, env=env)
    assert r.returncode == 0, (args, r.stderr[-400:])
    return r.stdout


def _write_fasta(path, names, seqs):
    path.write_bytes(b"".join(b">" + n + b"\n" + s + b"\n" for n, s in zip(names, seqs)))
    return str(path)


@pytest.mark.parametrize("scaled", (10, 100))
def test_cli_prints_the_bytes_of_gather(root, tmp_path, data_dir, scaled):
    p = sc.panel("zika-k16")
    sample = [p["seqs"][i] for i in (2, 7, 11)] + [p["seqs"][20][:len(p["seqs"][20]) // 2]]
    rf = os.path.join(data_dir, "zika.refs.fa.gz")
    qf = _write_fasta(tmp_path / "sample.fa", [b"a", b"b", b"c", b"d"], sample)
    q2 = _write_fasta(tmp_path / "other.fa", [b"e", b"f"], [p["seqs"][5], p["seqs"][30]])
    lone = _write_fasta(tmp_path / "lone.fa", [b"n"], [b"ACGT" * 100])
    opts = ["--scaled", str(scaled), "-k", "16"]
    qj, rj, qja, q3 = (str(tmp_path / n) for n in ("q.json", "r.json", "qa.json", "q3.json"))
    _run(root, "sketch", "-g", "-f", qf, "-o", qj, *opts)
    _run(root, "sketch", "-f", rf, "-o", rj, *opts)
    _run(root, "sketch", "-g", "-f", qf, "-o", qja, "--abund", *opts)
    _run(root, "sketch", "-f", q2, "-o", q3, *opts)                           # two sketches in one -Q file: two queries
    runs = (["-r", rf, "-f", qf, *opts], ["-r", rf, "-f", qf, "--abund", *opts], ["-r", rf, "-f", qf, "--min-shared", "5", *opts],
            ["-r", rf, "-f", lone, "-f", qf, "-f", q2, "-f", qf, "--max-rounds", "2", *opts], ["-R", rj, "-Q", qj], ["-R", rj, "-Q", qja, "--abund"],
            ["-R", rj, "-Q", q3, "-Q", qj, "--min-shared", "5"])
    seen = set()
    for args in runs:
        want = _run(root, "gather", *args)
        assert _run(root, "multigather", *args) == want, args
        seen.add(want)
    assert len(seen) >= 4 and all(len(s.split(b"\n")) >= 2 for s in seen)    # the runs differ from one another, and every one prints lines
