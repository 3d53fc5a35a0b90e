"""Abundances on the GPU: the run lengths of the keep step through rk_sketch_scaled_abund_batch, the weighted removal of gather
through rk_gather_scaled_abund and rk_gather_scaled_abund_device, and `rkmh sketch --abund` / `rkmh gather --abund`, against
tests/abund_model.py -- everything integer, bit for bit.  What the shared inputs hold is shown on the model's output by
tests/test_abund_cpu.py."""
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
import sourmash_model as sm

pytestmark = pytest.mark.gpu

GUARD = 64
K = 16


# ---- the keep step ----
def _sketch(c, seqs, ks, mh):
    """-> list of (values, abund); the values must also be the plain entry's"""
    from rkmh_amd import api
    rb, ro = api.pack(seqs)
    v, a, off = c.sketch_scaled_abund_batch(rb, ro, ks, mh)
    pv, poff = c.sketch_scaled_batch(rb, ro, ks, mh)
    assert v.dtype == np.uint64 and a.dtype == np.uint32 and len(a) == len(v) == int(off[-1]) and off[0] == 0 and len(off) == len(seqs) + 1
    assert off.tolist() == poff.tolist() and v.tolist() == pv.tolist(), "the values differ from rk_sketch_scaled_batch's"
    return [(v[int(off[i]):int(off[i + 1])], a[int(off[i]):int(off[i + 1])]) for i in range(len(seqs))]


def _equal(got, want, what):
    assert len(got) == len(want), what
    for i, ((gv, ga), (wv, wa)) in enumerate(zip(got, want)):
        assert gv.tolist() == wv.tolist(), (what, i, "values", len(gv), len(wv))
        assert ga.tolist() == wa.tolist(), (what, i, "abundances", ga.tolist()[:8], wa.tolist()[:8])
        assert (ga >= 1).all()


def _model(seqs, ks=(K,), pol=sm.DEFAULT, mh=am.FULL):
    return [am.sketch(s, list(ks), pol, mh) for s in seqs]


def _above1(want):
    return sum(int((a > 1).sum()) for _, a in want)


def test_repeated_units(ctx):
    """L distinct k-mers m times over: runs of about m sorted values that cross the 64-lane and the 1 024-element boundaries"""
    seqs = [ac.repeated_unit(L, m, K + 1) for L, m in ac.REPEATS]                # (k + 1: the default policy hashes len - k windows)
    want = _model(seqs)
    for (L, m), (v, a) in zip(ac.REPEATS, want):
        assert 1 <= len(v) <= L and int(a.sum()) == L * m and int(a.max()) >= m, (L, m, len(v), a.tolist()[:4])
    assert int(want[3][1].sum()) > 2 * 1024 and int(want[2][1].max()) >= 65
    _equal(_sketch(ctx, seqs, [K], am.FULL), want, "all units in one batch")
    for s, w in zip(seqs, want):
        _equal(_sketch(ctx, [s], [K], am.FULL), [w], "one unit alone")
    cut = _model(seqs, mh=scm.max_hash(2))
    assert 0 < sum(len(v) for v, _ in cut) < sum(len(v) for v, _ in want)
    _equal(_sketch(ctx, seqs, [K], scm.max_hash(2)), cut, "scaled 2")


def test_homopolymers(ctx):
    """one value whose run spans five blocks and ends at the last kept value; then more kept values than the in-LDS sorter takes"""
    for n in (5000, 20000):
        want = _model([b"A" * n])
        assert len(want[0][0]) == 1 and int(want[0][1][0]) in (n - K, n - K + 1) and int(want[0][1][0]) > (4096 if n == 5000 else 16384)
        _equal(_sketch(ctx, [b"A" * n], [K], am.FULL), want, n)
    seqs = [b"A" * 20000, b"ACGTTGCA" * 30, b"A" * 5000]
    want = _model(seqs)
    assert _above1(want) >= 3
    _equal(_sketch(ctx, seqs, [K], am.FULL), want, "long runs in a batch")


def test_runs_do_not_merge_across_sequences(ctx):
    seqs = [b"A" * 30, b"A" * 40, b"T" * 25]
    want = _model(seqs)
    assert [len(v) for v, _ in want] == [1, 1, 1] and len({int(v[0]) for v, _ in want}) == 1           # one value, shared by all three
    assert [int(a[0]) for _, a in want] == [30 - K, 40 - K, 25 - K]
    _equal(_sketch(ctx, seqs, [K], am.FULL), want, "adjacent sequences that share their only value")


def test_empty_segments(ctx):
    rng = np.random.default_rng(3)
    rnd = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=700)])
    seqs = [b"", b"A" * 30, b"ACGTACGT", b"N" * 300, b"A" * 40, b"", b"", rnd + rnd, rnd[:K], b"N" * 20 + b"C" * 50 + b"N" * 20, b""]
    want = _model(seqs)
    assert [len(v) for v, _ in want][:7] == [0, 1, 0, 0, 1, 0, 0] and len(want[-1][0]) == 0 and len(want[-3][0]) == 0
    assert _above1(want) > 600                                                                         # every k-mer of rnd twice
    _equal(_sketch(ctx, seqs, [K], am.FULL), want, "empty segments between others, and last")
    _equal(_sketch(ctx, seqs[:5] + [b""], [K], am.FULL), want[:5] + [want[0]], "a batch whose last sequence is empty")
    _equal(_sketch(ctx, [b""], [K], am.FULL), [want[0]], "one empty sequence")
    _equal(_sketch(ctx, [b"", b"N" * 40, b"ACGT"], [K], am.FULL), [want[0]] * 3, "nothing kept at all")


@pytest.mark.parametrize("name", ["default-k12", "mash-k16", "sourmash-k21", "default-k12-k16"])
def test_panel_sketches(name):
    import rkmh_amd
    p = sc.panel(name)
    full = _model(p["seqs"], p["ks"], p["pol"])
    assert _above1(full) > 100
    c = rkmh_amd.Context(0, policy_spec=p["spec"])
    try:
        for scaled in (1, 10, 1000):
            mh = scm.max_hash(scaled)
            want = [am.downsample(v, a, mh) for v, a in full]
            assert [v.tolist() for v, _ in want] == [s.tolist() for s in sc.sketches(name, scaled)]
            _equal(_sketch(c, p["seqs"], p["ks"], mh), want, (name, scaled))
    finally:
        c.close()


def test_many_short_reads(ctx):
    from rkmh_amd import api, synth
    p = sc.panel("default-k12")
    rb, ro = api.pack(p["seqs"])
    qb, qo = synth.generate_reads_fast(rb, ro, 0, 3000)
    reads = [bytes(qb[int(qo[i]):int(qo[i + 1])]) for i in range(3000)]
    mh = scm.max_hash(1000)
    want = _model(reads, (8,), sm.DEFAULT, mh)                                   # k = 8: short enough for a read to repeat a kept k-mer
    assert _above1(want) >= 1 and 1500 < sum(1 for v, _ in want if len(v) == 0) < 3000
    v, a, off = ctx.sketch_scaled_abund_batch(qb, qo, [8], mh)
    _equal([(v[int(off[i]):int(off[i + 1])], a[int(off[i]):int(off[i + 1])]) for i in range(3000)], want, "3000 reads")


# ---- weighted gather ----
def _device(ctx, q, a, rv, ro, min_shared=1, max_rounds=None, r_nvalues=None):
    """the resident-input entry on torch's arrays and stream, guard words on both sides of the rows and of wunique"""
    import torch
    nref = len(ro) - 1
    rows = nref if max_rounds is None else max_rounds

    def up(x, dt, view):
        x = np.array(x, dtype=dt)                            # (a writable copy: the shared inputs are read-only)
        return torch.from_numpy((x if len(x) else np.zeros(1, dtype=dt)).view(view)).cuda()
    d_q, d_a, d_rv, d_ro = up(q, np.uint64, np.int64), up(a, np.uint32, np.int32), up(rv, np.uint64, np.int64), up(ro, np.uint64, np.int64)
    d_out = torch.full((GUARD + rows * 4 + GUARD,), -7, dtype=torch.int32, device="cuda")
    d_wu = torch.full((GUARD + rows + GUARD,), -7, dtype=torch.int64, device="cuda")
    n = ctx.gather_scaled_abund_device(d_q.data_ptr(), d_a.data_ptr(), len(q), d_rv.data_ptr(), d_ro.data_ptr(), nref,
                                       len(rv) if r_nvalues is None else r_nvalues, d_out.data_ptr() + 4 * GUARD, d_wu.data_ptr() + 8 * GUARD,
                                       min_shared=min_shared, max_rounds=max_rounds, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out, wu = d_out.cpu().numpy(), d_wu.cpu().numpy()
    assert 0 <= n <= rows
    assert (out[:GUARD] == -7).all() and (out[GUARD + 4 * n:] == -7).all(), "written outside the rows"
    assert (wu[:GUARD] == -7).all() and (wu[GUARD + rows:] == -7).all(), "written outside wunique"
    assert (wu[GUARD + n:GUARD + min(rows, nref)] == 0).all(), "wunique beyond the rows written is zero"
    return out[GUARD:GUARD + 4 * n].reshape(n, 4), wu[GUARD:GUARD + n].view(np.uint64)


def _plain_device(ctx, q, rv, ro, max_rounds=None):
    import torch
    nref = len(ro) - 1
    rows = nref if max_rounds is None else max_rounds
    d_q, d_rv, d_ro = (torch.from_numpy(np.array(x, dtype=np.uint64).view(np.int64)).cuda() for x in (q, rv, ro))
    d_out = torch.zeros(rows * 4, dtype=torch.int32, device="cuda")
    n = ctx.gather_scaled_device(d_q.data_ptr(), len(q), d_rv.data_ptr(), d_ro.data_ptr(), nref, len(rv), d_out.data_ptr(), max_rounds=max_rounds,
                                 stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()[:4 * n].reshape(n, 4)


def _same(got, want, what):
    rows, wu = got
    wrows, wwu = want
    assert rows.dtype == np.int32 and rows.shape == wrows.shape and (rows == wrows).all(), (what, rows.tolist()[:4], wrows.tolist()[:4])
    assert wu.dtype == np.uint64 and wu.tolist() == [int(x) for x in wwu], (what, wu.tolist()[:4], list(wwu)[:4])


def _both_entries(ctx, q, a, refs, want, what, min_shared=1, max_rounds=None):
    rv, ro = scm.csr(refs)
    _same(ctx.gather_scaled_abund(q, a, rv, ro, min_shared=min_shared, max_rounds=max_rounds), want, (what, "host entry"))
    _same(_device(ctx, q, a, rv, ro, min_shared, max_rounds), want, (what, "device entry"))


def test_hand_checked_vectors_both_entries(ctx):
    for v in ac.gather_kat():
        _both_entries(ctx, v["q"], v["abund"], v["refs"], (v["want"], v["wunique"]), v["name"], v["min_shared"], v["max_rounds"])


@pytest.mark.parametrize("nref", gc.NREFS)
def test_random_sets(ctx, nref):
    q, a, refs, want, wunique, left = ac.random_case(nref)
    assert len(want) >= min(3, nref) and any(int(w) > int(u) for w, u in zip(wunique.tolist(), want[:, 1].tolist()))
    _both_entries(ctx, q, a, refs, (want, wunique), nref)
    rv, ro = scm.csr(refs)
    plain = ctx.gather_scaled(q, rv, ro)
    assert (plain == want).all() and (_plain_device(ctx, q, rv, ro) == want).all(), "the rows differ from the plain call's"
    assert sum(int(x) for x in wunique) + left == int(a.astype(np.uint64).sum())
    ones = np.ones(len(q), dtype=np.uint32)                                       # all abundances 1: wunique = unique
    rows, wu = ctx.gather_scaled_abund(q, ones, rv, ro)
    assert (rows == want).all() and wu.tolist() == want[:, 1].tolist()
    cut = int(want[len(want) // 2, 1]) + 1
    wr, ww, _ = am.gather_weighted(q, a, refs, cut, 10 ** 6)
    _both_entries(ctx, q, a, refs, (wr, ww), (nref, "min_shared", cut), min_shared=cut, max_rounds=10 ** 6 if nref > 1 else None)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_pick_lists_around_the_wave_and_the_workgroup(ctx, n):
    q, a, refs = ac.list_of(n)
    rows, wu, left = am.gather_weighted(q, a, refs)
    assert rows[0].tolist()[:3] == [1, n, n] and len(rows) == (2 if n > 1 else 1) and wu[0] >= n and (n == 1 or wu[0] > (1 << 32))
    _both_entries(ctx, q, a, refs, (rows, wu), n)


def test_a_pick_list_beyond_the_removal_grid(ctx):
    """300 000 hits: more than 1 024 workgroups of 256 lanes, so the stride loop of k_gather_remove_w runs"""
    n = 300_000
    q, a, refs = ac.list_of(n)
    assert n > 1024 * 256
    rows, wu, left = am.gather_weighted(q, a, refs)
    assert rows[0].tolist()[:3] == [1, n, n] and wu[0] > (1 << 32) and wu[0] + wu[1] + left == int(a.astype(np.uint64).sum())
    _both_entries(ctx, q, a, refs, (rows, wu), "300 000 hits")


def test_abundances_of_2_32_minus_1(ctx):
    v = [x for x in ac.gather_kat() if x["name"].startswith("three abundances of 2^32 - 1")][0]
    assert int(v["wunique"][0]) == 3 * am.SAT > (1 << 33)
    _both_entries(ctx, v["q"], v["abund"], v["refs"], (v["want"], v["wunique"]), v["name"])
    q, a, refs = ac.list_of(257)
    heavy = np.full(len(q), am.SAT, dtype=np.uint32)
    rows, wu, _ = am.gather_weighted(q, heavy, refs)
    assert wu[0] == 257 * am.SAT
    _both_entries(ctx, q, heavy, refs, (rows, wu), "every abundance 2^32 - 1")


def test_round_group_boundaries(ctx):
    for n in (0, 1, 16, 17, 33):
        q, a, refs = ac.staircase(n)
        rows, wu, _ = am.gather_weighted(q, a, refs)
        assert len(rows) == n
        _both_entries(ctx, q, a, refs, (rows, wu), ("staircase", n))
    q, a, refs = ac.staircase(33)
    for max_rounds in (1, 16, 20):
        rows, wu, _ = am.gather_weighted(q, a, refs, 1, max_rounds)
        assert len(rows) == max_rounds
        _both_entries(ctx, q, a, refs, (rows, wu), ("staircase cut", max_rounds), max_rounds=max_rounds)


def test_reuse_of_a_context(ctx):
    """a weighted call, then a plain one, and the other way round: nothing of the first call survives into the second"""
    q, a, refs, want, wunique, _ = ac.random_case(65)
    rv, ro = scm.csr(refs)
    small = [v for v in ac.gather_kat() if v["name"].startswith("chain of three")][0]
    sv, so = scm.csr(small["refs"])
    for entry in ("host", "device"):
        def weighted(q_, a_, v_, o_):
            return ctx.gather_scaled_abund(q_, a_, v_, o_) if entry == "host" else _device(ctx, q_, a_, v_, o_)

        def plain(q_, v_, o_):
            return ctx.gather_scaled(q_, v_, o_) if entry == "host" else _plain_device(ctx, q_, v_, o_)
        _same(weighted(q, a, rv, ro), (want, wunique), (entry, "large, weighted"))
        assert (plain(small["q"], sv, so) == small["want"]).all(), (entry, "small and plain after large and weighted")
        _same(weighted(small["q"], small["abund"], sv, so), (small["want"], small["wunique"]), (entry, "small, weighted: no wunique of the large call"))
        assert (plain(q, rv, ro) == want).all(), (entry, "large and plain")
        _same(weighted(q, a, rv, ro), (want, wunique), (entry, "large, weighted again"))
        _same(weighted(small["q"], small["abund"], sv, so), (small["want"], small["wunique"]), (entry, "small, weighted again"))


def test_rows_are_clamped_on_the_device(ctx):
    rng = np.random.default_rng(8)
    pl = sc.pool(rng, 3000)
    A = sc.random_sets(rng, 4, pl, lengths=[65, 129, 1000])
    q = gc.query_of(rng, A, pl)
    a = ac.abundances(rng, len(q), heavy=0.5)
    rv, ro = scm.csr(A)
    # fewer values behind the pointer than the offsets say: row 2 is cut short, row 3 lies outside altogether
    n = int(ro[2]) + 10
    cut = [A[0], A[1], A[2][:10], A[3][:0]]
    rows, wu, _ = am.gather_weighted(q, a, cut)
    assert len(rows) == 3 and (rows == gm.gather(q, cut)).all()
    _same(_device(ctx, q, a, rv, ro, r_nvalues=n), (rows, wu), "fewer values")
    down = np.array([ro[1], ro[0], ro[1], ro[2]], dtype=np.uint64)           # offsets that decrease: an empty row
    rows, wu, _ = am.gather_weighted(q, a, [A[0][:0], A[0], A[1]])
    _same(_device(ctx, q, a, rv, down), (rows, wu), "decreasing offsets")
    zero = np.array(a)                                                       # the device entry cannot refuse an abundance of 0: it adds nothing
    zero[::2] = 0
    rows, wu, _ = am.gather_weighted(q, a, A)
    got_rows, got_wu = _device(ctx, q, zero, rv, ro)
    assert (got_rows == rows).all()
    alive = np.ones(len(q), dtype=bool)
    for t, r in enumerate(rows[:, 0].tolist()):
        hit = np.isin(q, A[r]) & alive
        assert int(got_wu[t]) == int(zero[hit].astype(np.uint64).sum())
        alive &= ~hit


def test_host_entry_refusals(ctx):
    from rkmh_amd import api
    v = [x for x in ac.gather_kat() if x["name"].startswith("chain of three")][0]
    rv, ro = scm.csr(v["refs"])
    q, a = v["q"], v["abund"]
    zero = np.array(a)
    zero[4] = 0
    for bad in (dict(q=q[::-1].copy()), dict(a=zero), dict(ro=np.array([0, 6, 3, 14], dtype=np.uint64)), dict(min_shared=0), dict(max_rounds=0)):
        k = dict(q=q, a=a, ro=ro, min_shared=1, max_rounds=None)
        k.update(bad)
        with pytest.raises(api.RkmhError) as e:
            ctx.gather_scaled_abund(k["q"], k["a"], rv, k["ro"], min_shared=k["min_shared"], max_rounds=k["max_rounds"])
        assert e.value.code == -1, bad
    with pytest.raises(ValueError):
        ctx.gather_scaled_abund(q, a[:-1], rv, ro)
    lib, h = ctx._lib, ctx._h
    n = api.C.c_int(0)
    for nq, nref, ms, mr, code in ((1, 0, 1, 1, -1), (1, 1, 0, 1, -1), (1, 1, 1, 0, -1), (1 << 31, 1, 1, 1, -5)):
        assert lib.rk_gather_scaled_abund_device(h, 8, 8, nq, 8, 8, nref, 1, ms, mr, 8, 8, api.C.byref(n), None) == code   # before anything is read
    assert lib.rk_gather_scaled_abund_device(h, 8, None, 1, 8, 8, 1, 1, 1, 1, 8, 8, api.C.byref(n), None) == -1           # NULL abundances
    assert lib.rk_gather_scaled_abund_device(h, 8, 8, 1, 8, 8, 1, 1, 1, 1, 8, None, api.C.byref(n), None) == -1           # NULL wunique
    _same(ctx.gather_scaled_abund(q, a, rv, ro), (v["want"], v["wunique"]), "and the context still works")


# ---- the commands ----
def _run(root, *args):
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    r = subprocess.run([os.path.join(root, "bin", "rkmh")] + list(args), capture_output=True, env=env)
    assert r.returncode == 0, (args, r.stderr[-400:])
    return r.stdout.decode()


def test_cli_sketch_abund(root, tmp_path, data_dir):
    p = sc.panel("zika-k16")
    rf = os.path.join(data_dir, "zika.refs.fa.gz")
    mh = scm.max_hash(10)
    want = _model(p["seqs"], (16,), sm.DEFAULT, mh)
    assert _above1(want) > 0
    doc = json.loads(_run(root, "sketch", "--scaled", "10", "--abund", "-k", "16", "-f", rf))
    assert [d["name"].encode() for d in doc] == list(p["names"])
    for d, (v, a) in zip(doc, want):
        assert d["sketches"]["hashes"] == v.tolist() and d["sketches"]["abundances"] == a.tolist() and d["sketches"]["length"] == len(v)
        assert list(d["sketches"]) == sorted(d["sketches"]) and d["scaled"] == 10                     # "abundances" in its alphabetical place
    one = json.loads(_run(root, "sketch", "--scaled", "10", "--abund", "-g", "-k", "16", "-f", rf))
    uv, ua = am.merge(want, mh)
    assert len(one) == 1 and one[0]["sketches"]["hashes"] == uv.tolist() and one[0]["sketches"]["abundances"] == ua.tolist()
    assert int(ua.astype(np.uint64).sum()) == sum(int(a.sum()) for _, a in want) and int(ua.max()) > max(int(a.max()) for _, a in want)
    # without --abund: the bytes of a file that knows no abundances, and the same hashes
    plain = _run(root, "sketch", "--scaled", "10", "-k", "16", "-f", rf)
    assert "abundances" not in plain and [d["sketches"]["hashes"] for d in json.loads(plain)] == [d["sketches"]["hashes"] for d in doc]
    # a file with abundances loads back: dist ignores the key
    js, pj = str(tmp_path / "a.json"), str(tmp_path / "p.json")
    _run(root, "sketch", "--scaled", "10", "--abund", "-k", "16", "-f", rf, "-o", js)
    open(pj, "w").write(plain)
    assert _run(root, "dist", "-R", js) == _run(root, "dist", "-R", pj)


@pytest.mark.parametrize("scaled", [10, 100])
def test_cli_gather_abund(root, tmp_path, data_dir, scaled):
    p = sc.panel("zika-k16")
    names = [n.decode() for n in p["names"]]
    refs = sc.sketches("zika-k16", scaled)
    qv, qa = ac.z1_query(scaled)
    rf, qf = os.path.join(data_dir, "zika.refs.fa.gz"), os.path.join(data_dir, "z1.fq.gz")
    want = am.gather_text([qf], [(qv, qa)], names, refs)
    assert len(want.split("\n")) == (17 if scaled == 10 else 7) + 1 and int((qa > 1).sum()) > 0
    opts = ["--scaled", str(scaled), "-k", "16"]
    assert _run(root, "gather", "--abund", "-r", rf, "-f", qf, *opts) == want
    # without --abund: today's format, byte for byte
    plain = gm.gather_text([qf], [qv], names, refs)
    assert _run(root, "gather", "-r", rf, "-f", qf, *opts) == plain
    assert [ln.split("\t")[:7] for ln in want.split("\n")[:-1]] == [ln.split("\t") for ln in plain.split("\n")[:-1]]
    if scaled == 100:
        # the query through -Q from a `sketch --abund -g` file made at scaled 10 and cut to 100; the references' abundances are ignored
        qj, rj = str(tmp_path / "q10.json"), str(tmp_path / "r10.json")
        _run(root, "sketch", "-g", "--abund", "-f", qf, "-o", qj, "--scaled", "10", "-k", "16")
        _run(root, "sketch", "--abund", "-f", rf, "-o", rj, "--scaled", "10", "-k", "16")
        assert _run(root, "gather", "--abund", "-r", rf, "-Q", qj, *opts) == want
        assert _run(root, "gather", "--abund", "-R", rj, "-Q", qj, "--scaled", "100") == want
        assert _run(root, "gather", "-R", rj, "-Q", qj, "--scaled", "100") == plain                     # plain gather ignores the key
        at10 = am.gather_text([qf], [ac.z1_query(10)], names, sc.sketches("zika-k16", 10))
        assert _run(root, "gather", "--abund", "-R", rj, "-Q", qj) == at10                             # without --scaled: the files' own
        assert _run(root, "gather", "--abund", "-r", rf, "-f", qf, "--max-rounds", "2", *opts) == "".join(ln + "\n" for ln in want.split("\n")[:2])
