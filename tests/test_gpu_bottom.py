"""Bottom samples on the GPU (rk_sample_create_bottom, rk_sample_finish_bottom, rk_sample_bottom_state, rk_bottom_cut; include/
rkmh_amd.h "BOTTOM SAMPLES"): the cut against the model's cut on synthetic sets, and whole samples against the definition
(tests/bottom_model.py) and, at min_copies = 1, against rk_sketch_batch + rk_merge_sketches, integer for integer.  What the shared
inputs (tests/bottom_cases.py) hold is shown on the model by tests/test_bottom_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import bottom_cases as bc
import bottom_model as bm
import sample_cases as sc

pytestmark = pytest.mark.gpu

K = bc.K


@pytest.fixture(scope="module")
def contexts():
    """one context per policy, none with references"""
    import rkmh_amd
    cs = {name: rkmh_amd.Context(0, policy_spec=name) for name in bc.POLICIES}
    yield cs
    for c in cs.values():
        c.close()


@pytest.fixture(scope="module")
def c(contexts):
    return contexts["default"]


# ---- the cut ----
def test_cut_on_synthetic_sets(c):
    from rkmh_amd import api
    for name, (counts, S, m, distinct, place) in bc.cut_cases().items():
        v = bc.values(len(counts))
        want = bm.cut(v, counts, S, m, distinct)
        assert want[0] == place, name
        assert api.bottom_cut(v, counts, S, m, distinct, ctx=c) == want, name
    assert c.bottom_cut(np.zeros(0, np.uint64), np.zeros(0, np.uint32), 5) == (0, 0)


def test_cut_module_function_makes_its_own_context():
    from rkmh_amd import api
    counts, S, m, distinct, place = bc.cut_cases()["place 257 multiset m=2"]
    v = bc.values(len(counts))
    assert api.bottom_cut(v, counts, S, m, distinct) == (place, int(v[place - 1]))


def test_cut_where_the_scan_takes_two_sums_per_thread(c):
    counts, S, m, distinct, place = bc.wide_case()
    v = bc.values(len(counts))
    assert c.bottom_cut(v, counts, S, m, distinct) == (place, int(v[place - 1]))
    assert c.bottom_cut(v, counts, S, 4, distinct) == (0, 0)                  # nothing has four copies
    assert c.bottom_cut(v, counts, 5, 3, distinct) == (len(v), int(v[-1]))   # the five of three copies: the very last entry


def test_cut_refusals(c):
    import rkmh_amd
    lib = c._lib
    v, a = bc.values(4), np.ones(4, np.uint32)
    n, t = C.c_uint64(), C.c_uint64()
    pv, pa = v.ctypes.data_as(C.POINTER(C.c_uint64)), a.ctypes.data_as(C.POINTER(C.c_uint32))
    call = lambda ctx, vv, aa, nn, S, m, on, ot: lib.rk_bottom_cut(ctx, vv, aa, C.c_uint64(nn), S, C.c_uint64(m), 0, on, ot)
    assert call(c._h, pv, pa, 4, 2, 1, C.byref(n), C.byref(t)) == 0 and (n.value, t.value) == (2, int(v[1]))
    assert call(None, pv, pa, 4, 2, 1, C.byref(n), C.byref(t)) != 0
    assert call(c._h, None, pa, 4, 2, 1, C.byref(n), C.byref(t)) != 0
    assert call(c._h, pv, None, 4, 2, 1, C.byref(n), C.byref(t)) != 0
    assert call(c._h, pv, pa, 4, 2, 1, None, C.byref(t)) != 0
    assert call(c._h, pv, pa, 4, 2, 1, C.byref(n), None) != 0
    for S, m in ((0, 1), (-1, 1), (bc.MAX_SKETCH + 1, 1), (2, 0), (2, 1 << 32)):
        assert call(c._h, pv, pa, 4, S, m, C.byref(n), C.byref(t)) != 0, (S, m)
    assert call(c._h, pv, pa, (1 << 31) * bc.KEEP_BLK, 2, 1, C.byref(n), C.byref(t)) != 0    # refused before the arrays are looked at
    with pytest.raises(rkmh_amd.RkmhError, match="sketch size"):
        c.bottom_cut(v, a, 0)
    with pytest.raises(ValueError):
        c.bottom_cut(v, a[:3], 2)


# ---- samples ----
def _feed(ctx, groups, ks=(K,), S=1000, m=1, pending_cap=0, watch=None):
    """a fresh bottom sample fed group by group -> (row, len, bottom_state, stats); watch: takes the state after every feed"""
    s = ctx.sample_bottom(list(ks), S, m, pending_cap=pending_cap)
    try:
        for g in groups:
            b, off = sc.pack(g)
            s.add(b, off)
            if watch is not None:
                watch.append(s.bottom_state())
        row, n = s.finish_bottom()
        return row, n, s.bottom_state(), s.stats()
    finally:
        s.close()


def _check(ctx, policy, reads, ks=(K,), S=1000, m=1, groups=None, pending_cap=0, what=""):
    pol, distinct = bc.POLICIES[policy], bc.DISTINCT[policy]
    assert bool(ctx.policy.dedup) == distinct
    want = bm.direct(reads, ks, pol, S, m, distinct)
    row, n, state, st = _feed(ctx, groups if groups is not None else [list(reads)], ks, S, m, pending_cap)
    assert row.dtype == np.uint64 and len(row) == S
    assert n == len(want) and row[:n].tolist() == want, (what, n, len(want))
    assert not row[n:].any(), (what, "padding")
    assert st["nseq"] == len(reads) and st["nbases"] == sum(len(r) for r in reads), (what, st)
    if n == S:
        assert state["threshold"] >= want[-1] and state["qualifying_weight"] >= S, (what, state)
    if m == 1:   # the route `-g` has always taken: per-read rows united on the host
        from rkmh_amd import api
        b, off = sc.pack(reads)
        sk, ln = ctx.sketch_batch(b, off, list(ks), S)
        lrow, ln1 = api.merge_sketches(sk, ln, S, distinct=distinct)
        assert ln1 == n and lrow.tolist() == row.tolist(), (what, "rk_sketch_batch + rk_merge_sketches differ")
    return state, st


@pytest.mark.parametrize("policy", ["default", "mash", "sourmash"])
@pytest.mark.parametrize("ks", [(16,), (21,), (31,), (12, 16)])
def test_policies_and_k(contexts, policy, ks):
    reads = list(bc.reads300()[:40]) + [sc.tile_batch()[0][21]]   # 40 short reads and the 5 000-base one
    assert len(reads[-1]) == 5000
    for m in (1, 2):
        _check(contexts[policy], policy, reads, ks=ks, S=1000, m=m, groups=sc.batches(reads, 9), what=(policy, ks, m))


@pytest.mark.parametrize("policy", ["default", "sourmash"])
@pytest.mark.parametrize("S", [1, 64, 1000, bc.MAX_SKETCH])
def test_sketch_sizes(contexts, policy, S):
    reads = list(bc.reads300()[:160])     # some 21 000 windows: more than the largest sketch
    state, _ = _check(contexts[policy], policy, reads, S=S, groups=sc.batches(reads, 20), what=(policy, S))
    assert state["cuts"] >= 1, state


@pytest.mark.parametrize("policy", ["default", "sourmash"])
def test_fewer_values_than_the_sketch(contexts, policy):
    reads = list(bc.reads300()[:5])
    state, _ = _check(contexts[policy], policy, reads, S=5000, what="len < S")
    assert state["cuts"] == 0 and state["threshold"] == bm.FULL and state["qualifying_weight"] < 5000, state
    state, _ = _check(contexts[policy], policy, reads, S=5000, m=2, what="len < S, m = 2")
    assert state["cuts"] == 0
    row, n, state, st = _feed(contexts[policy], [], S=7)
    assert n == 0 and not row.any() and state["candidates"] == 0 and st["nseq"] == 0


@pytest.mark.parametrize("policy", ["default", "sourmash"])
@pytest.mark.parametrize("m", [1, 2, 3])
def test_min_copies(contexts, policy, m):
    reads = list(bc.reads300())
    _check(contexts[policy], policy, reads, S=300, m=m, groups=sc.batches(reads, 25), what=(policy, m))


@pytest.mark.parametrize("policy", ["default", "sourmash"])
def test_reads_fed_twice_in_different_batches(contexts, policy):
    first, again = bc.twice()
    groups = sc.batches(first, 11) + sc.batches(again, 17)
    state, _ = _check(contexts[policy], policy, list(first) + list(again), S=500, m=2, groups=groups, what="fed twice")
    assert state["cuts"] >= 1


def test_feeds_of_seven_at_every_capacity(c):
    reads = bc.reads300()
    groups = sc.batches(reads, bc.FOLD_BATCH)
    for m in (1, 2):
        want = bm.direct(reads, (K,), bc.POLICIES["default"], bc.FOLD_S, m, False)
        rows = []
        for cap in bc.FOLD_CAPS:
            watch = []
            row, n, state, st = _feed(c, groups, S=bc.FOLD_S, m=m, pending_cap=cap, watch=watch)
            assert row[:n].tolist() == want and n == len(want), (m, cap)
            assert state["cuts"] >= 3, (m, cap, state)
            t = [w["threshold"] for w in watch] + [state["threshold"]]
            assert all(a >= b for a, b in zip(t, t[1:])) and t[0] <= bm.FULL and t[-1] < t[0], (m, cap)
            assert st["nseq"] == 300
            if cap == 1:
                assert st["retries"] >= 1, st
            rows.append(row.tolist())
        assert all(r == rows[0] for r in rows)


@pytest.mark.parametrize("policy", ["default", "sourmash"])
def test_order_and_grouping(contexts, policy):
    reads = list(bc.reads300()[:120])
    rng = np.random.default_rng(6)
    perm = [reads[i] for i in rng.permutation(len(reads))]
    for m in (1, 2):
        for groups in ([reads], [perm], [reads[:1], reads[1:]], [reads[:77], reads[77:100], [], reads[100:]], sc.batches(perm, 13)):
            _check(contexts[policy], policy, reads, S=200, m=m, groups=groups, pending_cap=2000, what=(policy, m, len(groups)))


@pytest.mark.parametrize("policy", ["default", "sourmash"])
def test_homopolymer(contexts, policy):
    h = sc.homopolymer()
    state, _ = _check(contexts[policy], policy, [h], S=1000, what="one homopolymer")
    assert state["candidates"] == 1
    _check(contexts[policy], policy, [h, bc.reads300()[2], h], S=1000, m=2, pending_cap=1000, what="two homopolymers around a read")
    _check(contexts[policy], policy, [h, bc.reads300()[2], h], S=50, groups=[[h], [bc.reads300()[2]], [h]], what="S below the count")


@pytest.mark.parametrize("policy", ["default", "mash"])
def test_read_and_tile_edges(contexts, policy):
    _check(contexts[policy], policy, sc.edge_reads(), S=100, what="edge reads")
    _check(contexts[policy], policy, sc.edge_reads() + sc.edge_reads()[:9], S=20, m=2, groups=[sc.edge_reads(), sc.edge_reads()[:9]], what="edge reads, m = 2")
    reads, on_boundary = sc.tile_batch()
    assert sc.starts(reads)[on_boundary] == sc.HASH_TILE_WIN
    _check(contexts[policy], policy, reads, S=1000, what="tile batch")
    _check(contexts[policy], policy, [b"A"] + list(reads), ks=(21,), S=1000, what="tile batch shifted by one, k = 21")


def test_a_batch_larger_than_the_first_sub_batch(c):
    reads = bc.many_short()
    state, st = _check(c, "default", reads, S=1000, what="5 000 reads in one feed")
    assert state["cuts"] >= 1 and st["folds"] >= 2, (state, st)    # the first 4 096 reads were folded and cut before the rest went in
    _check(c, "default", reads, S=1000, m=2, what="5 000 reads in one feed, m = 2")


def test_slot_into_a_bottom_sample(c):
    from rkmh_amd import api
    reads, text = sc.fastq200()
    want = bm.direct(reads, (K,), bc.POLICIES["default"], 500, 1, False)
    slot = api.FastqSlot(c, max_bytes=1 << 16)
    s = c.sample_bottom([K], 500)
    try:
        assert slot.sample(text, s) == (0, 200)
        row, n = s.finish_bottom()
        assert n == len(want) == 500 and row.tolist() == want
        status, _ = slot.sample(sc.fastq_with_cr(), s)                       # refused whole: the sample as it was
        assert status != 0
        row2, n2 = s.finish_bottom()
        assert row2.tolist() == row.tolist() and s.stats()["nseq"] == 200
    finally:
        s.close()
        slot.destroy()


def test_retry_is_exact(c):
    reads = sc.retry_batch()
    state, st = _check(c, "default", reads, S=300, pending_cap=16, what="a pending array far below one batch")
    assert st["retries"] >= 1, st
    first = list(bc.reads300()[:30])
    groups = [first, list(reads), first]
    state, st = _check(c, "default", first + list(reads) + first, S=300, m=2, groups=groups, pending_cap=16, what="a retry behind a cut")
    assert st["retries"] >= 1 and state["cuts"] >= 1, (state, st)


@pytest.mark.parametrize("m", [1, 2])
def test_finish_gives_the_candidates(c, m):
    reads = list(bc.reads300()[:150])
    s = c.sample_bottom([K], 100, m, pending_cap=512)
    try:
        for g in sc.batches(reads, 15):
            b, off = sc.pack(g)
            s.add(b, off)
        v, a = s.finish()
        T = s.bottom_state()["threshold"]
        wv, wa = bm.counted(reads, (K,), bc.POLICIES["default"])
        keep = wv <= np.uint64(T)
        assert T < bm.FULL and v.tolist() == wv[keep].tolist() and a.tolist() == wa[keep].tolist()
        assert s.bottom_state()["candidates"] == len(v)
        if m == 2:
            assert int((a < 2).sum()) > 0          # values below T that do not qualify stay with their counts
        dv, da, n = s.device()
        assert n == len(v) and dv and da
        row, ln = s.finish_bottom()
        assert row[:ln].tolist() == bm.direct(reads, (K,), bc.POLICIES["default"], 100, m, False)
    finally:
        s.close()


def test_refusals(c):
    import rkmh_amd
    lib = c._lib
    for S, m in ((0, 1), (-3, 1), (bc.MAX_SKETCH + 1, 1), (10, 0), (10, 1 << 32)):
        with pytest.raises(rkmh_amd.RkmhError):
            c.sample_bottom([K], S, m)
    for ks in ([], [0], [65], list(range(8, 17))):
        with pytest.raises(rkmh_amd.RkmhError):
            c.sample_bottom(ks, 10)
    ks = np.array([K], np.int32)
    h = C.c_void_p()
    pk = ks.ctypes.data_as(C.POINTER(C.c_int))
    assert lib.rk_sample_create_bottom(None, pk, 1, 10, C.c_uint64(1), C.c_uint64(0), C.byref(h)) != 0
    assert lib.rk_sample_create_bottom(c._h, None, 1, 10, C.c_uint64(1), C.c_uint64(0), C.byref(h)) != 0
    assert lib.rk_sample_create_bottom(c._h, pk, 1, 10, C.c_uint64(1), C.c_uint64(0), None) != 0
    assert lib.rk_sample_finish_bottom(None, None, None) != 0 and lib.rk_sample_bottom_state(None, None, None, None, None) != 0
    s = c.sample_bottom([K], 10)
    scaled = c.sample([K], bm.FULL, abund=True)
    try:
        with pytest.raises(rkmh_amd.RkmhError, match="bottom sample"):
            s.add_sketch(np.array([5, 7], np.uint64), np.array([1, 1], np.uint32))
        assert lib.rk_sample_finish_bottom(s._h, None, None) != 0
        assert lib.rk_sample_bottom_state(s._h, None, None, None, None) == 0      # every pointer may be NULL
        row = np.zeros(10, np.uint64)
        n = C.c_int32()
        assert lib.rk_sample_finish_bottom(scaled._h, row.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n)) != 0
        assert "scaled sample" in lib.rk_last_error().decode()
        with pytest.raises(rkmh_amd.RkmhError):
            scaled.finish_bottom()
        with pytest.raises(rkmh_amd.RkmhError, match="scaled sample"):
            scaled.bottom_state()
        row, ln = s.finish_bottom()                                               # nothing refused has left a trace
        assert ln == 0 and s.stats()["nseq"] == 0
    finally:
        s.close()
        scaled.close()


def test_reset_equals_fresh(c):
    reads = list(bc.reads300()[:60])
    want = bm.direct(reads[30:], (K,), bc.POLICIES["default"], 50, 1, False)
    s = c.sample_bottom([K], 50, pending_cap=512)
    try:
        b, off = sc.pack(reads[:30])
        s.add(b, off)
        s.finish_bottom()
        assert s.bottom_state()["cuts"] >= 1 and s.bottom_state()["threshold"] < bm.FULL
        s.add(b, off)          # reset with values pending, too
        s.reset()
        assert s.bottom_state() == dict(threshold=bm.FULL, candidates=0, qualifying_weight=0, cuts=0)
        assert s.stats() == dict(folds=0, retries=0, nseq=0, nbases=0, kept=0, distinct=0)
        b, off = sc.pack(reads[30:])
        s.add(b, off)
        row, n = s.finish_bottom()
        assert row[:n].tolist() == want and s.stats()["nseq"] == 30
    finally:
        s.close()
