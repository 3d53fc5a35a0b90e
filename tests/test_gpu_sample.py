"""The sample accumulator on the GPU (rk_sample_*, rk_fastq_slot_sample; include/rkmh_amd.h "SAMPLE SKETCHES"): after any sequence of
adds the sample equals the union of the per-read abundance sketches -- against tests/abund_model.py and against
rk_sketch_scaled_abund_batch + rk_merge_scaled_abund, integer for integer.  What the shared inputs (tests/sample_cases.py) hold is
shown on the model by tests/test_sample_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import abund_model as am
import sample_cases as sc
import scaled_model as scm
import sourmash_model as sm

pytestmark = pytest.mark.gpu

K = sc.K


@pytest.fixture(scope="module")
def contexts():
    """one context per policy, none with references"""
    import rkmh_amd
    cs = {name: rkmh_amd.Context(0, policy_spec=name) for name in sc.POLICIES}
    yield cs
    for c in cs.values():
        c.close()


@pytest.fixture(scope="module")
def c(contexts):
    return contexts["default"]


def _library_union(ctx, reads, ks, mh):
    """the definition on the library's own entries: the per-read rows of rk_sketch_scaled_abund_batch united by rk_merge_scaled_abund"""
    from rkmh_amd import api
    b, off = sc.pack(reads)
    v, a, so = ctx.sketch_scaled_abund_batch(b, off, list(ks), mh)
    return api.merge_scaled_abund(v, a, so, mh)


def _feed(ctx, groups, ks=(K,), mh=sc.FULL, abund=True, pending_cap=0):
    """a fresh sample fed group by group -> (values, abund, stats)"""
    s = ctx.sample(list(ks), mh, abund=abund, pending_cap=pending_cap)
    try:
        for g in groups:
            b, off = sc.pack(g)
            s.add(b, off)
        v, a = s.finish()
        return v, a, s.stats()
    finally:
        s.close()


def _check(ctx, reads, ks=(K,), pol=sm.DEFAULT, mh=sc.FULL, groups=None, pending_cap=0, what=""):
    wv, wa, kept = sc.want(reads, ks, pol, mh)
    lv, la = _library_union(ctx, reads, ks, mh)
    assert lv.tolist() == wv.tolist() and la.tolist() == wa.tolist(), (what, "the library's own union differs from the model")
    v, a, st = _feed(ctx, groups if groups is not None else [list(reads)], ks, mh, True, pending_cap)
    assert v.dtype == np.uint64 and a.dtype == np.uint32
    assert v.tolist() == wv.tolist(), (what, "values", len(v), len(wv))
    assert a.tolist() == wa.tolist(), (what, "abundances")
    assert st["kept"] == kept == int(a.astype(np.uint64).sum()), (what, st, kept)
    assert st["distinct"] == len(wv) and st["nseq"] == len(reads) and st["nbases"] == sum(len(r) for r in reads), (what, st)
    pv, pa, _ = _feed(ctx, groups if groups is not None else [list(reads)], ks, mh, False, pending_cap)
    assert pa is None and pv.tolist() == wv.tolist(), (what, "without abundances")
    return st


# ---- read edges ----
@pytest.mark.parametrize("policy", ["default", "mash"])
def test_read_edges(contexts, policy):
    reads = sc.edge_reads()
    pol = sc.POLICIES[policy]
    assert [len(r) for r in reads[:6]] == [0, 1, K - 1, K, K + 1, K + 2]
    _check(contexts[policy], reads, pol=pol, what="all edge reads in one batch")
    for i, r in enumerate(reads):
        v, a, kept = sc.want([r], pol=pol)
        gv, ga, st = _feed(contexts[policy], [[r]])
        assert gv.tolist() == v.tolist() and ga.tolist() == a.tolist() and st["kept"] == kept, (policy, i, len(r))
    first_window = K + 1 if policy == "default" else K
    for n in (K - 1, K, K + 1):
        _, _, st = _feed(contexts[policy], [[reads[5][:n]]])
        assert st["kept"] == max(0, n - first_window + 1), (policy, n)


# ---- tile edges ----
def test_tile_edges(c):
    reads, on_boundary = sc.tile_batch()
    assert sc.starts(reads)[on_boundary] == sc.HASH_TILE_WIN
    _check(c, reads, what="tile batch")
    _check(c, reads, ks=(21,), what="tile batch, k = 21")
    # the same reads after a one-base read: every start moves by one, the boundary now cuts a read one base in
    _check(c, [b"A"] + list(reads), what="tile batch shifted by one")


# ---- policies and k ----
@pytest.mark.parametrize("policy", ["default", "mash", "sourmash"])
@pytest.mark.parametrize("ks", [(16,), (21,), (31,), (12, 16)])
def test_policies_and_k(contexts, policy, ks):
    reads = list(sc.reads300()[:40]) + [sc.tile_batch()[0][21]]   # 40 short reads and the 5 000-base one
    assert len(reads[-1]) == 5000
    _check(contexts[policy], reads, ks=ks, pol=sc.POLICIES[policy], mh=scm.max_hash(2), what=(policy, ks))


# ---- thresholds ----
def test_thresholds(c):
    reads = list(sc.reads300()[:50])
    full, _, _ = sc.want(reads)
    on_a_hash = int(full[len(full) // 3])
    for mh in (on_a_hash, on_a_hash - 1, scm.max_hash(2), sc.FULL):
        st = _check(c, reads, mh=mh, what=("max_hash", mh))
        assert st["distinct"] == int((full <= np.uint64(mh)).sum())
    assert _check(c, reads, mh=on_a_hash)["distinct"] == _check(c, reads, mh=on_a_hash - 1)["distinct"] + 1


# ---- folds and retries ----
def test_folds_at_every_capacity(c):
    reads = sc.reads300()
    groups = sc.batches(reads, sc.FOLD_BATCH)
    wv, wa, kept = sc.want(reads, mh=sc.FOLD_MH)
    for cap in sc.FOLD_CAPS:
        v, a, st = _feed(c, groups, mh=sc.FOLD_MH, pending_cap=cap)
        assert v.tolist() == wv.tolist() and a.tolist() == wa.tolist(), cap
        assert st["kept"] == kept and st["nseq"] == 300 and st["distinct"] == len(wv), (cap, st)
        if cap == 64:
            assert st["folds"] >= 3, st
        if cap == 0:
            assert st["retries"] == 0 and st["folds"] == 1, st
        pv, pa, _ = _feed(c, groups, mh=sc.FOLD_MH, abund=False, pending_cap=cap)
        assert pa is None and pv.tolist() == wv.tolist(), cap


def test_retry_is_exact(c):
    reads = sc.retry_batch()
    wv, wa, kept = sc.want(reads)
    v, a, st = _feed(c, [list(reads)], pending_cap=sc.RETRY_CAP)
    assert st["retries"] >= 1, st
    assert v.tolist() == wv.tolist() and a.tolist() == wa.tolist() and st["kept"] == kept and st["nseq"] == len(reads)
    # values that waited in the pending array before the batch that overflows are neither lost nor counted twice
    first = list(sc.reads300()[:3])
    wv, wa, kept = sc.want(first + list(reads))
    v, a, st = _feed(c, [first, list(reads)], pending_cap=sc.RETRY_CAP)
    assert st["retries"] >= 1 and v.tolist() == wv.tolist() and a.tolist() == wa.tolist() and st["kept"] == kept and st["nseq"] == 3 + len(reads)


# ---- abundances ----
def test_one_read_fed_70_times(c):
    read = sc.reads300()[1]
    wv, wa, kept = sc.want([read] * sc.REPEAT_FEEDS)
    for cap in (0, 4096):
        v, a, st = _feed(c, [[read]] * sc.REPEAT_FEEDS, pending_cap=cap)
        assert v.tolist() == wv.tolist() and a.tolist() == wa.tolist() and st["kept"] == kept, cap
    v, a, st = _feed(c, [[read] * sc.REPEAT_FEEDS])
    assert v.tolist() == wv.tolist() and a.tolist() == wa.tolist() and int(a.min()) >= 70


def test_homopolymer(c):
    h = sc.homopolymer()
    _check(c, [h], what="one homopolymer")
    _check(c, [h, sc.reads300()[2], h], what="two homopolymers around a read", pending_cap=1000)


def test_add_sketch_saturates(c):
    r1, r2 = sc.reads300()[1], sc.reads300()[2]
    v1, a1, _ = sc.want([r1])
    x = int(v1[len(v1) // 2])
    assert int(a1[len(v1) // 2]) == 1
    s = c.sample([K], sc.FULL, abund=True)
    try:
        s.add_sketch(np.array([x], np.uint64), np.array([am.SAT - 1], np.uint32))
        for r in (r1, r1, r2):
            b, off = sc.pack([r])
            s.add(b, off)
        v, a = s.finish()
        wv, wa = am.merge([(np.array([x], np.uint64), np.array([am.SAT - 1], np.uint32)), sc.want([r1, r1, r2])[:2]])
        assert v.tolist() == wv.tolist() and a.tolist() == wa.tolist()
        assert int(a[v.tolist().index(x)]) == am.SAT
        assert s.stats()["kept"] == am.SAT - 1 + sc.want([r1, r1, r2])[2]
        # a sketch with values above max_hash: cut off; united with what is there
        t = c.sample([K], int(v1[10]), abund=True)
        t.add_sketch(v1, a1)
        tv, ta = t.finish()
        assert tv.tolist() == v1[:11].tolist() and ta.tolist() == a1[:11].tolist()
        t.close()
    finally:
        s.close()


# ---- order ----
def test_order_and_grouping(c):
    reads = list(sc.reads300()[:120])
    wv, wa, kept = sc.want(reads, mh=sc.FOLD_MH)
    rng = np.random.default_rng(6)
    perm = [reads[i] for i in rng.permutation(len(reads))]
    for groups in ([reads], [perm], [reads[:1], reads[1:]], [reads[:77], reads[77:100], [], reads[100:]], sc.batches(perm, 13)):
        v, a, st = _feed(c, groups, mh=sc.FOLD_MH, pending_cap=2000)
        assert v.tolist() == wv.tolist() and a.tolist() == wa.tolist()
        assert st["kept"] == kept == int(a.astype(np.uint64).sum())
        assert st["nseq"] == len(reads) and st["nbases"] == sum(len(r) for r in reads)


# ---- device entries ----
def test_add_device_and_device_result(c):
    reads = list(sc.reads300()[:80])
    wv, wa, kept = sc.want(reads)
    b, off = sc.pack(reads)
    off32 = off.astype(np.uint32)
    lib = c._lib
    d_b, d_o = C.c_void_p(), C.c_void_p()
    assert lib.rk_device_alloc(c._h, len(b), C.byref(d_b)) == 0 and lib.rk_device_alloc(c._h, off32.nbytes, C.byref(d_o)) == 0
    assert lib.rk_device_upload(c._h, d_b, b.ctypes.data_as(C.c_void_p), len(b)) == 0
    assert lib.rk_device_upload(c._h, d_o, off32.ctypes.data_as(C.c_void_p), off32.nbytes) == 0
    s = c.sample([K], sc.FULL, abund=True, pending_cap=4096)
    try:
        s.add_device(d_b.value, d_o.value, len(reads))
        dv, da, n = s.device()
        assert n == len(wv) and dv and da
        hv, ha = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        assert lib.rk_device_download(c._h, hv.ctypes.data_as(C.c_void_p), C.c_void_p(dv), n * 8) == 0
        assert lib.rk_device_download(c._h, ha.ctypes.data_as(C.c_void_p), C.c_void_p(da), n * 4) == 0
        assert hv.tolist() == wv.tolist() and ha.tolist() == wa.tolist()
        st = s.stats()
        assert st["kept"] == kept and st["nseq"] == len(reads) and st["retries"] >= 1
    finally:
        s.close()
        lib.rk_device_free(c._h, d_b)
        lib.rk_device_free(c._h, d_o)


# ---- slot ----
def test_slot_sample(c):
    import rkmh_amd
    from rkmh_amd import api
    reads, text = sc.fastq200()
    wv, wa, kept = sc.want(reads)
    assert not c._lib.rk_num_references(c._h) > 0
    slot = api.FastqSlot(c, max_bytes=1 << 16)
    s = c.sample([K], sc.FULL, abund=True)
    try:
        assert slot.sample(text, s) == (0, 200)
        v, a = s.finish()
        assert v.tolist() == wv.tolist() and a.tolist() == wa.tolist()
        st = s.stats()
        assert st["nseq"] == 200 and st["nbases"] == sum(len(r) for r in reads) and st["kept"] == kept
        # a block with a carriage return is refused whole: status != 0, the sample as it was
        status, _ = slot.sample(sc.fastq_with_cr(), s)
        assert status != 0
        v2, a2 = s.finish()
        assert v2.tolist() == v.tolist() and a2.tolist() == a.tolist() and s.stats() == st
        # the same text through a device-text slot that reads it from caller memory
        dslot = api.FastqSlot(c, max_bytes=1 << 16, device_text=True)
        buf = np.frombuffer(text + b"\0" * 64, dtype=np.uint8).copy()
        s.reset()
        dslot.set_source(buf.ctypes.data)
        assert dslot.sample(len(text), s) == (0, 200)
        v3, a3 = s.finish()
        assert v3.tolist() == wv.tolist() and a3.tolist() == wa.tolist()
        dslot.destroy()
        # the slot entries that classify still ask for references
        with pytest.raises(rkmh_amd.RkmhError, match="rk_set_references"):
            slot.classify(text)
    finally:
        s.close()
        slot.destroy()


# ---- refusals ----
def test_refusals(c, contexts):
    import rkmh_amd
    from rkmh_amd import api
    lib = c._lib
    for ks in ([], list(range(8, 17)), [0], [65], [16, -1]):
        with pytest.raises(rkmh_amd.RkmhError):
            c.sample(ks, sc.FULL)
    with pytest.raises(rkmh_amd.RkmhError):
        c.sample([K], 0)
    ks = np.array([K], np.int32)
    h = C.c_void_p()
    assert lib.rk_sample_create(None, ks.ctypes.data_as(C.POINTER(C.c_int)), 1, C.c_uint64(sc.FULL), 1, 0, C.byref(h)) != 0
    assert lib.rk_sample_create(c._h, None, 1, C.c_uint64(sc.FULL), 1, 0, C.byref(h)) != 0
    assert lib.rk_sample_create(c._h, ks.ctypes.data_as(C.POINTER(C.c_int)), 1, C.c_uint64(sc.FULL), 1, 0, None) != 0
    assert lib.rk_sample_add_batch(None, None, None, 0) != 0 and lib.rk_sample_reset(None) != 0
    assert lib.rk_sample_add_batch_device(None, None, None, 1, None) != 0
    s = c.sample([K], sc.FULL, abund=True)
    plain = c.sample([K], sc.FULL, abund=False)
    slot = api.FastqSlot(contexts["mash"], max_bytes=1 << 16)
    try:
        b, off = sc.pack([b"ACGT" * 10, b"ACGT" * 10])
        assert lib.rk_sample_add_batch(s._h, None, None, 1) != 0
        assert lib.rk_sample_add_batch_device(s._h, None, None, 1, None) != 0
        assert lib.rk_sample_finish(s._h, None, None, None) != 0 and lib.rk_sample_device(s._h, None, None, None) != 0
        assert lib.rk_sample_stats(s._h, None) != 0
        with pytest.raises(rkmh_amd.RkmhError, match="decrease"):
            s.add(b, np.array([0, 40, 30], np.uint64))
        with pytest.raises(ValueError):
            s.add(b, np.array([0, 40, 4000], np.uint64))                  # the binding: offsets past the array
        with pytest.raises(rkmh_amd.RkmhError, match="another context"):
            slot.sample(sc.fastq200()[1], s)                               # a slot of another context
        for vals, ab in (([0, 5], [1, 1]), ([5, 5], [1, 1]), ([7, 5], [1, 1]), ([5, 7], [1, 0])):
            with pytest.raises(rkmh_amd.RkmhError):
                s.add_sketch(np.array(vals, np.uint64), np.array(ab, np.uint32))
        with pytest.raises(rkmh_amd.RkmhError):
            s.add_sketch(np.array([5, 7], np.uint64))                      # no abundances for a sample that has them
        plain.add_sketch(np.array([5, 7], np.uint64))
        assert plain.finish()[0].tolist() == [5, 7]
        plain.add_sketch(np.array([5, 9], np.uint64), np.array([3, 4], np.uint32))   # abundances given to a sample without them: ignored
        assert plain.finish()[0].tolist() == [5, 7, 9] and plain.stats()["kept"] == 4 and plain.finish()[1] is None
        v, a = s.finish()                                                  # nothing refused has left a trace
        assert len(v) == 0 and len(a) == 0 and s.stats()["nseq"] == 0
    finally:
        s.close()
        plain.close()
        slot.destroy()


# ---- reset ----
def test_reset_equals_fresh(c):
    reads = list(sc.reads300()[:60])
    wv, wa, kept = sc.want(reads[30:])
    s = c.sample([K], sc.FULL, abund=True, pending_cap=512)
    try:
        b, off = sc.pack(reads[:30])
        s.add(b, off)
        s.finish()
        s.add(b, off)          # reset with values pending, too
        s.reset()
        assert s.stats() == dict(folds=0, retries=0, nseq=0, nbases=0, kept=0, distinct=0)
        b, off = sc.pack(reads[30:])
        s.add(b, off)
        v, a = s.finish()
        st = s.stats()
        assert v.tolist() == wv.tolist() and a.tolist() == wa.tolist() and st["kept"] == kept and st["nseq"] == 30
    finally:
        s.close()
