"""The sample accumulator where one workgroup takes many tiles (rk_sample.hip): k_sample_keep under the device
entry's grid rule and past its cap of 4 096 workgroups, the piece cuts of rk_sample_add_batch, k_run_sums with long and short runs in
one wave and saturating in its wave path.  Every case of tests/sample_scale_cases.py goes through the entries with and without
abundances and is compared integer for integer with its expectation; the small ones also with rk_sketch_scaled_abund_batch +
rk_merge_scaled_abund.  That each case reaches what it is named for is shown without a GPU by tests/test_sample_scale_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import abund_model as am
import sample_cases as sc
import sample_scale_cases as ssc

pytestmark = pytest.mark.gpu

K = ssc.K
FRESH = dict(folds=0, retries=0, nseq=0, nbases=0, kept=0, distinct=0)


@pytest.fixture(scope="module")
def contexts():
    import rkmh_amd
    cs = {name: rkmh_amd.Context(0, policy_spec=name) for name in sc.POLICIES}
    yield cs
    for c in cs.values():
        c.close()


class _Resident:
    """a feed's arrays on the device (uint32 offsets), freed on exit"""

    def __init__(self, ctx, feed):
        self.ctx, self.ptrs = ctx, []
        assert int(feed.offsets[-1]) < 1 << 32
        self.bases = self._up(np.ascontiguousarray(feed.bases))
        self.offs = self._up(feed.offsets.astype(np.uint32))
        self.nseq = feed.nseq

    def _up(self, a):
        lib, h = self.ctx._lib, self.ctx._h
        p = C.c_void_p()
        assert lib.rk_device_alloc(h, a.nbytes, C.byref(p)) == 0
        self.ptrs.append(p)
        assert lib.rk_device_upload(h, p, a.ctypes.data_as(C.c_void_p), a.nbytes) == 0
        return p.value

    def free(self):
        for p in self.ptrs:
            self.ctx._lib.rk_device_free(self.ctx._h, p)
        self.ptrs = []


def _feed_all(ctx, s, feeds):
    for f in feeds:
        if f.route == "host":
            s.add(f.bases, f.offsets)
        else:
            r = _Resident(ctx, f)
            try:
                s.add_device(r.bases, r.offs, r.nseq)
            finally:
                r.free()


def _compare(case, v, a, st, abund, retries=True):
    kept = case.kept
    assert v.dtype == np.uint64 and len(v) == len(case.values), (case.name, "distinct", len(v), len(case.values))
    assert np.array_equal(v, case.values), (case.name, "values")
    if abund:
        assert a.dtype == np.uint32 and np.array_equal(a, case.abund), (case.name, "abundances")
        if int(case.abund.max()) < am.SAT:
            assert int(a.astype(np.uint64).sum()) == kept
    else:
        assert a is None
    assert st["kept"] == kept, (case.name, st, kept)
    assert st["distinct"] == len(case.values) and st["nseq"] == case.nseq and st["nbases"] == case.nbases, (case.name, st)
    if retries and case.retries == "none":
        assert st["retries"] == 0, (case.name, st)
    if retries and case.retries == "some":
        assert st["retries"] >= 1, (case.name, st)


def _run(ctx, case, abund):
    s = ctx.sample(list(case.ks), case.mh, abund=abund, pending_cap=case.pending_cap)
    try:
        _feed_all(ctx, s, case.feeds)
        v, a = s.finish()
        st = s.stats()
    finally:
        s.close()
    _compare(case, v, a, st, abund)
    return st


def _check(contexts, case):
    ctx = contexts[case.policy]
    if case.small:
        from rkmh_amd import api
        b, off = sc.pack(case.reads)
        lv, la, so = ctx.sketch_scaled_abund_batch(b, off, list(case.ks), case.mh)
        lv, la = api.merge_scaled_abund(lv, la, so, case.mh)
        assert np.array_equal(lv, case.values) and np.array_equal(la, case.abund), (case.name, "the library's own union differs from the model")
    st = _run(ctx, case, True)
    _run(ctx, case, False)
    return st


# ---- A: the stride ----
@pytest.mark.parametrize("name", [n for n in sorted(ssc.stride_cases()) if not n.startswith("three_feeds")])
def test_stride(contexts, name):
    _check(contexts, ssc.stride_cases()[name])


@pytest.mark.parametrize("name", [n for n in sorted(ssc.stride_cases()) if n.startswith("three_feeds")])
def test_three_feeds_reset_and_again(contexts, name):
    case = ssc.stride_cases()[name]
    ctx = contexts[case.policy]
    _check(contexts, case)
    for abund in (True, False):
        s = ctx.sample(list(case.ks), case.mh, abund=abund, pending_cap=case.pending_cap)
        try:
            _feed_all(ctx, s, case.feeds)
            v1, a1 = s.finish()
            st1 = s.stats()
            _compare(case, v1, a1, st1, abund)
            s.reset()
            assert s.stats() == FRESH
            _feed_all(ctx, s, case.feeds)
            v2, a2 = s.finish()
            st2 = s.stats()
            _compare(case, v2, a2, st2, abund, retries=False)   # (a reset keeps the pending array as grown: the second pass may not retry)
            assert np.array_equal(v1, v2) and (not abund or np.array_equal(a1, a2))
            assert {k: st2[k] for k in ("nseq", "nbases", "kept", "distinct")} == {k: st1[k] for k in ("nseq", "nbases", "kept", "distinct")}
        finally:
            s.close()


# ---- B: past the cap of 4 096 workgroups ----
@pytest.mark.parametrize("which", sorted(ssc.CAP_MH))
def test_past_the_grid_cap(contexts, which):
    case = ssc.cap_case(which)
    st = _check(contexts, case)
    if which == "quarter":
        assert st["retries"] == 0 and st["folds"] == 1, st


# ---- C: the piece cuts ----
def test_cut_by_bases(contexts):
    _check(contexts, ssc.cut_by_bases_case())


def test_long_read_alone_in_its_piece(contexts):
    _check(contexts, ssc.long_read_case())


def test_long_read_through_the_device_entry(contexts):
    _check(contexts, ssc.long_read_case(alone=True))


def test_cut_by_count(contexts):
    _check(contexts, ssc.cut_by_count_case())


# ---- D: k_run_sums ----
@pytest.mark.parametrize("i", range(3), ids=["whole", "cap_1000", "grouped_1000"])
def test_mixed_runs(contexts, i):
    case = ssc.mixed_cases()[i]
    st = _check(contexts, case)
    if i == 0:
        assert st["folds"] == 1, st
    if i == 2:
        assert st["folds"] >= 10, st


def test_saturation_in_the_wave_path(contexts):
    ctx = contexts["default"]
    x, read = ssc.saturation_case()
    reads = [read] * ssc.SAT_FEEDS
    v17, a17, kept17 = sc.want(reads)
    b, off = sc.pack(reads)
    for abund in (True, False):
        s = ctx.sample([K], ssc.FULL, abund=abund, pending_cap=ssc.MIX_CAP_WHOLE)
        try:
            if abund:
                s.add_sketch(np.array([x], np.uint64), np.array([ssc.SAT_START], np.uint32))
            else:
                s.add_sketch(np.array([x], np.uint64))
            folds = s.stats()["folds"]
            s.add(b, off)
            v, a = s.finish()
            st = s.stats()
            assert st["folds"] == folds + 1 and st["retries"] == 0, st          # one fold sees the run of x whole
            assert np.array_equal(v, v17)
            if abund:
                wv, wa = am.merge([(np.array([x], np.uint64), np.array([ssc.SAT_START], np.uint32)), (v17, a17)])
                assert np.array_equal(v, wv) and np.array_equal(a, wa)
                assert int(a[v.tolist().index(x)]) == am.SAT == (1 << 32) - 1
                assert st["kept"] == ssc.SAT_START + kept17 > int(a.astype(np.uint64).sum())
            else:
                assert a is None and st["kept"] == 1 + kept17
            assert st["nseq"] == ssc.SAT_FEEDS and st["nbases"] == ssc.SAT_FEEDS * len(read) and st["distinct"] == len(v17)
        finally:
            s.close()
