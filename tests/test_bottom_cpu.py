"""Bottom samples on the model (tests/bottom_model.py), without a GPU: the streaming accumulator equals the direct definition whatever
the batching, the definition at min_copies = 1 is the union of per-read sketches that `-g` has always printed, and the shared inputs
(tests/bottom_cases.py) hold what tests/test_gpu_bottom.py relies on.  The host half of the library (rk_bottom_emit) is checked too."""
import numpy as np
import pytest

import bottom_cases as bc
import bottom_model as bm
import dedup_model as dm
import pairs_model as pm
import sample_cases as sc
import sourmash_model as sm


def _hashes(reads, ks=(bc.K,), pol=sm.DEFAULT):
    return [bm.read_hashes(r, ks, pol) for r in reads]


@pytest.fixture(scope="module")
def h300():
    return _hashes(bc.reads300())


# ---- streaming equals the definition ----
@pytest.mark.parametrize("distinct", [False, True])
@pytest.mark.parametrize("m", [1, 2, 3])
def test_streaming_equals_direct(h300, m, distinct):
    reads = bc.reads300()
    rng = np.random.default_rng(40 + m)
    for S in (1, 64, 1000):
        want = bm.direct(reads, (bc.K,), sm.DEFAULT, S, m, distinct)
        for trial in range(3):
            s = bm.Stream(S, m, distinct)
            i = 0
            while i < len(h300):
                n = int(rng.integers(1, 40))
                for h in h300[i:i + n]:
                    s.feed(h)
                i += n
                if rng.random() < 0.7:
                    s.cut_now()
            assert s.finish() == want, (S, m, distinct, trial)
            assert all(a >= b for a, b in zip(s.thresholds, s.thresholds[1:]))


def test_random_multisets():
    rng = np.random.default_rng(41)
    for trial in range(60):
        S, m, distinct = int(rng.integers(1, 30)), int(rng.integers(1, 4)), bool(rng.integers(0, 2))
        w = rng.integers(1, 200, size=int(rng.integers(0, 600))).tolist()
        v, c = np.unique(np.asarray(w, dtype=np.uint64), return_counts=True)
        want = bm.emit(v, c, S, m, distinct)
        s = bm.Stream(S, m, distinct)
        i = 0
        while i < len(w):
            n = int(rng.integers(1, 50))
            s.feed(w[i:i + n])
            i += n
            s.cut_now()
        assert s.finish() == want, trial


# ---- at min_copies = 1: the union of per-read sketches ----
@pytest.mark.parametrize("policy", ["default", "mash", "sourmash"])
def test_m1_is_the_union_of_read_sketches(policy):
    reads, pol, distinct = list(bc.reads300()[:60]), bc.POLICIES[policy], bc.DISTINCT[policy]
    for S in (1, 64, 1000):
        per_read = [(dm.bottom_distinct if distinct else sm.bottom)(sm.calc_hashes(r, [bc.K], pol), S) for r in reads]
        pooled = np.sort(np.concatenate([pm.values(x) for x in per_read]))
        if distinct:
            pooled = np.unique(pooled)
        assert bm.direct(reads, (bc.K,), pol, S, 1, distinct) == pooled[:S].tolist(), (policy, S)


# ---- what the inputs hold ----
def _fold_stream(h300, m, distinct):
    """the fold test's feeds of seven reads, a cut after each"""
    s = bm.Stream(bc.FOLD_S, m, distinct)
    seen_at = {}
    for b, i in enumerate(range(0, len(h300), bc.FOLD_BATCH)):
        for h in h300[i:i + bc.FOLD_BATCH]:
            s.feed(h)
            for x in h:
                seen_at.setdefault(x, []).append(b)
        s.cut_now()
    return s, seen_at


def test_inputs_bring_at_least_three_cuts(h300):
    for m in (1, 2):
        for distinct in (False, True):
            s, _ = _fold_stream(h300, m, distinct)
            assert s.cuts >= 3, (m, distinct, s.cuts)
            assert len(set(s.thresholds)) >= 4


def test_a_candidate_qualifies_in_a_later_batch(h300):
    s, seen_at = _fold_stream(h300, 2, True)
    final = set(s.finish())
    late = [x for spared in s.spared for x in spared if x in final]
    assert late, "no value was kept below the threshold without qualifying and then made it into the sketch"
    x = late[0]
    assert len(set(seen_at[x])) >= 2 and seen_at[x][0] < seen_at[x][1]      # its second copy came with a later batch
    # and the reads fed twice: nothing qualifies before the second pass begins
    first, again = bc.twice()
    assert bm.direct(first, (bc.K,), sm.DEFAULT, 1000, 2, True) != bm.direct(first + again, (bc.K,), sm.DEFAULT, 1000, 2, True)
    v, c = bm.counted(first + again, (bc.K,), sm.DEFAULT)
    assert int(c.min()) >= 2


def test_a_count_alone_reaches_S():
    v, c = bm.counted([sc.homopolymer()], (bc.K,), sm.DEFAULT)
    assert len(v) == 1 and int(c[0]) >= 1000
    assert bm.direct([sc.homopolymer()], (bc.K,), sm.DEFAULT, 1000, 1, False) == [int(v[0])] * 1000
    assert bm.direct([sc.homopolymer()], (bc.K,), sm.DEFAULT, 1000, 1, True) == [int(v[0])]
    assert bm.cut(v, c, 1000, 1, False) == (1, int(v[0])) and bm.cut(v, c, 1000, 1, True) == (0, 0)


def test_many_short_is_more_than_a_first_sub_batch():
    reads = bc.many_short()
    assert len(reads) > 4096 and all(len(r) >= bc.K + 1 for r in reads)


def test_cut_places():
    cases = bc.cut_cases()
    assert {c[4] for c in cases.values()} >= set(bc.CUT_PLACES) | {0, 3012}
    for name, (counts, S, m, distinct, place) in cases.items():
        assert 1 <= S <= bc.MAX_SKETCH
        v = bc.values(len(counts))
        n, t = bm.cut(v, counts, S, m, distinct)
        assert n == place and t == (int(v[place - 1]) if place else 0), (name, n, place)
        if place:   # one entry earlier the weights are still below S
            assert int(bm.weights(counts[:place - 1], S, m, distinct).sum()) < S <= int(bm.weights(counts[:place], S, m, distinct).sum()), name
    counts = cases["3 000 unqualified entries in front of the crossing"][0]
    assert (counts[10:3010] == 1).all() and 3010 // bc.KEEP_BLK - 10 // bc.KEEP_BLK >= 2         # whole blocks of weight 0
    counts, S, m, distinct, place = cases["exactly S at a block's last entry"]
    assert place % bc.KEEP_BLK == 0 and int(bm.weights(counts[:place], S, m, distinct).sum()) == S
    counts, S, m, distinct, place = bc.wide_case()
    n = len(counts)
    assert n == 1024 * bc.KEEP_BLK + 5 and (n + bc.KEEP_BLK - 1) // bc.KEEP_BLK > 1024
    assert bm.cut(bc.values(n), counts, S, m, distinct) == (place, int(bc.values(n)[place - 1])) and (place - 1) // bc.KEEP_BLK == 1024


# ---- the library's host half ----
def test_emit_of_the_library():
    from rkmh_amd import api
    import rkmh_amd
    rng = np.random.default_rng(42)
    for name, (counts, S, m, distinct, _) in bc.cut_cases().items():
        v = bc.values(len(counts))
        row, n = api.bottom_emit(v, counts, S, m, distinct)
        want = bm.emit(v, counts, S, m, distinct)
        assert n == len(want) and row[:n].tolist() == want and not row[n:].any() and len(row) == S, name
    v, c = bm.counted(bc.reads300()[:40], (bc.K,), sm.DEFAULT)
    for S in (1, 7, 5000, bc.MAX_SKETCH):
        for m in (1, 2):
            for distinct in (False, True):
                row, n = api.bottom_emit(v, c, S, m, distinct)
                assert row[:n].tolist() == bm.emit(v, c, S, m, distinct) and not row[n:].any()
    assert api.bottom_emit(np.zeros(0, np.uint64), np.zeros(0, np.uint32), 5)[1] == 0
    for vals, cnts, S, m in (([5, 5], [1, 1], 4, 1), ([7, 5], [1, 1], 4, 1), ([0, 5], [1, 1], 4, 1), ([5], [1], 0, 1), ([5], [1], bc.MAX_SKETCH + 1, 1),
                             ([5], [1], 4, 0), ([5], [1], 4, 1 << 32)):
        with pytest.raises(rkmh_amd.RkmhError):
            api.bottom_emit(np.array(vals, np.uint64), np.array(cnts, np.uint32), S, m)
