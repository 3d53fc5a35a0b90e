"""CPU-only: what tests/sample_cases.py holds, shown on abund_model / scaled_model / sourmash_model, so that tests/test_gpu_sample.py
may rely on it: enough kept windows to force folds and a retry at the capacities used, a run of more than 64 equal values, a kept
window lost to each boundary rule -- and the property the accumulator rests on: the union does not depend on how reads are grouped."""
import numpy as np

import abund_model as am
import sample_cases as sc
import scaled_model as scm
import sourmash_model as sm

K = sc.K


def _kept(reads, mh, ks=(K,), pol=sm.DEFAULT):
    return sum(int(am.sketch(r, list(ks), pol, mh)[1].astype(np.uint64).sum()) for r in reads)


def test_totals_force_three_folds():
    """A fold takes at most the pending array's capacity, which is the capacity asked for or, once grown, the most one batch kept:
    a total of three times that cannot be folded in fewer than three folds."""
    reads = sc.reads300()
    per_batch = [_kept(b, sc.FOLD_MH) for b in sc.batches(reads, sc.FOLD_BATCH)]
    total = sum(per_batch)
    assert len(per_batch) == 43 and min(per_batch) > 64
    assert total > 3 * max(64, max(per_batch))
    assert total > 3 * 1024
    assert total == sc.want(reads, mh=sc.FOLD_MH)[2]


def test_retry_batch_exceeds_its_capacity():
    kept = _kept(sc.retry_batch(), sc.FULL)
    assert 2900 <= kept <= 3400 and kept > 2 * sc.RETRY_CAP


def test_runs_of_more_than_64_equal_values():
    v, a = am.sketch(sc.homopolymer(), [K], sm.DEFAULT, sc.FULL)
    assert len(v) == 1 and int(a[0]) == len(sc.homopolymer()) - K > 64
    read = sc.reads300()[1]
    v, a, kept = sc.want([read] * sc.REPEAT_FEEDS)
    assert len(v) > 50 and int(a.min()) >= sc.REPEAT_FEEDS > 64 and kept == int(a.astype(np.uint64).sum())


def test_a_kept_window_is_lost_to_each_boundary_rule():
    mh = sc.FULL
    reads = sc.reads300()[1:3]
    assert all(b"N" not in r for r in reads)
    # (1) a window that crosses a read start: the concatenation has windows, all kept, that the two reads do not have
    joined = _kept([reads[0] + reads[1]], mh)
    apart = _kept(reads, mh)
    assert joined == apart + K                                   # k - 1 windows across the start, and the last window the policy drops
    cross = sm.window_hashes(reads[0] + reads[1], K, sm.MASH)[len(reads[0]) - K + 1: len(reads[0])]
    assert len(cross) == K - 1 and (cross != 0).all()
    # (2) the last window of a read: len - k windows under the default policy, len - k + 1 under mash
    assert _kept(reads, mh, pol=sm.MASH) == apart + 2
    # (3) a read shorter than that has none: k bases are one window under mash and none under the default policy
    short = reads[0][:K]
    assert _kept([short], mh, pol=sm.MASH) == 1 and _kept([short], mh) == 0 and _kept([short[:K - 1]], mh, pol=sm.MASH) == 0
    # and the edge reads of the GPU test: only from k + 1 bases on is there a window under the default policy
    got = [_kept([r], mh) for r in sc.edge_reads()[:6]]
    assert got == [0, 0, 0, 0, 1, 2]
    got = [_kept([r], mh, pol=sm.MASH) for r in sc.edge_reads()[:6]]
    assert got == [0, 0, 0, 1, 2, 3]


def test_tile_batch_positions():
    reads, on_boundary = sc.tile_batch()
    st = sc.starts(reads)
    W = sc.HASH_TILE_WIN
    lens = sorted(len(r) for r in reads)
    assert lens.count(150) == 40 and lens.count(5000) == 1 and len(reads) == 43
    assert st[on_boundary] == W                                                         # a read start exactly on a tile boundary
    for b in range(W, int(st[-1]), W):                                                  # every other boundary is straddled by a read
        i = int(np.searchsorted(st, b, side="right")) - 1
        assert st[i] <= b < st[i + 1] and (b == W or st[i] < b)
    long_i = [len(r) for r in reads].index(5000)
    assert st[long_i] // W + 2 <= (st[long_i + 1] - 1) // W                             # the long read covers a whole tile and more
    assert 0 < int(st[-1]) % W < K                                                      # the last tile holds fewer than k bases


def test_union_is_independent_of_grouping():
    reads = list(sc.reads300()[:60])
    v, a, kept = sc.want(reads, mh=sc.FOLD_MH)
    assert int(a.max()) > 1 and kept == int(a.astype(np.uint64).sum())
    rng = np.random.default_rng(5)
    perm = [reads[i] for i in rng.permutation(len(reads))]
    for order in (perm, reads[::-1]):
        v2, a2, k2 = sc.want(order, mh=sc.FOLD_MH)
        assert v2.tolist() == v.tolist() and a2.tolist() == a.tolist() and k2 == kept
    # grouped: the union of the unions of groups, whatever the groups
    for n in (1, 7, 25):
        parts = [sc.want(g, mh=sc.FOLD_MH)[:2] for g in sc.batches(reads, n)]
        v3, a3 = am.merge(parts, sc.FOLD_MH)
        assert v3.tolist() == v.tolist() and a3.tolist() == a.tolist()
    # and the values alone are scaled_model's union
    plain = np.unique(np.concatenate([scm.sketch(r, [K], sm.DEFAULT, sc.FOLD_MH) for r in reads]))
    assert plain.tolist() == v.tolist()


def test_saturation_rule():
    v, a = am.merge([(np.array([5], np.uint64), np.array([am.SAT - 1], np.uint32)), (np.array([5], np.uint64), np.array([1], np.uint32)),
                     (np.array([5], np.uint64), np.array([1], np.uint32))])
    assert v.tolist() == [5] and a.tolist() == [am.SAT]
