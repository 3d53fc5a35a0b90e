"""CPU-only: every case of tests/sample_scale_cases.py reaches what it claims, and its expectation is right -- shown on abund_model,
sourmash_model and the replicas of launch_keep, feed_locked, the tile loop and the piece loop that sample_scale_cases.py holds (they
follow rkmh_amd/csrc/rk_sample.hip by reading), so that tests/test_gpu_sample_scale.py may rely on it."""
import numpy as np
import pytest

import abund_model as am
import sample_cases as sc
import sample_scale_cases as ssc

W, K = ssc.W, ssc.K
STRIDE = [n for n in ssc.stride_cases() if not ssc.is_host_form(n)]


def _tables(case, feed):
    """per launch of the feed: the position tables of the k it serves"""
    return [[ssc.window_table(feed.reads, k, case.pol, case.mh) for k in ks] for ks in ssc.launches(case.ks)]


def _same(a, b):
    return a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist()


# ---- the replicas themselves ----
def test_grid_rule():
    assert [ssc.grid_of(b) for b in (0, 1, 2048, 2049, 4096 * 2048, 4096 * 2048 + 1, ssc.UNKNOWN_BOUND)] == [1, 1, 1, 2, 4096, 4096, 4096]
    assert ssc.device_grids([100, 14341, 5]) == [4096, 1, 15]
    assert ssc.device_grids([1025, 10, 0, 10]) == [4096, 2, 1, 4096]      # a batch without bases: the next one is a first one again
    assert ssc.tiles_of(7 * W - 3, 3) == [[0, 3, 6], [1, 4], [2, 5]]
    assert ssc.tiles_of(2 * W, 4096) == [[0], [1]]
    assert ssc.launches((12, 16)) == [[16], [12]] and ssc.launches((21,)) == [[21]] and ssc.launches((16,)) == [[16]]


def test_piece_replica_equals_the_loop_as_written():
    rng = np.random.default_rng(7)
    for _ in range(200):
        lens = rng.integers(0, 40, size=int(rng.integers(1, 60)))
        off = np.concatenate([[int(rng.integers(0, 9))], lens]).cumsum()
        pb, ps = int(rng.integers(1, 80)), int(rng.integers(1, 9))
        got = ssc.pieces(off, pb, ps)
        assert got == ssc.pieces_plain(off, pb, ps)
        assert got[0][0] == 0 and got[-1][1] == len(lens) and all(a[1] == b[0] for a, b in zip(got, got[1:]))
        for i0, i1 in got:                      # whole sequences; a piece over the limit holds one sequence
            assert i1 - i0 <= ps and (off[i1] - off[i0] <= pb or i1 == i0 + 1)


def test_union_equals_merge():
    rng = np.random.default_rng(8)
    parts = []
    for _ in range(6):
        v = np.unique(rng.integers(1, 50, size=30).astype(np.uint64))
        parts.append((v, rng.integers(1, 9, size=len(v)).astype(np.uint32)))
    parts.append((np.array([5, 7], np.uint64), np.array([am.SAT - 3, am.SAT], np.uint32)))
    assert _same(ssc.union(parts), am.merge(parts))
    assert int(ssc.union(parts)[1].max()) == am.SAT


# ---- A: the stride ----
@pytest.mark.parametrize("name", sorted(ssc.stride_cases()))
def test_small_case_is_the_plain_model(name):
    c = ssc.stride_cases()[name]
    v, a, kept = sc.want(c.reads, c.ks, c.pol, c.mh)
    assert _same((c.values, c.abund), (v, a)) and c.kept == kept == int(c.abund.astype(np.uint64).sum())
    assert c.nseq == len(c.reads) and c.nbases == sum(len(r) for r in c.reads)
    assert int(c.abund.max()) < am.SAT


@pytest.mark.parametrize("name", STRIDE)
def test_stride_case_strides_carries_and_depends_on_it(name):
    c = ssc.stride_cases()[name]
    grids = ssc.case_grids(c)
    assert all(f.route == "device" for f in c.feeds) and grids[0] == ssc.GRID_CAP
    two_tiles = carried = False
    cut, mid = [], 0
    for f, g in zip(c.feeds, grids):
        two_tiles |= max(len(t) for t in ssc.tiles_of(f.nbases, g)) >= 2
        for tables in _tables(c, f):
            ends, _, m = ssc.staged_trace(tables, f.nbases, g)
            mid += m
            carried |= any(n > 0 for row in ends for _, n in row[:-1])
            cut += [t[: g * W] for t in tables]                 # the tile loop ending after its first trip: tiles 0 .. grid - 1 only
    assert two_tiles, "no workgroup takes two tiles"
    if c.mh == ssc.FULL:
        # every round of B keeps 193 to 256 values at FULL, so the flushes fall on every fourth round and on every tile's end: the
        # FULL forms flush in mid-tile and carry nothing; their _third and sparse siblings carry
        assert mid >= 1 and not carried
    else:
        assert carried, "no staged value waits across a tile edge"
        assert mid >= 1 or c.mh == ssc.SPARSE_MH
    assert not _same(ssc.sketch_of_tables(cut), (c.values, c.abund)), "the expectation does not depend on the later tiles"


def test_stride_shapes():
    cs = ssc.stride_cases()
    nb = sum(len(r) for r in ssc.B())
    assert nb == 6 * W + 5
    g = lambda n: ssc.case_grids(cs[n])
    assert g("grid1") == [4096, 1] and g("grid2") == [4096, 2] and g("grid3") == [4096, 3]
    assert ssc.tiles_of(nb, 1) == [list(range(7))]
    assert [len(t) for t in ssc.tiles_of(nb, 2)] == [4, 3] and [len(t) for t in ssc.tiles_of(nb, 3)] == [3, 2, 2]
    for n in STRIDE:
        if n.startswith("grid1"):
            assert g(n) == [4096, 1], n
    # at FULL the one workgroup flushes in mid-tile and carries values over every tile edge
    c = cs["grid1"]
    ends, flushes, mid = ssc.staged_trace(_tables(c, c.feeds[1])[0], nb, 1)
    assert flushes == 12 and mid == 6 and all(n == 0 for _, n in ends[0][:-1])
    c = cs["grid1_third"]
    ends, flushes, mid = ssc.staged_trace(_tables(c, c.feeds[1])[0], nb, 1)
    assert flushes >= 4 and mid >= 3 and all(n > 0 for _, n in ends[0][:-1])     # in mid-tile, and values wait across EVERY tile edge
    # at the sparse threshold it never fills the staging area: one flush, at its end, of values from all seven tiles
    c = cs["grid1_sparse"]
    ends, flushes, mid = ssc.staged_trace(_tables(c, c.feeds[1])[0], nb, 1)
    assert c.kept < ssc.SK_STAGE - ssc.SK_T and flushes == 0
    counts = [n for _, n in ends[0]]
    assert counts == sorted(counts) and counts[0] > 0 and len(set(counts[:-1])) == 6 and counts[-1] == c.kept - sc.want(ssc.primer(100), mh=c.mh)[2]
    # the retry: two launches, and B alone keeps more than the capacity
    c = cs["grid1_k12_16_retry"]
    assert len(ssc.launches(c.ks)) == 2 and sc.want(ssc.B(), c.ks)[2] > c.pending_cap == 1024
    c = cs["three_feeds_retry"]
    assert sc.want(ssc.B())[2] > c.pending_cap
    # three feeds: the third strides on the grid of twice the second
    c = cs["three_feeds"]
    assert g("three_feeds") == [4096, 1, ssc.grid_of(2 * nb)] == [4096, 1, 13]
    assert [len(t) for t in ssc.tiles_of(c.feeds[2].nbases, 13)] == [2] * 6 + [1] * 7


def test_offsets_that_do_not_begin_at_zero():
    cs = ssc.stride_cases()
    for name, lead in (("grid1_first_4099", 4099), ("host_first_5", 5), ("grid1_first_4099_third", 4099), ("host_first_5_third", 5)):
        c = cs[name]
        f = c.feeds[-1]
        assert int(f.offsets[0]) == lead and f.nbases == sum(len(r) for r in ssc.B()) and c.nbases == sum(len(r) for r in c.reads)
        junk = f.bases[:lead].tobytes()
        assert set(junk) <= set(b"ACGT")
        # a reader that took `first` as 0 would hash the bases in front: the bases from 0 on as one more read change the expectation
        wrong = sc.want(list(c.reads) + [junk + ssc.B()[0][:K]], mh=c.mh)
        assert not _same(wrong[:2], (c.values, c.abund))
    # 4 099 is no multiple of the tile, of a dword or of a round
    assert 4099 % W and 4099 % 4 and 4099 % ssc.SK_T


def test_runs_of_empty_reads():
    cs = ssc.stride_cases()
    for where in ("mid", "edge"):
        reads = ssc.with_empties(where)
        off = sc.starts(reads)
        at = int(np.flatnonzero(np.diff(off) == 0)[0])
        assert list(map(len, reads)).count(0) == 3000 and (np.diff(off)[at:at + 3000] == 0).all()
        assert len(reads[at - 1]) > 0 and len(reads[at + 3000]) > 0                                  # between two real reads
        assert (off[at] == W) if where == "edge" else (0 < off[at] < W and off[at] % ssc.SK_T)
        for n in ("grid1_empties_" + where, "host_empties_" + where):
            assert cs[n].nseq == len(cs[n].reads) >= 3043 and _same((cs[n].values, cs[n].abund), sc.want([r for r in cs[n].reads if r])[:2])
    assert cs["host_empties_mid"].values.tolist() == sc.want(ssc.B())[0].tolist()


# ---- B: past the cap ----
def test_block():
    blk = ssc.block()
    U = ssc.block_bases()
    assert len(blk) == 56 == len(set(blk)) and U % 2 == 1 and U % W != 0
    assert set(blk) <= set(sc.reads300())


def test_cap_cases():
    U, R = ssc.block_bases(), ssc.cap_R()
    assert R * U >= (4096 + 3) * W > (R - 1) * U
    for which, mh in ssc.CAP_MH.items():
        c = ssc.cap_case(which)
        f = c.feeds[0]
        assert f.route == "host" and f.nseq == 56 * R == c.nseq and f.nbases == R * U == c.nbases
        assert ssc.pieces(f.offsets) == [(0, 56 * R)]                                     # still one piece
        assert ssc.grid_of(f.nbases) == 4096
        tiles = ssc.tiles_of(f.nbases, 4096)
        ntiles = -(-R * U // W)
        assert ntiles >= 4096 + 3 and len(tiles) == 4096 and tiles[2] == [2, 4098]
        assert [len(t) for t in tiles] == [2] * (ntiles - 4096) + [1] * (2 * 4096 - ntiles)
        # the bytes are the block R times over, read by read
        rng = np.random.default_rng(9)
        for i in rng.integers(0, f.nseq, size=50).tolist() + [0, f.nseq - 1]:
            assert f.bases[int(f.offsets[i]): int(f.offsets[i + 1])].tobytes() == ssc.block()[i % 56]
        assert R * int(sc.want(ssc.block(), mh=mh)[1].max()) < am.SAT
        assert c.kept == int(c.abund.astype(np.uint64).sum()) and (c.abund % R == 0).all()   # every run has length R or a multiple
        if which != "quarter":
            assert c.kept > ssc.DEFAULT_PENDING and c.retries == "some"
            assert c.kept > ssc.SCAN_FIRST_TRIP                                               # the fold's scan takes its second trip
        else:
            assert c.kept < ssc.DEFAULT_PENDING and c.retries == "none"
        # the answer depends on the tiles past the cap: windows are kept in them
        t = ssc.window_table(ssc.block(), K, c.pol, mh)
        tail = np.arange(4096 * W, R * U) % U
        assert np.count_nonzero(t[tail]) > 0


def test_closed_form_of_the_repeated_block_at_three():
    for mh in (sc.FOLD_MH, ssc.FULL, ssc.CUT_MH):
        c = ssc.repeated_case("mini", 3, mh)
        f = c.feeds[0]
        reads = [f.bases[int(f.offsets[i]): int(f.offsets[i + 1])].tobytes() for i in range(f.nseq)]
        assert reads == list(ssc.block()) * 3
        v, a, kept = sc.want(reads, mh=mh)
        assert _same((c.values, c.abund), (v, a)) and c.kept == kept and c.nseq == 168 and c.nbases == 3 * ssc.block_bases()


# ---- C: the piece cuts ----
def test_cut_by_bases():
    U, R = ssc.block_bases(), ssc.cut_by_bases_R()
    assert R * U > ssc.PIECE_BASES + 2 * U >= (R - 1) * U
    c = ssc.cut_by_bases_case()
    f = c.feeds[0]
    got = ssc.pieces(f.offsets)
    assert len(got) == 2 and got[0][0] == 0 and got[1][1] == 56 * R
    cut = got[0][1]
    assert int(f.offsets[cut]) <= ssc.PIECE_BASES < int(f.offsets[cut + 1])
    assert cut % 56 != 0                                                  # the cut falls inside a block, not between two
    assert f.nbases - int(f.offsets[cut]) >= 2 * U                        # two blocks and more in the second piece: it keeps windows
    assert 0 < c.kept < ssc.DEFAULT_PENDING and R * int(sc.want(ssc.block(), mh=c.mh)[1].max()) < am.SAT
    assert ssc.grid_of(int(f.offsets[cut])) == 4096 and len(ssc.tiles_of(int(f.offsets[cut]), 4096)[0]) == 8   # 32 768 tiles on 4 096 workgroups
    # without the second piece the abundances are those of fewer repeats
    assert (c.abund.astype(np.uint64) > c.abund.astype(np.uint64) // R * (cut // 56 + 1)).all()


@pytest.mark.parametrize("policy", ["default", "mash"])
@pytest.mark.parametrize("extra", [0, 1, K - 1, K, K + 1, 77])
def test_closed_form_of_the_periodic_read_on_three_periods(policy, extra):
    pol = sc.POLICIES[policy]
    L = 3 * ssc.PERIOD + extra
    read = ssc.periodic_read(L).tobytes()
    assert len(read) == L and read[:ssc.PERIOD] == read[ssc.PERIOD: 2 * ssc.PERIOD]
    for mh in (ssc.FULL, sc.FOLD_MH):
        v, a = am.sketch(read, [K], pol, mh)
        cv, ca, kept = ssc.periodic_sketch(L, (K,), pol, mh)
        assert _same((cv, ca), (v, a)) and kept == int(a.astype(np.uint64).sum())
        assert 2 <= int(ca.min()) and int(ca.max()) >= 3


def test_long_read_case():
    c = ssc.long_read_case()
    f = c.feeds[0]
    i = c.note["long_index"]
    assert f.nseq == 21 and int(f.offsets[i + 1] - f.offsets[i]) == ssc.LONG_L == (64 << 20) + 5000
    assert ssc.pieces(f.offsets) == [(0, 10), (10, 11), (11, 21)]
    body = f.bases[int(f.offsets[i]): int(f.offsets[i + 1])]
    S = ssc.period_string()
    assert (body[: 3 * ssc.PERIOD] == np.tile(S, 3)).all() and (body[-ssc.PERIOD:] == np.roll(S, -((ssc.LONG_L - ssc.PERIOD) % ssc.PERIOD))).all()
    front, back = ssc.long_read_sides()
    assert f.bases[: int(f.offsets[10])].tobytes() == b"".join(front) and f.bases[int(f.offsets[11]): int(f.offsets[21])].tobytes() == b"".join(back)
    lv, la, lkept = ssc.periodic_sketch(ssc.LONG_L)
    assert lkept == ssc.LONG_L - K > ssc.DEFAULT_PENDING and len(lv) == ssc.PERIOD
    assert int(la.max()) == -(-(ssc.LONG_L - K) // ssc.PERIOD) and int(la.min()) == int(la.max()) - 1
    # every piece matters: each side's reads hold values that no other piece holds
    for side in (front, back):
        assert not set(sc.want(side)[0].tolist()) <= set(lv.tolist())
    assert set(sc.want(front)[0].tolist()) != set(sc.want(back)[0].tolist())
    assert c.kept == lkept + sc.want(front + back)[2] == int(c.abund.astype(np.uint64).sum())
    alone = ssc.long_read_case(alone=True)
    assert alone.feeds[0].route == "device" and alone.nseq == 1 and alone.nbases == ssc.LONG_L and _same((alone.values, alone.abund), (lv, la))
    assert ssc.device_grids([ssc.LONG_L]) == [4096] and len(ssc.tiles_of(ssc.LONG_L, 4096)[0]) == 9


def test_cut_by_count():
    c = ssc.cut_by_count_case()
    f = c.feeds[0]
    assert f.nseq == (1 << 22) + 3 == c.nseq and f.nbases < 5 << 20
    assert ssc.pieces(f.offsets) == [(0, 1 << 22), (1 << 22, (1 << 22) + 3)]
    lens = np.diff(f.offsets.astype(np.int64))
    real = np.flatnonzero(lens != 1)
    assert real.tolist() == list(ssc.COUNT_REAL_AT) == [0, (1 << 22) - 1, 1 << 22, (1 << 22) + 2]
    for i, r in zip(real.tolist(), ssc.count_reals()):
        assert f.bases[int(f.offsets[i]): int(f.offsets[i + 1])].tobytes() == r
    assert c.kept == sc.want(ssc.count_reals())[2]
    # the second piece holds values the first does not
    assert not set(sc.want(ssc.count_reals()[2:])[0].tolist()) <= set(sc.want(ssc.count_reals()[:2])[0].tolist())
    # a miniature through the plain model: one-base reads keep nothing
    m = ssc.cut_by_count_feed(11, (0, 7, 8, 10))
    assert ssc.pieces(m.offsets, ssc.PIECE_BASES, 8) == ssc.pieces_plain(m.offsets, ssc.PIECE_BASES, 8) == [(0, 8), (8, 11)]
    reads = [m.bases[int(m.offsets[i]): int(m.offsets[i + 1])].tobytes() for i in range(11)]
    assert [len(r) for r in reads].count(1) == 7 and _same(sc.want(reads)[:2], (c.values, c.abund))


# ---- D: k_run_sums ----
def test_mixed_runs_share_a_wave():
    distinct, reads = ssc.mixed_reads()
    assert len(set(distinct)) == 8 and all(112 <= len(r) <= 128 for r in distinct) and len(reads) == sum(ssc.MIX_MULT) == 528
    assert [reads.count(r) for r in distinct] == list(ssc.MIX_MULT)
    order = [distinct.index(r) for r in reads]
    stretches = np.diff(np.concatenate([[-1], np.flatnonzero(np.diff(order)), [len(order) - 1]]))
    assert int(stretches.max()) < 20                                      # interleaved, not grouped: the longest stretch of one read
    whole, cap1000, grouped = ssc.mixed_cases()
    assert whole.kept <= whole.pending_cap and cap1000.kept > 1000
    # the sorted pending array of the first form: run j is the abundance of value j; waves of 64 consecutive runs
    runs = whole.abund.astype(np.int64)
    assert set(ssc.MIX_MULT) <= set(runs.tolist())
    mixed = 0
    for j in range(0, len(runs), 64):
        w = runs[j:j + 64]
        mixed += int((w > ssc.LANE_RUN).sum() >= 2 and (w <= ssc.LANE_RUN).sum() >= 1)
    assert mixed >= 1 and mixed == (len(runs) + 63) // 64                 # here: every wave
    # the grouped form: no feed keeps more than the capacity (no retry), and all of them many times it (folds on resident counts)
    per = [sc.want(f.reads)[2] for f in grouped.feeds]
    assert max(per) <= 1000 and sum(per) > 10 * 1000 and _same((grouped.values, grouped.abund), (whole.values, whole.abund))


def test_saturation_in_the_wave_path():
    x, read = ssc.saturation_case()
    v, a, kept = sc.want([read] * ssc.SAT_FEEDS)
    assert int(a[v.tolist().index(x)]) == ssc.SAT_FEEDS
    assert 1 + ssc.SAT_FEEDS > ssc.LANE_RUN                               # the run of x: one resident count and 17 pending ones
    assert ssc.SAT_START + ssc.SAT_FEEDS > am.SAT > ssc.SAT_START
    wv, wa = am.merge([(np.array([x], np.uint64), np.array([ssc.SAT_START], np.uint32)), (v, a)])
    assert int(wa[wv.tolist().index(x)]) == am.SAT and kept < ssc.MIX_CAP_WHOLE
