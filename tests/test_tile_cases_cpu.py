"""The catalogue of tests/tile_cases.py on the CPU alone (oracle and tests/sourmash_model.py): the conditions that keep
tests/test_gpu_tile_classify.py from passing vacuously.  Each fails if a case loses its routing guarantee, its tie, its
multiplicity-limited row, its single valid window, its exact counter value.

`diff` (row field 2) is never 0: the scan of rkmh.cpp:874-883 replaces the maximum on `>` alone, so the winner of a tie is the first
reference and diff is its lead over the best EARLIER score, at least 1.  "A tie" is therefore checked on the shared counts themselves:
the maximum is attained by several references and the row names the first of them."""
import numpy as np
import pytest

import sourmash_model as sm
import tile_cases as tc


def _ragged_facts(orc, k, pol):
    rg = tc.ragged(k)
    refs = tc.base_panel()
    tc.assert_routed(refs, rg.reads, [k], pol)
    tc.assert_wholly_sketched(refs, [k], pol)
    sk = tc.want_sketches(orc, refs, [k], pol)
    rows = tc.want_rows(orc, refs, rg.reads, [k], pol, sketches=sk)
    assert rows.shape == (len(rg.reads), 4)
    tie = limited = hand = 0
    for i, r in enumerate(rg.reads):
        h = tc.window_hashes(orc, r, [k], pol)
        multi, plain = tc.shared_counts(sk, h)
        assert tc.row_from_shared(multi, h) == rows[i].tolist(), (k, str(pol), i)      # the helper and the arbiter agree
        back = tc.may_hand_back(sk, h, len(r), False)
        hand += back
        best = int(multi.max())
        if best > 0 and int((multi == best).sum()) >= 2 and (k < 3 or (not back and int(rows[i, 0]) > 0)):
            assert int(rows[i, 0]) == int(np.argmax(multi))                            # the first of the tied references
            tie += 1                                                                   # k >= 3: decided in the kernel, diff from an earlier score
        if not back and plain[int(rows[i, 0])] > multi[int(rows[i, 0])] > 0:
            limited += 1                                                               # min(mult_read, mult_ref) < mult_read
    for i in rg.two_n:
        h = tc.window_hashes(orc, rg.reads[i], [k], pol)
        assert int((h != 0).sum()) == 1 and len(h) >= 2, (k, i)
        assert int(rows[i, 3]) == 1
    return rows, tie, limited, hand


@pytest.mark.parametrize("k", tc.ALL_K)
def test_ragged_default_policy(orc, k):
    rows, tie, limited, hand = _ragged_facts(orc, k, tc.DEFAULT)
    n = len(rows)
    assert 2 * int((rows[:, 1] > 0).sum()) >= n, (k, int((rows[:, 1] > 0).sum()), n)
    # k <= 2: at most ten distinct k-mers, each more often in any reference than in a read of <= 400 bases (no row is limited by a
    # reference's multiplicity) and more than 30 times in half the reads (those go back to the general path); ties there involve
    # reference 0.  From k = 3 on every condition holds on rows the kernel itself answers.
    assert tie >= 1 and (limited >= 1 or k < 3), (k, tie, limited)
    if k >= 3:
        assert hand == 2, (k, hand)   # the two long tandem copies (40 and 57 units: more than 30 occurrences of a sketch hash)


@pytest.mark.parametrize("k", tc.ALL_K)
def test_uniform_sets(orc, k):
    refs = tc.base_panel()
    every = 1 if k in tc.FULL_L_K else 8
    Ls = tc.uniform_lengths(k, every)
    assert len(Ls) == 64 // every and Ls[0] == k + 1
    # window counts: consecutive (or every eighth), so T * windows takes both sides of the <= 32 split for every T <= 16
    for T in range(1, 17):
        res = {(T * tc.nwin(L, k)) % 64 for L in tc.uniform_lengths(k)}
        assert any(0 < r <= 32 for r in res) and any(r > 32 or r == 0 for r in res), (k, T)
    hits = 0
    for L in Ls:
        reads = tc.uniform(k, L)
        assert len(reads) == 37 and {len(r) for r in reads} == {L}
        tc.assert_routed(refs, reads, [k])
        if L == Ls[0] or L == Ls[-1]:
            hits += int((tc.want_rows(orc, refs, reads, [k], tc.DEFAULT)[:, 1] > 0).sum())
    assert hits >= 37, (k, hits)


@pytest.mark.parametrize("pol", [p for p in tc.CROSS if p.seed == 42], ids=str)
def test_ragged_policy_cross(orc, pol):
    for k in tc.CROSS_K:
        rows, tie, limited, _ = _ragged_facts(orc, k, pol)
        assert 2 * int((rows[:, 1] > 0).sum()) >= len(rows), (k, str(pol))
        assert tie >= 1 and (limited >= 1 or k < 3), (k, str(pol), tie, limited)
        if not pol.canon:
            continue
        reads = tc.ragged(k).reads
        d = n = 0
        for r in reads:
            a, b = sm.lexmin_differs(r, k, pol.model())
            d, n = d + a, n + b
        other = tc.want_rows(orc, tc.base_panel(), reads, [k], pol._replace(canon=0))
        # With every window inside the sketch (S = 2000) a row counts shared strand PAIRS, and each rule names a pair by one value:
        # rows cannot depend on the rule at any k (the sketches and every hash the kernel computes do).
        assert (other == rows).all(), (k, str(pol))
        if k == 1:
            continue    # two strand pairs, {A, T} and {C, G}: a quarter of the windows hashing differently cannot be asked for
        assert n > 0 and 4 * d >= n, (k, d, n)


def test_counter_width_rows(orc):
    refs, reads = tc.counter_width()
    big = len(refs) - 1
    for batch, windows in tc.counter_width_batches():
        tc.assert_routed(refs, batch, [24])
        rows = tc.want_rows(orc, refs, batch, [24], tc.DEFAULT)
        assert rows[:, 0].tolist() == [big] * len(batch) and rows[:, 1].tolist() == windows and rows[:, 3].tolist() == windows
        assert max(tc.nwin(len(r), 24) for r in batch) == max(windows)
    assert [max(w) for _, w in tc.counter_width_batches()] == [255, 256, 256, 257]


@pytest.mark.parametrize("k", [64, 24])
def test_prefetch_edges(orc, k):
    refs = tc.base_panel()
    for L in tc.PREFETCH_L:
        reads, at = tc.prefetch_edges(L, k)
        assert max(len(r) for r in reads) == L == len(reads[at])
        tc.assert_routed(refs, reads, [k], allow_long=(at,) if L > tc.FUSED_MAXLEN else ())
        sk = tc.want_sketches(orc, refs, [k], tc.DEFAULT)
        rows = tc.want_rows(orc, refs, reads, [k], tc.DEFAULT, sketches=sk)
        assert rows[at, 1] >= 100 and rows[at, 0] == 10                      # the long read means something
        back = [tc.may_hand_back(sk, tc.window_hashes(orc, r, [k], tc.DEFAULT), len(r), False) for r in reads]
        assert back == [i == at and L > tc.FUSED_MAXLEN for i in range(len(reads))]   # 1529: the only rerouted read


@pytest.mark.parametrize("nref", tc.PANEL_NREF)
def test_panel_edges(orc, nref):
    pe = tc.panel_edges(nref)
    assert len(pe.refs) == nref and {len(r) for r in pe.refs} == {80}
    for k in (24, 48):
        sk = tc.want_sketches(orc, pe.refs, [k], tc.DEFAULT)
        for batch in (pe.short, pe.long + pe.short):
            tc.assert_routed(pe.refs, batch, [k])
            tc.assert_wholly_sketched(pe.refs, [k])
            mw = max(tc.nwin(len(r), k) for r in batch)
            assert (mw <= 255) == (batch is pe.short)
            sparse = tc.sparse_rows(nref, mw)
            assert sparse == (nref >= (513 if mw <= 255 else 257))           # each panel size sits on one side of one switch
            rows = tc.want_rows(orc, pe.refs, batch, [k], tc.DEFAULT, sketches=sk)
            many = kept = 0
            for i, r in enumerate(batch):
                h = tc.window_hashes(orc, r, [k], tc.DEFAULT)
                multi, _ = tc.shared_counts(sk, h)
                assert tc.row_from_shared(multi, h) == rows[i].tolist()
                back = tc.may_hand_back(sk, h, len(r), sparse)
                if not back and multi.max() > 0 and int((multi == multi.max()).sum()) >= 3:
                    many += 1                                                # the maximum attained by >= 3 references, first index wins
                    assert rows[i, 0] == int(np.argmax(multi))
                kept += not back
                assert back == (sparse and int((multi > 0).sum()) > 128)
            assert many >= 1 and 2 * kept >= len(batch), (nref, k, many, kept)   # (reads of the two large families overflow a sparse row)


@pytest.mark.parametrize("k", [1, 48, 64])
def test_oracle_and_model_agree_beyond_two_murmur_blocks(orc, k):
    """One independent check of the arbiter itself: rows and sketches of the oracle (C) and of the model (numpy, written from the
    published algorithm) under canon=minhash."""
    refs, reads = tc.base_panel(), tc.ragged(k).reads
    for pol in (tc.DEFAULT, tc.Pol(1, 0, 0, 7)):
        a = tc.want_sketches(orc, refs, [k], pol)
        b = sm.sketch_refs(list(refs), [k], tc.S, pol.model())
        assert all(x.tolist() == y.tolist() for x, y in zip(a, b))
        assert (tc.want_rows(orc, refs, reads, [k], pol, sketches=a) == sm.classify(list(reads), b, [k], tc.S, pol.model())).all()


def test_mode_cases(orc):
    """the -M inputs: the mask removes hashes of these very reads (rows differ from the unmasked ones) and slot 0 / invalid windows
    are counted"""
    refs = tc.base_panel()
    for k in tc.MODE_K:
        reads = tc.ragged(k).reads
        h = np.concatenate([tc.window_hashes(orc, r, [k], tc.DEFAULT) for r in reads])
        assert (h == 0).sum() > 0                                            # invalid windows: counted in slot 0 (zero=count)
        masked = tc.want_rows(orc, refs, reads, [k], tc.DEFAULT, min_occ=2)
        plain = tc.want_rows(orc, refs, reads, [k], tc.DEFAULT)
        assert (masked[:, 3] < plain[:, 3]).sum() >= 10 and (masked[:, 1] > 0).sum() >= 10, k


# ---- the catalogue of the DEDUP forms (dedup=distinct): tests/test_gpu_tile_dedup.py -------------------------------------------------
import dedup_model as dm  # noqa: E402


def test_pol_dedup_field():
    """the new field is invisible where it is not set: every earlier policy text, and with it every earlier test id, stays as it was"""
    assert tc.Pol(0, 1, 0, 42) == tc.Pol(0, 1, 0, 42, 0) == tc.DEFAULT and tc.DEFAULT.dedup == 0
    assert str(tc.DEFAULT) == "fold=swap32,windows=len-k,canon=minhash,seed=42"
    assert [str(p) for p in tc.DEDUP] == ["fold=swap32,windows=len-k,canon=minhash,seed=42,dedup=distinct",
                                          "fold=swap32,windows=len-k,canon=lexmin,seed=42,dedup=distinct"]
    assert all("dedup" not in str(p) for p in tc.CROSS) and len({str(p) for p in tc.CROSS}) == 24
    assert all(p.dedup and p.seed == 42 for p in tc.DEDUP_CROSS) and len(set(tc.DEDUP_CROSS)) == 12
    assert tc.DEDUP[1]._replace(dedup=0) == tc.Pol(0, 1, 1, 42)


_DISTINCT_FACTS = {}


def _distinct_facts(orc, k, pol, reads=None):
    """(rows under the key, rows of the multiset rule on the same reads, reads that may be handed back) on ragged(k)"""
    key = (k, pol, reads)
    if key not in _DISTINCT_FACTS:
        refs = tc.base_panel()
        rd = tc.ragged(k).reads if reads is None else reads
        sk = tc.want_sketches(orc, refs, [k], pol)
        hs = tc.masked_hashes(orc, rd, [k], pol)
        rows = tc.rows_distinct(sk, hs)
        multi = tc.want_rows(orc, refs, rd, [k], pol._replace(dedup=0))
        back = [i for i, r in enumerate(rd) if tc.may_hand_back_distinct(sk, hs[i], len(r), False)]
        _DISTINCT_FACTS[key] = (rows, multi, back)
    return _DISTINCT_FACTS[key]


@pytest.mark.parametrize("k", tc.ALL_K)
def test_dedup_ragged_every_k(orc, k):
    """at every k the key changes at least four ragged rows (the tandem copies, and at small k nearly every read), and no read is
    within the kernel's hand-back limits: under the key there is none on how often a value occurs, so k = 1 and 2 are the kernel's too"""
    for pol in tc.DEDUP:
        rows, multi, back = _distinct_facts(orc, k, pol)
        assert rows.shape == multi.shape == (len(tc.ragged(k).reads), 4)
        assert int((rows != multi).any(axis=1).sum()) >= 4, (k, str(pol))
        assert (rows[:, 3] <= multi[:, 3]).all() and (rows[:, 1] <= multi[:, 1]).all()
        assert back == [], (k, str(pol), back)
        for i in tc.ragged(k).two_n:
            assert rows[i, 3] == 1
        every = 1 if k in tc.FULL_L_K else 8
        if pol.canon and every == 1:
            every = 8            # (the lexmin model is the slow one: the first and last length of each group of eight are enough here)
        for L in (tc.uniform_lengths(k, every)[0], tc.uniform_lengths(k, every)[-1]):
            _, _, uback = _distinct_facts(orc, k, pol, tc.uniform(k, L))
            assert uback == [], (k, L)


def test_dedup_every_field_differs(orc):
    """over the catalogue the key changes each of the four row fields somewhere"""
    seen = np.zeros(4, dtype=bool)
    for k in (1, 2, 3, 7):
        rows, multi, _ = _distinct_facts(orc, k, tc.DEDUP[0])
        seen |= (rows != multi).any(axis=0)
    assert seen.all(), seen


@pytest.mark.parametrize("pol", tc.DEDUP_CROSS, ids=str)
def test_dedup_policy_cross(orc, pol):
    for k in tc.DEDUP_CROSS_K:
        rows, multi, back = _distinct_facts(orc, k, pol)
        assert int((rows != multi).any(axis=1).sum()) >= 4 and back == [], (k, str(pol))
        assert 2 * int((rows[:, 1] > 0).sum()) >= len(rows), (k, str(pol))


def test_distinct_rows_are_the_models(orc):
    """want_rows / want_sketches under the key (hashes from the oracle or the lexmin model, the rule from dedup_model) against
    dedup_model.classify / sketch_refs on the numpy model's hashes, plain and under -M 2 with every bound the device tests use"""
    refs = tc.base_panel()
    for pol in tc.DEDUP:
        for k in (1, 24, 64):
            reads = list(tc.ragged(k).reads)
            sk = tc.want_sketches(orc, refs, [k], pol)
            other = dm.sketch_refs(list(refs), [k], tc.S, pol.model())
            assert all(a.tolist() == b.tolist() for a, b in zip(sk, other))
            assert (tc.want_rows(orc, refs, reads, [k], pol, sketches=sk) == dm.classify(reads, other, [k], tc.S, pol.model())).all()
            counter = sm.count_hashes(reads, [k], tc.COUNT_SLOTS, pol.model())
            for bound in (None, 3, 0):
                a = tc.want_rows(orc, refs, reads, [k], pol, sketches=sk, min_occ=2, bound=bound)
                b = dm.classify(reads, other, [k], tc.S, pol.model(), counter=counter, min_occ=2, bound=bound)
                assert (a == b).all(), (k, str(pol), bound)


def _uset(windows):
    u = 64
    while u < 2 * windows and u < 2 * tc.DEDUP_MAX_WINDOWS:
        u <<= 1
    return u


def test_set_ladder(orc):
    refs, k = tc.base_panel(), tc.LADDER_K
    assert [_uset(W) for W in tc.LADDER_W] == [64, 128, 128, 256, 256, 512, 512, 1024, 1024, 2048, 2048, 4096]
    assert [2 * W == _uset(W) for W in tc.LADDER_W] == [True, False] * 6           # every other set is exactly half full
    for pol in tc.DEDUP:
        sk = tc.want_sketches(orc, refs, [k], pol)
        for W in tc.LADDER_W:
            lad = tc.set_ladder(W)
            assert max(tc.nwin(len(r), k, pol) for r in lad.reads) == W
            assert lad.random == (5, 6, 7) and len({lad.reads[i] for i in lad.random}) == 1
            hs = tc.masked_hashes(orc, lad.reads, [k], pol)
            rows = tc.rows_distinct(sk, hs)
            assert [int(rows[i, 3]) for i in lad.random] == [W] * 3, (W, str(pol))      # every window its own value
            assert rows[lad.periodic, 3] == 11 and len(hs[lad.periodic]) == W, (W, str(pol))
            assert rows[lad.random[0], 1] >= (200 if W >= 512 else 1) and rows[lad.random[0], 0] == 10
            assert not any(tc.may_hand_back_distinct(sk, hs[i], len(r), False) for i, r in enumerate(lad.reads)), (W, str(pol))
        reads = tc.stale_set()
        rows = tc.want_rows(orc, refs, reads, [k], pol, sketches=sk)
        assert len(reads) == 37 and len(set(reads)) == 1 and len(reads[0]) == 150
        assert (rows == rows[0]).all() and rows[0].tolist() == [3, 126, 126, 126]


def test_several_k_in_one_set(orc):
    refs = tc.base_panel()
    for pol in tc.DEDUP:
        for ks in tc.K_LISTS:
            sk = tc.want_sketches(orc, refs, ks, pol)     # ([31, 33, 63]: the longest references are sketched to S of their 2573 hashes)
            for k in ks:
                for reads in (tc.ragged(k).reads, tc.uniform(k, k + 40)):
                    hs = tc.masked_hashes(orc, reads, ks, pol)
                    if reads is not tc.uniform(k, k + 40):   # a set sized from the first k alone would be too small for the longest ragged read
                        assert _uset(max(len(h) for h in hs)) > _uset(max(tc.nwin(len(r), ks[0], pol) for r in reads)), (ks, k)
                    assert not any(tc.may_hand_back_distinct(sk, h, len(r), False) for h, r in zip(hs, reads)), (ks, k, str(pol))
        ks = tc.LIMIT_KS
        tc.assert_wholly_sketched(refs, ks, pol)
        sk = tc.want_sketches(orc, refs, ks, pol)
        at_limit, beyond, at = tc.several_k_limit()
        for batch, windows in ((at_limit, 2048), (beyond, 2050)):
            hs = tc.masked_hashes(orc, batch, ks, pol)
            assert len(batch[at]) == max(len(r) for r in batch) <= tc.FUSED_MAXLEN
            assert len(hs[at]) == windows == sum(tc.nwin(len(batch[at]), k, pol) for k in ks)
            distinct = len(np.unique(hs[at][hs[at] != 0]))
            assert 1000 <= distinct <= tc.S and windows > tc.S, distinct                      # the kernel's to answer; the host entry routes by windows
            back = [tc.may_hand_back_distinct(sk, h, len(r), False) for h, r in zip(hs, batch)]
            assert back == [i == at and windows > tc.DEDUP_MAX_WINDOWS for i in range(len(batch))]
            rows = tc.rows_distinct(sk, hs)
            assert rows[at, 0] == 10 and rows[at, 1] >= 300 and rows[at, 3] == distinct


@pytest.mark.parametrize("k", [64, 24])
def test_prefetch_edges_dedup(orc, k):
    refs = tc.base_panel()
    for pol in tc.DEDUP:
        sk = tc.want_sketches(orc, refs, [k], pol)
        for L in tc.PREFETCH_L:
            reads, at = tc.prefetch_edges(L, k)
            hs = tc.masked_hashes(orc, reads, [k], pol)
            rows = tc.rows_distinct(sk, hs)
            assert rows[at, 1] >= 100 and rows[at, 0] == 10
            back = [tc.may_hand_back_distinct(sk, h, len(r), False) for h, r in zip(hs, reads)]
            assert back == [i == at and L > tc.FUSED_MAXLEN for i in range(len(reads))]


def test_exactly_s(orc):
    refs, S = tc.base_panel(), tc.EXACT_S
    for pol in tc.DEDUP:
        for k in tc.EXACT_K:
            reads = tc.exactly_s(orc, k, pol)
            sk = tc.want_sketches(orc, refs, [k], pol, sketch_size=S)
            assert all(len(x) == S for x in sk)
            hs = tc.masked_hashes(orc, reads, [k], pol)
            rows = tc.rows_distinct(sk, hs, sketch_size=S)
            for i, p in enumerate(tc.EXACT_P):
                assert len(hs[i]) > S and len(np.unique(hs[i][hs[i] != 0])) == p and (hs[i] != 0).all()
                assert rows[i, 3] == min(p, S)
                assert tc.may_hand_back_distinct(sk, hs[i], len(reads[i]), False, sketch_size=S) == (p > S)
            for i in range(len(tc.EXACT_P), len(reads)):
                assert 0 < len(hs[i]) < S and not tc.may_hand_back_distinct(sk, hs[i], len(reads[i]), False, sketch_size=S)
            assert (rows[len(tc.EXACT_P):, 1] > 0).sum() >= 3


def test_dedup_mode_cases(orc):
    """-M 2 under the key: the mask lowers field 3 on at least 30 rows and the best score on at least one"""
    refs = tc.base_panel()
    for pol in tc.DEDUP:
        for k in tc.MODE_K + (24,):
            reads = tc.ragged(k).reads
            plain, _, _ = _distinct_facts(orc, k, pol)
            masked = tc.want_rows(orc, refs, reads, [k], pol, min_occ=2)
            assert (masked[:, 3] < plain[:, 3]).sum() >= 30 and (masked[:, 1] < plain[:, 1]).sum() >= 1, (k, str(pol))
            capped = tc.want_rows(orc, refs, reads, [k], pol, min_occ=2, bound=3)
            assert (capped[:, 3] == np.minimum(masked[:, 3], 3)).all() and (capped[:, :3] == masked[:, :3]).all()
