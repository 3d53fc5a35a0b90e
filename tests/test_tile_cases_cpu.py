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
