"""CPU-only: the panels and read sets of tests/index_cases.py mean something.  A comparison of device rows with the oracle proves a
value form right only if (a) the key really takes that form and (b) the rows would differ had the form been decoded wrongly.  Here,
on the oracle and on Python restatements of the builder's rules alone:

  labels      every key's form under the restated rules (hash_form; kmer_forms: bases, the 5 % rule, inline / (base, exceptions) /
              plain) is the form the case intends, and the restated bucket fill shows the intended overflow chains
  routing     every short read meets the conditions under which the fused kernels answer (tile_cases.assert_routed, with the panel's
              S); every long read exceeds FUSED_MAXLEN
  mutations   the heart: at every labelled key the neighbouring mistake is made on the INPUT -- a multiplicity one less or one more, a
              member of a pair or list dropped, a member's id off by one or masked to 9 or 11 bits, the sign of an exception flipped
              (a -1 exception counted as +1: the reference gets the base's posting and one more; a +1 counted as -1 shows no later
              than the member dropped), a k-mer that misses turned into a hit on the last key of the chain it walks -- and after each
              the ORACLE's rows must change for at least one read of the set each reader answers: a long read (the general path), a
              short read for which tile_cases.may_hand_back is false (k_classify_tile must answer it), a short read for which
              index_cases.may_hand_back_kmer is false (k_classify_kmer must)

Exemptions -- all of them:
  1. A multiplicity above 30, before or after the change, is exempt from the k_classify_tile condition: the hit set's occurrence
     field has 5 bits, the kernel may hand back a read that holds a sketch hash more than 30 times, and fewer occurrences cannot tell
     such multiplicities apart.  The long reads and the reads k_classify_kmer answers (no such limit) must distinguish them.
  2. A multiplicity taken from, or the whole posting dropped for, the SECOND of the two identical references: no row of any read can
     show it -- the first twin scores at least as much and comes first, and diff only looks at earlier references.  (One more for the
     second twin, and its id off by one, do show and are not exempt.)
  3. A change that changes nothing is no mutation: an id masked to itself, an id moved outside the panel.
"""
import collections
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import index_cases as ic  # noqa: E402
import tile_cases as tc  # noqa: E402


def _labels(P):
    return {P.label[h]: h for h in P.boundary}


@pytest.mark.parametrize("name", ic.PANELS)
def test_every_key_takes_the_form_it_is_labelled_with(orc, name):
    P = ic.panel(orc, name)
    assert len(_labels(P)) == len(P.boundary) and set(P.hs) == set(P.kv) == set(P.post)
    kf = ic.kmer_forms(P)
    for h, post in P.post.items():
        assert ic.hash_form(post) == P.hs[h], (name, P.label.get(h), post)
        assert kf.form[h] == P.kv[h], (name, P.label.get(h), post, kf.form[h])
    # rows: within S, ascending, no two equal but the twins
    assert (P.ln <= P.S).all() and P.ln.min() > 0
    seen = collections.defaultdict(list)
    for r, row in enumerate(P.rows()):
        assert (np.diff(row.astype(object)) >= 0).all()
        seen[row.tobytes()].append(r)
    assert sorted(v for v in seen.values() if len(v) > 1) == ([list(P.dup)] if P.dup else [])
    # every key is the hash of exactly one k-mer of the text, and of no other window of it
    assert all(int(P.text.h[p]) == h for h, p in P.pos.items())
    hs, kv = P.counts("hs"), P.counts("kv")
    assert hs["single_once"] == kv["reference"] and hs["single_multi"] == kv["single_multi"] and hs["pair"] == kv["pair"]
    assert hs["list"] == kv["inline"] + kv["base_inline"] + kv["base_list"] + kv["plain"]
    if name == "forms":
        L = _labels(P)
        assert [P.hs[L[x]] for x in ("mult511", "mult512", "pair", "two(1,2)", "list3(2)")] == ["single_multi", "list", "pair", "list", "list"]
        assert [P.kv[L["list%d" % n]] for n in (3, 4, 5, 6, 7, 12)] == ["inline"] * 4 + ["plain"] * 2
        assert (kf.bases, kf.dropped) == ([], 1)                   # list12 was a base until the 5 % rule cleared it
    if name == "wide_ids":
        L = _labels(P)
        assert [P.hs[L[x]] for x in ("pair(5,2047)", "pair(5,2048)", "pair(2047,2048)")] == ["pair", "list", "list"]
        assert [P.kv[L[x]] for x in ("list(1,2,511)", "list(1,2,512)")] == ["inline", "plain"]
        assert len(kf.bases) == 4 and not kf.dropped
        for n in (15, 16, 17, 33):
            refs = sorted(P.post[L["list%d" % n]])
            assert len(refs) == n and {r & 3 for r in refs} == {0, 1, 2, 3}
    if name == "families":
        assert kf.bases[:2] == [list(ic.FAM_A), list(ic.FAM_B)] and sorted(map(tuple, kf.bases[2:])) == sorted(P.decoys) and not kf.dropped
        L = _labels(P)
        dist = {x: len(set(P.post[L[x]]) ^ set(ic.FAM_A)) for x in ("A", "A+1", "A-1", "A+4-4", "A+5-4", "A+6-5", "A+6-6")}
        assert dist == {"A": 0, "A+1": 1, "A-1": 1, "A+4-4": 8, "A+5-4": 9, "A+6-5": 11, "A+6-6": 12}
        assert [P.kv[L[x]] for x in dist] == ["base_inline"] * 4 + ["base_list"] * 2 + ["plain"]
        assert kv["base_inline"] >= 100 and kv["base_list"] == 2
    if name == "chains":
        assert not kf.bases and hs["list"] == 0


def test_the_bucket_fill_shows_the_chains(orc):
    P = ic.panel(orc, "chains")
    fill = ic.bucket_fill(P.post)
    assert fill.nb == 256 and len(P.post) < 640
    home = collections.Counter(hm for hm, _ in fill.stored.values())
    assert home[ic.CHAIN_LAST] == 19 and home[0] == 8 and home[ic.CHAIN_MID] == 17
    assert all(home[b] == 0 for b in (1, 2, 3, 4, ic.CHAIN_MID + 1, ic.CHAIN_MID + 2, ic.CHAIN_MID + 3))
    last = sorted(b for hm, b in fill.stored.values() if hm == ic.CHAIN_LAST)
    assert last.count(ic.CHAIN_LAST) == 8 and last[0] == 0 and fill.wrapped == 1        # the chain wraps to bucket 0 ...
    far = max(b for hm, b in fill.stored.values() if hm in (ic.CHAIN_LAST, 0) and b != ic.CHAIN_LAST)
    assert 1 <= far <= 4 and fill.longest_chain >= 4                                      # ... and runs on past it
    assert sorted(b for hm, b in fill.stored.values() if hm == ic.CHAIN_MID) == [ic.CHAIN_MID] * 8 + [ic.CHAIN_MID + 1] * 8 + [ic.CHAIN_MID + 2]
    assert fill.overflowed == (far - 0) + 1 + 2                                            # 255, 0 .. far - 1; the mid bucket and the next
    # the misses walk a chain: their home bucket is full and flagged, and they are no keys
    for p, mh in P.misses:
        assert mh not in P.post and P.text.count[mh] == 1
        assert sum(1 for _, b in fill.stored.values() if b == ((mh >> 32) & 255)) == ic.SLOTS


@pytest.mark.parametrize("name", ic.PANELS)
def test_reads_are_routed_as_meant(orc, name):
    P, rd = ic.panel(orc, name), ic.reads(orc, name)
    s = ic.short(rd)
    assert len(s) + len(rd.long) <= 900
    tc.assert_routed(range(P.nref), s, ic.KS)
    assert P.nref <= tc.MAX_REFS
    for r in s:
        assert len(r) <= tc.FUSED_MAXLEN and tc.nwin(len(r), ic.K) <= P.S, len(r)
    assert all(tc.nwin(len(r), ic.K) == 1 for r in rd.one)
    assert all(len(r) > tc.FUSED_MAXLEN and ic.LONG_MIN <= len(r) <= ic.LONG_MAX for r in rd.long)
    assert len(ic.batches(rd)) == (1 if name == "wide_ids" else 2)      # 8-bit and 16-bit counter fields
    if name == "forms":
        T = P.text
        first = int(T.h[T.tandem_at])
        assert [int((h == first).sum()) for h in ic.hashes(orc, rd.tandem)] == [1, 2, 29, 30, 31]
        for at, runs in ((T.a_at, rd.runs[:4]), (T.c_at, rd.runs[4:])):
            assert [int((h == int(T.h[at])).sum()) for h in ic.hashes(orc, runs)] == [510, 511, 512, 513]
        run_long = [int((h == int(T.h[T.a_at])).sum()) for h in ic.hashes(orc, rd.long[:4])] + [int((h == int(T.h[T.c_at])).sum()) for h in ic.hashes(orc, rd.long[4:8])]
        assert run_long == [510, 511, 512, 513] * 2
    if name == "wide_ids":                                                             # the sparse row's documented limit
        for h in ic.hashes(orc, s):
            assert len({r for x in set(h.tolist()) if x in P.post for r in P.post[x]}) < 128


def _changed(orc, P, seqs, base_rows, ids):
    """the places among ids whose oracle row differs from base_rows under the panel as it is now"""
    if not ids:
        return []
    got = ic.want_rows(orc, P, [seqs[i] for i in ids], threads=1)
    return [i for j, i in enumerate(ids) if (got[j] != base_rows[i]).any()]


@pytest.mark.parametrize("name", ic.PANELS)
def test_every_neighbouring_mistake_changes_a_row_each_reader_answers(orc, name):
    P, rd = ic.panel(orc, name), ic.reads(orc, name)
    s, lg = ic.short(rd), rd.long
    hs_s, hs_l = ic.hashes(orc, s), ic.hashes(orc, lg)
    sparse = tc.sparse_rows(P.nref, max(tc.nwin(len(r), ic.K) for r in s))
    assert sparse == (name == "wide_ids")
    tile_ok = [not tc.may_hand_back(P.hit_rows(h), h, len(r), sparse) for r, h in zip(s, hs_s)]
    kmer_ok = [not ic.may_hand_back_kmer(P.hit_rows(h), h, len(r), sparse) for r, h in zip(s, hs_s)]
    assert all(k or not t for t, k in zip(tile_ok, kmer_ok)) and sum(tile_ok) >= len(s) - 40
    base_s, base_l = ic.want_rows(orc, P, s), ic.want_rows(orc, P, lg)
    holds_s, holds_l = collections.defaultdict(list), collections.defaultdict(list)
    for where, hs in ((holds_s, hs_s), (holds_l, hs_l)):
        for i, h in enumerate(hs):
            for x in set(h.tolist()):
                where[x].append(i)
    muts = ic.mutations(P)
    assert len(muts) >= 4 * len(P.boundary) or name == "chains"
    kinds = collections.Counter(m.what for m in muts)
    missed = []
    for m in muts:
        aimed = P_probe = rd.probe_of.get((m.key, m.ref), [])
        first_s = [i for kind, i in aimed if kind == "short"]
        first_l = [i for kind, i in aimed if kind == "long"]
        with P.mutated(m.key, m.post):
            ch_s = _changed(orc, P, s, base_s, first_s)
            need_tile = not m.high and not any(tile_ok[i] for i in ch_s)
            need_kmer = not any(kmer_ok[i] for i in ch_s)
            if need_tile or need_kmer:
                ch_s += _changed(orc, P, s, base_s, [i for i in holds_s[m.key] if i not in first_s])
            ch_l = _changed(orc, P, lg, base_l, first_l) or _changed(orc, P, lg, base_l, [i for i in holds_l[m.key] if i not in first_l])
        lacks = [what for what, ok in (("k_classify_tile", m.high or any(tile_ok[i] for i in ch_s)), ("k_classify_kmer", any(kmer_ok[i] for i in ch_s)),
                                       ("general path", bool(ch_l))) if not ok]
        if lacks:
            missed.append((m.what, P.label.get(m.key, "miss"), m.ref, lacks))
    assert not missed, (len(missed), missed[:10])
    # the rows are back as they were
    assert (ic.want_rows(orc, P, s) == base_s).all()
    if name == "forms":
        assert kinds["multiplicity-1"] >= 20 and kinds["id&511"] == 0 and sum(m.high for m in muts) >= 12
    if name == "wide_ids":
        assert kinds["id&511"] >= 30 and kinds["id&2047"] >= 4
    if name == "families":
        assert kinds["sign"] >= 20
    if name == "chains":
        assert kinds["miss->hit"] == len(P.misses) == 24
