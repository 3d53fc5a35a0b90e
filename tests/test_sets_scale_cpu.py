"""The inputs of tests/sets_scale_cases.py without a GPU, so that tests/test_sets_scale_gpu.py cannot pass vacuously: the layouts lie
where the builders say (read back from the CSR arrays), the closed forms are right (every miniature against the Python models, the
full sizes against the host entries), and every case depends on what lies past its cap -- the answer computed from the input cut at
the cap differs from the expected one, and the counts a scan takes past entry 1 024 are neither all zero nor all equal."""
import os
import re

import numpy as np
import pytest

import abund_model as am
import gather_model as gm
import multigather_cases as mc
import scaled_model as scm
import search_cases as sec
import search_model as sem
import sets_scale_cases as ssc
import wdist_model as wm
from rkmh_amd import api
from test_multigather_cpu import _same as _same_mg

THREADS = 8
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rkmh_amd", "csrc")


def _same_hits(got, want, what):
    assert got.dtype == np.int32 and got.shape == want.shape and (got == want).all(), (what, got.shape, want.shape, got.tolist()[:4], want.tolist()[:4])


def _hits_differ(a, b):
    return a.shape != b.shape or bool((a != b).any())


def _mg_host(c, qv, qo, **kw):
    return api.multigather_scaled_host(c["rv"], c["ro"], qv, qo, threads=THREADS, **kw)


def test_the_caps_are_the_sources():
    text = {n: open(os.path.join(SRC, n)).read() for n in ("rk_sets.hpp", "rk_search.hip", "rk_gather.hip", "rk_multigather.hip", "rk_scaled.hip")}
    assert "__launch_bounds__(1024) void k_scan_blocks" in text["rk_sets.hpp"] and "(nblocks + 1023) / 1024" in text["rk_sets.hpp"]
    assert "KEEP_T = 256, KEEP_ROUNDS = 4" in text["rk_sets.hpp"] and ssc.KEEP_BLK == 256 * 4
    assert re.search(r"inline uint32_t wave_grid\([^}]*1u << 16\)", text["rk_sets.hpp"]) and ssc.WAVE_GRID == (1 << 16) * 4
    assert "(nkeys + SEARCH_T - 1) / SEARCH_T, 1024)" in text["rk_search.hip"] and "SEARCH_T = 256" in text["rk_search.hip"]
    assert "(longest + GATHER_T - 1) / GATHER_T, 1024)" in text["rk_gather.hip"] and "GATHER_T = 256" in text["rk_gather.hip"]
    assert "MG_MAX_SLICES = 64" in text["rk_multigather.hip"] and "MG_T * 8" in text["rk_multigather.hip"] and "MG_T = 256" in text["rk_multigather.hip"]
    assert re.search(r"inline uint32_t flat_grid\([^}]*1u << 16\)", text["rk_multigather.hip"])
    assert "((size_t)64 << 20) / row_bytes" in text["rk_scaled.hip"]
    assert api.RK_SEARCH_REF_BLOCK == ssc.REF_BLOCK


# ---- wide_collection ----
def _wide_layout(c, cap):
    nref, rv, ro = c["nref"], c["rv"], c["ro"]
    assert nref == cap + 5 and len(ro) == nref + 1 and int(ro[-1]) == len(rv) == c["npost"]
    lens = np.diff(ro.astype(np.int64))
    want = np.full(nref, 2)
    for r, n in c["marked"]:
        want[r] = 2 + n
    assert (lens == want).all() and [r for r, _ in c["marked"]] == [cap, cap + 4, 0, cap - 1]
    assert int(rv[int(ro[cap])]) == cap + 1 and (rv[ro[1:].astype(np.int64) - 1] == ssc.COMMON).all()      # the row at the cap; COMMON ends every row
    keys, n = np.unique(rv, return_counts=True)
    assert len(keys) == c["nkeys"] and int(n.max()) == c["longest"] == nref and int(np.argmax(n)) == len(keys) - 1
    return keys, n


def test_wide_collection_miniature_against_the_models():
    cap = 64
    c = ssc.wide_collection(cap)
    _wide_layout(c, cap)
    refs = scm.rows(c["rv"], c["ro"])
    _same_hits(sem.search(refs, c["queries"]), c["hits1"], "hits at 1")
    _same_hits(sem.search(refs, c["queries"], 3), c["hits3"], "hits at 3")
    assert (gm.gather(c["queries"][0], refs) == c["gather0"]).all()
    _same_mg(mc.answer(refs, c["queries"]), c["mg"], "multigather")
    rows, wu, _ = am.gather_weighted(c["queries"][0], np.ones(12, np.uint32), refs)
    assert (rows == c["gather0"]).all() and wu == c["gather0"][:, 1].tolist()


def test_wide_collection_past_the_grid_of_waves():
    cap = ssc.WAVE_GRID
    c = ssc.wide_collection(cap)
    keys, n = _wide_layout(c, cap)
    rv, ro, q0 = c["rv"], c["ro"], c["queries"][0]
    qv, qo = scm.csr(c["queries"])
    assert (c["nref"] + ssc.REF_BLOCK - 1) // ssc.REF_BLOCK == 33
    assert np.unique(c["hits1"][:, 1] // ssc.REF_BLOCK).tolist() == list(range(33)) and int((c["hits1"][:, 0] == 3).sum()) == c["nref"]
    _same_hits(api.search_scaled_host(rv, ro, qv, qo, threads=THREADS), c["hits1"], "hits at 1")
    _same_hits(api.search_scaled_host(rv, ro, qv, qo, min_shared=3, threads=THREADS), c["hits3"], "hits at 3")
    assert (api.gather_scaled_host(q0, rv, ro, threads=THREADS) == c["gather0"]).all()
    rows, wu = api.gather_scaled_abund_host(q0, np.ones(len(q0), np.uint32), rv, ro, threads=THREADS)
    assert (rows == c["gather0"]).all() and wu.tolist() == c["gather0"][:, 1].tolist()
    _same_mg(_mg_host(c, qv, qo), c["mg"], "multigather")
    # what lies past the cap decides the answer
    cv, co = ssc.cut_rows(rv, ro, cap)                                            # k_index_ids, k_gather_probe: the references of one trip
    assert _hits_differ(api.search_scaled_host(cv, co, qv, qo, threads=THREADS), c["hits1"])
    cut_gather = api.gather_scaled_host(q0, cv, co, threads=THREADS)              # k_gather_compact, k_gather_count: the candidates of one trip
    assert int((c["hits1"][:, 0] == 0).sum()) == c["nref"] > cap and _hits_differ(cut_gather, c["gather0"])
    assert len(keys) > ssc.LONGEST_GRID and int(n[:ssc.LONGEST_GRID].max()) == 1 != c["longest"]        # k_longest_list: the keys of one trip


# ---- deep_collection ----
@pytest.mark.parametrize("total", sec.KEY_TOTALS)
def test_deep_collection_is_key_edges(total):
    c, k = ssc.deep_collection(total, sec.KEY_EDGES), sec.key_edges(total)
    assert c["nkeys"] == k["nkeys"] and c["longest"] == k["longest"] and c["runs"] == k["runs"]
    assert len(c["refs"]) == 5 and all(a.tolist() == b.tolist() for a, b in zip(c["refs"], k["refs"]))


@pytest.mark.parametrize("total", ssc.DEEP_TOTALS)
def test_deep_collection_past_a_million_entries(total):
    M = ssc.MILLION
    c = ssc.deep_collection(total)
    s = np.sort(c["rv"])
    assert len(s) == total and all((r[1:] > r[:-1]).all() for r in c["refs"])    # every row ascends, distinct
    first = np.concatenate([[True], s[1:] != s[:-1]])
    assert int(first.sum()) == c["nkeys"] and int(s[-1]) == (1 << 64) - 1
    for e in ssc.DEEP_EDGES:
        if total >= e + 3:
            assert s[e - 3] < s[e - 2] == s[e - 1] == s[e] < s[e + 1], e                     # the run lies across the edge
    assert s[0] == s[1] < s[2] and s[-3] < s[-2] == s[-1]
    counts = np.add.reduceat(first.astype(np.int64), np.arange(0, total, ssc.KEEP_BLK))
    assert (counts == c["block_counts"]).all() and len(counts) == (total + ssc.KEEP_BLK - 1) // ssc.KEEP_BLK
    per = (len(counts) + ssc.SCAN_T - 1) // ssc.SCAN_T
    assert per == {M: 1, M + 1: 2, M + 1030: 2, 2049 * 1024 + 1: 3}[total]
    if total == M:
        assert len(counts) == ssc.SCAN_T                                                    # the cap itself: the last size of one count a thread
    elif total == M + 1:
        assert counts[ssc.SCAN_T:].tolist() == [0]                                           # entry 2^20 ends the last pair: it begins no value
    else:
        assert ssc.scan_counts_depend(counts)                                                # the block after the run across 2^20 counts 1 023
        assert int(counts[ssc.SCAN_T]) == ssc.KEEP_BLK - 1
    if per == 3:
        assert (len(counts) + per - 1) // per < ssc.SCAN_T                                   # idle tail threads
    for ms in (1, 2):
        want = ssc.deep_hits(total, ms)
        _same_hits(api.search_scaled_host(c["rv"], c["ro"], c["rv"], c["ro"], min_shared=ms, threads=THREADS), want, (total, ms))
    assert 5 <= len(ssc.deep_hits(total, 2)) < len(ssc.deep_hits(total, 1)) <= 25


# ---- many_queries ----
def test_many_queries_miniature_against_the_models():
    c = ssc.many_queries(67)
    queries = scm.rows(c["qv"], c["qo"])
    assert [q.tolist() for q in queries[65:]] == [q.tolist() for q in queries[:2]]           # the permutation starts over
    _same_hits(sem.search(c["refs"], queries), c["hits"], "hits")
    _same_mg(mc.answer(c["refs"], queries), c["plain"], "plain")
    abunds = [c["qa"][int(c["qo"][i]):int(c["qo"][i + 1])] for i in range(67)]
    _same_mg(mc.answer(c["refs"], queries, abunds=abunds), c["weighted"], "weighted")
    _same_mg(mc.answer(c["refs"], queries, c["ms"]), c["at_ms"], "at the median count")


@pytest.mark.parametrize("nq", ssc.MANY_NQ)
def test_many_queries_past_the_width_of_the_scan(nq):
    c = ssc.many_queries(nq)
    qv, qo = c["qv"], c["qo"]
    assert len(qo) == nq + 1 and int(qo[-1]) == len(qv) == len(c["qa"])
    lens = np.diff(qo.astype(np.int64))
    assert lens.min() == 0 and lens.max() == 4097
    _same_hits(api.search_scaled_host(c["rv"], c["ro"], qv, qo, threads=THREADS), c["hits"], nq)
    _same_mg(_mg_host(c, qv, qo), c["plain"], (nq, "plain"))
    _same_mg(_mg_host(c, qv, qo, max_rounds=2), mc.cut(c["plain"], 2), (nq, "max_rounds 2"))
    if nq == 1025:
        _same_mg(_mg_host(c, qv, qo, q_abund=c["qa"]), c["weighted"], (nq, "weighted"))
        _same_mg(_mg_host(c, qv, qo, min_shared=c["ms"]), c["at_ms"], (nq, "at the median count"))
    nhits = np.bincount(c["hits"][:, 0], minlength=nq)                                      # the search's count per workgroup (one reference block)
    nrows = np.diff(c["plain"][1].astype(np.int64))                                          # t[]: the rows of every query
    rcap2 = np.minimum(nhits, 2)                                                             # rcap[] at max_rounds 2
    if nq > ssc.SCAN_T:
        for counts in (nhits, nrows, rcap2, np.diff(c["at_ms"][1].astype(np.int64))):
            assert ssc.scan_counts_depend(counts), nq
    else:
        assert not ssc.scan_counts_depend(nhits)                                             # at the cap and one below it: nothing lies past it
    if nq == 2049:                                                                           # queries without a row and with several, on both sides
        for side in (nrows[:ssc.SCAN_T], nrows[ssc.SCAN_T:]):
            assert (side == 0).any() and (side > 1).any()
        assert (lens[ssc.SCAN_T:] == 0).any()


def test_many_queries_two_blocks():
    c = ssc.many_queries_two_blocks()
    qv, qo = c["qv"], c["qo"]
    nq, nblk = len(qo) - 1, (c["nref"] + ssc.REF_BLOCK - 1) // ssc.REF_BLOCK
    assert (nq, nblk, nq * nblk) == (1028, 2, 2056)
    _same_hits(api.search_scaled_host(c["rv"], c["ro"], qv, qo, threads=THREADS), c["hits"], "hits")
    _same_mg(_mg_host(c, qv, qo), c["plain"], "plain")
    per_wg = np.bincount(c["hits"][:, 0].astype(np.int64) * nblk + c["hits"][:, 1] // ssc.REF_BLOCK, minlength=nq * nblk)
    assert ssc.scan_counts_depend(per_wg) and per_wg[ssc.SCAN_T + 1] == 1                    # the second block holds one reference
    nrows = np.diff(c["plain"][1].astype(np.int64))
    assert ssc.scan_counts_depend(nrows) and nrows[:4].min() >= 1 and nrows[:4].max() > 1


# ---- flood_of_queries ----
def _flood_layout(c, cap):
    nq = cap + 3
    qo = c["qo"]
    assert len(qo) == nq + 1 and int(qo[-1]) == len(c["qv"])
    queries = scm.rows(c["qv"], c["qo"])
    for i in (0, 1, 6, 7, cap, cap + 1, cap + 2):
        assert queries[i].tolist() == list(ssc.FLOOD_KINDS[i % 7][0]), i
    nrows = np.diff(c["full"][1].astype(np.int64))
    assert nrows[cap:].min() >= 1 and len(set(nrows[cap:].tolist())) > 1                     # past the cap: rows, and of different counts
    assert (np.diff(c["one"][1].astype(np.int64)) == np.minimum(nrows, 1)).all()
    return queries


def test_flood_of_queries_miniature_against_the_models():
    c = ssc.flood_of_queries(64)
    queries = _flood_layout(c, 64)
    _same_hits(sem.search(c["refs"], queries), c["hits"], "hits")
    _same_mg(mc.answer(c["refs"], queries), c["full"], "every round")
    _same_mg(mc.answer(c["refs"], queries, 1, 1), c["one"], "one round")


def test_flood_of_queries_past_the_grid_of_waves():
    cap = ssc.WAVE_GRID
    c = ssc.flood_of_queries(cap)
    qv, qo = c["qv"], c["qo"]
    nq = cap + 3
    assert len(qo) == nq + 1 and int(qo[-1]) == len(qv)
    for i in (0, cap - 1, cap, cap + 1, cap + 2):
        assert qv[int(qo[i]):int(qo[i + 1])].tolist() == list(ssc.FLOOD_KINDS[i % 7][0]), i
    nrows = np.diff(c["full"][1].astype(np.int64))
    assert nrows[cap:].tolist() == [1, 1, 2]
    _same_hits(api.search_scaled_host(c["rv"], c["ro"], qv, qo, threads=THREADS), c["hits"], "hits")
    _same_mg(_mg_host(c, qv, qo), c["full"], "every round")
    _same_mg(_mg_host(c, qv, qo, max_rounds=1), c["one"], "one round")
    cut = _mg_host(c, *ssc.cut_rows(qv, qo, cap))                                           # k_mg_pack: the queries of one trip
    assert len(cut[0]) == len(c["full"][0]) - 4 and len(cut[0]) == int(c["full"][1][cap])
    assert ssc.scan_counts_depend(nrows) and ssc.scan_counts_depend(np.bincount(c["hits"][:, 0], minlength=nq))


# ---- long_pick ----
def _long_pick_layout(c, cap):
    q, refs = c["q"], c["refs"]
    assert c["n"] == cap + 300 == len(refs[0]) and len(q) == c["n"] + 500 and (np.diff(q.astype(np.int64)) > 0).all()
    assert [len(r) for r in refs] == [cap + 300, 250, 100, 500]
    assert np.isin(refs[1], refs[0][cap:]).sum() == 200 and not np.isin(refs[1], refs[0][:cap]).any()   # reference 1 lives in the tail
    assert np.isin(refs[2], refs[0][:100]).all() and not np.isin(refs[2], refs[1]).any()
    assert len(c["tail"]) == 300 and int((c["abund"][c["tail"]] == am.SAT).sum()) == 2 and int((c["abund"] == am.SAT).sum()) == 2
    assert int(c["wunique"][0]) > 2 * am.SAT and int(c["wunique"].sum()) == int(c["abund"].astype(np.uint64).sum())


def test_long_pick_miniature_against_the_models():
    c = ssc.long_pick(256)                                                                   # (the smallest cap at which the first pick is still reference 0: 556 > 500)
    _long_pick_layout(c, 256)
    assert (gm.gather(c["q"], c["refs"]) == c["rows"]).all()
    rows, wu, left = am.gather_weighted(c["q"], c["abund"], c["refs"])
    assert (rows == c["rows"]).all() and wu == c["wunique"].tolist() and left == 0
    cut = gm.gather(c["q"], (c["refs"][0][:256],) + c["refs"][1:])                           # the tail of the first pick stays in the query
    assert cut[:, 0].tolist() == [3, 0, 1]


def test_long_pick_past_the_removal_grid_and_the_slices():
    cap = ssc.REMOVE_GRID
    c = ssc.long_pick(cap)
    _long_pick_layout(c, cap)
    q, rv, ro = c["q"], c["rv"], c["ro"]
    assert (len(q) + ssc.MG_SLICE - 1) // ssc.MG_SLICE > ssc.MG_MAX_SLICES                   # multigather caps its slices: more than one trip a wave
    assert (api.gather_scaled_host(q, rv, ro, threads=THREADS) == c["rows"]).all()
    rows, wu = api.gather_scaled_abund_host(q, c["abund"], rv, ro, threads=THREADS)
    assert (rows == c["rows"]).all() and wu.tolist() == c["wunique"].tolist()
    one = np.array([0, len(q)], dtype=np.uint64)
    _same_mg(_mg_host(c, q, one), (c["rows"], np.array([0, 2], np.uint64), None), "multigather")
    _same_mg(_mg_host(c, q, one, q_abund=c["abund"]), (c["rows"], np.array([0, 2], np.uint64), c["wunique"]), "multigather, weighted")
    cv, co = scm.csr((c["refs"][0][:cap],) + c["refs"][1:])                                  # k_gather_remove: the hit list of one trip
    cut = api.gather_scaled_host(q, cv, co, threads=THREADS)
    assert cut[:, 0].tolist() == [0, 3, 1] and cut[2].tolist() == [1, 200, 200, 100]


# ---- long_query ----
def test_long_query_miniature_against_the_models():
    c = ssc.long_query(64)
    _same_hits(sem.search(c["refs"], [c["q"]]), c["hits"], "hits")
    _same_mg(mc.answer(c["refs"], [c["q"]]), c["mg"], "multigather")


def test_long_query_past_the_flat_grid():
    """the layout, the closed form, and -- they take a fraction of a second on 16.8 M values -- the host entries too"""
    cap = ssc.FLAT_GRID
    c = ssc.long_query()
    q, refs = c["q"], c["refs"]
    assert len(q) == cap + 1000 and int(q[0]) == 1 and int(q[-1]) == len(q) and c["qo"].tolist() == [0, len(q)]
    assert int(refs[0][0]) - 1 >= cap and len(refs[0]) == 500 and int(refs[1][-1]) == 300    # reference 0 lies past the cap altogether
    assert np.isin(refs[2], refs[0]).sum() == 100 and np.isin(refs[2], refs[1]).sum() == 100 and len(refs[2]) == 200
    assert c["mg"][0].tolist() == [[0, 500, 500, cap + 500], [1, 300, 300, cap + 200]]
    cut = sem.search(c["refs"], [q[:cap]])                                                   # k_mg_keypos: the values of one trip
    assert cut.tolist() == [[0, 1, 300], [0, 2, 100]] and _hits_differ(cut, c["hits"])
    _same_hits(api.search_scaled_host(c["rv"], c["ro"], q, c["qo"], threads=THREADS), c["hits"], "hits")
    _same_mg(_mg_host(c, q, c["qo"]), c["mg"], "multigather")


# ---- pair_matrix ----
def _sides(c, n):
    v = c["v"].reshape(n, 2)
    return [(v[i], c["wa"].reshape(n, 2)[i]) for i in range(n)], [(v[i], c["wb"].reshape(n, 2)[i]) for i in range(n)]


def test_pair_matrix_miniature_against_the_models():
    n = 30
    c = ssc.pair_matrix(n, "weighted")
    A, B = _sides(c, n)
    shared = ssc.pair_matrix(n, "plain")["shared"]
    assert shared.dtype == np.int32 and (scm.all_shared([a[0] for a in A]) == shared).all() and (c["weighted"][:, :, 0] == shared).all()
    assert (wm.all_pairs(A, B) == c["weighted"]).all() and (wm.all_pairs(A) == c["weighted_self"]).all()
    assert c["weighted"][3, 3, 0] == 2 and c["weighted"][3, 10, 0] == 1 and c["weighted"][3, 4, 0] == 0


@pytest.mark.parametrize("kind", sorted(ssc.PAIR_N))
def test_pair_matrix_past_one_row_block(kind):
    n = ssc.PAIR_N[kind]
    c = ssc.pair_matrix(n, kind)
    rows = ssc.rows_per_block(n, kind)
    assert n * n * ssc.PAIR_BYTES[kind] > ssc.ROW_BLOCK_BYTES and (rows, n - rows) == {"plain": (4092, 8), "weighted": (1398, 102)}[kind]
    assert c["off"].tolist() == list(range(0, 2 * n + 1, 2)) and (np.diff(c["v"].reshape(n, 2).astype(np.int64), axis=1) > 0).all()
    for want in ((c["shared"],) if kind == "plain" else (c["weighted"], c["weighted_self"])):
        # a second block written where the first one lies, or never: both the block and its place decide the answer
        assert want[rows:].any() and (want[rows:] != want[:n - rows]).any() and (want[rows:] != 0).any()
    if kind == "weighted":
        got = api.compare_scaled_abund_host(c["v"], c["wa"], c["off"], c["v"].copy(), c["wb"], c["off"].copy(), threads=THREADS)
        assert (got == c["weighted"]).all()
        assert (api.compare_scaled_abund_host(c["v"], c["wa"], c["off"], threads=THREADS) == c["weighted_self"]).all()


# ---- kept_past_a_million ----
def test_kept_past_a_million():
    c = ssc.kept_past_a_million()
    M = ssc.MILLION
    starts = c["starts"]
    assert [len(s) for s in c["seqs"]] == list(ssc.KEPT_LENGTHS)
    kept = [np.repeat(v, a.astype(np.int64)) for v, a in c["want"]]                           # a sequence's kept values as the device sorts them
    assert [len(k) for k in kept] == np.diff(starts).tolist()
    assert all(len(k) in (len(s) - ssc.KEPT_K, len(s) - ssc.KEPT_K + 1) for k, s in zip(kept, c["seqs"]))   # no window hashes to 0: every window the policy takes is kept
    assert starts[2] > M and starts[3] > starts[2] + 100_000                                 # the third sequence begins past entry 2^20
    for i in (1, 2):
        v, a = c["want"][i]
        at = int(np.argmax(a))
        assert int(a[at]) >= ssc.KEPT_RUN - ssc.KEPT_K + 1
        if i == 2:
            assert starts[2] + int(a[:at].astype(np.int64).sum()) > M                        # its run of equal values: on the far side of block 1 024
    flat = np.concatenate(kept)
    first = np.concatenate([[True], flat[1:] != flat[:-1]])
    first[starts[1:3]] = True
    counts = np.add.reduceat(first.astype(np.int64), np.arange(0, len(flat), ssc.KEEP_BLK))
    assert len(counts) > ssc.SCAN_T and ssc.scan_counts_depend(counts)
    assert int(first.sum()) == sum(len(v) for v, _ in c["want"])
    assert all(c["want"][i][0].tolist() == scm.sketch(c["seqs"][i], [ssc.KEPT_K], ssc.sm.DEFAULT, scm.FULL).tolist() for i in (0, 2))
