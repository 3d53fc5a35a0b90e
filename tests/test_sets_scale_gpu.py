"""The sketch-set kernels past their grid caps and scan widths, on the GPU: every case of tests/sets_scale_cases.py through every entry
that reaches the loop in question -- the second trip of a capped grid's stride loop, k_scan_blocks at two and three counts a thread,
the second row block of the pair matrix -- compared exactly with the closed forms.  The device entries run on torch's arrays and
stream with guard words around every output: the helpers are those of the search, gather, multigather and comparison tests.  That the
inputs lie where they say, that the closed forms are right and that every case depends on what lies past its cap is shown without a
GPU by tests/test_sets_scale_cpu.py."""
import numpy as np
import pytest

import multigather_cases as mc
import scaled_model as scm
import sets_scale_cases as ssc
import test_gather_gpu as tgg
import test_gpu_abund as tga
import test_gpu_scaled as tgsc
import test_gpu_search as tgs
import test_gpu_wdist as twd
import test_multigather_gpu as tmg

pytestmark = pytest.mark.gpu


def _indexes(ctx, rv, ro):
    """the index of a CSR side through both entries (the resident arrays only have to live until the build returns)"""
    import torch
    yield "host entry", ctx.scaled_index(rv, ro)
    d_rv, d_ro = tgs._up(rv), tgs._up(ro)
    yield "device entry", ctx.scaled_index_device(d_rv.data_ptr(), d_ro.data_ptr(), len(ro) - 1, len(rv), stream=torch.cuda.current_stream().cuda_stream)


def _search(idx, qv, qo, want, what, min_shared=1):
    tgs._same(idx.search(qv, qo, min_shared=min_shared), want, (what, "host entry"))
    total, hits = tgs._device(idx, [qv], min_shared, qo=qo)
    assert total == len(want), (what, total, len(want))
    tgs._same(hits, want, (what, "device entry"))


def _multigather(idx, qv, qo, want, what, qa=None, min_shared=1, max_rounds=None):
    """both entries; the device entry is asked with room for no row first, then for exactly the rows there are"""
    tmg._same(idx.multigather(qv, qo, q_abund=qa, min_shared=min_shared, max_rounds=max_rounds), want, (what, "host entry"))
    n, rows, off, wu = tmg._device(idx, [qv], None if qa is None else [qa], min_shared, max_rounds, qo=qo)
    assert n == len(want[0]), (what, n, len(want[0]))
    tmg._same((rows, off, wu), want, (what, "device entry"))


# ---- wide_collection: k_index_ids, k_longest_list, k_gather_probe, k_gather_compact, k_gather_count past 262 144 ----
def test_wide_collection_index_search_multigather(ctx):
    c = ssc.wide_collection(ssc.WAVE_GRID)
    qv, qo = scm.csr(c["queries"])
    for entry, idx in _indexes(ctx, c["rv"], c["ro"]):
        assert idx.stats() == dict(nref=c["nref"], npost=c["npost"], nkeys=c["nkeys"], longest_posting=c["longest"]), entry
        _search(idx, qv, qo, c["hits1"], (entry, 1))
        _search(idx, qv, qo, c["hits3"], (entry, 3), min_shared=3)
        _multigather(idx, qv, qo, c["mg"], entry)
        idx.close()


def test_wide_collection_gather(ctx):
    c = ssc.wide_collection(ssc.WAVE_GRID)
    q, rv, ro, want = c["queries"][0], c["rv"], c["ro"], c["gather0"]
    tgg._same(ctx.gather_scaled(q, rv, ro), want, "host entry")
    tgg._same(tgg._device(ctx, q, rv, ro), want, "device entry")
    ones = np.ones(len(q), dtype=np.uint32)                                       # all abundances 1: wunique = unique
    tga._same(ctx.gather_scaled_abund(q, ones, rv, ro), (want, want[:, 1]), "weighted, host entry")
    tga._same(tga._device(ctx, q, ones, rv, ro), (want, want[:, 1]), "weighted, device entry")


# ---- deep_collection: k_scan_blocks over the index build's blocks ----
@pytest.mark.parametrize("total", ssc.DEEP_TOTALS)
def test_keys_around_the_edges_of_the_compaction_past_a_million(ctx, total):
    """tests/test_gpu_search.py::test_keys_around_the_edges_of_the_compaction where the scan's threads take one, two and three block
    counts each, with a value held by three references across entry 2^20"""
    c = ssc.deep_collection(total)
    idx = ctx.scaled_index(c["rv"], c["ro"])
    s = idx.stats()
    assert s["nref"] == 5 and s["npost"] == total and s["nkeys"] == c["nkeys"] and s["longest_posting"] == c["longest"]
    for ms in (1, 2):
        _search(idx, c["rv"], c["ro"], ssc.deep_hits(total, ms), (total, ms), min_shared=ms)
    idx.close()


# ---- many_queries: k_scan_blocks over the search's workgroups and over multigather's rcap[] and t[] ----
@pytest.mark.parametrize("nq", ssc.MANY_NQ)
def test_many_queries(ctx, nq):
    c = ssc.many_queries(nq)
    qv, qo = c["qv"], c["qo"]
    idx = ctx.scaled_index(c["rv"], c["ro"])
    _search(idx, qv, qo, c["hits"], nq)
    _multigather(idx, qv, qo, c["plain"], nq)
    if nq == 1025:
        _multigather(idx, qv, qo, c["weighted"], (nq, "weighted"), qa=c["qa"])
        _multigather(idx, qv, qo, c["at_ms"], (nq, "min_shared", c["ms"]), min_shared=c["ms"])
        _multigather(idx, qv, qo, mc.cut(c["plain"], 2), (nq, "max_rounds 2"), max_rounds=2)
    idx.close()


def test_many_queries_two_blocks(ctx):
    c = ssc.many_queries_two_blocks()
    idx = ctx.scaled_index(c["rv"], c["ro"])
    _search(idx, c["qv"], c["qo"], c["hits"], "2 056 workgroups")
    _multigather(idx, c["qv"], c["qo"], c["plain"], "2 056 workgroups")
    idx.close()


# ---- flood_of_queries: k_mg_pack past 262 144 queries ----
def test_flood_of_queries(ctx):
    c = ssc.flood_of_queries(ssc.WAVE_GRID)
    qv, qo = c["qv"], c["qo"]
    idx = ctx.scaled_index(c["rv"], c["ro"])
    _search(idx, qv, qo, c["hits"], "flood")
    _multigather(idx, qv, qo, c["full"], "every round")
    _multigather(idx, qv, qo, c["one"], "one round", max_rounds=1)
    total = len(c["full"][0])
    n, rows, off, _ = tmg._device(idx, [qv], cap=total - 1, qo=qo)                 # room for all rows but the last one, which a query past the cap writes
    assert n == total and off.tolist() == c["full"][1].tolist() and (rows == c["full"][0][:total - 1]).all()
    idx.close()


# ---- long_pick: k_gather_remove, k_gather_remove_w past 262 144 hits; k_mg_remove at its 64 slices ----
def test_long_pick(ctx):
    c = ssc.long_pick(ssc.REMOVE_GRID)
    q, a, rv, ro, rows, wu = c["q"], c["abund"], c["rv"], c["ro"], c["rows"], c["wunique"]
    tgg._same(ctx.gather_scaled(q, rv, ro), rows, "host entry")
    tgg._same(tgg._device(ctx, q, rv, ro), rows, "device entry")
    tga._same(ctx.gather_scaled_abund(q, a, rv, ro), (rows, wu), "weighted, host entry")
    tga._same(tga._device(ctx, q, a, rv, ro), (rows, wu), "weighted, device entry")
    one, off = np.array([0, len(q)], dtype=np.uint64), np.array([0, 2], dtype=np.uint64)
    idx = ctx.scaled_index(rv, ro)
    _multigather(idx, q, one, (rows, off, None), "multigather")
    _multigather(idx, q, one, (rows, off, wu), "multigather, weighted", qa=a)
    idx.close()


# ---- long_query: k_mg_keypos past 16 777 216 query values ----
def test_long_query(ctx):
    c = ssc.long_query()
    idx = ctx.scaled_index(c["rv"], c["ro"])
    _search(idx, c["q"], c["qo"], c["hits"], "long query")
    _multigather(idx, c["q"], c["qo"], c["mg"], "long query")
    idx.close()


# ---- pair_matrix: the second 64 MB row block of compare_uploaded ----
def test_pair_matrix_plain(ctx):
    n = ssc.PAIR_N["plain"]
    c = ssc.pair_matrix(n, "plain")
    v, off, want = c["v"], c["off"], c["shared"]
    v2, off2 = v.copy(), off.copy()
    for lanes in (0, 8):
        tgsc._same(ctx.compare_scaled(v, off, lanes=lanes), want, ("a is b", lanes))
        tgsc._same(ctx.compare_scaled(v, off, v2, off2, lanes=lanes), want, ("two sides", lanes))
    tgsc._same(tgsc._device(ctx, v, off, v2, off2, 0), want, "device entry: no row blocks")


def test_pair_matrix_weighted(ctx):
    n = ssc.PAIR_N["weighted"]
    c = ssc.pair_matrix(n, "weighted")
    v, off, wa, wb = c["v"], c["off"], c["wa"], c["wb"]
    v2, off2 = v.copy(), off.copy()
    for lanes in (0, 8):
        twd._same(ctx.compare_scaled_abund(v, wa, off, lanes=lanes), c["weighted_self"], ("a is b", lanes))
        twd._same(ctx.compare_scaled_abund(v, wa, off, v2, wb, off2, lanes=lanes), c["weighted"], ("two sides", lanes))
    A = [(v[2 * i:2 * i + 2], wa[2 * i:2 * i + 2]) for i in range(n)]
    B = [(v[2 * i:2 * i + 2], wb[2 * i:2 * i + 2]) for i in range(n)]
    twd._same(twd._device(ctx, A, B, 0), c["weighted"], "device entry: no row blocks")


# ---- kept_past_a_million: k_scan_blocks over KEEP_FIRST's blocks, with and without abundances ----
def test_kept_past_a_million(ctx):
    c = ssc.kept_past_a_million()
    seqs, want = list(c["seqs"]), c["want"]
    plain = tgsc._sketch(ctx, seqs, [ssc.KEPT_K], scm.FULL)
    tgsc._equal_rows(plain, [v for v, _ in want], "three sequences in one chunk")
    both = tga._sketch(ctx, seqs, [ssc.KEPT_K], scm.FULL)                           # (its values are compared with the plain entry's in there)
    tga._equal(both, want, "three sequences in one chunk, abundances")
    for i, s in enumerate(seqs):                                                   # each sequence alone is its row of the batch
        tgsc._equal_rows(tgsc._sketch(ctx, [s], [ssc.KEPT_K], scm.FULL), [plain[i]], ("alone", i))
        tga._equal(tga._sketch(ctx, [s], [ssc.KEPT_K], scm.FULL), [both[i]], ("alone, abundances", i))
