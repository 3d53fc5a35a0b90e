"""Inputs for the sketch-set kernels past their grid caps and scan widths (tests/test_sets_scale_cpu.py, tests/test_sets_scale_gpu.py):
every kernel of rk_sets.hpp's layer that takes "one wave (or thread) per item" runs on a capped grid and strides, every compaction and
search hands its per-workgroup counts to the one-workgroup k_scan_blocks, and the pair matrix leaves the host entry in row blocks.
Each builder takes its cap as a parameter: the real cap gives the case the GPU runs, a small one a miniature that the Python models
answer.  Sides are emitted as CSR (values, offsets) straight from vectorised numpy; the expected answers are closed forms written
beside each construction.  Computed once per process and left unchanged (the two largest, long_query and pair_matrix, are built
for the one test that uses them and not kept)."""
import functools

import numpy as np

import abund_cases as ac
import abund_model as am
import multigather_cases as mc
import scaled_model as scm
import search_cases as sec
import search_model as sem
import sourmash_model as sm

# ---- the caps, each with the source line it mirrors ----
SCAN_T = 1024                    # rk_sets.hpp, k_scan_blocks: one workgroup of 1 024 threads, per = ceil(n / 1024) counts a thread
KEEP_BLK = 1024                  # rk_sets.hpp: KEEP_BLK = KEEP_T * KEEP_ROUNDS, the elements behind one count of a compaction
WAVE_GRID = (1 << 16) * 4        # rk_sets.hpp, wave_grid: at most 2^16 workgroups of 4 waves (k_index_ids, k_gather_probe, _compact, _count, k_mg_pack)
LONGEST_GRID = 1024 * 256        # rk_search.hip, index_build: k_longest_list on at most 1 024 workgroups of SEARCH_T threads
REMOVE_GRID = 1024 * 256         # rk_gather.hip, gather_run: remove_grid, at most 1 024 workgroups of GATHER_T threads over the pick's list
MG_MAX_SLICES = 64               # rk_multigather.hip: workgroups that share one query's values in k_mg_remove, at most
MG_SLICE = 256 * 8               # rk_multigather.hip, mg_rounds: `slices` gives a workgroup eight values per lane
FLAT_GRID = (1 << 16) * 256      # rk_multigather.hip, flat_grid: at most 2^16 workgroups of MG_T threads (k_mg_keypos, k_mg_init)
ROW_BLOCK_BYTES = 64 << 20       # rk_scaled.hip, compare_uploaded: the rows of the answer leave in blocks of at most 64 MB
PAIR_BYTES = {"plain": 4, "weighted": 32}   # one int32 a pair; (shared, dot, wa_in, wb_in) uint64 a pair
REF_BLOCK = sec.REF_BLOCK        # include/rkmh_amd.h: RK_SEARCH_REF_BLOCK
MILLION = SCAN_T * KEEP_BLK      # 2^20 elements: the most a compaction scans at one count a thread

COMMON = np.uint64((1 << 64) - 1)            # the largest key there can be: its posting list is the last one
EXTRA = 1 << 40


def _ro(a, dtype=np.uint64):
    a = np.ascontiguousarray(a, dtype=dtype)
    a.setflags(write=False)
    return a


def _offsets(lens):
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.asarray(lens, dtype=np.int64))
    return _ro(off)


def _by_row(row, values, nrows):
    """entries (row, value) -> the CSR side whose rows ascend"""
    order = np.lexsort((values, row))
    return _ro(values[order]), _offsets(np.bincount(row, minlength=nrows))


def _hits(rows):
    h = np.asarray(rows, dtype=np.int32).reshape(len(rows), 3)
    h.setflags(write=False)
    return h


def cut_rows(values, offsets, n):
    """the first n rows of a CSR side: what a launch that stopped after one trip over n rows would have seen"""
    return values[:int(offsets[n])], offsets[:n + 1]


def scan_counts_depend(counts, width=SCAN_T):
    """do the counts past entry `width` matter to a scan: they are there, not all zero and not all equal (a single count past the
    width -- n = width + 1 -- cannot differ from itself: it has to be non-zero)"""
    tail = np.asarray(counts)[width:]
    return len(tail) > 0 and bool(tail.any()) and (len(tail) == 1 or len(np.unique(tail)) > 1)


# ---- wide_collection: more references than wave_grid gives waves; more keys than k_longest_list gives threads ----
@functools.lru_cache(maxsize=None)
def wide_collection(cap):
    """nref = cap + 5 references.  Every one holds COMMON and one value of its own, r + 1.  Four marked rows hold extra values,
    EXTRA + j: reference cap three of them, nref - 1 two, 0 and cap - 1 one each.  Queries: 0 = all values of the marked rows and
    COMMON (12 values: it shares 5 | 4 | 3 | 3 with the marked rows and 1 with everyone); 1 = [own(cap)]; 2 = [own(cap - 1),
    own(nref - 1)]; 3 = [COMMON].
    Closed forms: nkeys = nref + 8 and the longest posting list, COMMON's nref entries, is the last key; the hits below; gather of
    query 0 picks cap (5 of 5), then -- COMMON gone -- nref - 1 (3 of 4), 0 (2 of 3) and cap - 1 (2 of 3): the 2 | 2 tie falls to the
    lower index, across the cap; every other candidate is left with 0, and the run stops."""
    nref = cap + 5
    marked = ((cap, 3), (nref - 1, 2), (0, 1), (cap - 1, 1))
    rows, vals, j = [np.arange(nref), np.arange(nref)], [np.arange(1, nref + 1, dtype=np.uint64), np.full(nref, COMMON)], 0
    extras = {}
    for r, n in marked:
        extras[r] = np.arange(EXTRA + j, EXTRA + j + n, dtype=np.uint64)
        rows.append(np.full(n, r))
        vals.append(extras[r])
        j += n
    rv, ro = _by_row(np.concatenate(rows), np.concatenate(vals).astype(np.uint64), nref)
    own = lambda r: np.uint64(r + 1)
    q0 = np.unique(np.concatenate([[own(r) for r, _ in marked], [COMMON]] + [extras[r] for r, _ in marked]).astype(np.uint64))
    queries = tuple(_ro(q) for q in (q0, [own(cap)], [own(cap - 1), own(nref - 1)], [COMMON]))
    every = np.arange(nref)
    n0 = np.ones(nref, dtype=np.int64)
    for r, n in marked:
        n0[r] = 2 + n
    hits1 = np.concatenate([np.stack([np.zeros(nref, np.int64), every, n0], axis=1), [[1, cap, 1], [2, cap - 1, 1], [2, nref - 1, 1]],
                            np.stack([np.full(nref, 3), every, np.ones(nref, np.int64)], axis=1)])
    hits3 = [[0, 0, 3], [0, cap - 1, 3], [0, cap, 5], [0, nref - 1, 4]]
    gather0 = [[cap, 5, 5, 7], [nref - 1, 3, 4, 4], [0, 2, 3, 2], [cap - 1, 2, 3, 0]]
    mg_rows = gather0 + [[cap, 1, 1, 0], [cap - 1, 1, 1, 1], [nref - 1, 1, 1, 0], [0, 1, 1, 0]]   # [COMMON] alone: the lowest index, then nothing is left
    return dict(nref=nref, rv=rv, ro=ro, queries=queries, marked=marked, nkeys=nref + 8, longest=nref, npost=2 * nref + 7,
                hits1=_hits(hits1), hits3=_hits(hits3), gather0=np.asarray(gather0, dtype=np.int32),
                mg=(np.asarray(mg_rows, dtype=np.int32), np.asarray([0, 4, 5, 7, 8], dtype=np.uint64), None))


# ---- deep_collection: the index's keys out of a compaction of more than 1 024 blocks ----
DEEP_EDGES = sec.KEY_EDGES + (MILLION,)
DEEP_TOTALS = (MILLION, MILLION + 1, MILLION + 1030, 2049 * KEEP_BLK + 1)   # per = 1 (the cap itself) | 2 | 2, two counts past the cap | 3, idle tail threads


@functools.lru_cache(maxsize=None)
def deep_collection(total, edges=DEEP_EDGES):
    """search_cases.key_edges(total) without its per-entry loop, and with one more edge at entry 2^20 -> dict(rv, ro, refs, nkeys,
    longest, runs, block_counts).  Five references whose values, concatenated and sorted, are `total` entries: the first and the last
    value are held by two references each, at every edge e with total >= e + 3 a value held by three stands at entries e - 2, e - 1,
    e, every other value is held by one; the i-th distinct value of multiplicity m is held by references i % 5 ... (i + m - 1) % 5.
    block_counts: the distinct values that begin in each block of 1 024 entries -- what k_keep_count<KEEP_RUN> hands to the scan."""
    runs = {} if total < 2 else {0: 2, total - 2: 2}
    for e in edges:
        if total >= e + 3:
            runs[e - 2] = 3
    first = np.ones(total, dtype=bool)                       # does a value begin at this entry
    for s, m in runs.items():
        first[s + 1:s + m] = False
    ith = np.cumsum(first) - 1                               # entry -> the index of its distinct value
    nkeys = int(ith[-1]) + 1
    start = np.flatnonzero(first)
    within = np.arange(total) - start[ith]
    values = (np.arange(1, nkeys + 1, dtype=np.uint64) << np.uint64(20)) + np.uint64(3)
    values[-1] = COMMON
    rv, ro = _by_row((ith + within) % 5, values[ith], 5)
    counts = np.add.reduceat(first.astype(np.int64), np.arange(0, total, KEEP_BLK))
    return dict(rv=rv, ro=ro, refs=tuple(scm.rows(rv, ro)), nkeys=nkeys, longest=max(list(runs.values()) + [1]), runs=runs, block_counts=counts)


@functools.lru_cache(maxsize=None)
def deep_hits(total, min_shared):
    """every reference of deep_collection(total) searched as a query: 25 intersections of sorted arrays (search_model.search)"""
    refs = deep_collection(total)["refs"]
    return _hits(sem.search(refs, refs, min_shared))


# ---- many_queries: more queries than the scan has threads ----
MANY_NQ = (1023, 1024, 1025, 2049)


@functools.lru_cache(maxsize=None)
def _many_base():
    """the 65 queries of multigather_cases.many_queries(), abundances for them, and their answers one by one"""
    m = mc.many_queries()
    refs, queries = m["refs"], m["queries"]
    abunds = tuple(ac.abundances(np.random.default_rng(9100 + i), len(q)) for i, q in enumerate(queries))
    rv, ro = scm.csr(refs)
    from rkmh_amd import api
    hits = api.search_scaled_host(rv, ro, *scm.csr(queries))
    plain = mc.answer(refs, queries, host=True)
    ms = mc.median_count(plain)
    return dict(refs=refs, rv=_ro(rv), ro=_ro(ro), queries=queries, abunds=abunds, hits=hits, plain=plain, ms=ms,
                weighted=mc.answer(refs, queries, abunds=abunds, host=True), at_ms=mc.answer(refs, queries, ms, host=True))


def _laid_out(ans, order):
    """the per-query blocks of an answer laid end to end in `order`"""
    per = mc.blocks(ans)
    rows = np.concatenate([per[i][0] for i in order] + [np.zeros((0, 4), np.int32)])
    off = _offsets([len(per[i][0]) for i in order])
    wu = None if ans[2] is None else np.concatenate([per[i][1] for i in order] + [np.zeros(0, np.uint64)])
    return rows, off, wu


def _renumbered(hits, order, nbase):
    """the hits of the base queries -> the hits of the queries base[order[0]], base[order[1]], ..."""
    lo = np.searchsorted(hits[:, 0], np.arange(nbase), side="left")
    hi = np.searchsorted(hits[:, 0], np.arange(nbase), side="right")
    n = (hi - lo)[order]
    src = np.concatenate([np.arange(lo[i], hi[i]) for i in order] + [np.zeros(0, np.int64)]).astype(np.int64)
    out = hits[src].copy()
    out[:, 0] = np.repeat(np.arange(len(order)), n)
    return _hits(out)


@functools.lru_cache(maxsize=None)
def many_queries(nq):
    """the 65 queries of multigather_cases.many_queries() over and over in one fixed permutation, nq of them -> dict(refs as CSR,
    qv, qo, qa, order, hits, plain, weighted, at_ms, ms): the answers are the per-query blocks laid end to end, the hits renumbered"""
    b = _many_base()
    perm = np.random.default_rng(19).permutation(len(b["queries"]))
    order = perm[np.arange(nq) % len(perm)]
    qv = np.concatenate([b["queries"][i] for i in order])
    qa = np.concatenate([b["abunds"][i] for i in order])
    return dict(rv=b["rv"], ro=b["ro"], refs=b["refs"], qv=_ro(qv), qa=_ro(qa, np.uint32), qo=_offsets([len(b["queries"][i]) for i in order]), order=order,
                hits=_renumbered(b["hits"], order, len(perm)), plain=_laid_out(b["plain"], order), weighted=_laid_out(b["weighted"], order),
                at_ms=_laid_out(b["at_ms"], order), ms=b["ms"])


@functools.lru_cache(maxsize=None)
def many_queries_two_blocks(times=257):
    """the four queries of search_cases.block_edges(8193) `times` over: nq = 1 028 queries x 2 reference blocks = 2 056 workgroups of
    the search, so the scan's threads take two counts each and pre[q * nblk] is read past entry 1 024"""
    c = sec.block_edges(REF_BLOCK + 1)
    refs, base = c["refs"], c["queries"]
    rv, ro = scm.csr(refs)
    from rkmh_amd import api
    order = np.arange(4 * times) % 4
    hits = api.search_scaled_host(rv, ro, *scm.csr(base))
    qv = np.concatenate([base[i] for i in order])
    return dict(rv=_ro(rv), ro=_ro(ro), nref=len(refs), qv=_ro(qv), qo=_offsets([len(base[i]) for i in order]), order=order,
                hits=_renumbered(hits, order, 4), plain=_laid_out(mc.answer(refs, base, host=True), order))


# ---- flood_of_queries: more queries than wave_grid gives waves to k_mg_pack ----
FLOOD_REFS = ((1, 2), (2, 3), (5,))
# kind of query -> its values, its hits (reference, shared), its gather rows (reference, unique, total, remaining)
FLOOD_KINDS = (
    ((), (), ()),
    ((1,), ((0, 1),), ((0, 1, 1, 0),)),
    ((2,), ((0, 1), (1, 1)), ((0, 1, 1, 0),)),                          # references 0 and 1 tie: the lower index; then nothing is left
    ((1, 3), ((0, 1), (1, 1)), ((0, 1, 1, 1), (1, 1, 1, 0))),
    ((7,), (), ()),                                                     # a value that no reference holds
    ((3, 5), ((1, 1), (2, 1)), ((1, 1, 1, 1), (2, 1, 1, 0))),
    ((2, 3), ((0, 1), (1, 2)), ((1, 2, 2, 0),)),
)


@functools.lru_cache(maxsize=None)
def flood_of_queries(cap):
    """nq = cap + 3 queries of 0, 1 or 2 values, query i of kind i % 7 (FLOOD_KINDS), against the three references of FLOOD_REFS ->
    dict(rv, ro, qv, qo, kind, hits, full, one): `full` the multigather answer at max_rounds None, `one` at max_rounds 1"""
    nq = cap + 3
    kind = np.arange(nq) % len(FLOOD_KINDS)
    tab = np.zeros((len(FLOOD_KINDS), 2), dtype=np.uint64)
    for k, (v, _, _) in enumerate(FLOOD_KINDS):
        tab[k, :len(v)] = v
    lens = np.asarray([len(v) for v, _, _ in FLOOD_KINDS])[kind]
    qv = tab[kind][np.arange(2)[None, :] < lens[:, None]]

    def laid(pick, width):
        """pick(kind) -> its tuples of `width` - 1 numbers, laid end to end over the queries -> (the tuples with the query in front, or
        as they are at width 4; their offsets)"""
        n = np.asarray([len(pick(k)) for k in range(len(FLOOD_KINDS))])[kind]
        most = max(len(pick(k)) for k in range(len(FLOOD_KINDS)))
        t = np.zeros((len(FLOOD_KINDS), most, width), dtype=np.int64)
        for k in range(len(FLOOD_KINDS)):
            for i, row in enumerate(pick(k)):
                t[k, i, width - len(row):] = row
        out = t[kind]
        if width == 3:
            out[:, :, 0] = np.arange(nq)[:, None]
        return out[np.arange(most)[None, :] < n[:, None]], _offsets(n)
    hits, _ = laid(lambda k: FLOOD_KINDS[k][1], 3)
    full, full_off = laid(lambda k: FLOOD_KINDS[k][2], 4)
    one, one_off = laid(lambda k: FLOOD_KINDS[k][2][:1], 4)
    rv, ro = scm.csr([np.asarray(r, dtype=np.uint64) for r in FLOOD_REFS])
    return dict(rv=_ro(rv), ro=_ro(ro), refs=tuple(scm.rows(rv, ro)), qv=_ro(qv), qo=_offsets(lens), kind=kind, hits=_hits(hits),
                full=(full.astype(np.int32), full_off, None), one=(one.astype(np.int32), one_off, None))


# ---- long_pick: a pick whose hit list is longer than one trip of the removal grid, and than 64 slices of multigather ----
@functools.lru_cache(maxsize=None)
def long_pick(cap):
    """Query: 3 i for i in 1 ... n = cap + 300, and the 500 values 3 j + 1.  Reference 0 holds the n; 1 holds the last 200 of them and
    50 foreign values (3 j + 2); 2 holds the first 100; 3 holds the 500.  Rows: (0, n, n, 500), (3, 500, 500, 0), and the run stops:
    reference 1 is never picked only because the tail of the first pick's list left the query.  abund: abund_cases.abundances, two
    of them 2^32 - 1 inside that tail; wunique = the abundances summed over the n, then over the 500."""
    n = cap + 300
    main = 3 * np.arange(1, n + 1, dtype=np.uint64)
    side = 3 * np.arange(1, 501, dtype=np.uint64) + np.uint64(1)
    foreign = 3 * np.arange(1, 51, dtype=np.uint64) + np.uint64(2)
    q = np.union1d(main, side)
    refs = (main, np.union1d(main[-200:], foreign), main[:100], side)
    abund = np.array(ac.abundances(np.random.default_rng(31), len(q)))
    abund[abund == am.SAT] = 7                                # the heavy ones stand where this case wants them
    abund[np.searchsorted(q, main[[n - 150, n - 1]])] = am.SAT
    in_main = np.isin(q, main)
    wunique = [int(abund[in_main].astype(np.uint64).sum()), int(abund[~in_main].astype(np.uint64).sum())]
    rv, ro = scm.csr(refs)
    rows = np.asarray([[0, n, n, 500], [3, 500, 500, 0]], dtype=np.int32)
    return dict(q=_ro(q), abund=_ro(abund, np.uint32), refs=tuple(_ro(r) for r in refs), rv=_ro(rv), ro=_ro(ro), rows=rows,
                wunique=np.asarray(wunique, dtype=np.uint64), n=n, tail=np.searchsorted(q, main[cap:]))


# ---- long_query: more query values than flat_grid gives threads to k_mg_keypos ----
def long_query(cap=FLAT_GRID):
    """(Not kept: 134 MB, and one test uses it.)  One query 1 ... cap + 1 000.  Reference 0 = its last 500 values (all at positions >= cap), 1 = its first 300, 2 = 100 of 1's
    and 100 of 0's.  Rows: (0, 500, 500, cap + 500), (1, 300, 300, cap + 200), and the run stops: reference 2 is left with 0."""
    n = cap + 1000
    q = np.arange(1, n + 1, dtype=np.uint64)
    refs = (q[-500:], q[:300], np.concatenate([q[100:200], q[-300:-200]]))
    rv, ro = scm.csr(refs)
    rows = np.asarray([[0, 500, 500, n - 500], [1, 300, 300, n - 800]], dtype=np.int32)
    return dict(q=_ro(q), qo=_offsets([n]), refs=tuple(_ro(r) for r in refs), rv=_ro(rv), ro=_ro(ro), hits=_hits([[0, 0, 500], [0, 1, 300], [0, 2, 200]]),
                mg=(rows, np.asarray([0, 2], dtype=np.uint64), None))


# ---- pair_matrix: an answer of more than one 64 MB row block ----
PAIR_N = {"plain": 4100, "weighted": 1500}                   # 16 810 000 pairs: 4 092 + 8 rows; 2 250 000 pairs: 1 398 + 102 rows


def rows_per_block(n, kind):
    return max(1, ROW_BLOCK_BYTES // (n * PAIR_BYTES[kind]))


def pair_matrix(n, kind):
    """row i = {i + 1, 10^6 + i % 7}: shared(i, j) = [i = j] + [i = j mod 7].  Abundances: side a gives the first value of row i
    i % 5 + 1 and the second i % 11 + 2, side b j % 3 + 1 and j % 13 + 5 -- the four fields of a pair are sums of at most two
    products, and a row block written at the wrong place shows in every one of them
    -> dict(v, off, wa, wb) and, kind "plain": shared int32 [n, n]; kind "weighted": weighted uint64 [n, n, 4], a against b, and
    weighted_self, a against itself.  (Not kept: an answer is 67 MB and more, and one test uses it.)"""
    i = np.arange(n, dtype=np.int64)
    v = np.stack([i + 1, 10 ** 6 + i % 7], axis=1).astype(np.uint64).reshape(-1)
    wa = np.stack([i % 5 + 1, i % 11 + 2], axis=1).astype(np.uint64)
    wb = np.stack([i % 3 + 1, i % 13 + 5], axis=1).astype(np.uint64)
    out = dict(v=_ro(v), off=_ro(2 * np.arange(n + 1)), wa=_ro(wa.reshape(-1), np.uint32), wb=_ro(wb.reshape(-1), np.uint32))
    same, mod7 = i[:, None] == i[None, :], i[:, None] % 7 == i[None, :] % 7
    if kind == "plain":
        out["shared"] = same.astype(np.int32) + mod7.astype(np.int32)
        return out
    same, mod7 = same.astype(np.uint64), mod7.astype(np.uint64)

    def fields(x, y):
        x0, x1, y0, y1 = x[:, 0, None], x[:, 1, None], y[None, :, 0], y[None, :, 1]
        return np.ascontiguousarray(np.stack([same + mod7, same * x0 * y0 + mod7 * x1 * y1, same * x0 + mod7 * x1, same * y0 + mod7 * y1], axis=2))
    out["weighted"], out["weighted_self"] = fields(wa, wb), fields(wa, wa)
    return out


# ---- kept_past_a_million: one chunk whose kept values fill more than 1 024 blocks of KEEP_FIRST ----
KEPT_LENGTHS = (200_000, 900_000, 150_000)
KEPT_K = 21
KEPT_RUN = 3000


@functools.lru_cache(maxsize=None)
def kept_past_a_million():
    """three random sequences at max_hash = FULL, k = 21: 1.25 M kept values in one chunk, the third sequence's from past entry 2^20
    on.  The second and the third sequence each hold a homopolymer of 3 000 bases: 2 980 equal values in a run (abundances) --
    wherever the hash of the second's falls among its sequence's 900 000, the third's run lies on the far side of block 1 024.
    -> dict(seqs, want: (values, abund) per sequence from abund_model.sketch, starts: where each sequence's kept values begin)"""
    rng = np.random.default_rng(41)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    seqs = []
    for i, n in enumerate(KEPT_LENGTHS):
        s = acgt[rng.integers(0, 4, size=n, dtype=np.uint8)].copy()
        if i == 1:
            s[400_000:400_000 + KEPT_RUN] = ord("A")
        if i == 2:
            s[70_000:70_000 + KEPT_RUN] = ord("C")
        seqs.append(s.tobytes())
    want = tuple(am.sketch(s, [KEPT_K], sm.DEFAULT, am.FULL) for s in seqs)
    starts = np.asarray([0] + [int(a.astype(np.int64).sum()) for _, a in want]).cumsum()   # every kept window is an entry until KEEP_FIRST has run
    return dict(seqs=tuple(seqs), want=want, starts=starts)
