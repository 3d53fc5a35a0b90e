"""The DEDUP forms of the hash-space kernel (dedup=distinct: k_classify_tile<0, MODE, -1, PF, CANON, true>, rk_classify.hip) against
the sketch rule of tests/dedup_model.py on the oracle's hashes (canon=minhash) and the numpy model's (canon=lexmin): rows compared bit
for bit as int32[n][4], reference sketches first.  The inputs and what makes them worth running are in tests/tile_cases.py (checked
without a GPU by tests/test_tile_cases_cpu.py).

As in tests/test_gpu_tile_classify.py every batch is classified twice: through rk_classify_batch (all rows must equal the model's) and
through rk_classify_batch_device with max_read_len = 0 (rows the kernel hands back stay flagged -2: every other row must equal the
model's, and a flag is accepted only where tile_cases.may_hand_back_distinct allows it) -- so the kernel's own rows are pinned, its
per-read set of distinct hashes with them: one set per read of a tile, cleared between tiles, sized from the windows of all k."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tile_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu

BOTH = pytest.mark.parametrize("pol", tc.DEDUP, ids=str)


def _device_rows(c, qb, qo):
    import torch
    n = len(qo) - 1
    d_b = torch.from_numpy(qb).cuda()
    d_o = torch.from_numpy(qo.astype(np.int64)).to(torch.int32).cuda()
    d_out = torch.full((max(n, 1), 4), -7, dtype=torch.int32, device="cuda")
    c.classify_device(d_b.data_ptr(), d_o.data_ptr(), n, d_out.data_ptr(), max_read_len=0, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()[:n]


class _Refs:
    """a context of its own for one policy, one list of k and one sketch size, reference sketches checked"""

    def __init__(self, orc, refs, ks, pol, sketch_size=tc.S):
        import rkmh_amd
        self.orc, self.refs, self.ks, self.pol, self.S = orc, refs, list(ks), pol, sketch_size
        self.sk = tc.want_sketches(orc, refs, self.ks, pol, sketch_size)
        self.c = rkmh_amd.Context(0, policy_spec=pol.spec())
        try:
            self.c.set_kmer_form(False)
            rb, ro = tc.pack(list(refs))
            self.c.set_references(rb, ro, self.ks, sketch_size)
            assert self.c.kmer_form()[0] is False
            sk, ln = self.c.get_reference_sketches()
            assert ln.tolist() == [len(x) for x in self.sk], (self.ks, str(pol))
            for j, x in enumerate(self.sk):
                assert (sk[j, : len(x)] == x).all(), ("reference sketch", self.ks, str(pol), j)
        except BaseException:
            self.c.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.c.close()

    def check(self, reads, what, min_occ=None, bound=None, allow_long=()):
        """one batch through both entry points; returns (rows of the host entry point, rows of the resident one)"""
        reads = list(reads)
        assert 0 < len(self.refs) <= tc.MAX_REFS
        assert all(len(r) <= tc.FUSED_MAXLEN or i in allow_long for i, r in enumerate(reads))
        hs = tc.masked_hashes(self.orc, reads, self.ks, self.pol, min_occ)
        if self.pol.dedup:
            want = tc.rows_distinct(self.sk, hs, self.S, bound)
        else:
            want = tc.want_rows(self.orc, self.refs, reads, self.ks, self.pol, sketches=self.sk, min_occ=min_occ)
        qb, qo = tc.pack(reads)
        got = self.c.classify(qb, qo)
        raw = _device_rows(self.c, qb, qo)
        self.compare(reads, what, hs, want, got, raw)
        return got, raw

    def compare(self, reads, what, hs, want, got, raw):
        assert got.shape == want.shape == raw.shape == (len(reads), 4)

        def report(rows, i):
            return "%s: k=%s policy=%s read %d of %d bases: got %s, want %s" % (what, self.ks, self.pol, i, len(reads[i]), rows[i].tolist(), want[i].tolist())
        flagged = raw[:, 0] == -2
        for i in np.nonzero((got != want).any(axis=1))[0][:3].tolist():
            raise AssertionError(report(got, i))
        for i in np.nonzero((raw != want).any(axis=1) & ~flagged)[0][:3].tolist():
            raise AssertionError("resident input, " + report(raw, i))
        mw = max([sum(tc.nwin(min(len(r), tc.FUSED_MAXLEN), k, self.pol) for k in self.ks) for r in reads] + [0])
        sparse = tc.sparse_rows(len(self.refs), mw)
        for i in np.nonzero(flagged)[0].tolist():
            if self.pol.dedup:
                cause = tc.may_hand_back_distinct(self.sk, hs[i], len(reads[i]), sparse, self.S)
            else:
                cause = tc.may_hand_back(self.sk, hs[i], len(reads[i]), sparse)
            assert cause, "handed back without cause, " + report(raw, i)


def _back(raw):
    return int((raw[:, 0] == -2).sum())


# ---- 1. every k: ragged reads, and uniform tiles on both sides of the split last step (which only the minhash form has) -------------
@BOTH
@pytest.mark.parametrize("k,start", [(k, 0) for k in tc.ALL_K] + [(k, j) for k in tc.FULL_L_K for j in range(1, 8)])
def test_every_k(orc, pol, k, start):
    with _Refs(orc, tc.base_panel(), [k], pol) as R:
        if start == 0:
            _, raw = R.check(tc.ragged(k).reads, "ragged")
            assert _back(raw) == 0, (k, _back(raw))     # no limit on how often a value occurs under the key: k = 1 and 2 are the kernel's too
        for L in tc.uniform_lengths(k, 8, start):
            _, raw = R.check(tc.uniform(k, L), "uniform(%d)" % L)
            assert _back(raw) == 0, (k, L, _back(raw))


# ---- 2. the policy cross at the block-structure edges ----------------------------------------------------------------------------
@pytest.mark.parametrize("k", tc.DEDUP_CROSS_K)
@pytest.mark.parametrize("pol", tc.DEDUP_CROSS, ids=str)
def test_policy_cross(orc, pol, k):
    with _Refs(orc, tc.base_panel(), [k], pol) as R:
        _, raw = R.check(tc.ragged(k).reads, "ragged")
        assert _back(raw) == 0


# ---- 3. the seven set sizes and their boundaries; one set per read of a tile; sets cleared between tiles ------------------------------
@BOTH
@pytest.mark.parametrize("W", tc.LADDER_W)
def test_set_ladder(orc, pol, W):
    lad = tc.set_ladder(W)
    with _Refs(orc, tc.base_panel(), [tc.LADDER_K], pol) as R:
        got, raw = R.check(lad.reads, "set_ladder(%d)" % W)
    assert _back(raw) == 0, (W, raw[:, 0].tolist())
    assert [int(raw[i, 3]) for i in lad.random] == [W] * 3 and raw[lad.periodic, 3] == 11


@BOTH
def test_sets_are_cleared_between_tiles(orc, pol):
    reads = tc.stale_set()
    with _Refs(orc, tc.base_panel(), [tc.LADDER_K], pol) as R:
        got, raw = R.check(reads, "stale_set")
    assert _back(raw) == 0 and (raw == raw[0]).all() and (got == got[0]).all() and raw[0, 3] == 126


# ---- 4. windows of several k in one set, and the 2048-window limit that only a list of k reaches ------------------------------------
@BOTH
@pytest.mark.parametrize("ks", tc.K_LISTS, ids=str)
def test_several_k_in_one_set(orc, pol, ks):
    with _Refs(orc, tc.base_panel(), ks, pol) as R:
        for k in ks:
            for what, reads in (("ragged(%d)" % k, tc.ragged(k).reads), ("uniform(%d)" % (k + 40), tc.uniform(k, k + 40))):
                _, raw = R.check(reads, what)
                assert _back(raw) == 0, (ks, what)


@BOTH
def test_window_limit(orc, pol):
    at_limit, beyond, at = tc.several_k_limit()
    with _Refs(orc, tc.base_panel(), tc.LIMIT_KS, pol) as R:
        _, raw = R.check(at_limit, "2048 windows")
        assert _back(raw) == 0 and raw[at, 1] >= 300, raw[at].tolist()       # the kernel's own answer
        _, raw = R.check(beyond, "2050 windows")                             # (may be handed back: the host entry's row is right all the same)
        assert _back(raw) <= 1 and (raw[np.arange(len(beyond)) != at, 0] != -2).all()


# ---- 5. PF = 2 | 3 | 6 at their byte edges ------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("k", [64, 24])
def test_prefetch_edges(orc, pol, k):
    with _Refs(orc, tc.base_panel(), [k], pol) as R:
        for L in tc.PREFETCH_L:
            reads, at = tc.prefetch_edges(L, k)
            _, raw = R.check(reads, "prefetch_edges(%d)" % L, allow_long=(at,) if L > tc.FUSED_MAXLEN else ())
            assert _back(raw) == (1 if L > tc.FUSED_MAXLEN else 0), (k, L, _back(raw))


# ---- 6. a read with exactly S distinct hashes -----------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("k", tc.EXACT_K)
def test_exactly_s_distinct(orc, pol, k):
    reads = tc.exactly_s(orc, k, pol)
    with _Refs(orc, tc.base_panel(), [k], pol, sketch_size=tc.EXACT_S) as R:
        got, raw = R.check(reads, "exactly_s")
    for i, p in enumerate(tc.EXACT_P):
        assert got[i, 3] == min(p, tc.EXACT_S)
        if p <= tc.EXACT_S:
            assert raw[i].tolist() == got[i].tolist(), (k, p, raw[i].tolist())     # more windows than S, no more distinct hashes: the kernel's
    assert (raw[len(tc.EXACT_P):, 0] != -2).all()


# ---- 7. the other classify modes ------------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("k", tc.MODE_K)
def test_first_level_filter_on_and_off(orc, pol, k, monkeypatch):
    """MODE 3 (the default: RKMH_PREFILTER unset) and MODE 0 (RKMH_PREFILTER=0, read at each set_references): the model's rows"""
    rows = []
    for env in (None, "0"):
        if env is None:
            monkeypatch.delenv("RKMH_PREFILTER", raising=False)
        else:
            monkeypatch.setenv("RKMH_PREFILTER", env)
        with _Refs(orc, tc.base_panel(), [k], pol) as R:
            rows.append(R.check(tc.ragged(k).reads, "RKMH_PREFILTER=%s" % env))
    assert (rows[0][0] == rows[1][0]).all() and (rows[0][1] == rows[1][1]).all()


def _masked(R, reads, k, bounds):
    """-M 2 counted over these very reads; one check per bound (None: the default, exact field 3)"""
    from rkmh_amd import api
    qb, qo = tc.pack(list(reads))
    out = []
    cnt = api.Counter(R.c, tc.COUNT_SLOTS)
    try:
        R.c.count_batch(qb, qo, cnt)
        R.c.set_depth_filter(cnt, 2)
        for bound in bounds:
            if bound is not None:
                R.c.set_min_num_bound(bound)
            out.append(R.check(reads, "-M 2, bound %s" % bound, min_occ=2, bound=bound))
    finally:
        R.c.set_depth_filter(None, 0)
        cnt.destroy()
    return out


@BOTH
@pytest.mark.parametrize("k", tc.MODE_K)
def test_depth_mask(orc, pol, k):
    """MODE 2: the exact per-window mask with the default bound and with bound 3, the per-key mask with bound 0"""
    with _Refs(orc, tc.base_panel(), [k], pol) as R:
        exact, three, zero = _masked(R, tc.ragged(k).reads, k, (None, 3, 0))
    assert (exact[0][:, :3] == three[0][:, :3]).all() and (exact[0][:, :3] == zero[0][:, :3]).all() and (zero[0][:, 3] == 0).all()


# ---- 8. MODE 4: RKMH_PRE_MASKED is read at the process's first tile launch, so the form needs a process of its own --------------------
MODE4_K = 24
MODE4_POLICIES = (tc.DEFAULT,) + tc.DEDUP


def masked_rows_of_this_process(orc=None):
    """{policy text: [host rows, resident rows]} of the exact -M 2 batch at k = 24; with an oracle, checked against the models as well"""
    import rkmh_amd
    from rkmh_amd import api
    out = {}
    reads = list(tc.ragged(MODE4_K).reads)
    qb, qo = tc.pack(reads)
    for pol in MODE4_POLICIES:
        if orc is not None:
            with _Refs(orc, tc.base_panel(), [MODE4_K], pol) as R:
                (got, raw), = _masked(R, reads, MODE4_K, (None,))
        else:
            c = rkmh_amd.Context(0, policy_spec=pol.spec())
            try:
                c.set_kmer_form(False)
                rb, ro = tc.pack(list(tc.base_panel()))
                c.set_references(rb, ro, [MODE4_K], tc.S)
                cnt = api.Counter(c, tc.COUNT_SLOTS)
                c.count_batch(qb, qo, cnt)
                c.set_depth_filter(cnt, 2)
                got, raw = c.classify(qb, qo), _device_rows(c, qb, qo)
                c.set_depth_filter(None, 0)
                cnt.destroy()
            finally:
                c.close()
        out[str(pol)] = [got.tolist(), raw.tolist()]
    return out


def test_mode4_in_a_child_process(orc, root):
    """The -M classify kernel behind the first-level filter (MODE 4) for the multiset form and both DEDUP forms: one fresh child
    process started with RKMH_PRE_MASKED=1 classifies the exact -M 2 batch at k = 24 and prints its rows; they must equal the models'
    and the rows of this process (MODE 2 on this small index, unless the variable was set when this process launched its first tile)."""
    mine = masked_rows_of_this_process(orc)            # compared with the models inside
    code = ("import json, sys; sys.path[:0] = [sys.argv[1], sys.argv[2]]; import test_gpu_tile_dedup as t; "
            "print('ROWS ' + json.dumps(t.masked_rows_of_this_process()))")
    env = dict(os.environ, RKMH_PRE_MASKED="1")
    env.pop("RKMH_PREFILTER", None)
    r = subprocess.run([sys.executable, "-c", code, root, HERE], capture_output=True, cwd=root, env=env, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [x for x in r.stdout.decode().splitlines() if x.startswith("ROWS ")]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    theirs = json.loads(lines[0][5:])
    reads = list(tc.ragged(MODE4_K).reads)
    refs = tc.base_panel()
    for pol in MODE4_POLICIES:
        got, raw = (np.array(x, dtype=np.int32) for x in theirs[str(pol)])
        sk = tc.want_sketches(orc, refs, [MODE4_K], pol)
        hs = tc.masked_hashes(orc, reads, [MODE4_K], pol, 2)
        want = tc.want_rows(orc, refs, reads, [MODE4_K], pol, sketches=sk, min_occ=2)
        R = _Refs.__new__(_Refs)
        R.orc, R.refs, R.ks, R.pol, R.S, R.sk = orc, refs, [MODE4_K], pol, tc.S, sk
        R.compare(reads, "RKMH_PRE_MASKED=1", hs, want, got, raw)
        assert (got == np.array(mine[str(pol)][0])).all() and (raw == np.array(mine[str(pol)][1])).all(), str(pol)
