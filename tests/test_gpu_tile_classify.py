"""Classification through the hash-space kernel (k_classify_tile, rk_classify.hip) against the oracle at every k from 1 to 64: rows
compared bit for bit as int32[n][4], reference sketches first.  The inputs and what makes them worth running are in
tests/tile_cases.py (checked without a GPU by tests/test_tile_cases_cpu.py).

Every batch is classified twice: through rk_classify_batch (host arrays; rows the kernel hands back are answered by the general path)
and through rk_classify_batch_device (resident arrays; such rows stay flagged -2).  All rows of the first must equal the oracle's; in
the second every row that is not flagged must, and a row may be flagged only where the kernel's documented per-read limits say so
(tile_cases.may_hand_back) -- so it is the fused kernel, not the general path behind it, whose rows are pinned."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tile_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu


class _Refs:
    """a context of its own for one policy and one list of k, the k-mer-space form forbidden, reference sketches checked"""

    def __init__(self, orc, refs, ks, pol=tc.DEFAULT):
        import rkmh_amd
        self.orc, self.refs, self.ks, self.pol = orc, refs, list(ks), pol
        self.sk = tc.want_sketches(orc, refs, self.ks, pol)
        self.c = rkmh_amd.Context(0, policy_spec=pol.spec())
        try:
            self.c.set_kmer_form(False)
            rb, ro = tc.pack(list(refs))
            self.c.set_references(rb, ro, self.ks, tc.S)
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

    def device_rows(self, qb, qo):
        import torch
        n = len(qo) - 1
        d_b = torch.from_numpy(qb).cuda()
        d_o = torch.from_numpy(qo.astype(np.int64)).to(torch.int32).cuda()
        d_out = torch.full((max(n, 1), 4), -7, dtype=torch.int32, device="cuda")
        self.c.classify_device(d_b.data_ptr(), d_o.data_ptr(), n, d_out.data_ptr(), max_read_len=0,
                               stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return d_out.cpu().numpy()[:n]

    def check(self, reads, what, min_occ=None, allow_long=()):
        """one batch; returns (rows of the host entry point, number of rows the kernel handed back)"""
        reads = list(reads)
        tc.assert_routed(self.refs, reads, self.ks, self.pol, allow_long)
        want = tc.want_rows(self.orc, self.refs, reads, self.ks, self.pol, sketches=self.sk, min_occ=min_occ)
        qb, qo = tc.pack(reads)
        got = self.c.classify(qb, qo)
        raw = self.device_rows(qb, qo)
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
            h = tc.window_hashes(self.orc, reads[i], self.ks, self.pol)
            assert tc.may_hand_back(self.sk, h, len(reads[i]), sparse), "handed back without cause, " + report(raw, i)
        return got, int(flagged.sum())


# ---- the default policy at every k: ragged reads, and uniform tiles on both sides of the split last step --------------------------
@pytest.mark.parametrize("k,start", [(k, 0) for k in tc.ALL_K] + [(k, j) for k in tc.FULL_L_K for j in range(1, 8)])
def test_default_policy_every_k(orc, k, start):
    with _Refs(orc, tc.base_panel(), [k]) as R:
        if start == 0:
            _, back = R.check(tc.ragged(k).reads, "ragged")
            if k >= 3:
                assert back <= 2, (k, back)       # at most the two long tandem copies: the kernel answered the rest
        for L in tc.uniform_lengths(k, 8, start):
            _, back = R.check(tc.uniform(k, L), "uniform(%d)" % L)
            assert back == 0 or k < 3, (k, L, back)


# ---- the policy cross at the block-structure edges -------------------------------------------------------------------------------
@pytest.mark.parametrize("k", tc.CROSS_K)
@pytest.mark.parametrize("pol", tc.CROSS, ids=str)
def test_policy_cross(orc, pol, k):
    with _Refs(orc, tc.base_panel(), [k], pol) as R:
        R.check(tc.ragged(k).reads, "ragged")


# ---- compile-time k (KT = 12, 16, 20, 21, 31) and the same sizes through the run-time form ----------------------------------------
@pytest.mark.parametrize("ks", [[k] for k in tc.SINGLE_K] + list(tc.K_LISTS), ids=str)
def test_compile_time_and_run_time_k(orc, ks):
    with _Refs(orc, tc.base_panel(), ks) as R:
        for k in ks:
            R.check(tc.ragged(k).reads, "ragged(%d)" % k)
            R.check(tc.uniform(k, k + 9), "uniform(%d)" % (k + 9))
            R.check(tc.uniform(k, k + 40), "uniform(%d)" % (k + 40))


# ---- 8-bit | 16-bit count fields ------------------------------------------------------------------------------------------------
def test_counter_width(orc):
    refs, _ = tc.counter_width()
    with _Refs(orc, refs, [24]) as R:
        for batch, windows in tc.counter_width_batches():
            got, back = R.check(batch, "counter_width %s" % windows)
            assert got[:, 1].tolist() == windows and back == 0     # max_shared is the window count, counted by the kernel itself


# ---- PF = 2 | 3 | 6 at their edges, and the first length the kernel hands back -----------------------------------------------------
@pytest.mark.parametrize("k", [64, 24])
def test_prefetch_edges(orc, k):
    with _Refs(orc, tc.base_panel(), [k]) as R:
        for L in tc.PREFETCH_L:
            reads, at = tc.prefetch_edges(L, k)
            _, back = R.check(reads, "prefetch_edges(%d)" % L, allow_long=(at,) if L > tc.FUSED_MAXLEN else ())
            assert back == (1 if L > tc.FUSED_MAXLEN else 0), (k, L, back)


# ---- dense | sparse counter rows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nref", tc.PANEL_NREF)
def test_panel_edges(orc, nref):
    pe = tc.panel_edges(nref)
    for k in (24, 48):
        with _Refs(orc, pe.refs, [k]) as R:
            for name, batch in (("short", pe.short), ("long", pe.long + pe.short)):
                _, back = R.check(batch, "panel_edges(%d) %s" % (nref, name))
                assert 2 * back <= len(batch), (nref, k, name, back)


# ---- the other modes of the kernel ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", tc.MODE_K)
def test_count_pass(orc, k):
    """MODE 1: every window of the batch, invalid ones in slot 0 (zero=count), into a full table and into a compact depth map"""
    import torch
    from rkmh_amd import api
    reads = list(tc.ragged(k).reads)
    h = np.concatenate([tc.window_hashes(orc, r, [k], tc.DEFAULT) for r in reads])
    want = np.bincount((h % np.uint64(tc.COUNT_SLOTS)).astype(np.int64), minlength=tc.COUNT_SLOTS)
    assert want[0] >= int((h == 0).sum()) > 0
    qb, qo = tc.pack(reads)
    with _Refs(orc, tc.base_panel(), [k]) as R:
        table = torch.zeros(tc.COUNT_SLOTS + 4, dtype=torch.int32, device="cuda")
        full = api.Counter(R.c, tc.COUNT_SLOTS, device_ptr=table.data_ptr())
        R.c.count_batch(qb, qo, full)
        R.c.synchronize()
        torch.cuda.synchronize()
        got = table.cpu().numpy()
        bad = np.nonzero(got[: tc.COUNT_SLOTS] != want)[0]
        assert len(bad) == 0 and (got[tc.COUNT_SLOTS:] == 0).all(), (k, bad[:5], got[bad[:5]], want[bad[:5]])
        R.c.set_min_num_bound(0)
        comp = api.Counter(R.c, tc.COUNT_SLOTS, compact=True)
        assert comp.compact and comp.entries > 0
        R.c.count_batch(qb, qo, comp)
        keys = np.unique(np.concatenate(R.sk))
        for key in keys[:: max(len(keys) // 300, 1)].tolist():       # a compact map answers for the slots of index keys
            assert comp.get(key) == want[key % tc.COUNT_SLOTS], (k, key)
        comp.destroy()
        full.destroy()


@pytest.mark.parametrize("k", tc.MODE_K)
def test_exact_depth_mask(orc, k):
    """MODE 2: set_depth_filter(cnt, 2) with the default unbounded min_num against the oracle's -M loop"""
    from rkmh_amd import api
    reads = list(tc.ragged(k).reads)
    qb, qo = tc.pack(reads)
    with _Refs(orc, tc.base_panel(), [k]) as R:
        cnt = api.Counter(R.c, tc.COUNT_SLOTS)
        R.c.count_batch(qb, qo, cnt)
        R.c.set_depth_filter(cnt, 2)
        want = tc.want_rows(orc, R.refs, reads, [k], tc.DEFAULT, sketches=R.sk, min_occ=2)
        got = R.c.classify(qb, qo)
        R.c.set_depth_filter(None, 0)
        cnt.destroy()
    assert got.shape == want.shape
    for i in np.nonzero((got != want).any(axis=1))[0][:3].tolist():
        raise AssertionError("-M 2: k=%d read %d of %d bases: got %s, want %s" % (k, i, len(reads[i]), got[i].tolist(), want[i].tolist()))


@pytest.mark.parametrize("k", tc.MODE_K)
def test_first_level_filter_on_and_off(orc, k, monkeypatch):
    """MODE 3 (the default: RKMH_PREFILTER unset) and MODE 0 (RKMH_PREFILTER=0, read at each set_references): the same rows"""
    rows = []
    for env in (None, "0"):
        if env is None:
            monkeypatch.delenv("RKMH_PREFILTER", raising=False)
        else:
            monkeypatch.setenv("RKMH_PREFILTER", env)
        with _Refs(orc, tc.base_panel(), [k]) as R:
            rows.append(R.check(tc.ragged(k).reads, "RKMH_PREFILTER=%s" % env)[0])
    assert (rows[0] == rows[1]).all()


# ---- both command lines -------------------------------------------------------------------------------------------------------
def test_stream_commands_at_k64(orc, root, tmp_path):
    """bin/rkmh stream -k 64 -s 2000 and python -m rkmh_amd.cli on the ragged reads (those with at least one base: a FASTA record
    needs a sequence line) and the base panel"""
    refs = tc.base_panel()
    reads = [r for r in tc.ragged(64).reads if len(r) > 0]
    fa, fq = tmp_path / "panel.fa", tmp_path / "reads.fa"
    fa.write_bytes(b"".join(b">ref%d\n%s\n" % (j, r) for j, r in enumerate(refs)))
    fq.write_bytes(b"".join(b">read%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    rows = tc.want_rows(orc, refs, reads, [64], tc.DEFAULT)
    want = "".join(orc.stream_line("ref%d" % mi, "read%d" % i, ms, d, n, tc.S) for i, (mi, ms, d, n) in enumerate(rows.tolist()))
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    for cmd in ([os.path.join(root, "bin", "rkmh"), "stream"], [sys.executable, "-m", "rkmh_amd.cli", "stream"]):
        r = subprocess.run(cmd + ["-r", str(fa), "-f", str(fq), "-k", "64", "-s", str(tc.S)], capture_output=True, env=env, cwd=root)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        got = r.stdout.decode()
        assert got.count("\n") == len(reads)
        for i, (g, w) in enumerate(zip(got.splitlines(), want.splitlines())):
            assert g == w, (cmd[-2:], i, len(reads[i]))
