"""Gather on the GPU: the kernels of rk_gather.hip through both entry points (rk_gather_scaled, rk_gather_scaled_device) and `rkmh
gather`, against tests/gather_model.py row for row and byte for byte.  What the shared inputs exercise is shown on the model's output
by tests/test_gather_cpu.py."""
import os
import subprocess

import numpy as np
import pytest

import dedup_model as dm
import gather_cases as gc
import gather_model as gm
import scaled_cases as sc
import scaled_model as scm
import sourmash_model as sm

pytestmark = pytest.mark.gpu

GUARD = 64


def _device(ctx, q, rv, ro, min_shared=1, max_rounds=None, r_nvalues=None):
    """the resident-input entry on torch's arrays and stream, guard words on both sides of the rows"""
    import torch
    nref = len(ro) - 1
    rows = nref if max_rounds is None else max_rounds

    def up(x):
        x = np.array(x, dtype=np.uint64)                     # (a writable copy: the shared inputs are read-only)
        return torch.from_numpy((x if len(x) else np.zeros(1, dtype=np.uint64)).view(np.int64)).cuda()
    d_q, d_rv, d_ro = up(q), up(rv), up(ro)
    d_out = torch.full((GUARD + rows * 4 + GUARD,), -7, dtype=torch.int32, device="cuda")
    n = ctx.gather_scaled_device(d_q.data_ptr(), len(q), d_rv.data_ptr(), d_ro.data_ptr(), nref, len(rv) if r_nvalues is None else r_nvalues,
                                 d_out.data_ptr() + 4 * GUARD, min_shared=min_shared, max_rounds=max_rounds,
                                 stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert 0 <= n <= rows
    assert (out[:GUARD] == -7).all() and (out[GUARD + 4 * n:] == -7).all(), "written outside the rows"
    return out[GUARD:GUARD + 4 * n].reshape(n, 4)


def _same(got, want, what):
    assert got.dtype == np.int32 and got.shape == want.shape and (got == want).all(), (what, got.tolist()[:4], want.tolist()[:4])


def _both_entries(ctx, q, refs, want, what, min_shared=1, max_rounds=None):
    rv, ro = scm.csr(refs)
    _same(ctx.gather_scaled(q, rv, ro, min_shared=min_shared, max_rounds=max_rounds), want, (what, "host entry"))
    _same(_device(ctx, q, rv, ro, min_shared, max_rounds), want, (what, "device entry"))


def test_hand_checked_vectors_both_entries(ctx):
    for v in gc.kat():
        _both_entries(ctx, v["q"], v["refs"], v["want"], v["name"], v["min_shared"], v["max_rounds"])


@pytest.mark.parametrize("nref", gc.NREFS)
def test_random_sets(ctx, nref):
    q, refs, want = gc.random_case(nref)
    assert len(want) >= min(3, nref)                        # not vacuous (one reference gives one row at most)
    _both_entries(ctx, q, refs, want, nref)
    cut = int(want[len(want) // 2, 1]) + 1                    # a min_shared that stops the run half way, and leaves candidates out
    w = gm.gather(q, refs, cut, 10 ** 6)
    assert len(w) < max(len(want), 2)
    _both_entries(ctx, q, refs, w, (nref, "min_shared", cut), min_shared=cut, max_rounds=10 ** 6 if nref > 1 else None)


def test_round_group_boundaries(ctx):
    from rkmh_amd import api
    B = api.RK_GATHER_BATCH
    for n in (0, 1, B - 1, B, B + 1, 2 * B + 1):
        q, refs = gc.staircase(n)
        want = gm.gather(q, refs)
        assert len(want) == n
        _both_entries(ctx, q, refs, want, ("staircase", n))
    q, refs = gc.staircase(2 * B + 1)
    for max_rounds in (1, B, B + 1):
        want = gm.gather(q, refs, 1, max_rounds)
        assert len(want) == max_rounds
        _both_entries(ctx, q, refs, want, ("staircase cut", max_rounds), max_rounds=max_rounds)


@pytest.fixture(scope="module")
def large():
    rng = np.random.default_rng(6)
    pl = sc.pool(rng, 300000)
    refs = sc.random_sets(rng, 9, pl, first=sc.LONG_ROW)      # one row of 70 000 values
    refs[1] = np.sort(rng.choice(pl, size=30000, replace=False))
    q = gc.query_of(rng, refs[:3], pl, size=200000)            # and a query of 200 000
    want = gm.gather(q, refs)
    assert len(q) == 200000 and len(want) >= 3 and want[0].tolist()[:3] == [0, sc.LONG_ROW, sc.LONG_ROW]
    return q, refs, want


def test_a_long_row_and_a_large_query(ctx, large):
    q, refs, want = large
    _both_entries(ctx, q, refs, want, "large")


def test_reuse_of_a_context(ctx, large):
    q, refs, want = large
    rv, ro = scm.csr(refs)
    small = [v for v in gc.kat() if v["name"] == "chain of three"][0]
    sv, so = scm.csr(small["refs"])
    for entry in ("host", "device"):
        def run(q_, v_, o_):
            return ctx.gather_scaled(q_, v_, o_) if entry == "host" else _device(ctx, q_, v_, o_)
        first = run(q, rv, ro)
        _same(first, want, (entry, "large"))
        _same(run(small["q"], sv, so), small["want"], (entry, "small after large"))   # no stale alive bytes or hit lists
        _same(run(q, rv, ro), first, (entry, "the same call again"))
        _same(run(small["q"], sv, so), small["want"], (entry, "small again"))


def test_rows_are_clamped_on_the_device(ctx):
    rng = np.random.default_rng(8)
    pl = sc.pool(rng, 3000)
    A = sc.random_sets(rng, 4, pl, lengths=[65, 129, 1000])
    q = gc.query_of(rng, A, pl)
    rv, ro = scm.csr(A)
    # fewer values behind the pointer than the offsets say: row 2 is cut short, row 3 lies outside altogether
    n = int(ro[2]) + 10
    want = gm.gather(q, [A[0], A[1], A[2][:10], A[3][:0]])
    assert len(want) == 3 and want[-1].tolist()[:2] == [2, len(np.setdiff1d(A[2][:10], np.concatenate([A[0], A[1]])))]
    _same(_device(ctx, q, rv, ro, r_nvalues=n), want, "fewer values")
    down = np.array([ro[1], ro[0], ro[1], ro[2]], dtype=np.uint64)           # offsets that decrease: an empty row
    _same(_device(ctx, q, rv, down), gm.gather(q, [A[0][:0], A[0], A[1]]), "decreasing offsets")
    with pytest.raises(ValueError):
        ctx.gather_scaled(q, rv[:n], ro)                                     # offsets past the values: refused by the binding


def test_host_entry_refusals(ctx):
    from rkmh_amd import api
    v = [x for x in gc.kat() if x["name"] == "chain of three"][0]
    rv, ro = scm.csr(v["refs"])
    q = v["q"]
    for bad in (dict(q=q[::-1].copy()), dict(q=np.array([1, 1, 2], dtype=np.uint64)), dict(ro=np.array([0, 6, 3, 14], dtype=np.uint64)),
                dict(min_shared=0), dict(max_rounds=0), dict(max_rounds=-1)):
        a = dict(q=q, ro=ro, min_shared=1, max_rounds=None)
        a.update(bad)
        with pytest.raises(api.RkmhError) as e:
            ctx.gather_scaled(a["q"], rv, a["ro"], min_shared=a["min_shared"], max_rounds=a["max_rounds"])
        assert e.value.code == -1, bad
    lib, h = ctx._lib, ctx._h
    n = api.C.c_int(0)
    for nq, nref, ms, mr, code in ((1, 0, 1, 1, -1), (1, 1, 0, 1, -1), (1, 1, 1, 0, -1), (1 << 31, 1, 1, 1, -5)):
        assert lib.rk_gather_scaled_device(h, 8, nq, 8, 8, nref, 1, ms, mr, 8, api.C.byref(n), None) == code   # before anything is read
    assert lib.rk_gather_scaled_device(h, 8, 1, 8, None, 1, 1, 1, 1, 8, api.C.byref(n), None) == -1
    _same(ctx.gather_scaled(q, rv, ro), v["want"], "and the context still works")


# ---- the command ----
def _run(root, *args):
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    r = subprocess.run([os.path.join(root, "bin", "rkmh")] + list(args), capture_output=True, env=env)
    assert r.returncode == 0, (args, r.stderr[-400:])
    return r.stdout.decode()


def _write_fasta(path, names, seqs):
    path.write_bytes(b"".join(b">" + n + b"\n" + s + b"\n" for n, s in zip(names, seqs)))
    return str(path)


RECORDS = (2, 7, 11, 20)


def _zika_sample(p):
    """records 2, 7, 11 and the first half of record 20"""
    return [p["seqs"][i] for i in RECORDS[:3]] + [p["seqs"][20][:len(p["seqs"][20]) // 2]]


@pytest.mark.parametrize("scaled,picks", [(10, 4), (100, 3)])
def test_cli_fasta_queries(root, tmp_path, data_dir, scaled, picks):
    p = sc.panel("zika-k16")
    names = [n.decode() for n in p["names"]]
    refs = sc.sketches("zika-k16", scaled)
    sample = _zika_sample(p)
    qsk = scm.merge([scm.sketch(s, [16], sm.DEFAULT, scm.max_hash(scaled)) for s in sample])
    rows = gm.gather(qsk, refs)
    assert len(rows) == picks and int(rows[0, 0]) == 2 and int(rows[-1, 1]) < 10 <= int(rows[-2, 1])
    if scaled == 10:                                                      # a pick that is none of the records the sample was made of: record 35
        assert int(rows[1, 0]) not in RECORDS and 11 not in rows[:, 0]   # explains more of what record 2 left than record 11 does
    rf = os.path.join(data_dir, "zika.refs.fa.gz")
    qf = _write_fasta(tmp_path / "sample.fa", [b"a", b"b", b"c", b"d"], sample)
    opts = ["--scaled", str(scaled), "-k", "16"]
    want = gm.gather_text([qf], [qsk], names, refs)
    direct = _run(root, "gather", "-r", rf, "-f", qf, *opts)
    assert direct == want and len(want.split("\n")) == picks + 1
    # the query through -Q after `rkmh sketch -g --scaled`, the references through -R
    qj, rj = str(tmp_path / "q.json"), str(tmp_path / "r.json")
    _run(root, "sketch", "-g", "-f", qf, "-o", qj, *opts)
    _run(root, "sketch", "-f", rf, "-o", rj, *opts)
    assert _run(root, "gather", "-r", rf, "-Q", qj, *opts) == want
    assert _run(root, "gather", "-R", rj, "-Q", qj) == want              # scaled and k come from the files
    assert _run(root, "gather", "-R", rj, "-f", qf) == want
    if scaled == 100:                                                     # files made at scaled 10 and gathered at 100: the bytes of the direct run
        qj10, rj10 = str(tmp_path / "q10.json"), str(tmp_path / "r10.json")
        _run(root, "sketch", "-g", "-f", qf, "-o", qj10, "--scaled", "10", "-k", "16")
        _run(root, "sketch", "-f", rf, "-o", rj10, "--scaled", "10", "-k", "16")
        assert _run(root, "gather", "-R", rj10, "-Q", qj10, "--scaled", "100") == want
        assert _run(root, "gather", "-R", rj10, "-Q", qj) == want        # without --scaled: the largest among the files
    # --min-shared 10 drops the last line; --max-rounds 2 keeps two
    cut = gm.gather_text([qf], [qsk], names, refs, min_shared=10)
    assert cut == "".join(ln + "\n" for ln in want.split("\n")[:picks - 1])
    assert _run(root, "gather", "-r", rf, "-f", qf, "--min-shared", "10", *opts) == cut
    assert _run(root, "gather", "-r", rf, "-f", qf, "--max-rounds", "2", *opts) == gm.gather_text([qf], [qsk], names, refs, max_rounds=2)
    # two query files are two queries; a query that nothing matches prints nothing
    lone = _write_fasta(tmp_path / "lone.fa", [b"n"], [b"ACGT" * 100])
    two = _run(root, "gather", "-r", rf, "-f", lone, "-f", qf, "-f", qf, *opts)
    assert two == want + want


def test_cli_fastq_query(root, tmp_path, data_dir):
    from rkmh_amd import api, synth
    p = sc.panel("sourmash-k21")
    names = [n.decode() for n in p["names"]]
    scaled = 100
    refs = sc.sketches("sourmash-k21", scaled)
    rb, ro = api.pack([p["seqs"][i] for i in (3, 17, 30)])
    nreads = 3000
    qb, qo = synth.generate_reads_fast(rb, ro, 0, nreads)
    fq = str(tmp_path / "sample.fq")
    synth.write_fastq(fq, qb, qo, synth.read_names(0, nreads))
    mh = scm.max_hash(scaled)
    qsk = scm.merge([scm.sketch(bytes(qb[int(qo[i]):int(qo[i + 1])]), [21], dm.SOURMASH, mh) for i in range(nreads)])
    rf = _write_fasta(tmp_path / "panel.fa", p["names"], p["seqs"])
    want = gm.gather_text([fq], [qsk], names, refs)
    assert len(want.split("\n")) >= 4                                      # at least the three records the reads were drawn from
    assert _run(root, "gather", "-r", rf, "-f", fq, "--scaled", str(scaled), "-k", "21", "--hash-policy", "sourmash") == want
