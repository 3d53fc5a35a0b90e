"""Scaled sketches on the GPU: k_scaled_pairs through both entry points (rk_compare_scaled, rk_compare_scaled_device) at every
`lanes` value, the keep step of the general path (rk_sketch_scaled_batch), and `rkmh sketch --scaled` / `rkmh dist --scaled`, against
tests/scaled_model.py bit for bit.  What the inputs exercise is shown on the model's output by tests/test_scaled_cpu.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import scaled_cases as sc
import scaled_model as scm
import sourmash_model as sm

pytestmark = pytest.mark.gpu

LANES = (0, 1, 8, 64)


def _device(ctx, av, ao, bv, bo, lanes, same=False, a_nvalues=None, b_nvalues=None):
    """the resident-input entry on torch's arrays and stream, guard words on both sides of the answer"""
    import torch
    na, nb = len(ao) - 1, len(bo) - 1

    def up(x):
        x = np.ascontiguousarray(x, dtype=np.uint64)
        return torch.from_numpy((x if len(x) else np.zeros(1, dtype=np.uint64)).view(np.int64)).cuda()
    d_av, d_ao = up(av), up(ao)
    d_bv, d_bo = (d_av, d_ao) if same else (up(bv), up(bo))
    guard = 64
    d_out = torch.full((guard + na * nb + guard,), -7, dtype=torch.int32, device="cuda")
    ctx.compare_scaled_device(d_av.data_ptr(), d_ao.data_ptr(), na, len(av) if a_nvalues is None else a_nvalues,
                              d_bv.data_ptr(), d_bo.data_ptr(), nb, len(bv) if b_nvalues is None else b_nvalues,
                              d_out.data_ptr() + 4 * guard, lanes=lanes, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[:guard] == -7).all() and (out[-guard:] == -7).all()
    return out[guard:-guard].reshape(na, nb)


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and len(bad) == 0, (what, len(bad), [(tuple(p), int(got[tuple(p)]), int(want[tuple(p)])) for p in bad[:3]])


def _both_entries(ctx, A, B, want, what, same=False):
    av, ao = scm.csr(A)
    bv, bo = (av, ao) if same else scm.csr(B)
    for lanes in LANES:
        _same(ctx.compare_scaled(av, ao, None if same else bv, None if same else bo, lanes=lanes), want, (what, lanes, "host entry"))
        _same(_device(ctx, av, ao, bv, bo, lanes, same=same), want, (what, lanes, "device entry"))


# ---- pairs: the hand-checked vectors (the first thing to run on a new kernel: single pairs) ----
def test_hand_checked_vectors_both_entries(ctx):
    for v in sc.kat():
        a, b, w = v["a"], v["b"], v["want"]
        _both_entries(ctx, [a], [b], np.array([[w]], dtype=np.int32), v["name"])
        _both_entries(ctx, [b], [a], np.array([[w]], dtype=np.int32), v["name"] + " (mirror)")
        _both_entries(ctx, [a, b], None, np.array([[len(a), w], [w, len(b)]], dtype=np.int32), v["name"] + " (self)", same=True)


# ---- pairs: random CSR sets ----
def _random_case(shape):
    na, nb = shape
    rng = np.random.default_rng(100 * na + nb)
    pl = sc.pool(rng, 6000)
    A = sc.random_sets(rng, na, pl)
    B = sc.random_sets(rng, nb, pl)
    for j in range(min(na, nb) // 2 + 1):
        B[j] = A[j]                                                          # some rows are on both sides
    return A, B


def test_random_sets_reach_every_length():
    drawn = {len(x) for shape in sc.SHAPES for side in _random_case(shape) for x in side}
    assert drawn == set(sc.LENGTHS), sorted(set(sc.LENGTHS) - drawn)


@pytest.mark.parametrize("shape", sc.SHAPES)
def test_random_sets(ctx, shape):
    A, B = _random_case(shape)
    want = scm.all_shared(A, B)
    assert shape == (1, 1) or (want > 0).any()
    _both_entries(ctx, A, B, want, shape)


def test_random_sets_self_and_a_long_row(ctx):
    rng = np.random.default_rng(5)
    pl = sc.pool(rng, 90000)
    A = sc.random_sets(rng, 9, pl, first=sc.LONG_ROW)                          # one row of 70 000 values, and a is b
    A[1] = np.sort(rng.choice(pl, size=4097, replace=False))
    want = scm.all_shared(A)
    assert want[0, 0] == sc.LONG_ROW and want[0, 1] > 1000 and want[1, 1] == 4097
    _both_entries(ctx, A, None, want, "self", same=True)
    B = sc.random_sets(rng, 3, pl, first=sc.LONG_ROW)                          # long against long
    _both_entries(ctx, A[:2], B, scm.all_shared(A[:2], B), "long rows")


def test_skewed_pairs(ctx):
    n = 4097
    base = np.arange(1, 2 * n, 2, dtype=np.uint64) * np.uint64(1 << 40)       # 4097 odd multiples of 2^40
    below = np.arange(1, n + 1, dtype=np.uint64)                              # all below base[0]
    above = base[-1] + np.arange(1, n + 1, dtype=np.uint64)
    superset = np.unique(np.concatenate([base, base + np.uint64(1 << 39)]))
    one_in, one_below, one_above, one_between = base[2048:2049], below[:1], above[-1:], base[7:8] + np.uint64(1)
    A = [below, above, base, one_in, one_below, one_above, one_between]
    B = [base, superset, one_in]
    want = np.array([[0, 0, 0], [0, 0, 0], [n, n, 1], [1, 1, 1], [0, 0, 0], [0, 0, 0], [0, 0, 0]], dtype=np.int32)
    _same(scm.all_shared(A, B), want, "the model")
    _both_entries(ctx, A, B, want, "skewed")
    _both_entries(ctx, B, A, want.T.copy(), "skewed (mirror)")


def test_rows_are_clamped_on_the_device_and_refused_on_the_host(ctx):
    from rkmh_amd import api
    rng = np.random.default_rng(8)
    pl = sc.pool(rng, 3000)
    A = sc.random_sets(rng, 4, pl, lengths=[65, 129, 1000])
    B = sc.random_sets(rng, 3, pl, lengths=[65, 129, 1000])
    av, ao = scm.csr(A)
    bv, bo = scm.csr(B)
    # fewer values behind the pointers than the offsets say: row 2 of a is cut short, row 3 of a and row 2 of b lie outside altogether
    an, bn = int(ao[2]) + 10, int(bo[2])
    Ac = [A[0], A[1], A[2][:10], A[3][:0]]
    Bc = [B[0], B[1], B[2][:0]]
    want = scm.all_shared(Ac, Bc)
    assert (want[:2, :2] > 0).any()
    for lanes in LANES:
        _same(_device(ctx, av, ao, bv, bo, lanes, a_nvalues=an, b_nvalues=bn), want, ("clamped", lanes))
    with pytest.raises(ValueError):
        ctx.compare_scaled(av[:an], ao, bv, bo)                              # offsets past the values: refused on the host entry
    with pytest.raises(ValueError):
        ctx.compare_scaled(av, ao, bv[:bn], bo)
    down = np.array([bo[1], bo[0], bo[1], bo[2]], dtype=np.uint64)           # offsets that decrease: an empty row on the device
    with pytest.raises(api.RkmhError) as e:
        ctx.compare_scaled(av, ao, bv, down)
    assert e.value.code == -1
    _same(_device(ctx, av, ao, bv, down, 0), scm.all_shared(A, [B[0][:0], B[0], B[1]]), "decreasing offsets")
    lib, h = ctx._lib, ctx._h
    out = np.zeros(16, np.int32)
    for na, nb, lanes in ((0, 1, 0), (1, 0, 0), (1, 1, 2), (1, 1, -1), (1, 1, 65)):
        assert lib.rk_compare_scaled_device(h, 8, 8, na, 1, 8, 8, nb, 1, lanes, 8, None) == -1       # refused before anything is read
        assert lib.rk_compare_scaled(h, av.ctypes.data_as(api._u64p), ao.ctypes.data_as(api._u64p), na, bv.ctypes.data_as(api._u64p),
                                     bo.ctypes.data_as(api._u64p), nb, lanes, out.ctypes.data_as(api._i32p)) == -1


# ---- keeping ----
def _ctx(spec):
    import rkmh_amd
    return rkmh_amd.Context(0, policy_spec=spec)


def _sketch(c, seqs, ks, mh):
    from rkmh_amd import api
    rb, ro = api.pack(seqs)
    v, off = c.sketch_scaled_batch(rb, ro, ks, mh)
    assert off[0] == 0 and len(off) == len(seqs) + 1 and int(off[-1]) == len(v) and (np.diff(off.astype(np.int64)) >= 0).all()
    return scm.rows(v, off)


def _equal_rows(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.uint64 and len(g) == len(w) and (g == w).all(), (what, i, len(g), len(w))


def test_threshold_sits_exactly_on_a_hash():
    p = sc.panel("sourmash-k21")
    seq, full = p["seqs"][3], p["full"][3]
    h = int(full[len(full) // 2])
    c = _ctx("sourmash")
    try:
        at, below, everything = (_sketch(c, [seq], [21], mh)[0] for mh in (h, h - 1, scm.FULL))
    finally:
        c.close()
    assert at.tolist() == full[:len(full) // 2 + 1].tolist() and at[-1] == h          # kept
    assert below.tolist() == full[:len(full) // 2].tolist()                          # dropped
    assert everything.tolist() == full.tolist()                                      # everything non-zero


@pytest.mark.parametrize("name", ["default-k12", "mash-k16", "sourmash-k21", "default-k12-k16"])
def test_panel_sketches(name):
    p = sc.panel(name)
    c = _ctx(p["spec"])
    try:
        for scaled in sc.SCALED:
            _equal_rows(_sketch(c, p["seqs"], p["ks"], scm.max_hash(scaled)), sc.sketches(name, scaled), (name, scaled))
        if name == "sourmash-k21":                                            # and the pairs of the device's own sketches
            got = _sketch(c, p["seqs"], p["ks"], scm.max_hash(10))
            v, off = scm.csr(got)
            _same(c.compare_scaled(v, off), sc.panel_shared(name, 10), name)
    finally:
        c.close()


def test_edge_sequences(ctx):
    k = 16
    rng = np.random.default_rng(2)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    long_ = bytes(rng.choice(acgt, size=500))
    seqs = [b"", b"ACGTACGT", long_[:k], b"N" * 300, long_.lower(), b"A" * 400, long_, long_[:k + 1], b"ACGTNACGT" * 40]
    got = _sketch(ctx, seqs, [k], scm.FULL)
    want = [scm.sketch(s, [k], sm.DEFAULT, scm.FULL) for s in seqs]
    _equal_rows(got, want, "edge batch")
    assert len(want[0]) == 0 and len(want[1]) == 0 and len(want[3]) == 0 and len(want[5]) == 1
    assert want[4].tolist() == want[6].tolist() and len(want[6]) > 400
    _equal_rows(_sketch(ctx, seqs, [k], scm.max_hash(3)), [scm.downsample(w, 3) for w in want], "edge batch, scaled 3")
    _equal_rows(_sketch(ctx, [b""], [k], scm.FULL), [np.zeros(0, np.uint64)], "one empty sequence")
    v, off = ctx.sketch_scaled_batch(np.zeros(16, np.uint8), np.zeros(1, np.uint64), [k], scm.FULL)
    assert len(v) == 0 and off.tolist() == [0]                                # no sequences


def test_many_short_reads(ctx):
    from rkmh_amd import api, synth
    p = sc.panel("default-k12")
    rb, ro = api.pack(p["seqs"])
    qb, qo = synth.generate_reads_fast(rb, ro, 0, 3000)
    reads = [bytes(qb[int(qo[i]):int(qo[i + 1])]) for i in range(3000)]
    mh = scm.max_hash(1000)
    v, off = ctx.sketch_scaled_batch(qb, qo, [16], mh)
    got = scm.rows(v, off)
    want = [scm.sketch(r, [16], sm.DEFAULT, mh) for r in reads]
    empty = sum(1 for w in want if len(w) == 0)
    assert 1500 < empty < 3000, empty                                       # most sketches are empty, not all
    _equal_rows(got, want, "3000 reads")


@pytest.fixture(scope="module")
def long_random():
    rng = np.random.default_rng(77)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    return [acgt[rng.integers(0, 4, size=30_000_000, dtype=np.uint8)].tobytes() for _ in range(3)]


def test_long_segment_route(ctx, long_random):
    """300 000 hashes kept at scaled 1: more than the in-LDS sorter holds, so the segment takes the whole-array sort"""
    s = long_random[1][:300_000]
    got = _sketch(ctx, [b"ACGT" * 10, s, s[:5000]], [21], scm.FULL)
    want = [scm.sketch(x, [21], sm.DEFAULT, scm.FULL) for x in (b"ACGT" * 10, s, s[:5000])]
    assert len(want[1]) > 290_000
    _equal_rows(got, want, "long segment")


def test_several_chunks(ctx, long_random):
    """three sequences of 30 M bases hold more hashes than one chunk (2^26): rows must equal the same sequence sketched alone"""
    mh = scm.max_hash(1000)
    together = _sketch(ctx, long_random, [21], mh)
    for i, s in enumerate(long_random):
        alone = _sketch(ctx, [s], [21], mh)[0]
        # a window's hash is the smaller of two strands' hashes, so it lies under max_hash with probability 2/1000 - 1/10^6:
        # 59 970 of 30 M windows are expected, with a standard deviation of 245
        assert 57_000 < len(alone) < 63_000
        _equal_rows([together[i]], [alone], ("chunks", i))
    head = long_random[2][:300_000]
    _equal_rows(_sketch(ctx, [head], [21], mh), [scm.sketch(head, [21], sm.DEFAULT, mh)], "the head of one of them against the model")


# ---- commands ----
def _run(root, *args, ok=True):
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    r = subprocess.run([os.path.join(root, "bin", "rkmh")] + list(args), capture_output=True, env=env)
    if ok:
        assert r.returncode == 0, (args, r.stderr[-400:])
        return r.stdout.decode()
    return r


def _write_fasta(path, names, seqs):
    path.write_bytes(b"".join(b">" + n + b"\n" + s + b"\n" for n, s in zip(names, seqs)))
    return str(path)


def test_cli_sketch_scaled(root, tmp_path, data_dir):
    p = sc.panel("zika-k16")
    js = str(tmp_path / "z.json")
    _run(root, "sketch", "--scaled", "100", "-k", "16", "-f", os.path.join(data_dir, "zika.refs.fa.gz"), "-o", js)
    doc = json.load(open(js))
    want = sc.sketches("zika-k16", 100)
    assert [d["name"].encode() for d in doc] == list(p["names"])
    for d, w, s in zip(doc, want, p["seqs"]):
        assert d["sketches"]["hashes"] == w.tolist() and d["sketches"]["length"] == len(w)
        assert d["scaled"] == 100 and d["maxHash"] == scm.max_hash(100) and d["kmer"] == "16" and d["seqLen"] == len(s)
    # without --scaled: no new key
    plain = json.loads(_run(root, "sketch", "-k", "16", "-s", "50", "-f", os.path.join(data_dir, "zika.fa.gz")))
    assert "scaled" not in plain[0] and "maxHash" not in plain[0] and plain[0]["sketches"]["length"] == 50


def test_cli_dist_scaled(root, tmp_path):
    p = sc.panel("zika-k16")
    names = [n.decode() for n in p["names"]]
    sk100 = sc.sketches("zika-k16", 100)
    rf = _write_fasta(tmp_path / "refs.fa", p["names"][:35], p["seqs"][:35])
    qf = _write_fasta(tmp_path / "queries.fa", p["names"][30:], p["seqs"][30:])
    opts = ["--scaled", "100", "-k", "16"]
    direct = _run(root, "dist", "-r", rf, "-f", qf, *opts)
    assert direct == scm.dist_text(names[:35], sk100[:35], names[30:], sk100[30:], 16)
    self_text = _run(root, "dist", "-r", rf, *opts)
    assert self_text == scm.dist_text(names[:35], sk100[:35], names[:35], sk100[:35], 16)
    # -d: the lines at or below the threshold, in the same order
    cut = sorted(float(ln.split("\t")[2]) for ln in self_text.split("\n")[:-1])[len(names)]
    kept = _run(root, "dist", "-r", rf, "-d", repr(cut), *opts)
    want = scm.dist_text(names[:35], sk100[:35], names[:35], sk100[:35], 16, max_dist=cut)
    assert kept == want and 35 < len(want.split("\n")) < 35 * 35
    # -R / -Q round-tripped through `rkmh sketch --scaled`; scaled and k come from the files
    rj, qj = str(tmp_path / "refs.json"), str(tmp_path / "queries.json")
    _run(root, "sketch", "-f", rf, "-o", rj, *opts)
    _run(root, "sketch", "-f", qf, "-o", qj, *opts)
    assert _run(root, "dist", "-R", rj, "-Q", qj) == direct
    assert _run(root, "dist", "-R", rj, "-f", qf) == direct and _run(root, "dist", "-r", rf, "-Q", qj, "-k", "16") == direct
    assert _run(root, "dist", "-R", rj, "--scaled", "100") == self_text
    # files made at scaled 10 and compared at 100: the bytes of the direct run
    rj10, qj10 = str(tmp_path / "refs10.json"), str(tmp_path / "queries10.json")
    _run(root, "sketch", "-f", rf, "-o", rj10, "--scaled", "10", "-k", "16")
    _run(root, "sketch", "-f", qf, "-o", qj10, "--scaled", "10", "-k", "16")
    assert _run(root, "dist", "-R", rj10, "-Q", qj10, "--scaled", "100") == direct
    assert _run(root, "dist", "-R", rj10, "-Q", qj) == direct                # without --scaled: the largest among the files
    sk10 = sc.sketches("zika-k16", 10)
    assert _run(root, "dist", "-R", rj10, "-Q", qj10) == scm.dist_text(names[:35], sk10[:35], names[30:], sk10[30:], 16)


def test_cli_whole_files_scaled(root, tmp_path):
    p = sc.panel("zika-k16")
    sk = sc.sketches("zika-k16", 100)
    groups = [list(range(0, 5)), list(range(3, 9))]
    files = [_write_fasta(tmp_path / ("g%d.fa" % i), [p["names"][j] for j in g], [p["seqs"][j] for j in g]) for i, g in enumerate(groups)]
    want = [scm.merge([sk[j] for j in g]) for g in groups]
    opts = ["--scaled", "100", "-k", "16"]
    js = str(tmp_path / "g.json")
    _run(root, "sketch", "-g", "-f", files[0], "-f", files[1], "-o", js, *opts)
    doc = json.load(open(js))
    assert [d["name"] for d in doc] == files
    for d, w, g in zip(doc, want, groups):
        assert d["sketches"]["hashes"] == w.tolist() and d["sketches"]["length"] == len(w) and d["seqLen"] == sum(len(p["seqs"][j]) for j in g)
        assert len(w) < sum(len(sk[j]) for j in g)                            # the records share hashes
    text = _run(root, "dist", "-g", "-r", files[0], "-r", files[1], *opts)
    assert text == scm.dist_text(files, want, files, want, 16)
    assert _run(root, "dist", "-R", js) == text


def test_stream_refuses_scaled_sketches(root, tmp_path, data_dir):
    js = str(tmp_path / "z.json")
    _run(root, "sketch", "--scaled", "100", "-k", "16", "-f", os.path.join(data_dir, "zika.fa.gz"), "-o", js)
    r = _run(root, "stream", "-R", js, "-f", os.path.join(data_dir, "z1.fq.gz"), "-k", "16", ok=False)
    assert r.returncode == 1 and r.stdout == b"" and b"scaled" in r.stderr and b"rkmh dist" in r.stderr
