"""Sketch comparison on the GPU: k_sketch_pairs through both entry points (rk_compare_sketches, rk_compare_sketches_device) and
through `rkmh dist`, against tests/pairs_model.py -- all four integers of every pair, bit for bit.  What the inputs exercise is shown
on the model's output by tests/test_pairs_cpu.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import pairs_cases as pc
import pairs_model as pm

pytestmark = pytest.mark.gpu


def _device(ctx, a, alens, b, blens, S, same=False):
    """the resident-input entry on torch's arrays and stream"""
    import torch
    na, nb = len(alens), len(blens)
    d_a = torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    d_al = torch.from_numpy(np.ascontiguousarray(alens, dtype=np.int32)).cuda()
    d_b, d_bl = (d_a, d_al) if same else (torch.from_numpy(np.ascontiguousarray(b).view(np.int64)).cuda(), torch.from_numpy(np.ascontiguousarray(blens, dtype=np.int32)).cuda())
    guard = 64                                                               # int32 on either side of the answer: nothing else is written
    d_out = torch.full((guard + na * nb * 4 + guard,), -7, dtype=torch.int32, device="cuda")
    ctx.compare_sketches_device(d_a.data_ptr(), d_al.data_ptr(), na, d_b.data_ptr(), d_bl.data_ptr(), nb, S, d_out.data_ptr() + 4 * guard,
                                stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[:guard] == -7).all() and (out[-guard:] == -7).all()
    return out[guard:-guard].reshape(na, nb, 4)


def _same(got, want, what):
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, (what, len(bad), [(tuple(p), got[tuple(p)].tolist(), want[tuple(p)].tolist()) for p in bad[:3]])


# ---- the hand-checked vectors (the first thing to run on a new kernel: single pairs) ----
def test_hand_checked_vectors_both_entries(ctx):
    for v in pc.kat():
        sk, ln = pm.rows([v["a"], v["b"]], v["S"])
        for got in (ctx.compare_sketches(sk[:1], ln[:1], sk[1:], ln[1:]), _device(ctx, sk[:1], ln[:1], sk[1:], ln[1:], v["S"])):
            assert got.shape == (1, 1, 4) and got[0, 0].tolist() == v["want"], v["name"]
        both = ctx.compare_sketches(sk, ln)                                  # the pair, its mirror and each against itself
        assert both[0, 1].tolist() == v["want"] and both[1, 0].tolist() == v["want"], v["name"]
        for i, x in enumerate((v["a"], v["b"])):
            d = len(set(x))
            assert both[i, i].tolist() == [len(x), d, min(d, v["S"]), min(d, v["S"])], v["name"]


# ---- tile edges ----
@pytest.mark.parametrize("S", sorted(pc.TILE_CASES))
def test_tile_edges(ctx, S):
    rng = np.random.default_rng(S)
    seen = np.zeros(3, dtype=np.int64)
    for na, nb in pc.TILE_CASES[S]:
        x, xl = pc.random_sketches(rng, na + nb, S)                          # one pool for both sides: they overlap
        a, al, b, bl = x[:na], xl[:na], x[na:], xl[na:]
        m = min(na, nb) // 2 + 1
        b[:m], bl[:m] = a[:m], al[:m]                                        # and some rows are on both sides
        want = pm.all_pairs(a, al, b, bl)
        seen += ((want[:, :, 0] > 0).sum(), (want[:, :, 0] != want[:, :, 1]).sum(), (want[:, :, 2] != want[:, :, 1]).sum())
        _same(ctx.compare_sketches(a, al, b, bl), want, (S, na, nb, "host entry"))
        _same(_device(ctx, a, al, b, bl, S), want, (S, na, nb, "device entry"))
    assert seen[0] > 0 and (S < 63 or (seen[1:] > 0).all()), seen              # shared values; repeats and the S-th union value matter
    n = pc.TILE_CASES[S][1][1]                                               # once with a is b
    a, al = pc.random_sketches(rng, n, S)
    want = pm.all_pairs(a, al)
    _same(ctx.compare_sketches(a, al), want, (S, n, "self, host entry"))
    _same(_device(ctx, a, al, a, al, S, same=True), want, (S, n, "self, device entry"))


def test_field0_is_hash_intersection_size(ctx):
    rng = np.random.default_rng(50)
    x, xl = pc.random_sketches(rng, 15, 257)
    a, al, b, bl = x[:10], xl[:10], x[10:], xl[10:]
    got = ctx.compare_sketches(a, al, b, bl)
    assert (got[:, :, 0] > 0).sum() >= 10
    for i in range(10):
        for j in range(5):
            assert got[i, j, 0] == ctx.hash_intersection_size(a[i, :al[i]], b[j, :bl[j]]), (i, j)


def test_lengths_are_clamped_on_the_device_and_refused_on_the_host(ctx):
    from rkmh_amd import api
    S = 100
    rng = np.random.default_rng(7)
    x, xl = pc.random_sketches(rng, 15, S)
    a, al, b, bl = x[:6], xl[:6], x[6:], xl[6:]
    a[:2] = np.sort(rng.integers(1, 1 << 62, size=(2, S), dtype=np.uint64), axis=1)   # full rows under the lengths that are wrong
    b[:2] = np.sort(rng.integers(1, 1 << 62, size=(2, S), dtype=np.uint64), axis=1)
    b[2], bl[2] = a[1], S
    al[0], al[1], bl[0], bl[1] = -3, S + 5, S + 5, -3
    want = pm.all_pairs(a, np.clip(al, 0, S), b, np.clip(bl, 0, S))
    assert want[1, 0, 3] == S and (want[0, :, :3] == 0).all() and (want[:, 1, :3] == 0).all() and want[1, 2, 0] == S
    _same(_device(ctx, a, al, b, bl, S), want, "clamped")
    for x, y in ((al, np.clip(bl, 0, S)), (np.clip(al, 0, S), bl)):
        with pytest.raises(api.RkmhError) as e:
            ctx.compare_sketches(a, x, b, y)
        assert e.value.code == -1
    for na, nb, s in ((0, 1, S), (1, 0, S), (1, 1, 0), (1, 1, 16385)):
        assert ctx._lib.rk_compare_sketches_device(ctx._h, 8, 8, na, 8, 8, nb, s, 8, None) == -1      # refused before anything is read


# ---- the bundled panel: device sketches, then device counts, against the model's ----
@pytest.mark.parametrize("name", sorted(pc.PANEL))
def test_panel(name):
    import rkmh_amd
    from rkmh_amd import api
    p = pc.panel(name)
    c = rkmh_amd.Context(0, policy_spec=p["spec"])
    try:
        rb, ro = api.pack(p["seqs"])
        sk, ln = c.sketch_batch(rb, ro, [p["k"]], pc.PANEL_S)
        assert (ln == p["ln"]).all() and (sk == p["sk"]).all(), "the sketches themselves differ"
        _same(c.compare_sketches(sk, ln), p["out"], (name, "host entry"))
        _same(_device(c, sk, ln, sk, ln, pc.PANEL_S, same=True), p["out"], (name, "device entry"))
        half = len(ln) // 2
        _same(c.compare_sketches(sk[half:], ln[half:], sk[:half + 3], ln[:half + 3]), p["out"][half:, :half + 3], (name, "two sets"))
    finally:
        c.close()


# ---- rkmh dist ----
def _run(root, *args):
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    r = subprocess.run([os.path.join(root, "bin", "rkmh")] + list(args), capture_output=True, env=env)
    assert r.returncode == 0, (args, r.stderr[-400:])
    return r.stdout.decode()


def _check_lines(text, ref_names, query_names, out, k):
    """out[q, r]: the model's counts; lines query by query, reference by reference; names and counts as text, the distance within 1e-6"""
    lines = text.split("\n")
    assert lines[-1] == ""
    at = 0
    for q, qn in enumerate(query_names):
        for r, rn in enumerate(ref_names):
            shared, _, common, denom = out[q, r].tolist()
            d = pm.mash_distance(common, denom, k)[1]
            f = lines[at].split("\t")
            at += 1
            assert f[:2] == [rn, qn] and f[3:] == ["%d/%d" % (common, denom), str(shared)], (q, r, f)
            assert abs(float(f[2]) - d) <= 1e-6 and not f[2].startswith("-"), (q, r, f)
            if common == denom:
                assert f[2] == "0"
    assert at == len(lines) - 1


def _write_fasta(path, names, seqs):
    path.write_bytes(b"".join(b">" + n + b"\n" + s + b"\n" for n, s in zip(names, seqs)))
    return str(path)


def test_cli_dist(root, tmp_path):
    p = pc.panel("default-k12")
    names = [n.decode() for n in p["names"]]
    rf = _write_fasta(tmp_path / "refs.fa", p["names"][:25], p["seqs"][:25])
    qf = _write_fasta(tmp_path / "queries.fa", p["names"][20:], p["seqs"][20:])
    common = ["-k", "12", "-s", str(pc.PANEL_S)]
    _check_lines(_run(root, "dist", "-r", rf, "-f", qf, *common), names[:25], names[20:], p["out"][20:, :25], 12)
    self_text = _run(root, "dist", "-r", rf, *common)
    _check_lines(self_text, names[:25], names[:25], p["out"][:25, :25], 12)
    # -d: the lines at or below the threshold, in the same order
    kept = _run(root, "dist", "-r", rf, "-d", "0.15", *common)
    want = [ln for ln in self_text.split("\n")[:-1] if float(ln.split("\t")[2]) <= 0.15]
    assert 25 < len(want) < 625 and kept.split("\n")[:-1] == want
    # sketches written by `rkmh sketch` and fed back: the same lines, k and the sketch size taken from the files
    rj, qj = str(tmp_path / "refs.json"), str(tmp_path / "queries.json")
    _run(root, "sketch", "-f", rf, "-o", rj, *common)
    _run(root, "sketch", "-f", qf, "-o", qj, *common)
    direct = _run(root, "dist", "-r", rf, "-f", qf, *common)
    assert _run(root, "dist", "-R", rj, "-Q", qj) == direct
    assert _run(root, "dist", "-R", rj, "-f", qf) == direct and _run(root, "dist", "-r", rf, "-Q", qj, "-k", "12") == direct
    assert _run(root, "dist", "-R", rj) == self_text


@pytest.mark.parametrize("spec", ["default", "sourmash"])
def test_cli_whole_files(root, tmp_path, spec):
    """-g: one sketch per FILE = the bottom S of the sketches of its records (no window spans two records), under the policy's dedup
    rule; `rkmh sketch -g` against the model, `dist -g` against the model's pairs of those, and the two round-tripped."""
    import dedup_model as dm
    import sourmash_model as sm
    p = pc.panel("default-k12")
    k, S = 12, 400
    pol, bottom = (dm.SOURMASH, dm.bottom_distinct) if spec == "sourmash" else (sm.DEFAULT, sm.bottom)
    groups = [list(range(0, 5)), list(range(3, 9))]                          # two multi-record files that share records
    files = [_write_fasta(tmp_path / ("g%d.fa" % i), [p["names"][j] for j in g], [p["seqs"][j] for j in g]) for i, g in enumerate(groups)]
    want = [bottom(np.concatenate([sm.calc_hashes(p["seqs"][j], [k], pol) for j in g]), S) for g in groups]
    spanning = bottom(sm.calc_hashes(b"".join(p["seqs"][j] for j in groups[0]), [k], pol), S)
    assert spanning.tolist() != want[0].tolist()                            # joined records would sketch differently
    opts = ["-k", str(k), "-s", str(S), "--hash-policy", spec]
    js = str(tmp_path / "g.json")
    _run(root, "sketch", "-g", "-f", files[0], "-f", files[1], "-o", js, *opts)
    doc = json.load(open(js))
    assert [d["name"] for d in doc] == files
    for d, w, g in zip(doc, want, groups):
        assert d["sketches"]["hashes"] == w.tolist() and d["sketches"]["length"] == S and d["kmer"] == str(k)
        assert d["seqLen"] == sum(len(p["seqs"][j]) for j in g)
    sk, ln = pm.rows([w.tolist() for w in want], S)
    out = pm.all_pairs(sk, ln)
    assert 0 < out[0, 1, 2] < out[0, 1, 3]
    text = _run(root, "dist", "-g", "-r", files[0], "-r", files[1], *opts)
    _check_lines(text, files, files, out, k)
    assert _run(root, "dist", "-R", js, "--hash-policy", spec) == text
    assert _run(root, "dist", "-g", "-r", files[0], "-r", files[1], "-f", files[1], *opts) == "".join(ln + "\n" for ln in text.split("\n")[2:4])
