"""Weighted comparison on the GPU: k_scaled_pairs<1 | 8 | 64, PairsWeighted> through rk_compare_scaled_abund and rk_compare_scaled_abund_device,
k_abund_row_sums through rk_abund_row_sums and its _device form, and `rkmh dist --abund`, against tests/wdist_model.py -- everything
integer, bit for bit.  What the shared inputs hold is shown on the model's output by tests/test_wdist_cpu.py."""
import os
import subprocess

import numpy as np
import pytest

import abund_model as am
import scaled_cases as sc
import scaled_model as scm
import wdist_cases as wc
import wdist_model as wm

pytestmark = pytest.mark.gpu

GUARD = 64
LANES = (0, 1, 8, 64)
U64, SAT = wm.U64, wm.SAT


def _up(x, dt, view):
    import torch
    x = np.array(x, dtype=dt)                                # (a writable copy: the shared inputs are read-only)
    return torch.from_numpy((x if len(x) else np.zeros(1, dtype=dt)).view(view)).cuda()


def _device(ctx, A, B, lanes, a_nvalues=None, b_nvalues=None, a_off=None):
    """the resident-input entry on torch's arrays and stream, guard words on both sides of the answer; B None: the arrays of A again"""
    import torch
    av, aw, ao = wm.csr(A)
    if a_off is not None:
        ao = a_off
    d_av, d_aw, d_ao = _up(av, np.uint64, np.int64), _up(aw, np.uint32, np.int32), _up(ao, np.uint64, np.int64)
    if B is None:
        bv, d_bv, d_bw, d_bo, nb = av, d_av, d_aw, d_ao, len(ao) - 1
    else:
        bv, bw, bo = wm.csr(B)
        d_bv, d_bw, d_bo, nb = _up(bv, np.uint64, np.int64), _up(bw, np.uint32, np.int32), _up(bo, np.uint64, np.int64), len(bo) - 1
    na = len(ao) - 1
    d_out = torch.full((GUARD + na * nb * 4 + GUARD,), -7, dtype=torch.int64, device="cuda")
    ctx.compare_scaled_abund_device(d_av.data_ptr(), d_aw.data_ptr(), d_ao.data_ptr(), na, len(av) if a_nvalues is None else a_nvalues,
                                    d_bv.data_ptr(), d_bw.data_ptr(), d_bo.data_ptr(), nb, len(bv) if b_nvalues is None else b_nvalues,
                                    d_out.data_ptr() + 8 * GUARD, lanes=lanes, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[:GUARD] == -7).all() and (out[GUARD + na * nb * 4:] == -7).all(), "written outside the answer"
    return out[GUARD:GUARD + na * nb * 4].view(np.uint64).reshape(na, nb, 4)


def _host(ctx, A, B, lanes):
    av, aw, ao = wm.csr(A)
    if B is None:
        return ctx.compare_scaled_abund(av, aw, ao, lanes=lanes)
    bv, bw, bo = wm.csr(B)
    return ctx.compare_scaled_abund(av, aw, ao, bv, bw, bo, lanes=lanes)


def _same(got, want, what):
    assert got.dtype == np.uint64 and got.shape == want.shape, (what, got.shape, want.shape)
    if not (got == want).all():
        at = tuple(int(x[0]) for x in np.nonzero((got != want).any(axis=-1)))
        raise AssertionError((what, "pair", at, "got", got[at].tolist(), "want", want[at].tolist()))


def _both_entries(ctx, A, B, want, what, lanes=LANES):
    for L in lanes:
        _same(_host(ctx, A, B, L), want, (what, "host entry, lanes", L))
        _same(_device(ctx, A, B, L), want, (what, "device entry, lanes", L))


def _want1(fields):
    return np.array([[fields]], dtype=np.uint64)


# ---- the vectors ----
def test_hand_checked_vectors_one_pair_a_launch(ctx):
    """a launch of one pair: one group of lanes with work, the others of its wave without (mirrors and rows against themselves: the next test)"""
    for v in wc.pair_kat():
        _both_entries(ctx, [v["a"]], [v["b"]], _want1(v["want"]), v["name"])


def test_hand_checked_vectors_all_rows_against_all(ctx):
    kat = wc.pair_kat()
    rows = [v["a"] for v in kat] + [v["b"] for v in kat]
    want = wm.all_pairs(rows)
    for i, v in enumerate(kat):                                                 # the vectors, their mirrors and every row against itself are in it
        assert tuple(want[i, len(kat) + i].tolist()) == v["want"] and tuple(want[len(kat) + i, i].tolist()) == wm.mirror(v["want"])
        assert int(want[i, i, 1]) == v["sums_a"][1] and int(want[len(kat) + i, len(kat) + i, 2]) == v["sums_b"][0]
    _both_entries(ctx, rows, rows, want, "all vectors")
    _both_entries(ctx, rows, None, want, "all vectors, self form")


# ---- random CSR sets ----
@pytest.mark.parametrize("shape", [(7, 8), (9, 65), (65, 3)])
def test_random_sets(ctx, shape):
    A, B, want = wc.random_case(*shape)
    assert int((want[:, :, 0] > 0).sum()) > len(A) and int((want[:, :, 1] > want[:, :, 0]).sum()) > 0
    _both_entries(ctx, A, B, want, shape)
    _same(ctx.compare_scaled(*scm.csr([v for v, _ in A]), *scm.csr([v for v, _ in B])).astype(np.uint64), want[:, :, 0], "shared is rk_compare_scaled's")


def test_random_sets_with_a_row_of_70000(ctx):
    A, B, want = wc.random_case(3, 5, long_row=True)
    assert len(A[0][0]) == sc.LONG_ROW and int(want[0, :, 0].max()) > 100 and int((want[:, :, 1] == U64).sum()) > 0
    _both_entries(ctx, A, B, want, "long row in a")
    back = np.ascontiguousarray(want.transpose(1, 0, 2)[:, :, [0, 1, 3, 2]])
    _both_entries(ctx, B, A, back, "long row in b")


def test_random_sets_against_themselves(ctx):
    A, _, want = wc.random_case(9, 9, self_form=True)
    sums = wm.all_row_sums(A)
    for i, (v, _) in enumerate(A):
        assert want[i, i].tolist() == [len(v), int(sums[i, 1]), int(sums[i, 0]), int(sums[i, 0])]
    _both_entries(ctx, A, None, want, "a = b, uploaded once")
    _both_entries(ctx, A, A, want, "a = b as two sides")


# ---- slice boundaries ----
def _staircase(n, step, w0, wstep):
    v = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(step))
    w = (np.uint32(w0) + np.arange(n, dtype=np.uint32) * np.uint32(wstep))
    return v, w


def test_identical_rows_at_the_slice_boundaries(ctx):
    """rows of 8, 9, 64, 65 and 128 values, each a prefix of the longest: every slice's first and last element is a shared value with an
    abundance of its own, so a value counted twice or dropped moves wa_in and wb_in"""
    A = [_staircase(n, 1000, 1, 3) for n in (8, 9, 64, 65, 128)]
    B = [_staircase(n, 1000, 100000, 7) for n in (8, 9, 64, 65, 128)]
    want = wm.all_pairs(A, B)
    for i, n in enumerate((8, 9, 64, 65, 128)):
        assert want[i, i, 0] == n and want[i, i, 2] == sum(1 + 3 * t for t in range(n)) and want[i, i, 3] == sum(100000 + 7 * t for t in range(n))
        assert want[i, 4, 0] == n and want[4, i, 0] == n
    _both_entries(ctx, A, B, want, "prefixes")
    for i in range(5):
        _both_entries(ctx, [A[i]], [B[i]], want[i:i + 1, i:i + 1], ("one pair", len(A[i][0])))


def test_4097_against_4097_and_against_1(ctx):
    a = _staircase(4097, 3, 1, 1)
    B = [_staircase(4097, 3, 5, 2)] + [(a[0][i:i + 1], np.array([9 + i], np.uint32)) for i in (0, 2048, 4096)] + [(np.array([2], np.uint64), np.array([4], np.uint32))]
    want = wm.all_pairs([a], B)
    assert want[0, :, 0].tolist() == [4097, 1, 1, 1, 0] and want[0, 1:4, 2].tolist() == [1, 2049, 4097] and want[0, 1:4, 3].tolist() == [9, 2057, 4105]
    _both_entries(ctx, [a], B, want, "4097 in a")
    _both_entries(ctx, B, [a], np.ascontiguousarray(want.transpose(1, 0, 2)[:, :, [0, 1, 3, 2]]), "4097 in b")


def test_side_order_when_b_is_the_shorter_row(ctx):
    a = _staircase(100, 10, 2, 1)                                             # 10, 20, ..., 1000 with abundances 2, 3, ...
    b = (np.array([10, 500, 1000], np.uint64), np.array([1000, 2000, 3000], np.uint32))
    want = wm.pair(a, b)
    assert want == (3, 2 * 1000 + 51 * 2000 + 101 * 3000, 2 + 51 + 101, 6000) and want[2] != want[3]
    _both_entries(ctx, [a], [b], _want1(want), "b shorter")
    _both_entries(ctx, [b], [a], _want1(wm.mirror(want)), "a shorter")
    _both_entries(ctx, [a, b], [b, a], wm.all_pairs([a, b], [b, a]), "both orders in one launch")


# ---- saturation ----
def test_dot_saturates_in_one_lane(ctx):
    r = (np.array([5, 9], np.uint64), np.array([SAT, SAT], np.uint32))
    want = (2, U64, 2 * SAT, 2 * SAT)
    assert wm.pair(r, r) == want and SAT * SAT < U64 < 2 * SAT * SAT
    _both_entries(ctx, [r], [r], _want1(want), "rows of 2")


def test_dot_saturates_in_the_shuffle_reduction(ctx):
    """rows of 16 that share the values at index 3 and 11 only: with 8 lanes they lie in slices 1 and 5, with 64 in lanes of their own"""
    va = np.arange(1, 17, dtype=np.uint64) * np.uint64(10)
    vb = va + np.uint64(1)
    vb[[3, 11]] = va[[3, 11]]
    wa, wb = np.full(16, 3, np.uint32), np.full(16, 5, np.uint32)
    wa[[3, 11]] = SAT
    wb[[3, 11]] = SAT
    want = (2, U64, 2 * SAT, 2 * SAT)
    assert wm.pair((va, wa), (vb, wb)) == want
    _both_entries(ctx, [(va, wa)], [(vb, wb)], _want1(want), "rows of 16")
    wb[11] = 2                                                                  # (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1 exactly: no saturation, the same number
    _both_entries(ctx, [(va, wa)], [(vb, wb)], _want1((2, U64, 2 * SAT, SAT + 2)), "exactly 2^64 - 1")
    wb[11] = 1
    _both_entries(ctx, [(va, wa)], [(vb, wb)], _want1((2, U64 - SAT, 2 * SAT, SAT + 1)), "one step below")


# ---- k_abund_row_sums ----
def _device_sums(ctx, w, off, nvalues=None):
    import torch
    n = len(off) - 1
    d_w, d_off = _up(w, np.uint32, np.int32), _up(off, np.uint64, np.int64)
    d_out = torch.full((GUARD + n * 2 + GUARD,), -7, dtype=torch.int64, device="cuda")
    ctx.abund_row_sums_device(d_w.data_ptr(), d_off.data_ptr(), n, len(w) if nvalues is None else nvalues, d_out.data_ptr() + 8 * GUARD,
                              stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[:GUARD] == -7).all() and (out[GUARD + n * 2:] == -7).all(), "written outside the sums"
    return out[GUARD:GUARD + n * 2].view(np.uint64).reshape(n, 2)


def test_row_sums(ctx):
    rng = np.random.default_rng(5)
    rows = [wc.weights(rng, n) for n in (0, 1, 63, 64, 65, 70000, 0)] + [np.array([SAT, SAT], np.uint32), np.array([SAT], np.uint32), np.arange(1, 200, dtype=np.uint32)]
    want = wm.all_row_sums(rows)
    assert want[7].tolist() == [2 * SAT, U64] and want[8].tolist() == [SAT, SAT * SAT] and want[9].tolist() == [199 * 100, 199 * 200 * 399 // 6]
    assert want[0].tolist() == [0, 0] and int(want[5, 1]) == U64 and int(want[5, 0]) > 70000
    w = np.concatenate(rows)
    off = np.zeros(len(rows) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    _same(ctx.abund_row_sums(w, off), want, "host entry")
    _same(_device_sums(ctx, w, off), want, "device entry")
    for i in range(len(rows)):                                                  # and every row alone
        _same(_device_sums(ctx, rows[i], np.array([0, len(rows[i])], np.uint64)), want[i:i + 1], ("alone", i))
    lens = rng.integers(0, 3, size=70001)                                       # more rows than the grid has waves (16 384 x 4): the stride loop's second trip
    w = wc.weights(rng, int(lens.sum()))
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    want = wm.all_row_sums([w[int(off[i]):int(off[i + 1])] for i in range(len(lens))])
    assert want[65536:, 0].any()
    _same(_device_sums(ctx, w, off), want, "70 001 short rows")
    _same(ctx.abund_row_sums(w, off), want, "70 001 short rows, host entry")


# ---- offsets past nvalues, abundances of 0, refusals ----
def test_rows_are_clamped_on_the_device(ctx):
    rng = np.random.default_rng(8)
    pl = sc.pool(rng, 3000)
    A = wc.with_weights(rng, sc.random_sets(rng, 4, pl, lengths=[65, 129, 1000]))
    B = wc.with_weights(rng, sc.random_sets(rng, 3, pl, lengths=[64, 500]))
    av, aw, ao = wm.csr(A)
    # fewer values behind the pointers than the offsets say: row 2 is cut short, row 3 lies outside altogether
    n = int(ao[2]) + 10
    cut = [A[0], A[1], (A[2][0][:10], A[2][1][:10]), (A[3][0][:0], A[3][1][:0])]
    want = wm.all_pairs(cut, B)
    assert (want[3] == 0).all() and int(want[:2, :, 0].sum()) > 0
    for L in LANES:
        _same(_device(ctx, A, B, L, a_nvalues=n), want, ("fewer values in a", L))
        _same(_device(ctx, B, A, L, b_nvalues=n), np.ascontiguousarray(want.transpose(1, 0, 2)[:, :, [0, 1, 3, 2]]), ("fewer values in b", L))
    down = np.array([ao[1], ao[0], ao[1], ao[2]], dtype=np.uint64)             # offsets that decrease: an empty row
    want = wm.all_pairs([(A[0][0][:0], A[0][1][:0]), A[0], A[1]], B)
    for L in LANES:
        _same(_device(ctx, A, B, L, a_off=down), want, ("decreasing offsets", L))
    sums = wm.all_row_sums([c[1] for c in cut])
    _same(_device_sums(ctx, aw, ao, nvalues=n), sums, "row sums, fewer values")
    # refused on the host, by the bindings, before anything is uploaded
    past = np.array(ao)
    past[-1] += 1
    with pytest.raises(ValueError):
        ctx.compare_scaled_abund(av, aw, past)
    with pytest.raises(ValueError):
        ctx.abund_row_sums(aw, past)


def test_an_abundance_of_zero(ctx):
    from rkmh_amd import api
    A, B, want = wc.random_case(7, 8)
    zero = [(v, np.where(np.arange(len(w)) % 2 == 0, 0, w).astype(np.uint32)) for v, w in A]
    tb = [dict(zip(v.tolist(), w.tolist())) for v, w in B]
    expect = np.array([[wm._pair(dict(zip(v.tolist(), w.tolist())), t) for t in tb] for v, w in zero], dtype=np.uint64)
    assert (expect[:, :, 0] == want[:, :, 0]).all() and (expect[:, :, 2] < want[:, :, 2]).any() and (expect[:, :, 3] == want[:, :, 3]).all()
    for L in LANES:                                                             # the device entry cannot refuse it: a 0 adds nothing
        _same(_device(ctx, zero, B, L), expect, ("zeros", L))
    for bad_a, bad_b in ((zero, B), (B, zero)):                                 # the entry on host arrays refuses it
        with pytest.raises(api.RkmhError) as e:
            _host(ctx, bad_a, bad_b, 0)
        assert e.value.code == -1
    with pytest.raises(api.RkmhError):
        ctx.abund_row_sums(*wm.csr(zero)[1:])
    with pytest.raises(api.RkmhError):
        ctx.compare_scaled_abund(*wm.csr(A), lanes=3)
    _same(_host(ctx, A, B, 0), want, "and the context still works")


# ---- the command ----
def _run(root, *args):
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    r = subprocess.run([os.path.join(root, "bin", "rkmh")] + list(args), capture_output=True, env=env)
    assert r.returncode == 0, (args, r.stderr[-400:])
    return r.stdout.decode()


def _write_fasta(path, names, seqs):
    path.write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in zip(names, seqs)))
    return str(path)


def _plain(sketches):
    return [v for v, _ in sketches]


@pytest.mark.parametrize("scaled", [10, 100])
@pytest.mark.parametrize("key", sorted(wc.FILES))
def test_cli_dist_abund_on_the_bundled_files(root, tmp_path, key, scaled):
    f = wc.file_full(key)
    sk = wc.file_sketches(key, scaled)
    path = f["path"] if f["first"] is None else _write_fasta(tmp_path / "records.fa", f["names"], f["seqs"])
    opts = ["-r", path, "--scaled", str(scaled), "-k", str(f["k"]), "--hash-policy", f["spec"]]
    got = _run(root, "dist", "--abund", *opts)
    assert got == wm.dist_text(f["names"], sk, f["names"], sk, f["k"])
    plain = _run(root, "dist", *opts)                                           # the switch has not moved the old output
    assert plain == scm.dist_text(f["names"], _plain(sk), f["names"], _plain(sk), f["k"])
    assert [ln.split("\t")[:6] for ln in got.split("\n")[:-1]] == [ln.split("\t") for ln in plain.split("\n")[:-1]]


def test_cli_dist_abund_forms(root, tmp_path):
    f = wc.file_full(("pave", "default"))
    names, seqs, k = f["names"], f["seqs"], f["k"]
    sk100 = wc.file_sketches(("pave", "default"), 100)
    rf = _write_fasta(tmp_path / "refs.fa", names[:30], seqs[:30])
    qf = _write_fasta(tmp_path / "queries.fa", names[25:], seqs[25:])
    opts = ["--scaled", "100", "-k", str(k)]
    direct = _run(root, "dist", "--abund", "-r", rf, "-f", qf, *opts)
    assert direct == wm.dist_text(names[:30], sk100[:30], names[25:], sk100[25:], k)
    assert any(ln.split("\t")[6] not in ("0", "1") for ln in direct.split("\n")[:-1])
    self_text = _run(root, "dist", "--abund", "-r", rf, *opts)
    assert self_text == wm.dist_text(names[:30], sk100[:30], names[:30], sk100[:30], k)
    for ln in self_text.split("\n")[:-1]:                                       # a sketch against itself: angular similarity 1, every window inside
        c = ln.split("\t")
        if c[0] == c[1] and c[7] != "0/0":
            assert c[6] == "1" and len(set(c[7].split("/"))) == 1 and c[7] == c[8], ln
    # -d filters on the distance column
    cut = sorted(float(ln.split("\t")[2]) for ln in self_text.split("\n")[:-1])[60]
    kept = _run(root, "dist", "--abund", "-r", rf, "-d", repr(cut), *opts)
    want = wm.dist_text(names[:30], sk100[:30], names[:30], sk100[:30], k, max_dist=cut)
    assert kept == want and 30 < len(want.split("\n")) < 30 * 30
    assert _run(root, "dist", "-r", rf, "-d", repr(cut), *opts) == scm.dist_text(names[:30], _plain(sk100[:30]), names[:30], _plain(sk100[:30]), k, max_dist=cut)


def test_cli_dist_abund_sketch_files(root, tmp_path):
    f = wc.file_full(("pave", "default"))
    names, seqs, k = f["names"], f["seqs"], f["k"]
    sk100, sk10 = wc.file_sketches(("pave", "default"), 100), wc.file_sketches(("pave", "default"), 10)
    rf = _write_fasta(tmp_path / "refs.fa", names[:30], seqs[:30])
    qf = _write_fasta(tmp_path / "queries.fa", names[25:], seqs[25:])
    opts = ["--scaled", "100", "-k", str(k)]
    direct = wm.dist_text(names[:30], sk100[:30], names[25:], sk100[25:], k)
    self_text = wm.dist_text(names[:30], sk100[:30], names[:30], sk100[:30], k)
    # -R / -Q round-tripped through `rkmh sketch --scaled --abund`; scaled and k come from the files
    rj, qj = str(tmp_path / "refs.json"), str(tmp_path / "queries.json")
    _run(root, "sketch", "--abund", "-f", rf, "-o", rj, *opts)
    _run(root, "sketch", "--abund", "-f", qf, "-o", qj, *opts)
    assert _run(root, "dist", "--abund", "-R", rj, "-Q", qj) == direct
    assert _run(root, "dist", "--abund", "-R", rj, "-f", qf) == direct and _run(root, "dist", "--abund", "-r", rf, "-Q", qj, "-k", str(k)) == direct
    assert _run(root, "dist", "--abund", "-R", rj, "--scaled", "100") == self_text
    plain_direct = scm.dist_text(names[:30], _plain(sk100[:30]), names[25:], _plain(sk100[25:]), k)
    assert _run(root, "dist", "-R", rj, "-Q", qj) == plain_direct and _run(root, "dist", "-r", rf, "-f", qf, *opts) == plain_direct
    # files made at scaled 10 and compared at 100: the cut is a prefix of both arrays
    rj10, qj10 = str(tmp_path / "refs10.json"), str(tmp_path / "queries10.json")
    _run(root, "sketch", "--abund", "-f", rf, "-o", rj10, "--scaled", "10", "-k", str(k))
    _run(root, "sketch", "--abund", "-f", qf, "-o", qj10, "--scaled", "10", "-k", str(k))
    assert _run(root, "dist", "--abund", "-R", rj10, "-Q", qj10, "--scaled", "100") == direct
    assert _run(root, "dist", "--abund", "-R", rj10, "-Q", qj) == direct       # without --scaled: the largest among the files
    assert _run(root, "dist", "--abund", "-R", rj10, "-Q", qj10) == wm.dist_text(names[:30], sk10[:30], names[25:], sk10[25:], k)
    assert _run(root, "dist", "-R", rj10, "-Q", qj10, "--scaled", "100") == plain_direct


def test_cli_dist_abund_whole_files(root, tmp_path):
    f = wc.file_full(("pave", "default"))
    names, seqs, k = f["names"], f["seqs"], f["k"]
    sk = wc.file_sketches(("pave", "default"), 100)
    mh = scm.max_hash(100)
    groups = [list(range(0, 5)), list(range(3, 9)), list(range(20, 22))]
    files = [_write_fasta(tmp_path / ("g%d.fa" % i), [names[j] for j in g], [seqs[j] for j in g]) for i, g in enumerate(groups)]
    want = [am.merge([sk[j] for j in g], mh) for g in groups]
    assert int(want[1][1].max()) > max(int(sk[j][1].max()) for j in groups[1]) or int(want[1][1].sum()) == sum(int(sk[j][1].sum()) for j in groups[1])
    opts = ["--scaled", "100", "-k", str(k)]
    args = [x for p in files for x in ("-r", p)]
    text = _run(root, "dist", "--abund", "-g", *args, *opts)
    assert text == wm.dist_text(files, want, files, want, k)
    js = str(tmp_path / "g.json")
    _run(root, "sketch", "--abund", "-g", "-f", files[0], "-f", files[1], "-f", files[2], "-o", js, *opts)
    assert _run(root, "dist", "--abund", "-R", js) == text
    assert _run(root, "dist", "-g", *args, *opts) == scm.dist_text(files, _plain(want), files, _plain(want), k)
