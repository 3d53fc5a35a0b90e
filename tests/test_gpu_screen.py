"""Screen on the GPU (rk_screen_*, rk_fastq_slot_screen, `rkmh screen`; include/rkmh_amd.h "SCREEN"): the counts of every key and the four
numbers of every reference against tests/screen_model.py, integer for integer -- at the edges of the tile walk, of the key lookup and
its directory, of the row kernels (row lengths around a wave, 8 193 references, counts up to and past 2^32), under contention on one
key, for every policy and k list, by every feed route; and the command on the HPV references.  What the shared inputs
(tests/screen_cases.py) hold is shown on the model by tests/test_screen_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sample_cases as sc
import screen_cases as cs
import screen_model as scm
import sourmash_model as sm

pytestmark = pytest.mark.gpu

K = cs.K
SAT = scm.SAT


@pytest.fixture(scope="module")
def contexts():
    """one context per policy, none with references"""
    import rkmh_amd
    c = {name: rkmh_amd.Context(0, policy_spec=name) for name in cs.POLICIES}
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(scope="module")
def c(contexts):
    return contexts["default"]


def _screen(ctx, rows, ks=(K,)):
    v, off = scm.to_csr(rows)
    return ctx.screen(list(ks), v, off)


def _feed(s, groups):
    for g in groups:
        b, off = sc.pack(g)
        s.add(b, off)


def _same_counts(s, rows, counts, what=""):
    keys, cnt = s.counts()
    wk, wc = scm.key_counts(rows, counts)
    assert keys.dtype == np.uint64 and cnt.dtype == np.uint64
    assert keys.tolist() == wk, (what, "keys")
    assert cnt.tolist() == wc, (what, "counts", [(k, a, b) for k, a, b in zip(wk, cnt.tolist(), wc) if a != b][:5])


def _same_rows(s, rows, counts, ms=(1, 2, 3), what=""):
    for m in ms:
        got = s.rows(m)
        assert got.dtype == np.uint32 and got.tolist() == scm.rows(rows, counts, m), (what, m)


def _check(ctx, rows, reads, ks=(K,), pol=sm.DEFAULT, groups=None, ms=(1, 2, 3), what=""):
    counts = scm.counted(reads, ks, pol)
    s = _screen(ctx, rows, ks)
    try:
        _feed(s, groups if groups is not None else [list(reads)])
        _same_counts(s, rows, counts, what)
        _same_rows(s, rows, counts, ms, what)
        st = s.stats()
        assert st["nseq"] == len(reads) and st["nbases"] == sum(len(r) for r in reads), (what, st)
        assert st["counted"] == sum(scm.key_counts(rows, counts)[1]), (what, st)
        return st
    finally:
        s.close()


def _rows_of(reads, seed, nref=3, length=40, ks=(K,), pol=sm.DEFAULT, **kw):
    return cs.rows_from(cs.hashes(reads, ks, pol), np.random.default_rng(seed), nref, length, **kw)


# ---- feed edges ----
@pytest.mark.parametrize("total", cs.TOTALS)
def test_totals_around_a_tile(c, total):
    reads = cs.single_read(total)
    h = cs.hashes(reads)
    rows = [sorted(set(h))] if h else [[5, 9]]
    rows.append(_rows_of(reads, total, 1, 30)[0])
    st = _check(c, rows, reads, what=total)
    assert st["counted"] >= len(h) == max(total - K, 0)       # every window is counted, by the first row at least


def test_reads_around_tile_edges(c):
    reads = cs.edge_batch()
    h = cs.hashes(reads)
    rows = [sorted(set(h))] + _rows_of(reads, 1, 2, 300, repeats=True)
    _check(c, rows, reads, what="one batch")
    for r in (b"A", b"ACGT" * 5, b"N" * 40, b""):
        _check(c, rows, [r], what=r[:4])
    s = _screen(c, rows)
    try:
        s.add(np.zeros(16, np.uint8), np.zeros(1, np.uint64))          # an empty batch
        assert s.stats()["nseq"] == 0 and not s.counts()[1].any() and s.rows(1).tolist() == [[0, 0, 0, 0]] * 3
    finally:
        s.close()


def test_one_batch_with_more_tiles_than_the_grid(c):
    block, R = cs.block(), cs.many_tiles_R()
    counts = {v: n * R for v, n in scm.counted(block, (K,), sm.DEFAULT).items()}
    rows = _rows_of(block, 2, 4, 500)
    b, off = sc.pack(list(block) * R)
    assert (int(off[-1]) + cs.W - 1) // cs.W > cs.GRID_CAP
    s = _screen(c, rows)
    try:
        s.add(b, off)
        _same_counts(s, rows, counts)
        _same_rows(s, rows, counts, (1, R, R + 1))
    finally:
        s.close()


# ---- lookup edges ----
def test_lookup_edges(c):
    reads = sc.reads300()[:60]
    h = sorted(set(cs.hashes(reads)))
    lo, hi, mid = h[0], h[-1], h[len(h) // 2]
    for rows, what in (([[mid]], "one key"), ([[lo, hi]], "two keys"), ([[lo]], "the smallest hash"), ([[hi]], "the largest hash"),
                       ([[hi - 1]], "a key one below a hash: the hash is the largest key + 1"), ([[lo + 1], [mid - 1, mid, mid + 1], [hi - 1, hi]], "neighbours"),
                       ([[1, 2, lo], [mid], [hi, scm.FULL]], "keys in the first and the last bucket, one alone in the middle"),
                       ([[1], [scm.FULL]], "no hash is a key"), ([h[::2], h[1::2], []], "every hash is a key; an empty row")):
        st = _check(c, rows, reads, what=what)
        if what == "two keys":
            assert st["nkeys"] == 2 and st["dir_buckets"] > 2, st                 # a directory larger than nkeys
    s = _screen(c, [[hi - 1]])
    try:
        _feed(s, [list(reads)])
        assert hi - 1 not in h and s.counts()[1].tolist() == [0] and s.stats()["dir_buckets"] > 1
    finally:
        s.close()


# ---- contention ----
def test_contention_on_one_key(c):
    reads = cs.homopolymers()
    (key,) = set(cs.hashes(reads[:1]))
    want = 2000 * (60 - K)
    for rows in ([[key]], [[key, key + 7], [3, key], [key]]):
        st = _check(c, rows, reads, ms=(1, want, want + 1), what=len(rows))
        assert st["counted"] == want


# ---- rows ----
def test_row_lengths_and_injected_counts(c):
    rng = np.random.default_rng(5)
    pool = np.unique(rng.integers(1, 1 << 62, size=40000, dtype=np.uint64)).tolist()
    lens = (1, 63, 64, 65, 1000, 16384)
    rows, at = [], 0
    for n in lens:                                            # overlapping rows: each begins inside the one before
        rows.append(pool[at:at + n])
        at += max(n // 2, 1)
    rows.append(sorted(rows[4] + rows[4][::2]))               # a row with repeats: a copy of row 4 once collapsed (owner tie -> row 4)
    rows.append(pool[30000:30050])                            # shares nothing
    used = sorted({v for r in rows[:-1] for v in r})
    big = [1, 2, 3, SAT - 1, SAT]
    counts = {v: int(big[i % 5]) if i % 3 == 0 else int(rng.integers(1, 50)) for i, v in enumerate(used) if i % 7}
    s = _screen(c, rows)
    try:
        vals = np.asarray(sorted(counts), np.uint64)
        s.add_counts(vals, np.asarray([counts[int(v)] for v in vals], np.uint32))
        _same_counts(s, rows, counts)
        _same_rows(s, rows, counts, (1, 2, 3, SAT))
        out = s.rows(1)
        assert out[-1].tolist() == [0, 0, 0, 0] and out[6, 0] == out[4, 0] and out[6, 2] == 0
        # past 2^32: 6 more on top of 2^32 - 1 reads as the clamp, the raw count does not wrap
        top = np.asarray([v for v in vals.tolist() if counts[v] == SAT][:40], np.uint64)
        s.add_counts(top, np.full(len(top), 6, np.uint32))
        for v in top.tolist():
            counts[v] += 6
        assert max(counts.values()) == (1 << 32) + 5
        _same_counts(s, rows, counts)
        _same_rows(s, rows, counts, (1, SAT))
        assert s.stats()["injected"] == sum(counts.values())
        # values that are no key are ignored
        s.add_counts(np.asarray([pool[39000], pool[39001]], np.uint64), np.asarray([9, 9], np.uint32))
        _same_counts(s, rows, counts)
    finally:
        s.close()


@pytest.mark.parametrize("nref", [1, 8193])
def test_many_short_rows(c, nref):
    rng = np.random.default_rng(nref)
    pool = np.unique(rng.integers(1, 1 << 40, size=3000, dtype=np.uint64)).tolist()
    rows = [sorted(set(int(x) for x in rng.choice(pool, size=int(rng.integers(0, 6))))) for _ in range(nref)]
    rows[0] = pool[:70]                                       # 70 postings and more on these keys: the owner kernel's wave path
    if nref > 1:
        for i in range(1, 80):
            rows[i] = sorted(set(rows[i]) | {pool[0], pool[1]})
        rows[nref - 1] = list(rows[7])                        # identical references far apart
    counts = {v: int(rng.integers(1, 4)) for v in pool[::2] + [pool[1]]}
    s = _screen(c, rows)
    try:
        vals = np.asarray(sorted(counts), np.uint64)
        s.add_counts(vals, np.asarray([counts[int(v)] for v in vals], np.uint32))
        _same_rows(s, rows, counts)
    finally:
        s.close()


# ---- policies and k ----
@pytest.mark.parametrize("policy", ["default", "mash", "sourmash"])
@pytest.mark.parametrize("ks", [(16,), (21,), (31,), (12, 16)])
def test_policies_and_k(contexts, policy, ks):
    pol = cs.POLICIES[policy]
    reads = list(sc.reads300()[:80]) + list(sc.edge_reads())
    rows = _rows_of(reads, 7, 3, 200, ks=ks, pol=pol, repeats=True)
    _check(contexts[policy], rows, reads, ks=ks, pol=pol, what=(policy, ks))


# ---- against the sample accumulator and the weighted comparison ----
def test_shared_equals_the_sample_route(c):
    reads = sc.reads300()
    rows = _rows_of(reads, 8, 5, 300, repeats=True)
    smp = c.sample([K], scm.FULL, abund=True)
    s = _screen(c, rows)
    try:
        b, off = sc.pack(list(reads))
        smp.add(b, off)
        v, a = smp.finish()
        coll = [scm.collapse(r) for r in rows]
        rv, ro = scm.to_csr(coll)
        out = c.compare_scaled_abund(v, a, np.asarray([0, len(v)], np.uint64), rv, np.ones(len(rv), np.uint32), ro)
        s.add(b, off)
        assert s.rows(1)[:, 0].tolist() == out[0, :, 0].tolist()
    finally:
        smp.close()
        s.close()


# ---- invariance, routes ----
def test_groups_order_twice_and_reset(c):
    reads = list(sc.reads300()[:140])
    rows = _rows_of(reads, 9, 4, 300)
    counts = scm.counted(reads, (K,), sm.DEFAULT)
    rng = np.random.default_rng(3)
    s = _screen(c, rows)
    try:
        for n in (1, 3, 7):
            cut = [0] + sorted(rng.choice(np.arange(1, len(reads)), size=n - 1, replace=False).tolist()) + [len(reads)]
            groups = [reads[a:b] for a, b in zip(cut[:-1], cut[1:])]
            rng.shuffle(groups)
            s.reset()
            assert s.stats()["nseq"] == 0 and not s.counts()[1].any()
            _feed(s, groups)
            _same_counts(s, rows, counts, n)
            _same_rows(s, rows, counts, what=n)
        _feed(s, [[reads[i] for i in rng.permutation(len(reads))]])               # twice: every count doubles
        twice = {v: 2 * n for v, n in counts.items()}
        _same_counts(s, rows, twice)
        _same_rows(s, rows, twice, (1, 2, 4))
    finally:
        s.close()


class _Resident:
    """arrays on the device through the library's own allocator, freed on exit"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def up(self, a):
        lib, h = self.ctx._lib, self.ctx._h
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert lib.rk_device_alloc(h, a.nbytes, C.byref(p)) == 0
        self.ptrs.append(p)
        assert lib.rk_device_upload(h, p, a.ctypes.data_as(C.c_void_p), a.nbytes) == 0
        return p.value

    def down(self, ptr, a):
        assert self.ctx._lib.rk_device_download(self.ctx._h, a.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), a.nbytes) == 0
        return a

    def free(self):
        for p in self.ptrs:
            self.ctx._lib.rk_device_free(self.ctx._h, p)
        self.ptrs = []


def test_host_device_and_slot_routes(c, contexts):
    import rkmh_amd
    from rkmh_amd import api
    reads, text = sc.fastq200()
    rows = _rows_of(reads, 10, 3, 300, ks=(16,))
    counts = scm.counted(reads, (16,), sm.DEFAULT)
    s = _screen(c, rows, ks=(16,))
    slot = api.FastqSlot(c, max_bytes=1 << 16)
    other = api.FastqSlot(contexts["mash"], max_bytes=1 << 16)
    dev = _Resident(c)
    try:
        assert slot.screen(text, s) == (0, 200)
        _same_counts(s, rows, counts, "slot")
        st = s.stats()
        assert slot.screen(sc.fastq_with_cr(), s)[0] != 0                         # not four lines per record: nothing is added
        assert s.stats() == st
        _same_counts(s, rows, counts, "a refused block")
        with pytest.raises(rkmh_amd.RkmhError, match="another context"):
            other.screen(text, s)
        s.reset()
        b, off = sc.pack(list(reads))
        G = 64                                                                    # guard words around d_out4
        out = np.full(G + 4 * len(rows) + G, 0xA5A5A5A5, dtype=np.uint32)
        d_b, d_o, d_out = dev.up(b), dev.up(off.astype(np.uint32)), dev.up(out)
        s.add_device(d_b, d_o, len(reads), c.stream)
        s.rows_device(d_out + 4 * G, 2, c.stream)
        c.synchronize()
        dev.down(d_out, out)
        assert (out[:G] == 0xA5A5A5A5).all() and (out[G + 4 * len(rows):] == 0xA5A5A5A5).all(), "written outside d_out4"
        assert out[G:G + 4 * len(rows)].reshape(-1, 4).tolist() == scm.rows(rows, counts, 2)
        _same_counts(s, rows, counts, "device")
        assert s.stats()["nseq"] == 200
    finally:
        dev.free()
        s.close()
        slot.destroy()
        other.destroy()


# ---- refusals ----
def test_refusals(c):
    import rkmh_amd
    lib = c._lib
    v, off = scm.to_csr([[1, 2, 3], [2, 5]])
    for ks in ([], list(range(8, 17)), [0], [65]):
        with pytest.raises(rkmh_amd.RkmhError):
            c.screen(ks, v, off)
    for bad_v, bad_off, word in (([1, 3, 2, 2, 5], [0, 3, 5], "descends"), ([0, 2, 3, 2, 5], [0, 3, 5], "is 0"), ([1, 2, 3, 2, 5], [0, 3, 2], "decrease")):
        with pytest.raises(rkmh_amd.RkmhError, match=word):
            c.screen([K], np.asarray(bad_v, np.uint64), np.asarray(bad_off, np.uint64))
    ks = np.array([K], np.int32)
    kp, vp, op = ks.ctypes.data_as(C.POINTER(C.c_int)), v.ctypes.data_as(C.POINTER(C.c_uint64)), off.ctypes.data_as(C.POINTER(C.c_uint64))
    h = C.c_void_p()
    assert lib.rk_screen_create(None, kp, 1, vp, op, 2, C.byref(h)) == -1 and lib.rk_screen_create(c._h, kp, 1, vp, None, 2, C.byref(h)) == -1
    assert lib.rk_screen_create(c._h, kp, 1, None, op, 2, C.byref(h)) == -1 and lib.rk_screen_create(c._h, kp, 1, vp, op, 2, None) == -1
    assert lib.rk_screen_create(c._h, kp, 1, vp, op, 0, C.byref(h)) == -1 and lib.rk_screen_create(c._h, kp, 1, vp, op, 1 << 31, C.byref(h)) == -5
    assert lib.rk_screen_reset(None) != 0 and lib.rk_screen_add_batch(None, None, None, 0) != 0 and lib.rk_screen_add_batch_device(None, None, None, 1, None) != 0
    assert lib.rk_screen_rows(None, 1, None) != 0 and lib.rk_screen_counts(None, None, None, None) != 0 and lib.rk_screen_stats(None, None) != 0
    lib.rk_screen_destroy(None)
    s = c.screen([K], v, off)
    try:
        assert lib.rk_screen_add_batch(s._h, None, None, 1) != 0 and lib.rk_screen_add_batch_device(s._h, None, None, 1, None) != 0
        assert lib.rk_screen_rows(s._h, 1, None) != 0 and lib.rk_screen_rows_device(s._h, 1, None, None) != 0
        assert lib.rk_screen_counts(s._h, None, None, None) != 0 and lib.rk_screen_stats(s._h, None) != 0
        assert lib.rk_screen_add_counts(s._h, None, None, 1) != 0
        for m in (0, 1 << 32):
            with pytest.raises(rkmh_amd.RkmhError, match="min_copies"):
                s.rows(m)
        b, _ = sc.pack([b"ACGT" * 10, b"ACGT" * 10])
        with pytest.raises(rkmh_amd.RkmhError, match="decrease"):
            s.add(b, np.array([0, 40, 30], np.uint64))
        with pytest.raises(ValueError):
            s.add(b, np.array([0, 40, 4000], np.uint64))
        for vals, word in (([3, 2], "does not ascend"), ([2, 2], "does not ascend"), ([0, 2], "is 0")):
            with pytest.raises(rkmh_amd.RkmhError, match=word):
                s.add_counts(np.asarray(vals, np.uint64), np.asarray([1, 1], np.uint32))
        assert not s.counts()[1].any() and s.stats()["nkeys"] == 4 and s.stats()["nref"] == 2
    finally:
        s.close()


# ---- the command ----
def _run(root, *args, env=None):
    e = dict(os.environ)
    e.pop("RKMH_POLICY", None)
    e.update(env or {})
    r = subprocess.run([os.path.join(root, "bin", "rkmh")] + list(args), capture_output=True, env=e)
    assert r.returncode == 0, (args, r.stderr[-400:])
    return r.stdout.decode()


def test_cli_on_the_hpv_references(root, data_dir, tmp_path):
    import gzip
    import json
    from rkmh_amd import api, synth
    fa = os.path.join(data_dir, "all_pave_ref.fa.gz")
    text = gzip.open(os.path.join(data_dir, "minION25.fq.gz")).read()
    fq, bz = str(tmp_path / "reads.fq"), str(tmp_path / "reads.bgzf.fq.gz")
    open(fq, "wb").write(text)
    open(bz, "wb").write(synth.bgzf_compress(text, level=6, block=20000))
    opts = ["-k", "21", "-s", "1000", "--hash-policy", "mash"]
    rj = str(tmp_path / "refs.json")
    _run(root, "sketch", "-f", fa, "-o", rj, *opts)
    doc = json.load(open(rj))
    names = [d["name"] for d in doc]
    rows = [[int(x) for x in d["sketches"]["hashes"]] for d in doc]
    assert len(rows) == 182 and all(len(r) == 1000 for r in rows)
    reads = api.parse_files([fq])
    seqs = [bytes(reads["bases"][int(reads["offsets"][i]):int(reads["offsets"][i + 1])]) for i in range(reads["nseq"])]
    assert len(seqs) == 25
    counts = scm.counted(seqs, (21,), sm.MASH)
    lens = [len(scm.collapse(r)) for r in rows]

    def want(path, m, owned, min_shared=1, min_identity=0.0):
        out = []
        for i, r in enumerate(scm.rows(rows, counts, m)):
            sh, med = (r[2], r[3]) if owned else (r[0], r[1])
            if sh >= min_shared and scm.identity(sh, lens[i], 21) >= min_identity:
                out.append(scm.line(sh, lens[i], med, 21, names[i], path))
        return "".join(out)

    small = {"RKMH_RAW_BLOCK_KB": "64"}                                            # several blocks through the slots
    for m, w, env in ((1, [], None), (1, ["-w"], None), (2, ["-w"], small)):
        got = _run(root, "screen", "-r", fa, "-f", fq, "--min-copies", str(m), *w, *opts, env=env)
        assert got == want(fq, m, bool(w)) and (got or m == 2), (m, w)
    for m, w in ((2, []), (1, ["-w"])):                                            # the bgzip'd file: the same bytes but for its name
        assert _run(root, "screen", "-r", fa, "-f", bz, "--min-copies", str(m), *w, *opts) == want(bz, m, bool(w)), (m, w, "bgzf")
    assert len(want(fq, 1, False).splitlines()) > len(want(fq, 1, True).splitlines()) > 0
    # -R, two files in command-line order, the thresholds
    two = _run(root, "screen", "-R", rj, "-f", bz, "-f", fq, "--min-shared", "5", "--min-identity", "0.8", "--hash-policy", "mash")
    assert two == want(bz, 1, False, 5, 0.8) + want(fq, 1, False, 5, 0.8)
