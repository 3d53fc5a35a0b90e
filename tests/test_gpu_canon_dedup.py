"""canon=lexmin (policy U2) on the device, bit-exact against the pure-Python model of tests/sourmash_model.py (integers: no
tolerance) -- every hashing form: the inner-ABI hashes, reference sketches, classification rows of the k-mer-space kernel
(k <= 16), its wide form (k = 17 .. 20), the hash-space kernels and the general path, the -M count / mask passes, `call`, the
cache tags, and both command lines.  (dedup=, the second key the file is named after, does not exist yet.)

Every classification input first shows, on the model's output, that the two strand rules really differ on it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sourmash_model as sm  # noqa: E402

pytestmark = pytest.mark.gpu

LEXMIN = "mash,canon=lexmin"
LEXMIN_POL = sm.LEXMIN
MESSY = (b"ACGTTGCAAGGCTTAACCGGTTAACGATCGATCGGCTAGCTAGGATCCGATTACAGATTACAcgtagctagctagcatcgatcgatgcatgcNACGTAGCTAGCTAGCTAGGATCGATCGAT"
         b"CGATRYACGATCGATCGACTAGCTAGCATCGACTGACTAGCTACGATCGACTAGCTAGCTAGCTAGCTAGCATCGATCGATCAGCTACGACTAGCATCGACTGCATGCATGCATGCAAAA"
         b"AAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAATTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTT"
         b"TTTTTTTTTTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTnACGTGCATGCATCGATCGTAGCTAGCTAGCTAGCTGATCGATCGTAG")


def _spec(fold, drop, canon):
    return "fold=%s,windows=%s,canon=%s" % (("swap32", "h1", "w2w1")[fold], "len-k" if drop else "len-k+1", "lexmin" if canon else "minhash")


def _seqs(bases, offsets):
    b = bases.tobytes() if hasattr(bases, "tobytes") else bytes(bases)
    return [b[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)]


def _differs(seqs, ks, pol):
    d = n = 0
    for s in seqs:
        for k in ks:
            a, b = sm.lexmin_differs(s, k, pol)
            d, n = d + a, n + b
    return d, n


def _classify_both(rb, ro, qb, qo, ks, S, spec=LEXMIN, pol=LEXMIN_POL, kmer_form=True, check_refs=True, want_kmer_form=None):
    """Rows of a context under `spec` and of the model under `pol` for every read; the guard first: on the model's hashes, at
    least a quarter of the valid windows of the first reads hash differently under canon=lexmin and canon=minhash."""
    import rkmh_amd
    reads = _seqs(qb, qo)
    d, n = _differs(reads[:100], ks, pol)
    assert n > 0 and 4 * d >= n, (d, n)
    refs = _seqs(rb, ro)
    want_sk = sm.sketch_refs(refs, ks, S, pol)
    want = sm.classify(reads, want_sk, ks, S, pol)
    c = rkmh_amd.Context(0, policy_spec=spec)
    try:
        c.set_kmer_form(kmer_form)
        c.set_references(rb, ro, ks, S)
        if want_kmer_form is not None:
            assert c.kmer_form()[0] == want_kmer_form      # the kernel family the case is meant for
        if check_refs:
            sk, ln = c.get_reference_sketches()
            assert ln.tolist() == [len(x) for x in want_sk]
            for j, x in enumerate(want_sk):
                assert (sk[j, :len(x)] == x).all(), j
        got = c.classify(qb, qo)
    finally:
        c.close()
    assert got.shape == want.shape                     # every read of the input is compared
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    return got, want_sk


@pytest.fixture(scope="module")
def panel(data_dir):
    from rkmh_amd import api
    return api.parse_files([os.path.join(data_dir, "all_pave_ref.fa.gz")])


# ---- 1. the inner ABI: rk_calc_hashes / rk_calc_hash ----
@pytest.mark.parametrize("canon", [0, 1])
def test_calc_hashes_every_form(canon):
    import rkmh_amd
    ks = [8, 11, 12, 15, 16, 17, 20, 21, 31, 32, 33, 48, 64]
    d, n = sm.lexmin_differs(MESSY, 16, sm.MASH)
    assert 4 * d >= n > 100
    for fold in (0, 1, 2):
        for drop in (0, 1):
            pol = dict(sm.DEFAULT, fold=fold, drop_last=drop, canon=canon)
            c = rkmh_amd.Context(0, policy_spec=_spec(fold, drop, canon))
            try:
                for k in ks:
                    assert c.calc_hashes(MESSY, [k]).tolist() == sm.window_hashes(MESSY, k, pol).tolist(), (fold, drop, k)
                    for i in (0, 57, 91, 96, 230, 400):   # single k-mers, lower case / N / IUPAC among them
                        assert c.calc_hash(MESSY[i:i + k]) == sm.kmer_hash(MESSY[i:i + k], pol), (fold, drop, k, i)
                assert c.calc_hashes(MESSY, [12, 16, 33]).tolist() == sm.calc_hashes(MESSY, [12, 16, 33], pol).tolist()
                h, ho = c.hash_batch(np.frombuffer(MESSY, dtype=np.uint8), np.array([0, 200, 200, 215, len(MESSY)], dtype=np.uint64), [16, 21])
                want = [sm.calc_hashes(MESSY[a:b], [16, 21], pol) for a, b in ((0, 200), (200, 200), (200, 215), (215, len(MESSY)))]
                assert h.tolist() == np.concatenate(want).tolist() and ho.tolist() == np.cumsum([0] + [len(x) for x in want]).tolist()
            finally:
                c.close()


def test_lexmin_known_answers_on_the_device(golden_dir):
    """The vectors of tests/golden/gen_lexmin_kat.py (an independent murmur, the published strand rule) through rk_calc_hash."""
    import rkmh_amd
    vec = json.load(open(os.path.join(golden_dir, "lexmin_kat.json")))["vectors"]
    c = rkmh_amd.Context(0, policy_spec=LEXMIN)
    try:
        for v in vec:
            assert c.calc_hash(v["kmer"].encode()) == v["h1"], v
            assert c.calc_hashes(v["kmer"].encode(), [v["k"]]).tolist() == [v["h1"]], v
    finally:
        c.close()


# ---- 3. reference sketches, 4. classification rows ----
@pytest.mark.parametrize("k,kmer_form", [(16, True), (16, False), (12, True), (18, True), (24, True)])
def test_classify_panel_lexmin(panel, k, kmer_form):
    """2 000 reads of the C2 generator against the 182-reference panel: k = 16 and 12 (k-mer-space kernel; k = 16 also with that
    form forbidden: the fused hash-space kernel), 18 (wide k-mers), 24 (hash space); reference sketches (S = 1000) included."""
    from rkmh_amd import synth
    rb, ro = panel["bases"], panel["offsets"]
    qb, qo = synth.generate_reads_fast(rb, ro, 0, 2000)
    got, _ = _classify_both(rb, ro, qb, qo, [k], 1000, kmer_form=kmer_form,
                            want_kmer_form={(16, True): True, (16, False): False, (12, True): True, (18, True): True, (24, True): False}.get((k, kmer_form)))
    assert (got[:, 1] > 0).mean() > 0.5


def test_classify_two_ks_lexmin(panel):
    from rkmh_amd import synth
    rb, ro = panel["bases"], panel["offsets"]
    qb, qo = synth.generate_reads_fast(rb, ro, 3000, 4000)
    _classify_both(rb, ro, qb, qo, [12, 16], 1000)


def test_classify_zika_and_minion_lexmin(data_dir):
    """z1.fq.gz against the zika references (tie-heavy) and the nanopore reads against HPV16 at k = 12, S = 1000 (long reads: the
    general path), default fold and windows as well as the mash ones."""
    from rkmh_amd import api
    for refs, reads, k in (("zika.refs.fa.gz", "z1.fq.gz", 16), ("hpv_16.fa.gz", "minION25.fq.gz", 12)):
        R = api.parse_files([os.path.join(data_dir, refs)])
        Q = api.parse_files([os.path.join(data_dir, reads)])
        _classify_both(R["bases"], R["offsets"], Q["bases"], Q["offsets"], [k], 1000)
        _classify_both(R["bases"], R["offsets"], Q["bases"], Q["offsets"], [k], 1000, spec="canon=lexmin", pol=dict(sm.DEFAULT, canon=1))


def test_tandem_repeat_reference_and_low_complexity_reads(panel):
    """A hand-made reference with a tandem repeat next to panel genomes, and 150-bp low-complexity reads -- (AC)n, (ACGTTGCA)n,
    homopolymer runs with one N -- mixed into a normal tile."""
    from rkmh_amd import synth
    rng = np.random.default_rng(11)
    unit = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 37).tolist())
    flank = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 600).tolist())
    refs = _seqs(panel["bases"], panel["offsets"])[:20] + [flank[:300] + unit * 40 + flank[300:]]
    want_dup = sm.bottom(sm.calc_hashes(refs[-1], [16], LEXMIN_POL), 1000)
    assert len(np.unique(want_dup)) < len(want_dup)          # the repeat really puts repeated values into the sketch
    rb = np.frombuffer(b"".join(refs), dtype=np.uint8).copy()
    ro = np.cumsum([0] + [len(r) for r in refs]).astype(np.uint64)
    qb, qo = synth.generate_reads_fast(rb, ro, 0, 500)
    reads = _seqs(qb, qo)
    low = [(b"AC" * 75), (b"ACGTTGCA" * 19)[:150], b"A" * 80 + b"N" + b"A" * 69, b"T" * 30 + b"N" + b"G" * 119, (unit * 5)[:150]]
    reads = reads[:250] + low + reads[250:]
    qb = np.frombuffer(b"".join(reads), dtype=np.uint8).copy()
    qo = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)
    _classify_both(rb, ro, qb, qo, [16], 1000)


def test_depth_mask_lexmin(panel):
    """One -M 2 run: the count pass and the mask hash by the same strand rule (slots = h % slots of the lexmin hash)."""
    import rkmh_amd
    from rkmh_amd import api, synth
    rb, ro = panel["bases"], panel["offsets"]
    qb, qo = synth.generate_reads_fast(rb, ro, 0, 1500)
    reads, refs = _seqs(qb, qo), _seqs(rb, ro)
    slots = 1000003
    counter = sm.count_hashes(reads, [16], slots, LEXMIN_POL)
    want_sk = sm.sketch_refs(refs, [16], 1000, LEXMIN_POL)
    want = sm.classify(reads, want_sk, [16], 1000, LEXMIN_POL, counter=counter, min_occ=2)
    plain = sm.classify(reads, want_sk, [16], 1000, LEXMIN_POL)
    assert (want[:, 3] < plain[:, 3]).sum() >= 100 and (want[:, 1] < plain[:, 1]).any()   # the mask removes hashes of these very reads
    c = rkmh_amd.Context(0, policy_spec=LEXMIN)
    try:
        c.set_references(rb, ro, [16], 1000)
        cnt = api.Counter(c, slots)
        c.count_batch(qb, qo, cnt)
        for h in sm.calc_hashes(reads[0], [16], LEXMIN_POL).tolist() + sm.calc_hashes(reads[-1], [16], LEXMIN_POL).tolist():
            assert cnt.get(h) == counter[h % slots], h
        c.set_depth_filter(cnt, 2)
        got = c.classify(qb, qo)
    finally:
        c.close()
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:5]


# ---- 5. the command lines ----
def _stream_lines(ref_names, read_names, rows, S):
    out = []
    for name, (mi, ms, d, n) in zip(read_names, rows.tolist()):
        out.append("%s\t%s\t%d\t%d%s\t%s\t%s\n" % (ref_names[mi].decode(), name.decode(), ms, S, "FAIL:DEPTH" if n <= -1 else "",
                                                  "FAIL:MATCHES" if ms < -1 else "", "" if d > 0 else "FAIL:DIFF"))
    return "".join(out)


def test_cli_lexmin(root, data_dir, tmp_path):
    from rkmh_amd import api
    exe = os.path.join(root, "bin", "rkmh")
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    zr, zq = os.path.join(data_dir, "zika.refs.fa.gz"), os.path.join(data_dir, "z1.fq.gz")
    R, Q = api.parse_files([zr]), api.parse_files([zq])
    refs, reads = _seqs(R["bases"], R["offsets"]), _seqs(Q["bases"], Q["offsets"])
    d, n = _differs(reads[:100], [16], LEXMIN_POL)
    assert 4 * d >= n > 0
    sk = sm.sketch_refs(refs, [16], 1000, LEXMIN_POL)
    want = _stream_lines(R["names"], Q["names"], sm.classify(reads, sk, [16], 1000, LEXMIN_POL), 1000)
    for cmd in ([exe, "stream"], [sys.executable, "-m", "rkmh_amd.cli", "stream"]):
        r = subprocess.run(cmd + ["-r", zr, "-f", zq, "-k", "16", "-s", "1000", "--hash-policy", LEXMIN], capture_output=True, env=env, cwd=root)
        assert r.returncode == 0, r.stderr
        assert r.stdout.decode() == want, cmd
    r = subprocess.run([exe, "stream", "-r", zr, "-f", zq, "-k", "16", "-s", "1000"], capture_output=True, env=dict(env, RKMH_POLICY=LEXMIN))
    assert r.returncode == 0 and r.stdout.decode() == want
    # hash: name, then every k-mer hash
    hp = os.path.join(data_dir, "hpv_16.fa.gz")
    H = api.parse_files([hp])
    r = subprocess.run([exe, "hash", "-f", hp, "-k", "12", "--hash-policy", LEXMIN], capture_output=True, env=env)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.decode().rstrip("\n").split("\n")
    seqs = _seqs(H["bases"], H["offsets"])
    assert len(lines) == len(seqs)
    for line, s in zip(lines, seqs):
        assert [int(x) for x in line.split("\t")[1:]] == sm.window_hashes(s, 12, LEXMIN_POL).tolist()
    # sketch records the extended text, "canonical" stays "true"; stream -R refuses another strand rule and takes the same one
    js = tmp_path / "lexmin.json"
    r = subprocess.run([exe, "sketch", "-f", zr, "-k", "16", "-s", "1000", "-o", str(js), "--hash-policy", LEXMIN], capture_output=True, env=env)
    assert r.returncode == 0, r.stderr
    doc = json.load(open(js))
    text = "fold=h1,windows=len-k+1,zero=count,mask=lt,freqmax=incl,canon=lexmin,seed=42"
    assert doc[0]["hashPolicy"] == text and doc[0]["canonical"] == "true"
    r = subprocess.run([exe, "stream", "-R", str(js), "-f", zq, "--hash-policy", "mash"], capture_output=True, env=env)
    assert r.returncode == 1 and r.stdout == b"" and ("--hash-policy " + text).encode() in r.stderr
    r = subprocess.run([exe, "stream", "-R", str(js), "-f", zq, "--hash-policy", LEXMIN], capture_output=True, env=env)
    assert r.returncode == 0, r.stderr
    assert r.stdout.decode() == want


def test_cli_filter_lexmin(orc, root, data_dir):
    """bin/rkmh filter and rkmh_amd.cli filter under canon=lexmin: the reads the model's rows let pass (the oracle module only
    lends its statement of the decision rule and of the record format; the rows are the model's)."""
    from rkmh_amd import api
    exe = os.path.join(root, "bin", "rkmh")
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    zr, zq = os.path.join(data_dir, "zika.refs.fa.gz"), os.path.join(data_dir, "z1.fq.gz")
    R, Q = api.parse_files([zr]), api.parse_files([zq])
    refs, reads = _seqs(R["bases"], R["offsets"]), _seqs(Q["bases"], Q["offsets"])
    sk = sm.sketch_refs(refs, [16], 1000, LEXMIN_POL)
    rows = sm.classify(reads, sk, [16], 1000, LEXMIN_POL)
    for flags, mm, md in (([], -1, 0), (["-N", "2", "-D", "1"], 2, 1), (["-N", "5"], 5, 0)):
        parts = [orc.filter_record(Q["names"][i], sm.to_upper(reads[i]), Q["quals"][i]) for i in range(len(reads))
                 if orc.filter_decision(rows[i], mm, md)[3]]
        assert 0 < len(parts) < len(reads), flags
        for cmd in ([exe, "filter"], [sys.executable, "-m", "rkmh_amd.cli", "filter"]):
            r = subprocess.run(cmd + ["-r", zr, "-f", zq, "-k", "16", "-s", "1000", "--hash-policy", LEXMIN] + flags, capture_output=True, env=env, cwd=root)
            assert r.returncode == 0, r.stderr
            assert r.stdout == b"".join(parts), (cmd, flags)
    minhash = sm.classify(reads, sm.sketch_refs(refs, [16], 1000, sm.MASH), [16], 1000, sm.MASH)
    assert (minhash != rows).any()              # the other strand rule gives other rows on this input


# ---- `call`: the candidate k-mers (canonical_bytes) and the depth pass hash by one rule ----
@pytest.mark.parametrize("k", [8, 16, 17, 31, 33, 64])
def test_call_records_do_not_depend_on_the_strand_rule(orc, k):
    """A record of `call` holds depths, never hashes, and the depth of a k-mer is the number of read windows holding it or its
    reverse complement -- whichever 64-bit value names that strand pair (the depth table is exact; distinct pairs share a value
    with probability 2^-64).  So under canon=lexmin the records must equal the oracle's records for canon=minhash, and they do only
    if the candidates built base by base (canonical_bytes) hash exactly as the read windows counted before (canonical_window):
    a candidate hashed by another rule finds depth 0 and its record vanishes."""
    import rkmh_amd
    import call_cases as cc
    case, want = cc.checked_oracle(orc, "ksweep_k%d" % k)          # the case's own non-vacuity check: there are records
    assert len(want) > 0
    rb, ro = orc.pack(case.ref_seqs)
    qb, qo = orc.pack(case.reads)
    pad = lambda b: np.concatenate([np.asarray(b, dtype=np.uint8), np.zeros(16, dtype=np.uint8)])  # noqa: E731
    p = case.policy
    spec = "fold=%s,windows=%s,seed=%d,canon=lexmin" % (("swap32", "h1", "w2w1")[p.get("fold", 0)],
                                                         "len-k" if p.get("drop_last_window", 1) else "len-k+1", p.get("seed", 42))
    d, n = _differs(case.reads, [k], dict(sm.DEFAULT, fold=p.get("fold", 0), drop_last=p.get("drop_last_window", 1)))
    assert 4 * d >= n > 0
    c = rkmh_amd.Context(0, policy_spec=spec)
    try:
        got = cc.device_records(c.call(pad(rb), ro, pad(qb), qo, case.k, case.w))
    finally:
        c.close()
    assert got == want, (len(got), len(want))


# ---- caches: a file made under one strand rule is neither reused nor accepted under the other ----
def test_kmer_cache_and_depth_map_tag_separate_the_strand_rules(panel, tmp_path):
    import rkmh_amd
    from rkmh_amd import api, synth
    rb, ro = panel["bases"], panel["offsets"]
    qb, qo = synth.generate_reads_fast(rb, ro, 0, 500)
    cache = str(tmp_path / "k18.rkkc")

    def run(spec, expect_state):
        c = rkmh_amd.Context(0, policy_spec=spec)
        try:
            c.set_kmer_cache(cache)
            c.set_references(rb, ro, [18], 1000)
            assert c.kmer_form()[0]
            assert c.kmer_cache_state() == expect_state, (spec, c.kmer_cache_state())
            return c.classify(qb, qo), c.depth_map_tag([18], qb, qo)
        finally:
            c.close()

    rows_m, tag_m = run("mash", 2)                      # no file: enumerated, written
    assert run("mash", 1)[0].tolist() == rows_m.tolist()    # loaded
    rows_l, tag_l = run(LEXMIN, 2)                      # the other strand rule: the file is not reused
    rows_l2, tag_l2 = run(LEXMIN, 1)
    assert rows_l2.tolist() == rows_l.tolist() and (rows_l != rows_m).any()
    run("mash", 2)
    assert tag_l == tag_l2 and tag_l != tag_m
    # a depth map saved under one rule is refused under the other, accepted under its own
    path = str(tmp_path / "depth.bin")
    c = rkmh_amd.Context(0, policy_spec="mash")
    try:
        c.set_references(rb, ro, [18], 1000)
        cnt = api.Counter(c, 100003)
        c.count_batch(qb, qo, cnt)
        cnt.save(path, tag_m)
        cnt.load(path, tag_m)
        with pytest.raises(api.RkmhError):
            cnt.load(path, tag_l)
    finally:
        c.close()
