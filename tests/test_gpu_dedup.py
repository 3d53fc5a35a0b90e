"""dedup=distinct (policy U6) on the device, bit for bit against tests/dedup_model.py: the distinct bottom-S of k_sort_intersect
(in-LDS compaction, the de-duplication pass in front of the block pre-select and of the multi-block select), reference sketches,
rows of the DEDUP forms of k_classify_tile and of the general path behind them, one -M run, both command lines.  Inputs and their
non-vacuity conditions: tests/dedup_cases.py (checked without a GPU by tests/test_policy_dedup_cpu.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dedup_cases as dc  # noqa: E402
import dedup_model as dm  # noqa: E402
import sourmash_model as sm  # noqa: E402

pytestmark = pytest.mark.gpu

SOURMASH_TEXT = "fold=h1,windows=len-k+1,zero=count,mask=lt,freqmax=incl,canon=lexmin,dedup=distinct,seed=42"


@pytest.fixture(scope="module")
def arrays():
    a = dc.raw_arrays()
    dc.raw_conditions(a)
    return a


@pytest.fixture(scope="module")
def ctx():
    import rkmh_amd
    c = rkmh_amd.Context(0, policy_spec="sourmash")
    yield c
    c.close()


# ---- raw hash arrays ----
def test_minhashes_distinct(ctx, arrays):
    for name, (h, S) in arrays.items():
        got, back = ctx.minhashes(h, S)
        assert got.tolist() == dm.bottom_distinct(h, S).tolist(), name
        assert back.tolist() == np.sort(h).tolist(), name           # the caller's array comes back sorted, every copy in it


def test_minhashes_multiset_is_untouched(arrays):
    import rkmh_amd
    c = rkmh_amd.Context(0, policy_spec="mash,canon=lexmin")
    try:
        for name, (h, S) in arrays.items():
            assert c.minhashes(h, S)[0].tolist() == sm.bottom(h, S).tolist(), name
    finally:
        c.close()


def test_minhashes_frequency_filter_distinct(ctx, arrays):
    """The same arrays through rk_minhashes_frequency_filter, with a depth table that removes the smallest value."""
    import torch
    from rkmh_amd import api
    removed = 0
    for name, (h, S) in arrays.items():
        counter = dc.filter_counter(h)
        table = torch.from_numpy(np.concatenate([counter, np.zeros(4, dtype=np.int32)])).cuda()
        cnt = api.Counter(ctx, len(counter), device_ptr=table.data_ptr())
        try:
            got, _ = ctx.minhashes(h, S, counter=cnt, min_count=1, max_count=1)
        finally:
            cnt.destroy()
        want = dm.bottom_distinct(dm.frequency_filter(h, counter, 1, 1), S)
        assert got.tolist() == want.tolist(), name
        plain = dm.bottom_distinct(h, S)
        removed += len(plain) > 0 and (len(want) == 0 or want[0] != plain[0])
    assert removed >= len(arrays) - 4          # the table really removes the smallest value


# ---- reference sketches ----
@pytest.mark.parametrize("spec", [s for s, _ in dc.SPECS])
def test_reference_sketches(spec, data_dir):
    import rkmh_amd
    from rkmh_amd import api
    pol = dict(dc.SPECS)[spec]
    refs = dc.references()
    Z = api.parse_files([os.path.join(data_dir, "zika.refs.fa.gz")])
    zb = Z["bases"].tobytes()
    zika = [zb[int(Z["offsets"][i]):int(Z["offsets"][i + 1])] for i in range(min(4, len(Z["offsets"]) - 1))]
    c = rkmh_amd.Context(0, policy_spec=spec)
    try:
        for seqs, S in ((refs, dc.S_SEQ), (refs, 16), (zika, dc.S_SEQ)):
            rb, ro = dc.pack(seqs)
            c.set_references(rb, ro, [16], S)
            assert not c.kmer_form()[0]                       # dedup=distinct classifies through k_classify_tile
            sk, ln = c.get_reference_sketches()
            want = dm.sketch_refs(seqs, [16], S, pol)
            assert ln.tolist() == [len(x) for x in want]
            for j, x in enumerate(want):
                assert sk[j, :len(x)].tolist() == x.tolist() and (sk[j, len(x):] == 0).all(), j
            got, lens = c.sketch_batch(rb, ro, [16], S)
            assert lens.tolist() == ln.tolist() and (got == sk).all()
    finally:
        c.close()


# ---- rows ----
def _device_rows(c, qb, qo):
    import torch
    n = len(qo) - 1
    d_b = torch.from_numpy(qb).cuda()
    d_o = torch.from_numpy(qo.astype(np.int64)).to(torch.int32).cuda()
    d_out = torch.full((max(n, 1), 4), -7, dtype=torch.int32, device="cuda")
    c.classify_device(d_b.data_ptr(), d_o.data_ptr(), n, d_out.data_ptr(), max_read_len=0, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()[:n]


@pytest.mark.parametrize("k", dc.ROW_K)
@pytest.mark.parametrize("spec", [s for s, _ in dc.SPECS])
def test_rows(spec, k):
    import rkmh_amd
    pol = dict(dc.SPECS)[spec]
    reads, kinds, want, _ = dc.row_conditions(k, pol)
    refs = dc.references()
    rb, ro = dc.pack(refs)
    qb, qo = dc.pack(reads)
    c = rkmh_amd.Context(0, policy_spec=spec)
    try:
        c.set_references(rb, ro, [k], dc.S_SEQ)
        got = c.classify(qb, qo)
        dev = _device_rows(c, qb, qo)
    finally:
        c.close()
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (bad[:5], [kinds[i] for i in bad[:5]], got[bad[:5]], want[bad[:5]])
    flagged = dev[:, 0] == -2
    bad = np.nonzero(~flagged & (dev != want).any(axis=1))[0]
    assert len(bad) == 0, (bad[:5], [kinds[i] for i in bad[:5]], dev[bad[:5]], want[bad[:5]])
    wrong = [i for i in np.nonzero(flagged)[0] if not dc.flag_allowed(reads[i], k, pol)]
    assert not wrong, (wrong[:5], [kinds[i] for i in wrong[:5]])
    # the kernel's own rows: reads with more windows than S whose distinct hashes fit, 256 and 257 windows among them
    own = [i for i in np.nonzero(~flagged)[0] if len(sm.window_hashes(reads[i], k, pol)) > dc.S_SEQ]
    assert len(own) >= 8


def test_depth_mask_distinct():
    """One -M 2 run: the count pass counts windows as before, the mask comes before the distinct selection; exact and bounded field 3."""
    import rkmh_amd
    from rkmh_amd import api
    k, pol = 16, dm.SOURMASH
    reads, _, plain, _ = dc.row_conditions(k, pol)
    refs = dc.references()
    slots = 100003
    counter = sm.count_hashes(reads, [k], slots, pol)
    sk = dm.sketch_refs(refs, [k], dc.S_SEQ, pol)
    want = dm.classify(reads, sk, [k], dc.S_SEQ, pol, counter=counter, min_occ=2)
    assert (want[:, 3] < plain[:, 3]).sum() >= 30 and (want[:, 1] < plain[:, 1]).any()
    rb, ro = dc.pack(refs)
    qb, qo = dc.pack(reads)
    c = rkmh_amd.Context(0, policy_spec="sourmash")
    try:
        c.set_references(rb, ro, [k], dc.S_SEQ)
        cnt = api.Counter(c, slots)
        c.count_batch(qb, qo, cnt)
        h = sm.calc_hashes(reads[20], [k], pol)
        assert len(np.unique(h)) < len(h) and all(cnt.get(int(x)) == counter[int(x % np.uint64(slots))] for x in h)   # windows, not distinct values
        c.set_depth_filter(cnt, 2)
        got = c.classify(qb, qo)
        assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:5]
        for bound in (3, 0):
            c.set_min_num_bound(bound)
            got = c.classify(qb, qo)
            capped = dm.classify(reads, sk, [k], dc.S_SEQ, pol, counter=counter, min_occ=2, bound=bound)
            assert (got == capped).all(), (bound, np.nonzero((got != capped).any(axis=1))[0][:5])
    finally:
        c.close()


def test_general_path_long_reads(data_dir):
    """Nanopore reads (thousands of windows: the block pre-select behind the de-duplication pass) against HPV16, S = 64."""
    from rkmh_amd import api
    import rkmh_amd
    R = api.parse_files([os.path.join(data_dir, "hpv_16.fa.gz")])
    Q = api.parse_files([os.path.join(data_dir, "minION25.fq.gz")])
    seqs = lambda P: [P["bases"].tobytes()[int(P["offsets"][i]):int(P["offsets"][i + 1])] for i in range(len(P["offsets"]) - 1)]  # noqa: E731
    refs, reads = seqs(R), seqs(Q)[:12] + [b"ACGTTGCA" * 700, b"AC" * 3000]
    qb, qo = dc.pack(reads)
    want = dm.classify(reads, dm.sketch_refs(refs, [12], dc.S_SEQ, dm.SOURMASH), [12], dc.S_SEQ, dm.SOURMASH)
    assert want[-1, 3] < 4 and want[-2, 3] <= 8
    c = rkmh_amd.Context(0, policy_spec="sourmash")
    try:
        c.set_references(R["bases"], R["offsets"], [12], dc.S_SEQ)
        got = c.classify(qb, qo)
    finally:
        c.close()
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:5]


# ---- the command lines ----
def _write(tmp_path, name, records, fastq):
    p = tmp_path / name
    with open(p, "wb") as f:
        for i, s in enumerate(records):
            f.write((b"@r%d\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n") if fastq else (b">ref%d\n" % i + s + b"\n"))
    return str(p)


def test_command_lines_sourmash(orc, root, tmp_path):
    exe = os.path.join(root, "bin", "rkmh")
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    k, S, pol = 16, dc.S_SEQ, dm.SOURMASH
    reads, _, rows, multi = dc.row_conditions(k, pol)
    keep = [i for i, r in enumerate(reads) if len(r) > 0]           # (a FASTQ record needs a sequence line)
    reads, rows, multi = [reads[i] for i in keep], rows[keep], multi[keep]
    refs = dc.references()
    fa, fq = _write(tmp_path, "refs.fa", refs, False), _write(tmp_path, "reads.fq", reads, True)
    want = "".join("ref%d\tr%d\t%d\t%d\t\t%s\n" % (mi, i, ms, S, "" if d > 0 else "FAIL:DIFF") for i, (mi, ms, d, n) in enumerate(rows.tolist()))
    common = ["-r", fa, "-f", fq, "-k", str(k), "-s", str(S)]
    for cmd in ([exe], [sys.executable, "-m", "rkmh_amd.cli"]):
        r = subprocess.run(cmd + ["stream"] + common + ["--hash-policy", "sourmash"], capture_output=True, env=env, cwd=root)
        assert r.returncode == 0, r.stderr
        assert r.stdout.decode() == want, cmd
        for flags, mm, md in ((["-N", "2", "-D", "1"], 2, 1), (["-N", "5"], 5, 0)):
            parts = [orc.filter_record(b"r%d" % i, sm.to_upper(reads[i]), b"I" * len(reads[i])) for i in range(len(reads))
                     if orc.filter_decision(rows[i], mm, md)[3]]
            other = [i for i in range(len(reads)) if orc.filter_decision(multi[i], mm, md)[3] != orc.filter_decision(rows[i], mm, md)[3]]
            assert 0 < len(parts) < len(reads) and other, flags       # the multiset rule lets other reads pass
            r = subprocess.run(cmd + ["filter"] + common + ["--hash-policy", "sourmash"] + flags, capture_output=True, env=env, cwd=root)
            assert r.returncode == 0, r.stderr
            assert r.stdout == b"".join(parts), (cmd, flags)
    # hash: every window's hash, copies included (the key acts on sketches)
    r = subprocess.run([exe, "hash", "-f", fa, "-k", str(k), "--hash-policy", "sourmash"], capture_output=True, env=env)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.decode().rstrip("\n").split("\n")
    assert len(lines) == len(refs)
    for line, s in zip(lines, refs):
        assert [int(x) for x in line.split("\t")[1:]] == sm.window_hashes(s, k, pol).tolist()
    # sketch records the text; stream -R refuses a sketch of the other rule, both ways round
    js, jm = str(tmp_path / "distinct.json"), str(tmp_path / "multiset.json")
    for path, spec in ((js, "sourmash"), (jm, "mash,canon=lexmin")):
        r = subprocess.run([exe, "sketch", "-f", fa, "-k", str(k), "-s", str(S), "-o", path, "--hash-policy", spec], capture_output=True, env=env)
        assert r.returncode == 0, r.stderr
    doc = json.load(open(js))
    assert doc[0]["hashPolicy"] == SOURMASH_TEXT
    assert "dedup" not in json.load(open(jm))[0]["hashPolicy"]
    r = subprocess.run([exe, "stream", "-R", jm, "-f", fq, "--hash-policy", "sourmash"], capture_output=True, env=env)
    assert r.returncode == 1 and r.stdout == b"", r.stderr
    r = subprocess.run([exe, "stream", "-R", js, "-f", fq, "--hash-policy", "mash,canon=lexmin"], capture_output=True, env=env)
    assert r.returncode == 1 and r.stdout == b"" and SOURMASH_TEXT.encode() in r.stderr
    r = subprocess.run([exe, "stream", "-R", js, "-f", fq, "--hash-policy", "sourmash"], capture_output=True, env=env)
    assert r.returncode == 0, r.stderr
    assert r.stdout.decode() == want
    # a k-mer cache written under the multiset rule is not reused: the distinct rule keeps no k-mer-space structures
    cache = str(tmp_path / "k16.rkkc")
    r = subprocess.run([exe, "stream"] + common + ["--hash-policy", "mash,canon=lexmin", "--kmer-cache", cache], capture_output=True, env=env)
    assert r.returncode == 0 and os.path.exists(cache), r.stderr
    before = open(cache, "rb").read()
    r = subprocess.run([exe, "stream"] + common + ["--hash-policy", "sourmash", "--kmer-cache", cache], capture_output=True, env=env)
    assert r.returncode == 0 and r.stdout.decode() == want and open(cache, "rb").read() == before
