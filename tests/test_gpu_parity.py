"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on the same inputs --
bit-exact hashes, sketches and per-read (max_id, max_shared, diff, min_num)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import _call_fixture, golden, rand_dna

pytestmark = pytest.mark.gpu


def _pad(b):
    out = np.zeros(len(b) + 16, dtype=np.uint8)
    out[: len(b)] = b
    return out


@pytest.fixture(scope="module")
def pave(orc, data_dir):
    recs = orc.kseq_parse_file(os.path.join(data_dir, "all_pave_ref.fa.gz"))
    rb, ro = orc.pack([r[1] for r in recs])
    return [r[0] for r in recs], _pad(rb), ro


def test_extension_is_loaded_from_tree():
    import rkmh_amd
    rkmh_amd.load_library()
    maps = open("/proc/self/maps").read()
    assert "rkmh_amd/lib/librkmh_amd.so" in maps


@pytest.mark.parametrize("fold", [0, 1, 2])
@pytest.mark.parametrize("drop", [0, 1])
def test_calc_hashes_bit_exact_all_policies(orc, fold, drop):
    import rkmh_amd
    c = rkmh_amd.Context(0, fold=fold, drop_last_window=drop)
    pol = orc.default_policy(fold=fold, drop_last_window=drop)
    rng = np.random.default_rng(100 + fold * 2 + drop)
    for k in (1, 3, 8, 12, 15, 16, 17, 20, 24, 31, 32, 33, 48, 64):
        for n in (0, k - 1, k, k + 1, 70, 257, 5000):
            if n < 0:
                continue
            s = rand_dna(rng, n, b"ACGTACGTACGTACGTacgtN")
            want = orc.calc_hashes(orc.to_upper(s), [k], pol)
            got = c.calc_hashes(s, [k])
            assert got.dtype == np.uint64 and len(got) == len(want)
            assert (got == want).all(), (k, n)
    c.close()


def test_calc_hash_single_kmer(ctx, orc):
    for kmer in (b"ACGTACGTACGT", b"ACGTACGTACGTACGT", b"GATTACAGATTACAGATTAC", b"ACGTNCGTACGTACGT", b"A", b"acgtacgtacgtacgt"):
        assert ctx.calc_hash(kmer) == orc.calc_hash(orc.to_upper(kmer))


def test_to_upper(ctx, orc):
    s = bytes(range(1, 128)) * 3
    assert ctx.to_upper(s) == orc.to_upper(s)


def test_multi_k_and_long_sequence_tiles(ctx, orc, pave):
    _, rb, ro = pave
    seq = bytes(rb[: int(ro[3])])  # ~23 kb: several 2048-window tiles, lower case + IUPAC
    for ks in ([16], [12, 16, 20], [31], [7, 33]):
        want = orc.calc_hashes(orc.to_upper(seq), ks)
        got = ctx.calc_hashes(seq, ks)
        assert (got == want).all(), ks


def test_unaligned_starts(ctx, orc):
    rng = np.random.default_rng(5)
    seqs = [rand_dna(rng, int(n), b"ACGTN" * 3 + b"ACGT" * 10) for n in rng.integers(0, 300, size=200)]
    bases, offs = orc.pack(seqs)
    h, ho = ctx.hash_batch(_pad(bases), offs, [16])
    for i, s in enumerate(seqs):
        assert (h[int(ho[i]): int(ho[i + 1])] == orc.calc_hashes(s, [16])).all(), i


def test_minhashes_and_intersection_mirrors(ctx, orc):
    rng = np.random.default_rng(9)
    for n, S in ((0, 10), (1, 10), (50, 10), (200, 1000), (3000, 1000), (16384, 2000)):
        h = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
        h[rng.random(n) < 0.1] = 0
        if n > 10:
            h[5] = h[6] = h[7]  # duplicates survive (no dedup)
        mins, srt = ctx.minhashes(h, S)
        assert (mins == orc.minhashes(h, S)).all()
        assert (srt == np.sort(h)).all()
    # inputs longer than the in-LDS sorter (the reference calls minhashes on whole references, rkmh.cpp:822): exact bottom S by
    # radix select, the caller's array back sorted ascending by a whole-array device sort
    for n, S, zero_frac, few in ((16385, 1000, 0.1, 0), (100000, 1000, 0.1, 0), (3000000, 2000, 0.3, 0), (50000, 1000, 1.0, 0),
                                 (70000, 1000, 0.0, 300), (200000, 16384, 0.05, 0)):
        h = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
        h[rng.random(n) < zero_frac] = 0
        if few:                      # fewer kept hashes than S: all of them
            h[few:] = 0
            rng.shuffle(h)
        h[1000:1040] = h[999]        # a run of duplicates (no dedup), possibly of the threshold value
        h[-1] = np.uint64((1 << 64) - 1)
        mins, srt = ctx.minhashes(h, S)
        want = orc.minhashes(h, S)
        assert len(mins) == len(want) and (mins == want).all(), (n, S)
        assert (srt == np.sort(h)).all(), (n, S)
    # minhashes_frequency_filter (rkmh.cpp:835-836) on a long input: the table is a torch tensor the counter wraps
    import torch
    import rkmh_amd
    slots = 100003
    hL = rng.integers(1, 1 << 40, size=60000, dtype=np.uint64)
    hL[rng.random(60000) < 0.05] = 0
    counts = np.bincount((hL % np.uint64(slots)).astype(np.int64), minlength=slots).astype(np.int32)
    counts[0] = 1 << 20
    t = torch.from_numpy(counts).cuda()
    cntL = rkmh_amd.Counter(ctx, slots=slots, device_ptr=t.data_ptr())
    for S, mx in ((1000, 1), (1000, 0), (5000, 2)):
        mins, srt = ctx.minhashes(hL, S, counter=cntL, min_count=0, max_count=mx)
        hs = np.sort(hL)
        want = hs[(hs != 0) & (counts[(hs % np.uint64(slots)).astype(np.int64)] <= mx)][:S]
        assert len(mins) == len(want) and (mins == want).all(), (S, mx)
        assert (srt == hs).all()
    cntL.destroy()
    a = np.sort(rng.integers(1, 500, size=300, dtype=np.uint64))
    b = np.sort(rng.integers(1, 500, size=1000, dtype=np.uint64))
    assert ctx.hash_intersection_size(a, b) == orc.hash_intersection_size(a, b)
    assert ctx.hash_intersection_size(np.array([0, 0, 5, 5, 5], np.uint64), np.array([0, 5, 5], np.uint64)) == 2
    assert ctx.hash_intersection_size(np.zeros(0, np.uint64), b) == 0
    # the materialising 7-argument form filter's helpers call (equiv.hpp:308,340,364)
    for a0, al, b0, bl, cap in ((0, 300, 0, 1000, 1000), (7, 200, 100, 600, 1000), (0, 300, 0, 1000, 5), (10, 0, 0, 1000, 10), (0, 300, 1000, 0, 10)):
        got = ctx.hash_intersection(a, a0, al, b, b0, bl, cap)
        assert (got == orc.hash_intersection(a, a0, al, b, b0, bl, cap)).all() and len(got) == len(orc.hash_intersection(a, a0, al, b, b0, bl, cap))
    big_a = np.sort(rng.integers(1, 3000, size=5000, dtype=np.uint64))
    big_b = np.sort(rng.integers(1, 3000, size=7000, dtype=np.uint64))
    got = ctx.hash_intersection(big_a, 0, 5000, big_b, 0, 7000, 5000)
    want = orc.hash_intersection(big_a, 0, 5000, big_b, 0, 7000, 5000)
    assert len(got) == len(want) == ctx.hash_intersection_size(big_a, big_b) and (got == want).all()
    z = ctx.hash_intersection(np.array([0, 0, 5, 5, 5], np.uint64), 0, 5, np.array([0, 5, 5], np.uint64), 0, 3, 10)
    assert list(z) == [5, 5]
    with pytest.raises(ValueError):
        ctx.hash_intersection(a, 0, 301, b, 0, 10, 10)


def test_counter_mirror(ctx, orc):
    import rkmh_amd
    cnt = rkmh_amd.Counter(ctx, slots=1009)
    s = b"ACGTTGCAAGGCTTAACCGGTTAAGGCCATATATATATATGCGCGCGC" * 3
    h = ctx.calc_hashes(s, [8], counter=cnt)
    want = {}
    for v in orc.calc_hashes(s, [8]):
        want[int(v) % 1009] = want.get(int(v) % 1009, 0) + 1
    for v in set(int(x) for x in h):
        assert cnt.get(v) == want[v % 1009]
    cnt.increment(12345)
    assert cnt.get(12345) == want.get(12345 % 1009, 0) + 1
    masked = ctx.mask_by_frequency(h, cnt, 4)
    assert (masked == np.array([v if cnt.get(int(v)) >= 4 else 0 for v in h], dtype=np.uint64)).all()
    mins, _ = ctx.minhashes(h, 20, counter=cnt, min_count=0, max_count=3)
    keep = np.array([v for v in np.sort(h) if v != 0 and cnt.get(int(v)) <= 3], dtype=np.uint64)[:20]
    assert (mins == keep).all()
    cnt.destroy()


def test_ref_sketches_bit_exact(ctx, orc, pave):
    _, rb, ro = pave
    for ks, S in (([16], 1000), ([12], 1000), ([20], 2000), ([12, 16], 500)):
        want_sk, want_ln = orc.sketch_refs(rb, ro, ks, S, threads=4)
        sk, ln = ctx.sketch_batch(rb, ro, ks, S)
        assert (ln == want_ln).all()
        assert (sk == want_sk).all()


def _classify_both(ctx, orc, rb, ro, qb, qo, ks, S, **kw):
    """The device's rows against the oracle's -- the oracle sketches the references ITSELF (a wrong device sketch cannot hide
    behind rows computed from it), and the device's sketches must equal the oracle's."""
    ctx.set_references(rb, ro, ks, S)
    sk, ln = ctx.get_reference_sketches()
    wsk, wln = orc.sketch_refs(rb, ro, ks, S, threads=8)
    assert (ln == wln).all() and (sk == wsk).all(), "reference sketches differ from the oracle's"
    want = orc.classify_stream(qb, qo, ks, S, wsk, wln, threads=8, **kw)
    got = ctx.classify(qb, qo)
    return got, want


@pytest.mark.parametrize("tag", ["c1_hpv16_minion25", "zika_z1", "c2mini_pave", "c2mini_pave_k12_k16"])
def test_classify_matches_golden_and_oracle(ctx, orc, golden_dir, data_dir, tag):
    from rkmh_amd import synth
    g = golden(golden_dir, tag)
    refs = orc.kseq_parse_file(os.path.join(data_dir, g["ref_file"]))
    rb, ro = orc.pack([r[1] for r in refs])
    rb = _pad(rb)
    rn = [r[0].decode() for r in refs]
    if "reads_file" in g:
        reads = orc.kseq_parse_file(os.path.join(data_dir, g["reads_file"]))
        qn = [r[0].decode() for r in reads]
        qb, qo = orc.pack([r[1] for r in reads])
        qb = _pad(qb)
    else:
        qb, qo = synth.generate_reads(rb, ro, 0, 1000)
        qn = [n.decode() for n in synth.read_names(0, 1000)]
    got, want = _classify_both(ctx, orc, rb, ro, qb, qo, g["ks"], g["sketch_size"])
    assert (got == want).all()
    rows = [[qn[i], rn[got[i, 0]], int(got[i, 1]), int(got[i, 2]), int(got[i, 3])] for i in range(len(qn))]
    assert rows == g["rows"]


def test_depth_filter_path_matches_golden(ctx, orc, golden_dir, pave):
    import rkmh_amd
    from rkmh_amd import synth
    g = golden(golden_dir, "c2mini_pave_M2")
    rn, rb, ro = pave
    qb, qo = synth.generate_reads(rb, ro, 0, 1000)
    ctx.set_references(rb, ro, g["ks"], g["sketch_size"])
    cnt = rkmh_amd.Counter(ctx, slots=g["kwargs"]["counter_slots"])
    ctx.count_batch(qb, qo, cnt)
    ctx.set_depth_filter(cnt, g["kwargs"]["min_kmer_occ"])
    try:
        got = ctx.classify(qb, qo)
    finally:
        ctx.set_depth_filter(None, 0)
    rows = [[int(got[i, 1]), int(got[i, 2]), int(got[i, 3])] for i in range(1000)]
    assert rows == [r[2:] for r in g["rows"]]
    assert [rn[got[i, 0]].decode() for i in range(1000)] == [r[1] for r in g["rows"]]
    cnt.destroy()


def test_max_samples_reference_path(ctx, orc, pave):
    _, rb, ro = pave
    n = 40
    ctx.set_references(rb, ro[: n + 1], [16], 1000, max_samples=1, counter_slots=5000011)
    sk, ln = ctx.get_reference_sketches()
    wsk, wln = orc.sketch_refs(rb, ro[: n + 1], [16], 1000, threads=4, max_samples=1, counter_slots=5000011)
    assert (ln == wln).all() and (sk == wsk).all()


def test_edge_cases(ctx, orc):
    rng = np.random.default_rng(21)
    refs = [rand_dna(rng, 600) for _ in range(5)]
    refs.append(refs[1])                     # exact duplicate reference -> ties, first wins
    refs.append(b"A" * 300)                  # homopolymer: one hash repeated (multiset semantics)
    reads = [
        b"", b"ACGT", refs[0][:16], refs[0][:17], refs[1][100:250], refs[2][5:155].lower(),
        b"N" * 150, refs[3][:70] + b"N" + refs[3][71:150], b"A" * 150, b"A" * 40, refs[4][:1024], refs[4][:600],
        rand_dna(rng, 150), (refs[0][:100] + refs[2][:100]), b"ACGT" * 40,
    ]
    rb, ro = orc.pack(refs)
    qb, qo = orc.pack(reads)
    for ks, S in (([16], 1000), ([16], 50), ([12], 1000), ([8, 16], 100), ([16], 1)):
        got, want = _classify_both(ctx, orc, _pad(rb), ro, _pad(qb), qo, ks, S)
        assert (got == want).all(), (ks, S, got, want)


def test_long_reads_take_general_path(ctx, orc, pave):
    """Reads longer than the fused kernel's limit and sketches smaller than the read (bottom-S matters)."""
    _, rb, ro = pave
    rng = np.random.default_rng(4)
    reads = []
    for i in range(40):
        r = int(rng.integers(0, 182))
        L = int(rng.integers(200, 6000))
        st = int(rng.integers(0, int(ro[r + 1] - ro[r]) - L))
        reads.append(bytes(rb[int(ro[r]) + st: int(ro[r]) + st + L]))
    reads += [reads[0][:150], reads[1][:100]]  # mixed with fused-eligible ones
    qb, qo = orc.pack(reads)
    got, want = _classify_both(ctx, orc, rb, ro, _pad(qb), qo, [16], 1000)
    assert (got == want).all()
    got, want = _classify_both(ctx, orc, rb, ro, _pad(qb), qo, [16], 64)  # S < windows even for 150 bp reads
    assert (got == want).all()
    # the complete resident entry point: same batch living in HBM, nothing left flagged
    import torch
    for S in (1000, 64):
        got, want = _classify_both(ctx, orc, rb, ro, _pad(qb), qo, [16], S)
        n = len(reads)
        d_b = torch.from_numpy(_pad(qb)).cuda()
        d_o = torch.from_numpy(qo.astype(np.int64)).to(torch.int32).cuda()
        d_out = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        ctx.classify_device_all(d_b.data_ptr(), d_o.data_ptr(), n, d_out.data_ptr(), max_read_len=0,
                                stream=torch.cuda.current_stream().cuda_stream)
        assert (d_out.cpu().numpy() == want).all(), S


def test_bottom_s_preselection_with_duplicate_heavy_sequences(ctx, orc):
    """The in-block radix pre-selection (sequences with more hashes than the sketch keeps) on multisets that stress
    it: one hash repeated thousands of times (homopolymer: the threshold bucket never shrinks, all 64 bits get
    decided), short tandem repeats (a handful of distinct hashes, each hundreds of times), N runs, mixed with random
    sequence; as references (sketches) and as reads (classification), for sketch sizes around the bucket limits."""
    rng = np.random.default_rng(77)
    base = rand_dna(rng, 9000)
    seqs = [
        b"A" * 5000,                                   # one hash, 4984 copies
        b"AC" * 2500,                                  # two hashes
        b"ACG" * 1700, b"ACGTT" * 1100,                # 3 / 5 distinct hashes
        b"A" * 3000 + base[:3000],                     # duplicates below/above random hashes
        base[:4000] + b"N" * 700 + base[4000:7000],    # zero hashes in the middle
        (b"ACGTTGCAAC" * 30 + base[:200]) * 12,        # repeats mixed with unique stretches
        base, base[:2100], base[:1100], base[::-1][:3333],
    ]
    rb, ro = orc.pack(seqs)
    reads = seqs + [base[100:250], b"A" * 150, base[500:1650]]
    qb, qo = orc.pack(reads)
    for ks, S in (([16], 1000), ([16], 1), ([16], 7), ([16], 300), ([16], 1024), ([16], 2000), ([12], 1000), ([8, 16], 1500)):
        ctx.set_references(_pad(rb), ro, ks, S)
        sk, ln = ctx.get_reference_sketches()
        wsk, wln = orc.sketch_refs(rb, ro, ks, S)
        assert (ln == wln).all() and (sk == wsk).all(), (ks, S)
        got, want = _classify_both(ctx, orc, _pad(rb), ro, _pad(qb), qo, ks, S)
        assert (got == want).all(), (ks, S, got, want)


def test_c3_like_all_bundled_references(ctx, orc, data_dir):
    """SURVEY 8(d) C3 in miniature: every bundled FASTA concatenated (~270 viral references, many of them near
    duplicates of each other => ties and two-posting index values) against synthetic 150 bp reads, k=16, s=1000,
    through the host entry point and the resident one, plus a batch mixing short and long reads."""
    import torch
    from rkmh_amd import synth
    seqs = []
    for f in ("all_pave_ref.fa.gz", "zika.refs.fa.gz", "dengue.fa.gz", "new_refs.fa.gz", "hpv_16.fa.gz",
              "zika.fa.gz", "yellow_fever.fa.gz", "hpv_16_allFasta.fa.gz"):
        seqs += [r[1] for r in orc.kseq_parse_file(os.path.join(data_dir, f))]
    assert len(seqs) > 250
    rb, ro = orc.pack(seqs)
    rb = _pad(rb)
    qb, qo = synth.generate_reads_fast(rb, ro, 0, 30000)
    got, want = _classify_both(ctx, orc, rb, ro, qb, qo, [16], 1000)
    assert (got == want).all()
    d_b = torch.from_numpy(qb).cuda()
    d_o = torch.from_numpy(qo.astype(np.int64)).to(torch.int32).cuda()
    d_out = torch.empty((30000, 4), dtype=torch.int32, device="cuda")
    ctx.classify_device(d_b.data_ptr(), d_o.data_ptr(), 30000, d_out.data_ptr(), max_read_len=150,
                        stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == want).all()
    # a mixed batch: short reads interleaved with reads far longer than the sketch (routing + gather/scatter)
    rng = np.random.default_rng(9)
    mixed = []
    for i in range(600):
        r = int(rng.integers(0, len(seqs)))
        L = 150 if i % 3 else int(rng.integers(1200, 5000))
        L = min(L, len(seqs[r]))
        st = int(rng.integers(0, len(seqs[r]) - L + 1))
        mixed.append(seqs[r][st:st + L])
    mb, mo = orc.pack(mixed)
    got, want = _classify_both(ctx, orc, rb, ro, _pad(mb), mo, [16], 1000)
    assert (got == want).all()


def test_resident_entry_point_with_too_small_length_hint(ctx, orc):
    """rk_classify_batch_device trusts max_read_len for its tile geometry (and for the width of its packed counters).
    A batch that breaks the promise must never be answered wrongly: every row is either exact or flagged -2."""
    import torch
    rng = np.random.default_rng(5)
    refs = [rand_dna(rng, 450) for _ in range(5)]          # shorter than the sketch: every k-mer is a sketch hash
    # period-20 tandem repeat: a 400 bp read scores 380 on it with only 20 distinct hashes (each 19 times), i.e. neither the
    # hit multiset (64 keys, 30 occurrences) nor anything else but the 8-bit counter itself would notice
    refs.append(rand_dna(rng, 20) * 24)
    reads = []
    for i in range(400):
        r = refs[i % 6]
        reads += [r[:400], r[100:150], r[200:250], r[300:350]] if i % 2 else [r[50:100], r[:430], r[10:60], r[5:45]]
    rb, ro = orc.pack(refs)
    qb, qo = orc.pack(reads)
    qb = _pad(qb)
    got, want = _classify_both(ctx, orc, _pad(rb), ro, qb, qo, [16], 1000)   # host entry point measures the lengths itself
    assert (got == want).all()
    n = len(reads)
    d_b = torch.from_numpy(qb).cuda()
    d_o = torch.from_numpy(qo.astype(np.int64)).to(torch.int32).cuda()
    d_out = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    for hint in (150, 120, 200):
        d_out.zero_()
        ctx.classify_device(d_b.data_ptr(), d_o.data_ptr(), n, d_out.data_ptr(), max_read_len=hint,
                            stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        ok = (out[:, 0] == -2) | (out == want).all(axis=1)
        assert ok.all(), (hint, np.nonzero(~ok)[0][:10], out[~ok][:5], want[~ok][:5])
        assert (out[:, 0] != -2).any()


def test_two_contexts_from_two_host_threads(orc, pave):
    """The reference calls mkmh concurrently from OpenMP threads; here the rule is one rk_ctx per host thread.  Two threads,
    each with its own context on the same GPU, classify different batches (short and long reads) at the same time."""
    import threading
    import rkmh_amd
    from rkmh_amd import synth
    _, rb, ro = pave
    jobs = []
    for j, (lo, n, L) in enumerate(((0, 30000, 150), (70000, 4000, 2500))):
        qb, qo = synth.generate_reads_fast(rb, ro, lo, lo + n, read_len=L)
        jobs.append((qb, qo))
    ref_ctx = rkmh_amd.Context(0)
    ref_ctx.set_references(rb, ro, [16], 1000)
    sk, ln = ref_ctx.get_reference_sketches()
    wants = [orc.classify_stream(qb, qo, [16], 1000, sk, ln, threads=8) for qb, qo in jobs]
    errors = []

    def run(j):
        try:
            c = rkmh_amd.Context(0)
            c.set_reference_sketches(sk, ln, [16], 1000)
            for _ in range(4):
                got = c.classify(jobs[j][0], jobs[j][1])
                if not (got == wants[j]).all():
                    errors.append((j, "mismatch"))
            c.close()
        except Exception as e:  # noqa: BLE001
            errors.append((j, repr(e)))

    ts = [threading.Thread(target=run, args=(j,)) for j in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    ref_ctx.close()
    assert not errors, errors


def test_error_paths_of_the_c_abi(orc, pave):
    """Limits and misuse come back as error codes + rk_last_error text (the reference aborts or has undefined behaviour);
    the context stays usable afterwards."""
    import rkmh_amd
    _, rb, ro = pave
    c = rkmh_amd.Context(0)
    qb, qo = orc.pack([bytes(rb[:150]), bytes(rb[200:350])])
    qb = _pad(qb)
    with pytest.raises(rkmh_amd.RkmhError, match="rk_set_references"):
        c.classify(qb, qo)                                   # classify before references
    with pytest.raises(rkmh_amd.RkmhError):
        c.set_references(rb, ro, [65], 1000)                 # k > RK_MAX_K
    with pytest.raises(rkmh_amd.RkmhError):
        c.set_references(rb, ro, [0], 1000)                  # k < 1
    with pytest.raises(rkmh_amd.RkmhError):
        c.set_references(rb, ro, list(range(8, 17)), 1000)   # more than RK_MAX_KS k-mer sizes
    with pytest.raises(rkmh_amd.RkmhError):
        c.set_references(rb, ro, [16], 16385)                # sketch > RK_MAX_SKETCH
    with pytest.raises(rkmh_amd.RkmhError):
        c.set_references(rb, ro, [16], 0)
    with pytest.raises(rkmh_amd.RkmhError):
        c.set_references(rb, ro[:1], [16], 1000)             # zero references (UB in the reference, rkmh.cpp:848)
    with pytest.raises(rkmh_amd.RkmhError):
        c.hash_batch(qb, qo, [70])
    # still alive and exact
    c.set_references(rb, ro, [16], 1000)
    sk, ln = c.get_reference_sketches()
    assert (c.classify(qb, qo) == orc.classify_stream(qb, qo, [16], 1000, sk, ln, threads=1)).all()
    c.close()


def test_bench_json_contract(root):
    """bench.py --full prints ONE JSON line with the driver's fields, the roofline object and (N=1) the CPU baseline."""
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--reads", "30000", "--steps", "3", "--warmup", "1",
                        "--cpu-seconds", "0.5", "--spinup-seconds", "0", "--c4-genome-mb", "120", "--c4-reads", "200000"], capture_output=True, cwd=root)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k, t in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                 ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str),
                 ("config", dict), ("roofline", dict), ("cpu_baseline", dict)):
        assert isinstance(d[k], t), (k, d[k])
    assert d["vs_baseline"] is None and d["n_gpus"] == 1 and d["steps"] == 3 and d["scaling"] == "weak"
    assert "workload" in d["config"] and "model" not in d["config"]
    rf = d["roofline"]
    assert rf["bound"] in ("hbm", "mfma") and rf["unit"] == "GB/s" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    cb = d["cpu_baseline"]
    assert cb["kind"] in ("port", "reference") and cb["cores"] >= 1 and cb["value"] > 0 and "bit-exact" in cb["oracle_check"]
    assert d["host_path"]["value"] > 0 and d["host_path"]["pageable_value"] > 0 and d["e2e"]["output_lines"] == d["e2e"]["reads"]
    df = d["depth_filter"]
    assert df["count_pass_ms"] > 0 and df["masked_classify_ms"] > 0 and df["slots"] == 200000000 and df["min_num_bound"] == 0
    assert df["count_pass_full_table_ms"] > 0 and df["masked_classify_exact_min_num_ms"] > 0 and df["oracle_checked_reads"] >= 4 * 30000
    assert d["oracle_checked_ref_sketches"] == 182 and d["c3_panel"]["oracle_checked_ref_sketches"] >= 260
    # every timed batch is sampled against the oracle, not only the first
    assert cb["oracle_checked_reads"] > 30000 and "other 3 timed batches" in cb["oracle_check"]
    # informational legs for BASELINE configs 3, 4 and 5 (never `value`)
    c3, c4, c5 = d["c3_panel"], d["c4_filter"], d["c5_call"]
    assert c3["references"] >= 260 and c3["kernel_ms"] > 0 and c3["rerouted_rows"] == 0 and c3["oracle_checked_reads"] > 0
    assert c4["k"] == 20 and c4["sketch_size"] == 2000 and c4["kernel_ms"] > 0 and c4["M2_count_pass_ms"] > 0 and c4["M2_masked_classify_ms"] > 0
    assert c4["oracle_checked_reads"] > 0
    # config 4 as a whole command (here scaled down): device front ends against the host parsers, byte for byte
    fs = c4["full_size"]
    assert "error" not in fs, fs
    assert fs["oracle_checked_ref_sketches"] == 2 and fs["oracle_checked_reads"] >= 20000 and fs["oracle_checked_reads_passing"] > 0
    for key in ("plain", "M2"):
        assert fs[key]["identical_to_host_parsed_run"] is True and fs[key]["wall_s"] > 0 and fs[key]["reads_passing"] > 0
        assert any("references through the device" in x for x in fs[key]["stages"]) and any("device front end" in x for x in fs[key]["stages"])
    assert c5["k"] == 12 and c5["wall_s"] > 0 and c5["vcf_rows"] >= 5 and c5["reads"] > 50000


def test_bench_plain_run_dumps_its_last_step(root, orc, tmp_path):
    """A plain bench.py run (no --full) prints the contract fields and the roofline object and nothing it would need further runs
    for; --dump-outputs DIR writes the rows of its last timed step: here warm-up 1 + 3 timed steps over 4 batches of 20000 reads
    (and a clock ramp that must not shift them) end on batch 3, reads 60000..79999, bit-exact against the CPU oracle."""
    from rkmh_amd import api, synth
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--reads", "20000", "--steps", "3", "--warmup", "1",
                        "--spinup-seconds", "0.05", "--dump-outputs", str(tmp_path)], capture_output=True, cwd=root, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k, t in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                 ("ms_per_step", float), ("higher_is_better", bool), ("dtype", str), ("config", dict), ("roofline", dict)):
        assert isinstance(d[k], t), (k, d[k])
    assert d["steps"] == 3 and d["warmup"] == 1 and abs(d["value"] - 20000 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    for k in ("cpu_baseline", "host_path", "depth_filter", "c3_panel", "c4_filter", "c5_call", "e2e", "oracle_checked_ref_sketches"):
        assert k not in d, k
    assert sorted(os.listdir(tmp_path)) == ["read_index.npy", "rows.npy"]
    rows, idx = np.load(tmp_path / "rows.npy"), np.load(tmp_path / "read_index.npy")
    assert rows.dtype == np.float64 and idx.dtype == np.float64 and rows.shape == (20000, 4)
    assert (idx == np.arange(60000, 80000)).all()
    refs = api.parse_files([os.path.join(root, "tests", "golden", "data", "all_pave_ref.fa.gz")])
    rb, ro = refs["bases"], refs["offsets"]
    qb, qo = synth.generate_reads_fast(rb, ro, 60000, 80000)
    sk, ln = orc.sketch_refs(rb, ro, [16], 1000, threads=8)
    assert (rows == orc.classify_stream(qb, qo, [16], 1000, sk, ln, threads=8)).all()


def test_bench_spawns_its_own_ranks(root, tmp_path):
    """`python bench.py --gpus 2` with no launcher around it (WORLD_SIZE unset): bench.py starts torch.distributed.run as a child
    process before it has touched the GPU, the two ranks run (here on GPU 0 over gloo), and the one JSON line comes through."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(RKMH_BENCH_ONE_DEVICE="1", RKMH_DIST_BACKEND="gloo")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--c3-total-reads", "80000", "--steps", "4", "--warmup", "1",
                        "--spinup-seconds", "0", "--dump-outputs", str(tmp_path)], capture_output=True, cwd=root, env=env, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 4 and "cpu_baseline" not in d and "c3_panel" not in d
    assert d["scaling"] == "strong" and d["config"]["reads_per_gpu"] == 40000
    # --dump-outputs: every rank writes the rows of its own shard
    for rk in (0, 1):
        rows, idx = np.load(tmp_path / ("rows_rank%d.npy" % rk)), np.load(tmp_path / ("read_index_rank%d.npy" % rk))
        assert rows.shape == (40000, 4) and (idx == np.arange(40000 * rk, 40000 * (rk + 1))).all()
        assert (rows[:, 0] >= 0).all() and (rows[:, 1] <= rows[:, 3]).all()


def test_bench_two_ranks_launched_like_the_driver(root):
    """The driver's N>1 launch line (torch.distributed.run, one rank per GPU) with both ranks on GPU 0 and gloo instead of RCCL
    (a one-GPU box).  N > 1 measures BASELINE config 3: a FIXED total of reads against every bundled reference (266 sequences),
    sharded over the ranks -- strong scaling; rank 0 prints ONE line, value = all reads over the slowest rank's time; with --full
    every rank sampled its rows against the oracle, no CPU baseline."""
    env = dict(os.environ, RKMH_BENCH_ONE_DEVICE="1", RKMH_DIST_BACKEND="gloo")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29547", os.path.join(root, "bench.py"), "--full", "--gpus", "2", "--c3-total-reads", "100001", "--c3-launch-reads", "30000",
                        "--steps", "4", "--warmup", "1", "--spinup-seconds", "0"], capture_output=True, cwd=root, env=env, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["scaling"] == "strong" and "cpu_baseline" not in d
    assert abs(d["value"] - 100001 * 4 / (d["ms_per_step"] * 4e-3)) / d["value"] < 1e-6
    cfg = d["config"]
    assert "(C3)" in cfg["workload"] and cfg["references"] >= 260 and cfg["reads_total"] == 100001 and cfg["reads_per_gpu"] == 100001 // 2
    assert cfg["launches_per_step"] == 2 and cfg["sketch_broadcast_ms"] >= 0 and "2 rank" in cfg["parallelism"]
    assert d["oracle_checked_reads"] >= 2 * 4096 and d["oracle_checked_ref_sketches"] == cfg["references"]


def test_resident_input_entry_point(ctx, orc, pave):
    import torch
    from rkmh_amd import synth
    _, rb, ro = pave
    qb, qo = synth.generate_reads_fast(rb, ro, 5000, 25000)
    ctx.set_references(rb, ro, [16], 1000)
    sk, ln = ctx.get_reference_sketches()
    want = orc.classify_stream(qb, qo, [16], 1000, sk, ln, threads=8)
    d_b = torch.from_numpy(qb).cuda()
    d_o = torch.from_numpy(qo.astype(np.int64)).to(torch.int32).cuda()  # uint32 values, bit pattern kept
    d_out = torch.empty((20000, 4), dtype=torch.int32, device="cuda")
    for mrl in (150, 0):
        d_out.zero_()
        ctx.classify_device(d_b.data_ptr(), d_o.data_ptr(), 20000, d_out.data_ptr(), max_read_len=mrl,
                            stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == want).all()


def test_full_size_properties(ctx, orc, pave):
    """C2 at full size (1M reads): properties that need no CPU pass over everything."""
    from rkmh_amd import synth
    _, rb, ro = pave
    n = 1000000
    qb, qo = synth.generate_reads_fast(rb, ro, 0, n)
    ctx.set_references(rb, ro, [16], 1000)
    out = ctx.classify(qb, qo)
    assert out.shape == (n, 4)
    assert (out[:, 0] >= 0).all() and (out[:, 0] < 182).all()
    assert (out[:, 3] <= 134).all() and (out[:, 3] >= 0).all()
    assert (out[:, 1] >= 0).all() and (out[:, 1] <= out[:, 3]).all()
    assert (out[:, 2] >= 0).all() and (out[:, 2] <= out[:, 1] + 1).all()
    # idempotence + sharding invariance: any slice classified alone gives the same rows
    for lo, hi in ((0, 1000), (123457, 130001), (n - 777, n)):
        sub = ctx.classify(np.concatenate([qb[lo * 150: hi * 150], np.zeros(16, np.uint8)]), qo[: hi - lo + 1])
        assert (sub == out[lo:hi]).all()
    # a bounded random sample against the oracle
    sk, ln = ctx.get_reference_sketches()
    idx = np.random.default_rng(1).integers(0, n - 2000, size=5)
    for lo in idx:
        lo = int(lo)
        want = orc.classify_stream(qb[lo * 150: (lo + 2000) * 150], qo[:2001], [16], 1000, sk, ln, threads=8)
        assert (out[lo: lo + 2000] == want).all()
    # most reads come back to a reference that shares >= 5 sketch hashes (1 % error reads of 150 bp)
    assert (out[:, 1] >= 5).mean() > 0.9


@pytest.mark.parametrize("preset", ["default", "mash"])
@pytest.mark.parametrize("how", ["flag", "env"])
def test_cli_hash_policy_presets(root, data_dir, golden_dir, preset, how):
    """--hash-policy / RKMH_POLICY (rk_policy_parse) through bin/rkmh and rkmh_amd.cli: stdout equals the committed goldens of
    tests/golden/gen_golden.py for both presets -- `mash` = the first 64 bits of the murmur output over all len-k+1 windows."""
    import hashlib
    exe = os.path.join(root, "bin", "rkmh")
    g = json.load(open(os.path.join(golden_dir, "cli_%s.json" % preset)))
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    flag = ["--hash-policy", preset] if how == "flag" else []
    if how == "env":
        env["RKMH_POLICY"] = "fold=w2w1" if preset == "default" else "mash"   # (the flag is applied after the variable)
        flag = ["--hash-policy", "default"] if preset == "default" else []
    r = subprocess.run([exe, "classify", "-r", os.path.join(data_dir, "hpv_16.fa.gz"), "-f", os.path.join(data_dir, "minION25.fq.gz"),
                        "-k", "12", "-s", "1000"] + flag, capture_output=True, env=env)
    assert r.returncode == 0, r.stderr
    assert r.stdout.decode() == g["classify_c1"]
    for cmd in ([exe, "stream"], [sys.executable, "-m", "rkmh_amd.cli", "stream"]):
        r = subprocess.run(cmd + ["-r", os.path.join(data_dir, "zika.refs.fa.gz"), "-f", os.path.join(data_dir, "z1.fq.gz"), "-N", "2",
                                  "-D", "1", "-k", "16"] + flag, capture_output=True, env=env, cwd=root)
        assert r.returncode == 0, r.stderr
        assert r.stdout.decode() == g["stream_zika_N2_D1"], cmd
    r = subprocess.run([exe, "hash", "-f", os.path.join(data_dir, "hpv_16.fa.gz"), "-k", "12"] + flag, capture_output=True, env=env)
    assert r.returncode == 0, r.stderr
    h = g["hash_hpv16_k12"]
    fields = r.stdout.decode().rstrip("\n").split("\t")
    assert len(fields) - 1 == h["n_hashes"] and [int(x) for x in fields[1:7]] == h["first"]
    assert hashlib.sha256(r.stdout).hexdigest() == h["sha256"]


def test_cli_hash_policy_is_checked(root, data_dir, tmp_path):
    """Text rk_policy_parse does not know ends the run; sketches record their policy and stream -R refuses another one."""
    exe = os.path.join(root, "bin", "rkmh")
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    for bad in ("fold=xx", "nonsense", "seed=-"):
        r = subprocess.run([exe, "stream", "-r", os.path.join(data_dir, "hpv_16.fa.gz"), "-f", os.path.join(data_dir, "minION25.fq.gz"),
                            "--hash-policy", bad], capture_output=True, env=env)
        assert r.returncode == 1 and r.stdout == b"" and b"hash policy" in r.stderr
    r = subprocess.run([sys.executable, "-m", "rkmh_amd.cli", "stream", "-r", os.path.join(data_dir, "hpv_16.fa.gz"), "-f",
                        os.path.join(data_dir, "minION25.fq.gz"), "--hash-policy", "fold=xx"], capture_output=True, env=env, cwd=root)
    assert r.returncode == 1 and r.stdout == b"" and b"hash policy" in r.stderr
    js = tmp_path / "mash.json"
    r = subprocess.run([exe, "sketch", "-f", os.path.join(data_dir, "zika.refs.fa.gz"), "-k", "16", "-o", str(js), "--hash-policy", "mash"],
                       capture_output=True, env=env)
    assert r.returncode == 0, r.stderr
    doc = json.load(open(js))
    assert doc[0]["hashPolicy"] == "fold=h1,windows=len-k+1,zero=count,mask=lt,freqmax=incl,seed=42" and doc[0]["hashSeed"] == 42
    r = subprocess.run([exe, "stream", "-R", str(js), "-f", os.path.join(data_dir, "z1.fq.gz")], capture_output=True, env=env)
    assert r.returncode == 1 and r.stdout == b"" and b"--hash-policy fold=h1,windows=len-k+1" in r.stderr
    g = json.load(open(os.path.join(root, "tests", "golden", "cli_mash.json")))
    r = subprocess.run([exe, "stream", "-R", str(js), "-f", os.path.join(data_dir, "z1.fq.gz"), "-N", "2", "-D", "1", "--hash-policy", "mash"],
                       capture_output=True, env=env)
    assert r.returncode == 0, r.stderr
    assert r.stdout.decode() == g["stream_zika_N2_D1"]


def test_cli_stream_and_hash_output(ctx, orc, root, data_dir, golden_dir, tmp_path):
    exe = os.path.join(root, "bin", "rkmh")
    g = golden(golden_dir, "c1_hpv16_minion25")
    r = subprocess.run([exe, "classify", "-r", os.path.join(data_dir, "hpv_16.fa.gz"), "-f",
                        os.path.join(data_dir, "minION25.fq.gz"), "-k", "12", "-s", "1000"], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert b"CLASSIFY COMMAND IS TEMPORARILY UNAVAILABLE" in r.stderr
    want = "".join(orc.stream_line(x[1], x[0], x[2], x[3], x[4], 1000) for x in g["rows"])
    assert r.stdout.decode() == want
    # stream with flags + default k notice
    g = golden(golden_dir, "zika_z1")
    r = subprocess.run([exe, "stream", "-r", os.path.join(data_dir, "zika.refs.fa.gz"), "-f",
                        os.path.join(data_dir, "z1.fq.gz"), "-N", "2", "-D", "1", "-t", "4"], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert b"No kmer size(s) provided. Will use a default kmer size of 16." in r.stderr
    want = "".join(orc.stream_line(x[1], x[0], x[2], x[3], x[4], 1000, min_matches=2, min_diff=1) for x in g["rows"])
    assert r.stdout.decode() == want
    # -M path through the CLI (counter = 200M slots as rkmh.cpp:739)
    from rkmh_amd import synth, api
    refs = api.parse_files([os.path.join(data_dir, "all_pave_ref.fa.gz")])
    qb, qo = synth.generate_reads(refs["bases"], refs["offsets"], 0, 300)
    names = synth.read_names(0, 300)
    fq = tmp_path / "r.fq"
    synth.write_fastq(str(fq), qb, qo, names)
    r = subprocess.run([exe, "stream", "-r", os.path.join(data_dir, "all_pave_ref.fa.gz"), "-f", str(fq), "-k", "16",
                        "-M", "2"], capture_output=True)
    assert r.returncode == 0, r.stderr
    rb, ro = refs["bases"], refs["offsets"]
    sk, ln = orc.sketch_refs(rb, ro, [16], 1000, threads=4)
    o4 = orc.classify_stream(qb, qo, [16], 1000, sk, ln, threads=4, min_kmer_occ=2)
    want = "".join(orc.stream_line(refs["names"][o4[i, 0]].decode(), names[i].decode(), o4[i, 1], o4[i, 2], o4[i, 3], 1000)
                   for i in range(300))
    assert r.stdout.decode() == want
    # hash sub-command: name then every hash
    r = subprocess.run([exe, "hash", "-f", os.path.join(data_dir, "hpv_16.fa.gz"), "-k", "12"], capture_output=True)
    assert r.returncode == 0, r.stderr
    rec = orc.kseq_parse_file(os.path.join(data_dir, "hpv_16.fa.gz"))[0]
    h = orc.calc_hashes(orc.to_upper(rec[1]), [12])
    assert r.stdout.decode() == rec[0].decode() + "".join("\t%d" % v for v in h) + "\n"
    # no arguments -> help on stderr, exit 1
    r = subprocess.run([exe], capture_output=True)
    assert r.returncode == 1 and r.stdout == b"" and b"Usage" in r.stderr
    r = subprocess.run([exe, "stream"], capture_output=True)
    assert r.returncode == 1


def test_python_cli_single_rank(orc, root, data_dir, golden_dir):
    """python -m rkmh_amd.cli (the torch.distributed form) at world size 1: same lines as the golden, incl. -M."""
    import sys
    g = golden(golden_dir, "zika_z1")
    r = subprocess.run([sys.executable, "-m", "rkmh_amd.cli", "stream", "-r", os.path.join(data_dir, "zika.refs.fa.gz"), "-f",
                        os.path.join(data_dir, "z1.fq.gz"), "-k", "16"], capture_output=True, cwd=root)
    assert r.returncode == 0, r.stderr
    want = "".join(orc.stream_line(x[1], x[0], x[2], x[3], x[4], 1000) for x in g["rows"])
    assert r.stdout.decode() == want
    r = subprocess.run([sys.executable, "-m", "rkmh_amd.cli", "stream", "-r", os.path.join(data_dir, "zika.refs.fa.gz"), "-f",
                        os.path.join(data_dir, "z1.fq.gz"), "-k", "16", "-M", "2"], capture_output=True, cwd=root)
    assert r.returncode == 0, r.stderr
    refs = orc.kseq_parse_file(os.path.join(data_dir, "zika.refs.fa.gz"))
    reads = orc.kseq_parse_file(os.path.join(data_dir, "z1.fq.gz"))
    rb, ro = orc.pack([x[1] for x in refs])
    qb, qo = orc.pack([x[1] for x in reads])
    sk, ln = orc.sketch_refs(rb, ro, [16], 1000, threads=4)
    o4 = orc.classify_stream(qb, qo, [16], 1000, sk, ln, threads=4, min_kmer_occ=2)
    want = "".join(orc.stream_line(refs[o4[i, 0]][0].decode(), reads[i][0].decode(), o4[i, 1], o4[i, 2], o4[i, 3], 1000)
                   for i in range(len(reads)))
    assert r.stdout.decode() == want


def test_counter_add_staged_and_unaligned(root):
    """rk_counter_add / rk_counter_copy, the in-process reduce and broadcast of a multi-device -M run: the STAGED branch (the other
    device's table brought over piece by piece through two buffers; forced here for two tables of one device with
    RKMH_COUNTER_STAGED=1, several 64 MB pieces + a ragged tail) and tables that are only 4-byte aligned (a slice of a tensor the
    counter wraps: the add falls back to dword accesses)."""
    import sys
    code = r"""
import os, sys, numpy as np, torch
sys.path.insert(0, %r)
import rkmh_amd
from rkmh_amd import api
ctx = rkmh_amd.Context(0)
slots = 40000003
g = torch.Generator(device="cuda").manual_seed(7)
for off in (0, 1):          # 16-byte aligned / only 4-byte aligned tables
    a = torch.randint(0, 1000, (slots + 4,), dtype=torch.int32, device="cuda", generator=g)
    b = torch.randint(0, 1000, (slots + 4,), dtype=torch.int32, device="cuda", generator=g)
    want = (a + b)[off:off + slots].clone()
    a0, b0 = a.clone(), b.clone()
    ca = api.Counter(ctx, slots=slots, device_ptr=a[off:].data_ptr())
    cb = api.Counter(ctx, slots=slots, device_ptr=b[off:].data_ptr())
    torch.cuda.synchronize()      # the tables were filled on torch's stream; the library works on its context's own
    ca.add(cb)
    torch.cuda.synchronize()
    assert bool((a[off:off + slots] == want).all()) and bool((b == b0).all())
    assert bool((a[:off] == a0[:off]).all()) and bool((a[off + slots:] == a0[off + slots:]).all())      # nothing outside the table
    cb.copy_from(ca)
    torch.cuda.synchronize()
    assert bool((b[off:off + slots] == want).all()) and bool((b[off + slots:] == b0[off + slots:]).all())
    ca.destroy(); cb.destroy()
ctx.close()
print("COUNTER_ADD_OK")
""" % root
    for staged in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, cwd=root, env=dict(os.environ, RKMH_COUNTER_STAGED=staged), timeout=600)
        assert r.returncode == 0 and b"COUNTER_ADD_OK" in r.stdout, (staged, r.stderr.decode()[-3000:])


def test_rccl_path_at_world_size_one(orc, root, data_dir, golden_dir):
    """The RCCL code path of rkmh_amd/dist.py executed for real on a one-GPU box: a process group of ONE rank on the nccl backend
    (RKMH_DIST_FORCE=1 keeps the collectives from short-cutting at world size 1) through broadcast_sketches, allreduce_counter
    (the table an rk_counter wraps) and gather_rows on device tensors -- and the whole python CLI with -M 2 the same way,
    whose lines must equal the oracle's."""
    import sys
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, RKMH_DIST_FORCE="1", RKMH_DIST_BACKEND="nccl", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0",
               MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    code = r"""
import os, sys, numpy as np, torch
sys.path.insert(0, %r)
import rkmh_amd
from rkmh_amd import api, dist as rdist
rank, local, world = rdist.init()
assert torch.distributed.is_initialized() and torch.distributed.get_backend() == "nccl" and world == 1
rng = np.random.default_rng(3)
sk0 = rng.integers(0, np.iinfo(np.uint64).max, size=(9, 64), dtype=np.uint64)
ln0 = rng.integers(0, 65, size=9).astype(np.int32)
sk, ln = rdist.broadcast_sketches(sk0, ln0, 9, 64, src=0, device=torch.device("cuda", 0))
assert (sk == sk0).all() and (ln == ln0).all() and sk.dtype == np.uint64
ctx = rkmh_amd.Context(0)
t = torch.zeros(100003, dtype=torch.int32, device="cuda:0")
cnt = api.Counter(ctx, slots=100003, device_ptr=t.data_ptr())
for key in (5, 5, 100003 + 5, 77):
    cnt.increment(key)
ctx.synchronize()
rdist.allreduce_counter(t)
torch.cuda.synchronize()
assert cnt.get(5) == 3 and cnt.get(77) == 1 and int(t.sum().item()) == 4
rows = np.arange(4000, dtype=np.int32).reshape(1000, 4)
got = rdist.gather_rows(rows, dst=0)
assert got.shape == (1000, 4) and (got == rows).all()
cnt.destroy(); ctx.close()
torch.distributed.destroy_process_group()
print("RCCL_WS1_OK")
""" % root
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, cwd=root, env=env, timeout=600)
    assert r.returncode == 0 and b"RCCL_WS1_OK" in r.stdout, r.stderr.decode()[-3000:]
    s = socket.socket(); s.bind(("127.0.0.1", 0)); env["MASTER_PORT"] = str(s.getsockname()[1]); s.close()
    r = subprocess.run([sys.executable, "-m", "rkmh_amd.cli", "stream", "-r", os.path.join(data_dir, "zika.refs.fa.gz"), "-f",
                        os.path.join(data_dir, "z1.fq.gz"), "-k", "16", "-M", "2"], capture_output=True, cwd=root, env=env, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    refs = orc.kseq_parse_file(os.path.join(data_dir, "zika.refs.fa.gz"))
    reads = orc.kseq_parse_file(os.path.join(data_dir, "z1.fq.gz"))
    rb, ro = orc.pack([x[1] for x in refs])
    qb, qo = orc.pack([x[1] for x in reads])
    sk, ln = orc.sketch_refs(rb, ro, [16], 1000, threads=4)
    o4 = orc.classify_stream(qb, qo, [16], 1000, sk, ln, threads=4, min_kmer_occ=2)
    want = "".join(orc.stream_line(refs[o4[i, 0]][0].decode(), reads[i][0].decode(), o4[i, 1], o4[i, 2], o4[i, 3], 1000)
                   for i in range(len(reads)))
    # (librccl prints a version banner to stdout on some boxes: result lines are the ones with tabs)
    got = "".join(l + "\n" for l in r.stdout.decode().splitlines() if "\t" in l)
    assert got == want


def test_many_references_sparse_counters(ctx, orc):
    """Large panels: per-read counters become a 128-entry map of the references a read really hits (any number of
    references up to 16384 on the fused path).  Unrelated references, families of near-identical references (a read hits
    dozens of them: ties, diff against earlier members), families larger than the map (overflow => general path),
    duplicated references, through both entry points; and a panel beyond the fused limit."""
    import torch
    rng = np.random.default_rng(77)
    refs = [rand_dna(rng, 220) for _ in range(2100)]                   # unrelated, short: every k-mer is a sketch hash
    fam = rand_dna(rng, 900)
    for j in range(90):                                                 # a family of 90 near-identical references
        r = bytearray(fam)
        for q in rng.integers(0, 900, size=6):
            r[q] = b"ACGT"[int(rng.integers(0, 4))]
        refs.insert(int(rng.integers(0, len(refs))), bytes(r))
    big = rand_dna(rng, 700)
    refs += [big] * 150                                                 # 150 identical references: more than the map holds
    reads = [refs[int(i)][20:170] for i in rng.integers(0, len(refs), size=300)]
    reads += [fam[i:i + 150] for i in range(0, 700, 50)] + [big[100:250], rand_dna(rng, 150), b"A" * 150]
    rb, ro = orc.pack(refs)
    qb, qo = orc.pack(reads)
    rbp, qbp = _pad(rb), _pad(qb)
    for ks, S in (([16], 1000), ([16], 120), ([12, 16], 1000)):
        got, want = _classify_both(ctx, orc, rbp, ro, qbp, qo, ks, S)
        assert (got == want).all(), (ks, S, np.nonzero((got != want).any(axis=1))[0][:5])
    assert (got[:300, 1] > 50).all()
    # resident entry point: exact or flagged, and the unrelated-reference reads are answered by the fused kernel itself
    ctx.set_references(rbp, ro, [16], 1000)
    sk, ln = ctx.get_reference_sketches()
    want = orc.classify_stream(qbp, qo, [16], 1000, sk, ln, threads=8)
    n = len(reads)
    d_b = torch.from_numpy(qbp).cuda()
    d_o = torch.from_numpy(qo.astype(np.int64)).to(torch.int32).cuda()
    d_out = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    ctx.classify_device(d_b.data_ptr(), d_o.data_ptr(), n, d_out.data_ptr(), max_read_len=150,
                        stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    ok = (out[:, 0] == -2) | (out == want).all(axis=1)
    assert ok.all()
    assert (out[:, 0] != -2).mean() > 0.8
    # beyond the fused limit: everything through the general path
    refs2 = [rand_dna(rng, 60) for _ in range(17000)]
    reads2 = [refs2[int(i)][5:55] for i in rng.integers(0, 17000, size=40)]
    rb2, ro2 = orc.pack(refs2)
    qb2, qo2 = orc.pack(reads2)
    got, want = _classify_both(ctx, orc, _pad(rb2), ro2, _pad(qb2), qo2, [16], 1000)
    assert (got == want).all()


def test_depth_filter_with_long_reads(ctx, orc, pave):
    """-M path where some reads exceed the fused kernel's length limit (count + classify through the tile hasher)."""
    import rkmh_amd
    _, rb, ro = pave
    reads = [bytes(rb[int(ro[i]) + 100: int(ro[i]) + 100 + L]) for i, L in ((0, 150), (1, 3000), (2, 150), (0, 2000), (5, 150))] * 3
    qb, qo = orc.pack(reads)
    qb = _pad(qb)
    ctx.set_references(rb, ro, [16], 1000)
    sk, ln = ctx.get_reference_sketches()
    cnt = rkmh_amd.Counter(ctx, slots=1000003)
    ctx.count_batch(qb, qo, cnt)
    ctx.set_depth_filter(cnt, 3)
    try:
        got = ctx.classify(qb, qo)
    finally:
        ctx.set_depth_filter(None, 0)
    want = orc.classify_stream(qb, qo, [16], 1000, sk, ln, threads=4, min_kmer_occ=3, counter_slots=1000003)
    assert (got == want).all()
    cnt.destroy()


def test_long_sequences_radix_select(ctx, orc, pave):
    """Sequences with more hashes than the LDS sorter holds (> 16384): exact bottom-S by radix select."""
    import rkmh_amd
    _, rb, ro = pave
    rng = np.random.default_rng(12)
    big = bytes(rb[: int(ro[40])])                 # ~300 kb of concatenated HPV genomes (lower case + IUPAC)
    rnd = rand_dna(rng, 200000, b"ACGT")
    low = (b"ACGTTGCA" * 4000)                     # highly repetitive: many equal hashes around the threshold
    tiny = rand_dna(rng, 20000, b"ACGT")           # 19984 hashes: just above the limit
    seqs = [big, rnd, low, tiny, rnd[:9000]]
    bases, offs = orc.pack(seqs)
    bases = _pad(bases)
    for ks, S in (([16], 1000), ([20], 2000), ([12, 16], 16384), ([16], 7)):
        want_sk, want_ln = orc.sketch_refs(bases, offs, ks, S, threads=4)
        sk, ln = ctx.sketch_batch(bases, offs, ks, S)
        assert (ln == want_ln).all(), (ks, S, ln, want_ln)
        assert (sk == want_sk).all(), (ks, S)
    # as references (+ the -I filter) and as long reads
    ctx.set_references(bases, offs, [16], 1000, max_samples=3, counter_slots=5000011)
    sk, ln = ctx.get_reference_sketches()
    wsk, wln = orc.sketch_refs(bases, offs, [16], 1000, threads=4, max_samples=3, counter_slots=5000011)
    assert (ln == wln).all() and (sk == wsk).all()
    ctx.set_references(rb, ro, [16], 1000)
    sk, ln = ctx.get_reference_sketches()
    reads = [big[1000:60000], rnd[:30000], big[5:155]]
    qb, qo = orc.pack(reads)
    got = ctx.classify(_pad(qb), qo)
    want = orc.classify_stream(qb, qo, [16], 1000, sk, ln, threads=4)
    assert (got == want).all()


def _filter_expect(orc, refs, reads, ks, S, min_occ=None, max_samples=None, min_matches=-1, min_diff=0):
    rb, ro = orc.pack([orc.to_upper(x[1]) for x in refs])
    qb, qo = orc.pack([x[1] for x in reads])
    if max_samples is not None and max_samples < 100000:
        sk, ln = orc.sketch_refs(rb, ro, ks, S, threads=4, max_samples=max_samples, counter_slots=10000000, distinct=True)
    else:
        sk, ln = orc.sketch_refs(rb, ro, ks, S, threads=4)
    kw = {} if min_occ is None else dict(min_kmer_occ=min_occ, counter_slots=10000000)
    rows = orc.classify_stream(qb, qo, ks, S, sk, ln, threads=4, **kw)
    return rows, ln


def test_cli_filter(orc, root, data_dir, tmp_path):
    """rkmh filter (main_filter, rkmh.cpp:996-1424): passing reads in file mode, 'Sample:' lines in -i mode."""
    from rkmh_amd import synth, api
    exe = os.path.join(root, "bin", "rkmh")
    refs = orc.kseq_parse_file(os.path.join(data_dir, "all_pave_ref.fa.gz"))[:60]
    ref_fa = tmp_path / "refs.fa"
    ref_fa.write_bytes(b"".join(b">" + r[0] + b" some comment\n" + r[1] + b"\n" for r in refs))
    R = api.parse_files([str(ref_fa)])
    qb, qo = synth.generate_reads(R["bases"], R["offsets"], 0, 400)
    names = synth.read_names(0, 400)
    rng = np.random.default_rng(3)
    seqs = [bytes(qb[int(qo[i]): int(qo[i + 1])]) for i in range(400)]
    for i in range(0, 400, 7):                       # some reads that match nothing, some lower case
        seqs[i] = rand_dna(rng, 150)
    seqs[5] = seqs[5].lower()
    quals = [bytes(rng.integers(33, 74, size=150).astype(np.uint8).tolist()) for _ in range(400)]
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"".join(b"@" + names[i] + b"\n" + seqs[i] + b"\n+\n" + quals[i] + b"\n" for i in range(400)))
    reads = [(names[i], seqs[i], quals[i]) for i in range(400)]
    for flags, kw in (([], {}), (["-N", "8", "-D", "2"], dict(min_matches=8, min_diff=2)),
                      (["-M", "2", "-N", "3"], dict(min_occ=2, min_matches=3)),
                      (["-I", "2", "-D", "1"], dict(max_samples=2, min_diff=1))):
        r = subprocess.run([exe, "filter", "-r", str(ref_fa), "-f", str(fq), "-k", "16", "-s", "1000"] + flags, capture_output=True)
        assert r.returncode == 0, r.stderr
        rows, _ = _filter_expect(orc, refs, reads, [16], 1000, min_occ=kw.get("min_occ"), max_samples=kw.get("max_samples"))
        want = b""
        npass = 0
        for i in range(400):
            ref, shared, diff_ok, ok = orc.filter_decision(rows[i], kw.get("min_matches", -1), kw.get("min_diff", 0))
            if ok:
                want += orc.filter_record(names[i], orc.to_upper(seqs[i]), quals[i])
                npass += 1
        assert 0 < npass < 400, (flags, npass)
        assert r.stdout == want, flags
        import sys                                    # the torch.distributed form of the command, world size 1
        r = subprocess.run([sys.executable, "-m", "rkmh_amd.cli", "filter", "-r", str(ref_fa), "-f", str(fq), "-k", "16", "-s", "1000"] + flags,
                           capture_output=True, cwd=root)
        assert r.returncode == 0, r.stderr
        assert r.stdout == want, ("python cli", flags)
    # -i: classify what arrives on STDIN (no -f): one line per read
    r = subprocess.run([exe, "filter", "-r", str(ref_fa), "-k", "16", "-N", "4", "-i"], input=fq.read_bytes(), capture_output=True)
    assert r.returncode == 0, r.stderr
    rows, ln = _filter_expect(orc, refs, reads, [16], 1000)
    want = ""
    for i in range(400):
        ref, shared, diff_ok, ok = orc.filter_decision(rows[i], 4, 0)
        uni = 0 if ref is None else min(int(rows[i][3]), int(ln[ref]))
        want += orc.filter_stdin_line(names[i].decode(), "" if ref is None else refs[ref][0].decode(), shared, uni, int(rows[i][3]),
                                      diff_ok, min_matches=4)
    assert r.stdout.decode() == want


def test_cli_filter_and_stream_at_scale(orc, root, data_dir, tmp_path):
    """bin/rkmh filter -M / -I and stream -M on 150 k reads (many pipeline batches, a loaded count pass): stdout
    identical to the oracle's decisions, twice."""
    from rkmh_amd import synth, api
    exe = os.path.join(root, "bin", "rkmh")
    n = 150000
    refs = orc.kseq_parse_file(os.path.join(data_dir, "all_pave_ref.fa.gz"))[:60]
    ref_fa = tmp_path / "refs.fa"
    ref_fa.write_bytes(b"".join(b">" + r[0] + b"\n" + r[1] + b"\n" for r in refs))
    R = api.parse_files([str(ref_fa)])
    qb, qo = synth.generate_reads_fast(R["bases"], R["offsets"], 0, n)
    names = synth.read_names(0, n)
    seqs = [bytes(qb[i * 150: (i + 1) * 150]) for i in range(n)]
    rng = np.random.default_rng(8)
    for i in range(0, n, 11):
        seqs[i] = rand_dna(rng, 150)
    q = b"I" * 150
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"".join(b"@" + names[i] + b"\n" + seqs[i] + b"\n+\n" + q + b"\n" for i in range(n)))
    reads = [(names[i], seqs[i], q) for i in range(n)]
    for flags, kw in ((["-M", "2", "-N", "3"], dict(min_occ=2, min_matches=3)), (["-I", "2", "-D", "1"], dict(max_samples=2, min_diff=1))):
        rows, _ = _filter_expect(orc, refs, reads, [16], 1000, min_occ=kw.get("min_occ"), max_samples=kw.get("max_samples"))
        parts = []
        for i in range(n):
            ref, shared, diff_ok, ok = orc.filter_decision(rows[i], kw.get("min_matches", -1), kw.get("min_diff", 0))
            if ok:
                parts.append(orc.filter_record(names[i], orc.to_upper(seqs[i]), q))
        want = b"".join(parts)
        assert 0 < len(parts) < n
        for rep in range(2):
            r = subprocess.run([exe, "filter", "-r", str(ref_fa), "-f", str(fq), "-k", "16", "-s", "1000"] + flags, capture_output=True)
            assert r.returncode == 0, r.stderr
            assert r.stdout == want, (flags, rep, len(r.stdout), len(want))
    # stream -M 2 (200 M-slot table as in the reference): the lines in input order
    rb, ro = orc.pack([orc.to_upper(x[1]) for x in refs])
    qb2, qo2 = orc.pack(seqs)
    sk, ln = orc.sketch_refs(rb, ro, [16], 1000, threads=4)
    rows = orc.classify_stream(qb2, qo2, [16], 1000, sk, ln, threads=orc.max_threads(), min_kmer_occ=2, counter_slots=200000000)
    want = "".join(orc.stream_line(refs[int(rw[0])][0].decode(), names[i].decode(), int(rw[1]), int(rw[2]), int(rw[3]), 1000)
                   for i, rw in enumerate(rows))
    for rep in range(2):
        r = subprocess.run([exe, "stream", "-r", str(ref_fa), "-f", str(fq), "-k", "16", "-s", "1000", "-M", "2"], capture_output=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout.decode() == want, (rep, len(r.stdout), len(want))


def test_call_matches_oracle(ctx, orc, root, data_dir, tmp_path):
    """rkmh call (main_call, rkmh.cpp:1455-1904): VCF rows identical to the literal single-threaded restatement."""
    exe = os.path.join(root, "bin", "rkmh")
    rec, reads, fa, fq = _call_fixture(orc, data_dir, tmp_path)
    for k, w in ((12, 100), (16, 30)):
        r = subprocess.run([exe, "call", "-r", str(fa), "-f", str(fq), "-k", str(k), "-w", str(w)], capture_output=True)
        assert r.returncode == 0, r.stderr
        assert b"Parsing sequences..." in r.stderr
        rows = orc.call_rows([rec[0].decode()], [rec[1]], reads, k, w)
        want = orc.CALL_HEADER % str(fa) + "".join(rows)
        assert r.stdout.decode() == want, (k, w)
        assert len(rows) >= 5
    # the planted variants are found (sanity of the workload, not of parity)
    assert any("\t501\t" in x or "\t1201\t" in x for x in rows)
    # two references: the depth window carries over from one to the next (Appendix C.9); records through the C ABI
    refs2 = [(b"partA", rec[1][:3000]), (b"partB", rec[1][2500:6000])]
    rb, ro = orc.pack([x[1] for x in refs2])
    qb, qo = orc.pack(reads)
    got = ctx.call(_pad(rb), ro, _pad(qb), qo, 12, 50)
    agg = {}
    for g in got:
        key = "%s\t%d\t.\t%s\t%s" % (refs2[g["ref"]][0].decode(), g["pos"], g["orig"], g["alt"])
        a = agg.setdefault(key, [0, 0, 0, 0])
        a[0] += 1; a[1] = max(a[1], g["alt_depth"]); a[2] = max(a[2], g["avg_d"]); a[3] = max(a[3], g["depth"])
    mine = ["%s\t99\tPASS\tKC=%d;MD=%d;RD=%d;OD=%d\n" % (k_, *agg[k_]) for k_ in sorted(agg, key=lambda s: s.encode())]
    assert mine == orc.call_rows([x[0].decode() for x in refs2], [x[1] for x in refs2], reads, 12, 50)
    # argument checks of the CLI
    r = subprocess.run([exe, "call", "-r", str(fa), "-f", str(fq), "-k", "12", "-k", "16"], capture_output=True)
    assert r.returncode == 1 and b"Only a single kmer size may be used for calling." in r.stderr
    r = subprocess.run([exe, "call", "-r", str(fa), "-f", str(fq), "-k", "12", "-d"], capture_output=True)
    assert r.returncode == 0 and r.stdout == b""


def test_call_at_c5_scale(orc, root, data_dir, tmp_path):
    """C5: 1000x coverage of HPV16 (52 k reads of 150 bp) with planted SNPs and deletions, -k 12: the VCF
    rows of bin/rkmh call equal the literal restatement of main_call, twice (the depth map is filled by atomics)."""
    exe = os.path.join(root, "bin", "rkmh")
    rec, reads, fa, fq = _call_fixture(orc, data_dir, tmp_path, cov=1000, seed=9)
    rows = orc.call_rows([rec[0].decode()], [rec[1]], reads, 12, 100)
    want = orc.CALL_HEADER % str(fa) + "".join(rows)
    assert len(rows) >= 5 and len(reads) > 50000
    for rep in range(2):
        r = subprocess.run([exe, "call", "-r", str(fa), "-f", str(fq), "-k", "12"], capture_output=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout.decode() == want, rep


def test_json_sketches_roundtrip(orc, root, data_dir, golden_dir, tmp_path):
    """rkmh sketch -> JSON (schema of dump_hash_json, rkmh.cpp:489-525) -> rkmh stream -R: same lines as sketching anew."""
    import json
    exe = os.path.join(root, "bin", "rkmh")
    js = tmp_path / "refs.json"
    r = subprocess.run([exe, "sketch", "-f", os.path.join(data_dir, "zika.refs.fa.gz"), "-k", "16", "-s", "1000", "-o", str(js)],
                       capture_output=True)
    assert r.returncode == 0, r.stderr
    doc = json.load(open(js))
    refs = orc.kseq_parse_file(os.path.join(data_dir, "zika.refs.fa.gz"))
    rb, ro = orc.pack([x[1] for x in refs])
    sk, ln = orc.sketch_refs(rb, ro, [16], 1000, threads=4)
    assert len(doc) == len(refs)
    for i, d in enumerate(doc):
        assert list(d.keys()) == ["alphabet", "canonical", "hashBits", "hashPolicy", "hashSeed", "hashType", "kmer", "name", "preserveCase", "seqLen", "sketches"]
        assert d["hashPolicy"] == "fold=swap32,windows=len-k,zero=count,mask=lt,freqmax=incl,seed=42"
        assert d["name"] == refs[i][0].decode() and d["kmer"] == "16" and d["hashSeed"] == 42 and d["hashBits"] == 64
        assert d["hashType"] == "MurmurHash3_x64_128" and d["alphabet"] == "ATGC" and d["seqLen"] == len(refs[i][1])
        assert d["sketches"]["length"] == 1000 and d["sketches"]["hashes"] == [int(x) for x in sk[i, :ln[i]]]
    g = golden(golden_dir, "zika_z1")
    r = subprocess.run([exe, "stream", "-R", str(js), "-f", os.path.join(data_dir, "z1.fq.gz")], capture_output=True)
    assert r.returncode == 0, r.stderr
    want = "".join(orc.stream_line(x[1], x[0], x[2], x[3], x[4], 1000) for x in g["rows"])
    assert r.stdout.decode() == want


# RKMH_TEST_LONG=1 mixes in reads of 5-20 kb (general path: radix pre-selection, tile hasher) for soak runs
_RAND_LENS = [0, 3, 15, 16, 17, 60, 150, 150, 150, 300, 800, 1528, 1529, 1700] + \
    ([5000, 9000, 20000] if os.environ.get("RKMH_TEST_LONG") else [])


# soak: RKMH_TEST_SEEDS=2000 [RKMH_TEST_SEED_BASE=100000 for inputs no earlier run has seen]
_SEED_BASE = int(os.environ.get("RKMH_TEST_SEED_BASE", "0"))


# seeds that once failed (kept forever): 500118 = k-mer-space form, tiles of unequal reads under len-k: lanes without a window were
# queued with the k-mer at their position (a read's dropped last window is a real sketch k-mer) and counted for read 0
_REGRESSION_SEEDS = [500118]


@pytest.mark.parametrize("seed", list(range(_SEED_BASE, _SEED_BASE + int(os.environ.get("RKMH_TEST_SEEDS", "48")))) + _REGRESSION_SEEDS)
def test_randomized_differential(orc, seed):
    """Random ragged batches (lengths 0..1700, lower case, N runs, repeats, shared and duplicated references, 1-3 k-mer
    sizes, tiny to large sketches, every fold / window policy, with and without -M) against the oracle."""
    import rkmh_amd
    rng = np.random.default_rng(1000 + seed)
    fold = int(rng.integers(0, 3))
    drop = int(rng.integers(0, 2))
    nk = int(rng.integers(1, 4))
    ks = sorted(set(int(x) for x in rng.choice([8, 11, 12, 15, 16, 17, 20, 24, 31, 32, 33], size=nk, replace=False)))
    if seed % 3 == 0:
        ks = [16]
    S = int(rng.choice([1, 5, 40, 200, 1000, 3000]))
    nref = int(rng.integers(1, 40))
    many = seed % 10 == 7                                     # a large panel: the sparse-counter form of the fused kernel
    if many:
        nref = int(rng.integers(520, 1400))
    base = rand_dna(rng, 3000)
    refs = []
    for i in range(nref):
        kind = rng.integers(0, 4)
        if many and kind != 3:
            r = rand_dna(rng, int(rng.integers(40, 260))) if kind else base[: int(rng.integers(100, 400))]
        elif kind == 0:
            r = rand_dna(rng, int(rng.integers(50, 4000)))
        elif kind == 1:                                       # mutated copy of a shared ancestor: shared sketch hashes
            r = bytearray(base[: int(rng.integers(500, 3000))])
            for j in np.nonzero(rng.random(len(r)) < 0.02)[0]:
                r[j] = b"ACGT"[int(rng.integers(0, 4))]
            r = bytes(r)
        elif kind == 2:                                       # low complexity: repeated hashes inside one sketch
            unit = rand_dna(rng, int(rng.integers(1, 40)))
            r = (unit * (3000 // len(unit) + 1))[: int(rng.integers(100, 3000))]
        else:
            r = refs[int(rng.integers(0, len(refs)))] if refs else base
        refs.append(r)
    reads = []
    nreads = int(rng.integers(50, 400))
    uniform_len = int(rng.choice([0, 0, 100, 150, 251]))     # some batches of equal-length reads (the fast tile path)
    for i in range(nreads):
        src = refs[int(rng.integers(0, nref))]
        L = uniform_len if uniform_len else int(rng.choice(_RAND_LENS))
        if rng.random() < 0.15 or len(src) < L + 1:
            r = bytearray(rand_dna(rng, L))
        else:
            st = int(rng.integers(0, len(src) - L + 1))
            r = bytearray(src[st:st + L])
        for j in np.nonzero(rng.random(len(r)) < 0.01)[0]:
            r[j] = b"ACGT"[int(rng.integers(0, 4))]
        if rng.random() < 0.1 and len(r) > 20:
            a = int(rng.integers(0, len(r) - 5))
            r[a:a + int(rng.integers(1, 5))] = b"N" * 1
        if rng.random() < 0.1:
            r = bytearray(bytes(r).lower())
        if rng.random() < 0.05 and len(r) > 40:               # a read with an internal repeat: duplicate k-mers
            r = bytearray(bytes(r[:40]) * (len(r) // 40 + 1))[: len(r)]
        reads.append(bytes(r))
    rb, ro = orc.pack(refs)
    qb, qo = orc.pack(reads)
    c = rkmh_amd.Context(0, fold=fold, drop_last_window=drop)
    pol = orc.default_policy(fold=fold, drop_last_window=drop)
    try:
        c.set_references(_pad(rb), ro, ks, S)
        sk, ln = c.get_reference_sketches()
        wsk, wln = orc.sketch_refs(rb, ro, ks, S, pol, threads=4)
        assert (ln == wln).all() and (sk == wsk).all()
        got = c.classify(_pad(qb), qo)
        want = orc.classify_stream(qb, qo, ks, S, sk, ln, pol, threads=4)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (seed, ks, S, fold, drop, bad[:5], got[bad[:5]], want[bad[:5]], [len(reads[i]) for i in bad[:5]])
        if seed % 2 == 0:                                     # -M path on the same batch
            slots = 100003
            cnt = rkmh_amd.Counter(c, slots=slots)
            c.count_batch(_pad(qb), qo, cnt)
            c.set_depth_filter(cnt, 2)
            got = c.classify(_pad(qb), qo)
            c.set_depth_filter(None, 0)
            want = orc.classify_stream(qb, qo, ks, S, sk, ln, pol, threads=4, min_kmer_occ=2, counter_slots=slots)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert len(bad) == 0, ("-M", seed, ks, S, bad[:5], got[bad[:5]], want[bad[:5]])
            # the bounded forms (rk_set_min_num_bound): the mask per index key, min_num clamped -- and, at bound 0, the compact depth
            # map, which must either equal the full table's verdicts or refuse the batch because a read outgrows the sketch
            for bound in (0, int(rng.integers(1, 7))):
                c.set_min_num_bound(bound)
                c.set_depth_filter(cnt, 2)
                got = c.classify(_pad(qb), qo)
                c.set_depth_filter(None, 0)
                w = want.copy()
                w[:, 3] = np.minimum(w[:, 3], bound)
                bad = np.nonzero((got != w).any(axis=1))[0]
                assert len(bad) == 0, ("-M bounded", seed, ks, S, bound, bad[:5], got[bad[:5]], w[bad[:5]])
            c.set_min_num_bound(0)
            comp = rkmh_amd.Counter(c, slots=slots, compact=True)
            nwin = max([sum(max(0, len(r) - k + 1 - drop) for k in ks) for r in reads] + [0])
            try:
                c.count_batch(_pad(qb), qo, comp)
                refused = False
            except rkmh_amd.api.NeedFullDepthMap:
                refused = True
            assert refused == (nwin > S or max(len(r) for r in reads) > 1528), (seed, nwin, S)
            if not refused:
                c.set_depth_filter(comp, 2)
                got = c.classify(_pad(qb), qo)
                c.set_depth_filter(None, 0)
                w = want.copy()
                w[:, 3] = 0
                bad = np.nonzero((got != w).any(axis=1))[0]
                assert len(bad) == 0, ("-M compact", seed, ks, S, bad[:5], got[bad[:5]], w[bad[:5]])
            comp.destroy()
            c.set_min_num_bound(-1)
            cnt.destroy()
        if seed % 4 == 0:                                     # pass 1 in both device forms (rk_count.hip): identical tables
            import torch
            slots = int(rng.choice([1, 97, 32768, 32769, 100003, 5000000]))
            tabs = []
            try:
                for form in ("0", "1"):
                    os.environ["RKMH_COUNT_BINS"] = form
                    t = torch.zeros(slots + 8, dtype=torch.int32, device="cuda")
                    cnt = rkmh_amd.Counter(c, slots=slots, device_ptr=t.data_ptr() + 4 * (seed % 8 // 4))
                    c.count_batch(_pad(qb), qo, cnt)
                    c.count_batch(_pad(qb), qo, cnt)          # twice: the second pass adds to a table that is not zero
                    cnt.destroy()
                    tabs.append(t.cpu().numpy())
            finally:
                os.environ.pop("RKMH_COUNT_BINS", None)
            assert (tabs[0] == tabs[1]).all(), ("count forms", seed, ks, slots, int((tabs[0] != tabs[1]).sum()))
            h, _ = c.hash_batch(_pad(qb), qo, ks)
            off = seed % 8 // 4
            assert int(tabs[0][off:off + slots].sum()) == 2 * len(h) and tabs[0][:off].sum() == 0 and tabs[0][off + slots:].sum() == 0
    finally:
        c.close()


@pytest.mark.parametrize("ragged", [False, True])
def test_count_pass_is_repeatable_under_load(data_dir, ragged):
    """The -M count pass at the reference's table size (HASHTCounter(200 000 000), rkmh.cpp:739) on 1 M short reads: the
    memory pipe is full of atomics, which is when the tile prefetch of the fused kernel used to land late (a register
    copy taken before its `s_waitcnt`: every repetition then produced a different table).  The table must be the same
    in every repetition and equal the one derived from rk_hash_batch (general hashing kernel, no atomics)."""
    import torch
    import rkmh_amd
    from rkmh_amd import api, synth
    n, L, slots = 1000000, 100, 200000000
    dev = torch.device("cuda", 0)
    c = rkmh_amd.Context(0)
    try:
        refs = api.parse_files([os.path.join(data_dir, "all_pave_ref.fa.gz")])
        rb, ro = refs["bases"], refs["offsets"]
        c.set_references(rb, ro, [16], 1000)
        qb, qo = synth.generate_reads_fast(rb, ro, 0, n, read_len=L, threads=8)
        if ragged:   # unequal lengths (20..100, some shorter than k), lower case and N runs: the bitmap-walking form of the pass
            qb, qo = _ragged(qb, n, L, seed=3)
        d_b = torch.from_numpy(_pad(qb)).to(dev)
        d_o = torch.from_numpy(qo.astype(np.int64)).to(torch.int32).to(dev)
        table = torch.zeros(slots, dtype=torch.int32, device=dev)
        cnt = rkmh_amd.Counter(c, slots=slots, device_ptr=table.data_ptr())
        h, ho = c.hash_batch(_pad(qb), qo, [16])
        assert len(h) == int(ho[-1]) and (ragged or len(h) == n * (L - 16))
        want = torch.bincount(torch.from_numpy((h % np.uint64(slots)).astype(np.int64)).to(dev), minlength=slots).to(torch.int32)
        for rep in range(6):
            table.zero_()
            torch.cuda.synchronize()
            c.count_device(d_b.data_ptr(), d_o.data_ptr(), n, cnt)
            c.synchronize()
            ndiff = int((table != want).sum().item())
            assert ndiff == 0, (rep, ndiff)
        cnt.destroy()
    finally:
        c.close()


@pytest.mark.parametrize("slots,ks,ragged,unaligned", [(200000000, [16], False, False), (70000001, [20], True, False), (5000011, [12, 16], True, True),
                                                        (1009, [16], False, False), (32768 * 1024 + 5, [15], True, True)])
def test_count_pass_slot_partitioned_equals_atomic(data_dir, slots, ks, ragged, unaligned):
    """Pass 1 of -M (rkmh.cpp:904-910) in its two device forms: one global atomic per window (RKMH_COUNT_BINS=0) and the
    slot-partitioned form that counts in LDS and adds to the table with plain stores (rk_count.hip; RKMH_COUNT_BINS=1 forces it at
    any size).  Both tables must equal the bincount of rk_hash_batch's hashes modulo the table size: one sub-range only (1009 slots),
    one sub-range per bin, several per bin (200 M slots: 6), an exact multiple + 5 (a bin whose last sub-range is 5 slots), a table
    that is only 4-byte aligned, several k-mer sizes, reads of unequal length with N runs and reads shorter than k.  Two batches
    are counted into the same table from two streams without synchronising in between: the passes are chained by the library."""
    import torch
    import rkmh_amd
    from rkmh_amd import api, synth
    n, L = 150000, 100
    dev = torch.device("cuda", 0)
    c = rkmh_amd.Context(0)
    try:
        refs = api.parse_files([os.path.join(data_dir, "all_pave_ref.fa.gz")])
        rb, ro = refs["bases"], refs["offsets"]
        c.set_references(rb, ro, ks, 1000)
        batches = []
        for seed in (0, 1):
            qb, qo = synth.generate_reads_fast(rb, ro, seed * n, (seed + 1) * n, read_len=L, threads=8)
            if ragged:
                qb, qo = _ragged(qb, n, L, seed=3 + seed)
            batches.append((qb, qo))
        want = torch.zeros(slots, dtype=torch.int64, device=dev)
        want_b = []
        for qb, qo in batches:
            h, ho = c.hash_batch(_pad(qb), qo, ks)
            want_b.append(torch.bincount(torch.from_numpy((h % np.uint64(slots)).astype(np.int64)).to(dev), minlength=slots))
            want += want_b[-1]
        want = want.to(torch.int32)
        store = torch.zeros(slots + 4, dtype=torch.int32, device=dev)
        table = store[1:slots + 1] if unaligned else store[:slots]
        assert (table.data_ptr() % 16 != 0) == unaligned
        cnt = rkmh_amd.Counter(c, slots=slots, device_ptr=table.data_ptr())
        dbs = [(torch.from_numpy(_pad(qb)).to(dev), torch.from_numpy(qo.astype(np.int64)).to(torch.int32).to(dev)) for qb, qo in batches]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        try:
            for form in ("1", "0", "1"):
                os.environ["RKMH_COUNT_BINS"] = form
                store.zero_()
                torch.cuda.synchronize()
                for (d_b, d_o), st in zip(dbs, streams):
                    c.count_device(d_b.data_ptr(), d_o.data_ptr(), n, cnt, stream=st.cuda_stream)
                torch.cuda.synchronize()
                ndiff = int((table != want).sum().item())
                assert ndiff == 0, (form, ndiff)
                assert int(store[0].item()) == 0 or not unaligned
                assert int(store[slots + (1 if unaligned else 0):].abs().sum().item()) == 0   # nothing written past the table
            # mixed: a partitioned pass followed at once by an atomic one on another stream
            store.zero_()
            torch.cuda.synchronize()
            os.environ["RKMH_COUNT_BINS"] = "1"
            c.count_device(dbs[0][0].data_ptr(), dbs[0][1].data_ptr(), n, cnt, stream=streams[0].cuda_stream)
            os.environ["RKMH_COUNT_BINS"] = "0"
            c.count_device(dbs[1][0].data_ptr(), dbs[1][1].data_ptr(), n, cnt, stream=streams[1].cuda_stream)
            torch.cuda.synchronize()
            assert int((table != want).sum().item()) == 0
            # ... and the other way round: atomics still landing when the plain adds would start
            store.zero_()
            torch.cuda.synchronize()
            os.environ["RKMH_COUNT_BINS"] = "0"
            c.count_device(dbs[0][0].data_ptr(), dbs[0][1].data_ptr(), n, cnt, stream=streams[0].cuda_stream)
            os.environ["RKMH_COUNT_BINS"] = "1"
            c.count_device(dbs[1][0].data_ptr(), dbs[1][1].data_ptr(), n, cnt, stream=streams[1].cuda_stream)
            torch.cuda.synchronize()
            assert int((table != want).sum().item()) == 0
            # three streams in the order atomic, atomic, partitioned: the partitioned pass must wait for BOTH atomic passes (they
            # share one event, so the atomic passes are chained and the event of the second covers the first)
            store.zero_()
            torch.cuda.synchronize()
            s3 = streams + [torch.cuda.Stream()]
            os.environ["RKMH_COUNT_BINS"] = "0"
            c.count_device(dbs[0][0].data_ptr(), dbs[0][1].data_ptr(), n, cnt, stream=s3[0].cuda_stream)
            c.count_device(dbs[1][0].data_ptr(), dbs[1][1].data_ptr(), n, cnt, stream=s3[1].cuda_stream)
            os.environ["RKMH_COUNT_BINS"] = "1"
            c.count_device(dbs[0][0].data_ptr(), dbs[0][1].data_ptr(), n, cnt, stream=s3[2].cuda_stream)
            torch.cuda.synchronize()
            assert int((table != (2 * want_b[0] + want_b[1]).to(torch.int32)).sum().item()) == 0
        finally:
            os.environ.pop("RKMH_COUNT_BINS", None)
        cnt.destroy()
    finally:
        c.close()


@pytest.mark.parametrize("entries,k", [("5.3", 16), ("41", 16), ("17.7", 12), ("9.9", 14)])
def test_kmer_space_filter_of_any_sector_count(root, entries, k):
    """The group filter of the k-mer-space kernel has ANY number of sectors (the hashed core is scaled by a 32 x 32 high product),
    chosen by entries per sector.  The knob is read once per process, so each forced density runs in its own interpreter: 30 000
    C2 reads (1 in 1000 with an N) and 5 000 reads of unequal length against the oracle, sector counts that are no power of two,
    from far sparser to far denser than the shipped rule."""
    if os.environ.get("RKMH_KMER_PREFILTER") == "0":
        pytest.skip("the k-mer-space form is switched off for this run")
    code = r"""
import os, sys
import numpy as np
root = sys.argv[1]; k = int(sys.argv[2])
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "oracle"))
import oracle, rkmh_amd
from rkmh_amd import api, synth
refs = api.parse_files([os.path.join(root, "tests", "golden", "data", "all_pave_ref.fa.gz")])
rb, ro = refs["bases"], refs["offsets"]
ctx = rkmh_amd.Context(0)
ctx.set_references(rb, ro, [k], 1000)
assert ctx.kmer_form()[0]
sk, ln = ctx.get_reference_sketches()
qb, qo = synth.generate_reads_fast(rb, ro, 0, 30000)
assert (ctx.classify(qb, qo) == oracle.classify_stream(qb, qo, [k], 1000, sk, ln, threads=8)).all()
rng = np.random.default_rng(5)
qb2, _ = synth.generate_reads_fast(rb, ro, 40000, 45000)
lens = rng.integers(0, 151, size=5000)
offs = np.zeros(5001, np.uint64); offs[1:] = np.cumsum(lens)
b2 = np.concatenate([qb2[i * 150:i * 150 + int(lens[i])] for i in range(5000)] + [np.zeros(64, np.uint8)])
assert (ctx.classify(b2, offs) == oracle.classify_stream(b2, offs, [k], 1000, sk, ln, threads=8)).all()
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code, root, str(k)], capture_output=True, env=dict(os.environ, RKMH_KF4_ENTRIES=entries))
    assert r.returncode == 0 and r.stdout.strip().endswith(b"ok"), r.stderr.decode()[-2000:]


def test_count_pass_slot_partitioned_degenerate_batches(ctx, pave):
    """The slot-partitioned count pass on batches that stress its binning: no window at all (every read shorter than k), every
    window the same k-mer (poly-A reads: one slot receives 1.7 M increments, one bin receives every entry, the LDS rank counters of
    the counting sort run up to the chunk size), and two k-mers alternating.  Tables equal the atomic form's and the closed form."""
    import torch
    import rkmh_amd
    _, rb, ro = pave
    ctx.set_references(rb, ro, [16], 1000)
    slots = 50000017
    dev = torch.device("cuda", 0)

    def run(reads):
        qb = np.frombuffer(b"".join(reads), np.uint8)
        qo = np.zeros(len(reads) + 1, np.int64)
        np.cumsum([len(r) for r in reads], out=qo[1:])
        d_b = torch.from_numpy(_pad(qb)).to(dev)
        d_o = torch.from_numpy(qo).to(torch.int32).to(dev)
        tabs = []
        for form in ("0", "1"):
            os.environ["RKMH_COUNT_BINS"] = form
            t = torch.zeros(slots, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()   # (the fill is torch's stream's, the count pass the context's)
            cnt = rkmh_amd.Counter(ctx, slots=slots, device_ptr=t.data_ptr())
            ctx.count_device(d_b.data_ptr(), d_o.data_ptr(), len(reads), cnt)
            torch.cuda.synchronize()
            cnt.destroy()
            tabs.append(t)
        assert bool((tabs[0] == tabs[1]).all())
        return tabs[1]

    try:
        t = run([b"ACGTACGTACG"] * 5000 + [b""] * 10 + [b"ACGTTGCAACGTTGC"] * 100)      # 11 and 15 bases: no 16-mer
        assert int(t.sum().item()) == 0
        n, L = 20000, 100
        t = run([b"A" * L] * n)
        nw = int(ctx.calc_hashes(b"A" * L, [16]).shape[0])
        h = int(ctx.calc_hashes(b"A" * 16 + b"C", [16])[0]) if nw else 0
        assert nw in (84, 85) and int(t.sum().item()) == n * nw and int(t.max().item()) == n * nw
        assert int(t[int(np.uint64(ctx.calc_hashes(b"A" * L, [16])[0]) % np.uint64(slots))].item()) == n * nw and h != 0
        t = run([b"AC" * 50] * n)                                                           # two k-mers (ACAC.., CACA..), canonical forms
        hs = ctx.calc_hashes(b"AC" * 50, [16])
        want = {}
        for v in hs:
            want[int(np.uint64(v) % np.uint64(slots))] = want.get(int(np.uint64(v) % np.uint64(slots)), 0) + n
        assert int(t.sum().item()) == n * len(hs)
        for sl, c in want.items():
            assert int(t[sl].item()) == c
    finally:
        os.environ.pop("RKMH_COUNT_BINS", None)


def _ragged(qb, n, L, seed, lo=20):
    """Cuts equal-length synthetic reads to unequal lengths (lo..L, 1 % shorter than any k), adds N runs and lower case."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, L + 1, size=n)
    short = rng.random(n) < 0.01
    lens[short] = rng.integers(0, 12, size=int(short.sum()))
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    idx = np.repeat(np.arange(n, dtype=np.int64) * L - offs[:-1], lens) + np.arange(offs[-1], dtype=np.int64)
    b = qb[idx].copy()
    b[rng.random(len(b)) < 0.002] = ord("N")
    low = rng.random(len(b)) < 0.01
    b[low] = b[low] | 0x20
    return b, offs.astype(np.uint64)


@pytest.mark.parametrize("ks,depth,L", [([16], True, 150), ([15], False, 150), ([12, 16], False, 100), ([15], True, 100), ([21], True, 150),
                                        ([16], False, -150), ([16], True, -150), ([20], True, -100),
                                        ([12, 20], False, 100),          # several k, one of them outside 8..16: the hash-space multi-k kernel
                                        ([12, 14, 16], False, -150)])    # several k in k-mer space, reads of unequal length
def test_every_kernel_form_at_scale(orc, data_dir, ks, depth, L):
    """300 k reads through the fused kernel's other instantiations -- run-time k, several k, the masked (-M) form with a
    200 M-slot table -- against the oracle, three launches each.  (Randomized batches are a few hundred reads: too
    short-lived for timing-dependent faults, which is how the stale tile prefetch of the count pass stayed rare there.)"""
    import torch
    import rkmh_amd
    from rkmh_amd import api, synth
    n, S, slots = 300000, 1000, 200000000
    dev = torch.device("cuda", 0)
    c = rkmh_amd.Context(0)
    try:
        refs = api.parse_files([os.path.join(data_dir, "all_pave_ref.fa.gz")])
        rb, ro = refs["bases"], refs["offsets"]
        c.set_references(rb, ro, ks, S)
        sk, ln = c.get_reference_sketches()
        ragged = L < 0                       # negative L: reads of unequal length up to |L| (tiles walk byte positions)
        L = abs(L)
        qb, qo = synth.generate_reads_fast(rb, ro, 0, n, read_len=L, threads=8)
        if ragged:
            qb, qo = _ragged(qb, n, L, seed=L + len(ks), lo=60)
            qb = _pad(qb)
        pol = orc.default_policy()
        want = orc.classify_stream(qb, qo, ks, S, sk, ln, pol, threads=orc.max_threads(),
                                   **({"min_kmer_occ": 2, "counter_slots": slots} if depth else {}))
        d_b = torch.from_numpy(qb).to(dev)
        d_o = torch.from_numpy(qo.astype(np.int64)).to(torch.int32).to(dev)
        d_out = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        cnt = None
        if depth:
            table = torch.zeros(slots, dtype=torch.int32, device=dev)
            cnt = rkmh_amd.Counter(c, slots=slots, device_ptr=table.data_ptr())
        for rep in range(3):
            if depth:
                table.zero_()
                torch.cuda.synchronize()
                c.count_device(d_b.data_ptr(), d_o.data_ptr(), n, cnt)
                c.set_depth_filter(cnt, 2)
            d_out.zero_()
            torch.cuda.synchronize()   # (the fill runs on torch's stream, the classification on the context's: without this the fill can
                                       # land on rows the kernel has already written -- seen once in ~40 runs, with another process on the GPU)
            c.classify_device_all(d_b.data_ptr(), d_o.data_ptr(), n, d_out.data_ptr(), max_read_len=L)
            c.synchronize()
            got = d_out.cpu().numpy()
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert len(bad) == 0, (rep, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
        if depth:
            c.set_depth_filter(None, 0)
            cnt.destroy()
    finally:
        c.close()


def test_other_paths_at_scale(ctx, orc, pave):
    """The paths the randomized batches only exercise with a handful of reads, at sizes that keep the GPU busy for
    milliseconds, every row against the oracle: the host entry point (slot pipeline, pinned staging) on 300 k short
    reads; 4 000 long reads (3-9 kb: tile hasher, radix pre-selection, sort + intersect); a 700-reference panel
    (sparse per-read counters) on 40 k reads."""
    from rkmh_amd import synth
    _, rb, ro = pave
    T = orc.max_threads()
    ctx.set_references(rb, ro, [16], 1000)
    sk, ln = ctx.get_reference_sketches()
    n = 300000
    qb, qo = synth.generate_reads_fast(rb, ro, 5000000, 5000000 + n)
    want = orc.classify_stream(qb, qo, [16], 1000, sk, ln, threads=T)
    for rep in range(2):
        got = ctx.classify(_pad(qb), qo)
        assert (got == want).all(), rep
    # long reads
    rng = np.random.default_rng(12)
    reads = []
    for i in range(4000):
        r = int(rng.integers(0, 182))
        rl = int(ro[r + 1] - ro[r])
        L = min(int(rng.integers(3000, 9000)), rl)
        st = int(rng.integers(0, rl - L + 1))
        x = bytearray(rb[int(ro[r]) + st: int(ro[r]) + st + L])
        for j in np.nonzero(rng.random(L) < 0.08)[0]:               # nanopore-like error rate
            x[j] = b"ACGT"[int(rng.integers(0, 4))]
        reads.append(bytes(x))
    lb, lo_ = orc.pack(reads)
    want = orc.classify_stream(lb, lo_, [16], 1000, sk, ln, threads=T)
    for rep in range(2):
        got = ctx.classify(_pad(lb), lo_)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (rep, len(bad), got[bad[:3]], want[bad[:3]])
    # the same long reads with -M 2 (count pass and mask on the general kernels)
    import rkmh_amd
    lslots = 10000000
    lwant = orc.classify_stream(lb, lo_, [16], 1000, sk, ln, threads=T, min_kmer_occ=2, counter_slots=lslots)
    lcnt = rkmh_amd.Counter(ctx, slots=lslots)
    try:
        ctx.count_batch(_pad(lb), lo_, lcnt)
        ctx.set_depth_filter(lcnt, 2)
        for rep in range(2):
            got = ctx.classify(_pad(lb), lo_)
            bad = np.nonzero((got != lwant).any(axis=1))[0]
            assert len(bad) == 0, ("long -M", rep, len(bad), got[bad[:3]], lwant[bad[:3]])
    finally:
        ctx.set_depth_filter(None, 0)
        lcnt.destroy()
    # a large panel: 700 references derived from the bundled ones (mutated copies), 40 k reads
    prefs = []
    for i in range(700):
        r = i % 182
        x = bytearray(rb[int(ro[r]): int(ro[r + 1])][:3000])
        for j in np.nonzero(rng.random(len(x)) < 0.03 * (i // 182))[0]:
            x[j] = b"ACGT"[int(rng.integers(0, 4))]
        prefs.append(bytes(x))
    pb, po = orc.pack(prefs)
    ctx.set_references(_pad(pb), po, [16], 1000)
    psk, pln = ctx.get_reference_sketches()
    qb, qo = synth.generate_reads_fast(pb, po, 0, 40000)
    want = orc.classify_stream(qb, qo, [16], 1000, psk, pln, threads=T)
    for rep in range(2):
        got = ctx.classify(_pad(qb), qo)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (rep, len(bad), got[bad[:3]], want[bad[:3]])
    # the same panel with -M 2, through both masked kernel forms (with and without the first-level filter)
    import rkmh_amd
    slots = 10000000
    want = orc.classify_stream(qb, qo, [16], 1000, psk, pln, threads=T, min_kmer_occ=2, counter_slots=slots)
    cnt = rkmh_amd.Counter(ctx, slots=slots)
    ctx.count_batch(_pad(qb), qo, cnt)
    ctx.set_depth_filter(cnt, 2)
    try:
        for force in ("1", "0"):
            os.environ["RKMH_PRE_MASKED"] = force
            got = ctx.classify(_pad(qb), qo)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert len(bad) == 0, (force, len(bad), got[bad[:3]], want[bad[:3]])
    finally:
        os.environ.pop("RKMH_PRE_MASKED", None)
        ctx.set_depth_filter(None, 0)
        cnt.destroy()


def test_counter_serialisation(ctx, orc, root, data_dir, tmp_path):
    """Depth-map save/load.  -p itself stays a no-op as in the reference; the build's own --depth-map-cache saves/reuses a map and
    refuses one whose recorded provenance (reads, k list, hashing policy) does not match the run."""
    import rkmh_amd
    cnt = rkmh_amd.Counter(ctx, slots=100003)
    h = ctx.calc_hashes(b"ACGTTGCAAGGCTTAACCGGTTAAGGCCATATATATATATGCGCGCGC" * 4, [8], counter=cnt)
    f = tmp_path / "c.bin"
    cnt.save(str(f))
    other = rkmh_amd.Counter(ctx, slots=100003)
    other.load(str(f))
    for v in set(int(x) for x in h):
        assert other.get(v) == cnt.get(v) > 0
    wrong = rkmh_amd.Counter(ctx, slots=99991)
    with pytest.raises(rkmh_amd.RkmhError):
        wrong.load(str(f))
    for c in (cnt, other, wrong):
        c.destroy()
    exe = os.path.join(root, "bin", "rkmh")
    base = [exe, "stream", "-r", os.path.join(data_dir, "zika.refs.fa.gz"), "-f", os.path.join(data_dir, "z1.fq.gz"), "-k", "16", "-M", "2"]
    plain = subprocess.run(base, capture_output=True)
    assert plain.returncode == 0 and len(plain.stdout) > 1000
    # -p is parsed and ignored, as in the reference (rkmh.cpp:665-667, body commented out): no file appears, same lines
    ign = subprocess.run(base + ["-p", str(tmp_path / "ignored.map")], capture_output=True)
    assert ign.returncode == 0 and ign.stdout == plain.stdout and not (tmp_path / "ignored.map").exists()
    # the build's own cache flag: first run saves, second run loads instead of counting
    args = base + ["--depth-map-cache", str(tmp_path / "depth.map")]
    a = subprocess.run(args, capture_output=True)
    assert a.returncode == 0 and (tmp_path / "depth.map").exists(), a.stderr
    b = subprocess.run(args, capture_output=True)
    assert b.returncode == 0 and a.stdout == b.stdout == plain.stdout
    # a map counted from OTHER reads, or with another k, is refused with a diagnostic instead of being used
    import gzip
    recs = gzip.open(os.path.join(data_dir, "z1.fq.gz"), "rb").read().split(b"\n")
    (tmp_path / "half.fq").write_bytes(b"\n".join(recs[:4 * 400]) + b"\n")
    other_reads = [x if x != os.path.join(data_dir, "z1.fq.gz") else str(tmp_path / "half.fq") for x in args]
    r = subprocess.run(other_reads, capture_output=True)
    assert r.returncode != 0 and b"provenance" in r.stderr, r.stderr
    other_k = [x if x != "16" else "14" for x in args]
    r = subprocess.run(other_k, capture_output=True)
    assert r.returncode != 0 and b"provenance" in r.stderr, r.stderr
    # library level: tagged files need the identical tag; untagged and tagged do not mix
    qb = np.frombuffer(b"ACGTTGCAAGGCTTAACCGGTTAAGGCCATATATATATATGCGCGCGC" * 4, dtype=np.uint8)
    qo = np.array([0, 96, 192], dtype=np.uint64)
    tag = ctx.depth_map_tag([8], qb, qo)
    assert tag != ctx.depth_map_tag([9], qb, qo) and tag != ctx.depth_map_tag([8], qb, np.array([0, 95, 192], dtype=np.uint64))
    # the fingerprint covers EVERY base: one substitution in the middle of a 40 MB read set with unchanged lengths is another read set
    big = np.frombuffer(rand_dna(np.random.default_rng(77), 40000000), dtype=np.uint8).copy()
    bo = np.arange(0, 40000001, 100, dtype=np.uint64)
    t_big = ctx.depth_map_tag([16], big, bo)
    assert t_big == ctx.depth_map_tag([16], big.copy(), bo)
    edited = big.copy()
    edited[20000001] = ord("A") if edited[20000001] != ord("A") else ord("C")
    assert t_big != ctx.depth_map_tag([16], edited, bo)
    cnt = rkmh_amd.Counter(ctx, slots=100003)
    cnt.increment(12345)
    cnt.save(str(tmp_path / "t.bin"), tag=tag)
    cnt.load(str(tmp_path / "t.bin"), tag=tag)
    assert cnt.get(12345) == 1
    with pytest.raises(rkmh_amd.RkmhError):
        cnt.load(str(tmp_path / "t.bin"))
    with pytest.raises(rkmh_amd.RkmhError):
        cnt.load(str(tmp_path / "t.bin"), tag=ctx.depth_map_tag([9], qb, qo))
    with pytest.raises(rkmh_amd.RkmhError):
        cnt.load(str(f), tag=tag)   # f is the untagged file from above
    # round-1 files ("RKHT1", no tag field) still load as untagged
    v1 = tmp_path / "v1.bin"
    import struct
    v1.write_bytes(b"RKHT1\n" + struct.pack("<QQ", 100003, 1) + struct.pack("<Ii", 7, 5))
    cnt.load(str(v1))
    assert cnt.get(7) == 5 and cnt.get(12345) == 0
    cnt.destroy()


def test_panel_too_large_for_lds_counters(orc):
    """45 000 references: beyond the fused kernel (16 384) and beyond what one block's LDS holds as a dense counter row,
    so the general path counts in global rows (SortArgs::gcount).  Short and long reads, every row against the oracle."""
    import rkmh_amd
    T = min(16, os.cpu_count() or 1)
    rng = np.random.default_rng(77)
    nref, S = 45000, 16
    genome = rand_dna(rng, 60 * nref + 200, b"ACGT")
    refs = [genome[60 * i: 60 * i + 90] for i in range(nref)]      # neighbours overlap by 30 bases: shared hashes, ties
    rb, ro = orc.pack(refs)
    reads = []
    for i in range(300):
        a = int(rng.integers(0, len(genome) - 700))
        n = int(rng.choice([40, 150, 600]))
        reads.append(genome[a: a + n])
    reads += [b"", b"ACGT", b"N" * 50]
    qb, qo = orc.pack(reads)
    c = rkmh_amd.Context(0)
    try:
        c.set_references(_pad(rb), ro, [16], S)
        sk, ln = c.get_reference_sketches()
        wsk, wln = orc.sketch_refs(rb, ro, [16], S, threads=T)
        assert (sk == wsk).all() and (ln == wln).all()
        want = orc.classify_stream(qb, qo, [16], S, wsk, wln, threads=T)
        for rep in range(2):
            got = c.classify(_pad(qb), qo)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert len(bad) == 0, (rep, len(bad), got[bad[:3]], want[bad[:3]])
        assert (want[:, 1] > 0).sum() > 200
    finally:
        c.close()


def _hpv16_inputs(orc, data_dir, n_synth=300, seed=5):
    types = orc.kseq_parse_file(os.path.join(data_dir, "all_pave_ref.fa.gz"))
    subs = orc.kseq_parse_file(os.path.join(data_dir, "new_refs.fa.gz"))
    rng = np.random.default_rng(seed)
    reads = []
    for i in range(n_synth):   # reads drawn from the HPV16 sublineage genomes (1 % substitutions, either strand, some with an N)
        name, seq = subs[int(rng.integers(0, len(subs)))][:2]
        seq = orc.to_upper(seq)
        L = int(rng.choice([60, 150, 250, 400]))
        a = int(rng.integers(0, len(seq) - L))
        r = bytearray(seq[a: a + L])
        for p in np.nonzero(rng.random(L) < 0.01)[0]:
            r[p] = b"ACGT"[int(rng.integers(0, 4))]
        if i % 50 == 7:
            r[int(rng.integers(0, L))] = ord("N")
        if i % 9 == 0:
            r = bytearray(bytes(r).lower())
        if rng.random() < 0.5:
            r = bytearray(bytes(r)[::-1].translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca")))
        reads.append((b"s%04d_%s" % (i, name), bytes(r)))
    reads += [(b"empty", b""), (b"short", b"ACGTACGT"), (b"polyA", b"A" * 80)]
    return types, subs, reads


@pytest.mark.parametrize("ks,extra", [([16], []), ([12, 16], []), ([16], ["-M", "2"])])
def test_hpv16_command_against_the_oracle(orc, root, data_dir, tmp_path, ks, extra):
    """bin/rkmh hpv16 (rkmh.cpp:2366-2723) == oracle.hpv16 byte for byte: stdout, the lineage .tst file, the stderr tables.
    Reads: synthetic HPV16 sublineage reads (incl. lower case, N, other strand), the reference's own nanopore reads (long), and
    reads of an unrelated virus (no matches at all)."""
    types, subs, reads = _hpv16_inputs(orc, data_dir)
    reads += [r[:2] for r in orc.kseq_parse_file(os.path.join(data_dir, "minION25.fq.gz"))[:6]]
    reads += [r[:2] for r in orc.kseq_parse_file(os.path.join(data_dir, "z1.fq.gz"))[:40]]
    # a rolling-circle read: three copies of an HPV16 genome (23.7 kb: more k-mers than the batched path's sorter holds)
    reads.append((b"rolling_circle", orc.to_upper(subs[0][1]) * 3))
    fq = tmp_path / "reads.fa"
    fq.write_bytes(b"".join(b">" + n + b"\n" + s + b"\n" for n, s in reads))
    args = [os.path.join(root, "bin", "rkmh"), "hpv16", "-f", str(fq), "-R", data_dir]
    for k in ks:
        args += ["-k", str(k)]
    r = subprocess.run(args + extra, capture_output=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    mo = 2 if extra else None
    want, tst, err = orc.hpv16([t[0] for t in types], [t[1] for t in types], [t[0] for t in subs], [t[1] for t in subs],
                               [x[0] for x in reads], [x[1] for x in reads], ks, min_kmer_occ=mo)
    got = r.stdout.decode().splitlines(keepends=True)
    assert len(got) == len(want) == len(reads)
    for g, w in zip(got, want):
        assert g == w
    assert (tmp_path / ("lineage_specific_hashes.%d.tst" % ks[0])).read_text() == tst
    assert [l for l in r.stderr.decode().splitlines() if l.startswith("\t") or "kmer table created" in l] == err
    # the workload means something: most synthetic reads name HPV16 and match their own lineage best
    hits = [w.split("\t") for w in want[:300]]
    assert sum(1 for h in hits if h[1].startswith(b"gi|333031".decode()) or "HPV16" in h[1]) > 250
    assert sum(1 for h, (n, _) in zip(hits, reads[:300]) if h[3].split(":")[0] == n.decode().split("_")[1][0]) > 150


def test_classify_groups_entry_point(orc, data_dir):
    """rk_classify_groups_batch: argmax over the first references only, raw set-intersection counts for the rest; a read with more
    hashes than the list capacity is refused instead of being bottom-s truncated."""
    import rkmh_amd
    rng = np.random.default_rng(3)
    genome = rand_dna(rng, 6000, b"ACGT")
    lists_src = [genome[0:2000], genome[1500:3500], genome[3000:5000], genome[4000:6000], genome[500:900]]
    k, S = 16, 4096
    lists = np.zeros((len(lists_src), S), dtype=np.uint64)
    lens = np.zeros(len(lists_src), dtype=np.int32)
    full = []
    for i, s in enumerate(lists_src):
        h = np.unique(orc.calc_hashes(s, [k]))
        h = h[h != 0]
        lists[i, : len(h)] = h
        lens[i] = len(h)
        full.append(h)
    reads = [genome[a: a + n] for a, n in ((100, 300), (1600, 200), (1600, 200), (4100, 1000), (0, 20), (5000, 700))] + [b"ACGT" * 50, b""]
    qb, qo = orc.pack(reads)
    c = rkmh_amd.Context(0)
    try:
        c.set_reference_sketches(lists, lens, [k], S)
        out, tail = c.classify_groups(_pad(qb), qo, 3)
        for i, r in enumerate(reads):
            h = np.sort(orc.calc_hashes(orc.to_upper(r), [k]))
            cnt = [orc.hash_set_intersection_size(h, f) for f in full]
            best = int(np.argmax(cnt[:3])) if len(h) else 0
            assert out[i, 0] == best and out[i, 1] == cnt[best] and out[i, 3] == int((h != 0).sum()), (i, out[i], cnt)
            assert list(tail[i]) == cnt[3:], (i, tail[i], cnt)
        with pytest.raises(rkmh_amd.RkmhError):
            c.classify_groups(_pad(np.frombuffer(rand_dna(rng, 5000, b"ACGT"), dtype=np.uint8)), np.array([0, 5000], dtype=np.uint64), 3)
    finally:
        c.close()


def test_hpv16_cli_matches_committed_golden(root, data_dir, golden_dir, tmp_path):
    """bin/rkmh hpv16 on the reference's bundled nanopore reads == tests/golden/hpv16_minion25.json (stdout, stderr tables, .tst)."""
    import hashlib
    g = json.load(open(os.path.join(golden_dir, "hpv16_minion25.json")))
    r = subprocess.run([os.path.join(root, "bin", "rkmh"), "hpv16", "-f", os.path.join(data_dir, g["reads_file"]), "-R", data_dir, "-k", "16"],
                       capture_output=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout.decode().splitlines(keepends=True) == g["stdout_lines"]
    assert [l for l in r.stderr.decode().splitlines() if l.startswith("\t") or "kmer table created" in l] == g["stderr_tables"]
    assert hashlib.sha256((tmp_path / "lineage_specific_hashes.16.tst").read_bytes()).hexdigest() == g["tst_sha256"]


@pytest.mark.parametrize("k,fold,drop", [(16, 0, 1), (16, 1, 1), (16, 2, 0), (16, 0, 0), (12, 0, 1), (12, 1, 0), (8, 0, 1), (9, 2, 0),
                                         (10, 0, 1), (11, 1, 1), (13, 0, 0), (14, 2, 1), (15, 0, 1)])
def test_kmer_space_form_every_policy(orc, pave, k, fold, drop):
    """The k-mer-space form of the fused kernel (MODE_ 5: windows filtered and resolved by packed k-mer, no hashing) for every
    fold / window policy and both k it exists for: active, and every row equal to the oracle on 150 bp reads (plain tiles),
    reads of unequal length with N / lower case (the other loop form inside the same kernel) and reads shorter than k."""
    import rkmh_amd
    from rkmh_amd import synth
    _, rb, ro = pave
    T = min(16, os.cpu_count() or 1)
    pol = orc.default_policy(fold=fold, drop_last_window=drop)
    c = rkmh_amd.Context(0, fold=fold, drop_last_window=drop)
    try:
        c.set_references(rb, ro, [k], 1000)
        active, found = c.kmer_form()
        assert active and found > (100000 if k >= 12 else 1000)   # (4^8 / 2 k-mers exist at k = 8)
        sk, ln = c.get_reference_sketches()
        wsk, wln = orc.sketch_refs(rb, ro, [k], 1000, policy=pol, threads=T)
        assert (sk == wsk).all() and (ln == wln).all()
        # every sketch hash of a real sequence has its source k-mer as a preimage, so found >= distinct keys; equality says that the
        # WHOLE 4^k universe holds no second k-mer hashing to any key (and none hashing to 0) -- true for this panel at every k >= 12
        distinct = len(np.unique(sk[sk != 0]))
        assert found >= distinct
        if k >= 12:
            assert found == distinct, (found, distinct)
        qb, qo = synth.generate_reads_fast(rb, ro, 7000, 7000 + 60000)
        want = orc.classify_stream(qb, qo, [k], 1000, wsk, wln, policy=pol, threads=T)
        got = c.classify(_pad(qb), qo)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (len(bad), got[bad[:3]], want[bad[:3]])
        rng = np.random.default_rng(k * 10 + fold)
        reads = []
        for i in range(3000):
            L = int(rng.integers(0, 170))
            a = int(rng.integers(0, len(rb) - 400))
            r = bytearray(bytes(rb[a: a + L]))
            if i % 7 == 0 and L > 3:
                r[int(rng.integers(0, L))] = ord("N")
            reads.append(bytes(r))
        qb2, qo2 = orc.pack(reads)
        want = orc.classify_stream(qb2, qo2, [k], 1000, wsk, wln, policy=pol, threads=T)
        got = c.classify(_pad(qb2), qo2)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (len(bad), got[bad[:3]], want[bad[:3]])
    finally:
        c.close()


@pytest.mark.parametrize("ks,fold,drop", [([12, 16], 0, 1), ([8, 16], 1, 0), ([12, 14, 16], 0, 1), ([9, 10, 11, 12, 13, 14, 15, 16], 2, 1), ([16, 10], 0, 0)])
def test_kmer_space_form_several_k(orc, pave, ks, fold, drop):
    """Several k-mer sizes, each from 8 to 16 (the reference's `-k 12 -k 16` usage, rkmh.cpp:680-682): one filter + map per size, the
    tile's windows walked once per size over the same per-read counters.  Active, and every row equal to the oracle on 150 bp reads,
    on reads of unequal length with N / lower case and reads shorter than the sizes, for several fold / window policies and for the
    largest number of sizes the ABI takes."""
    import rkmh_amd
    from rkmh_amd import synth
    _, rb, ro = pave
    T = min(16, os.cpu_count() or 1)
    pol = orc.default_policy(fold=fold, drop_last_window=drop)
    c = rkmh_amd.Context(0, fold=fold, drop_last_window=drop)
    try:
        c.set_references(rb, ro, ks, 1000)
        active, found = c.kmer_form()
        assert active and found > 1000
        sk, ln = c.get_reference_sketches()
        wsk, wln = orc.sketch_refs(rb, ro, ks, 1000, policy=pol, threads=T)
        assert (sk == wsk).all() and (ln == wln).all()
        qb, qo = synth.generate_reads_fast(rb, ro, 9000, 9000 + 40000)
        want = orc.classify_stream(qb, qo, ks, 1000, wsk, wln, policy=pol, threads=T)
        got = c.classify(_pad(qb), qo)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (len(bad), got[bad[:3]], want[bad[:3]])
        rng = np.random.default_rng(len(ks) * 10 + fold)
        reads = []
        for i in range(3000):
            L = int(rng.integers(0, 170))
            a = int(rng.integers(0, len(rb) - 400))
            r = bytearray(bytes(rb[a: a + L]))
            if i % 7 == 0 and L > 3:
                r[int(rng.integers(0, L))] = ord("N")
            if i % 11 == 0:
                r = bytearray(bytes(r).lower())
            reads.append(bytes(r))
        qb2, qo2 = orc.pack(reads)
        want = orc.classify_stream(qb2, qo2, ks, 1000, wsk, wln, policy=pol, threads=T)
        got = c.classify(_pad(qb2), qo2)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (len(bad), got[bad[:3]], want[bad[:3]])
    finally:
        c.close()


def test_kmer_space_form_with_imported_sketches_and_keys_without_a_preimage(orc):
    """The enumeration works from the sketch HASHES alone: imported sketches (the multi-GPU broadcast, -R files) get the k-mer-space
    form too, and a sketch hash that no k-mer of the universe produces (random 64-bit values here) simply never matches --
    exactly what the oracle's merge says."""
    import rkmh_amd
    rng = np.random.default_rng(11)
    genome = rand_dna(rng, 30000, b"ACGT")
    refs = [genome[i * 5000: i * 5000 + 6000] for i in range(5)]
    S = 512
    sk = np.zeros((len(refs) + 1, S), dtype=np.uint64)
    ln = np.zeros(len(refs) + 1, dtype=np.int32)
    for i, r in enumerate(refs):
        m = orc.minhashes(orc.calc_hashes(r, [16]), S)
        m[::3] = np.sort(rng.integers(1, 2**63, size=len(m[::3]), dtype=np.uint64))   # a third of the entries: no preimage
        m = np.sort(m)
        sk[i, : len(m)] = m
        ln[i] = len(m)
    fake = np.sort(rng.integers(1, 2**63, size=S, dtype=np.uint64))                    # a reference made of nothing real
    sk[-1] = fake
    ln[-1] = S
    reads = [genome[a: a + 150] for a in rng.integers(0, len(genome) - 150, size=5000)]
    qb, qo = orc.pack(reads)
    c = rkmh_amd.Context(0)
    try:
        c.set_reference_sketches(sk, ln, [16], S)
        active, found = c.kmer_form()
        real = len(np.unique(np.concatenate([orc.calc_hashes(r, [16]) for r in refs])))
        assert active and 0 < found < real   # only keys that ARE some k-mer's hash were found
        want = orc.classify_stream(qb, qo, [16], S, sk, ln, threads=8)
        got = c.classify(_pad(qb), qo)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (len(bad), got[bad[:3]], want[bad[:3]])
        assert (want[:, 1] > 0).mean() > 0.5 and (want[:, 0] != len(refs)).all()
    finally:
        c.close()


def test_kmer_space_form_steps_aside_when_the_map_cannot_be_built(orc, pave):
    """If two k-mers ever shared a sketch hash the exact k-mer map is not built and the hash-space kernels serve the panel (forced
    here through RKMH_KMAP_FORCE_DUP): same rows."""
    import rkmh_amd
    from rkmh_amd import synth
    _, rb, ro = pave
    qb, qo = synth.generate_reads_fast(rb, ro, 100, 20100)
    rows = []
    for force in (False, True):
        if force:
            os.environ["RKMH_KMAP_FORCE_DUP"] = "1"
        try:
            c = rkmh_amd.Context(0)
            c.set_references(rb, ro, [16], 1000)
            assert c.kmer_form()[0] == (not force)
            rows.append(c.classify(_pad(qb), qo))
            c.close()
        finally:
            os.environ.pop("RKMH_KMAP_FORCE_DUP", None)
    assert (rows[0] == rows[1]).all()


def test_idle_lanes_never_reach_the_drain_as_kmers(orc, pave):
    """Regression (k-mer-space form, the loop form for tiles that are not plain): with a SATURATED hash-space filter every lane
    passes it, including lanes that hold no window.  Such a lane must not be queued: its entry would be the k-mer at the lane's
    position -- under len-k the dropped last window of a read is a real sketch k-mer -- counted for read 0 of the tile."""
    import rkmh_amd
    _, rb, ro = pave
    T = min(16, os.cpu_count() or 1)
    rng = np.random.default_rng(8)
    reads = []
    for i in range(4000):   # error-free reads cut from the references (their last window hits with high probability), lengths 99 / 100
        r = int(rng.integers(0, len(ro) - 1))
        L = 100 - (i % 2)
        a = int(rng.integers(int(ro[r]), int(ro[r + 1]) - L))
        reads.append(orc.to_upper(bytes(rb[a: a + L])))
    qb, qo = orc.pack(reads)
    os.environ["RKMH_PRE_MAXKB"] = "16"          # 131072 filter bits for 163 k keys x 2 bits: ~92 % of the bits set
    try:
        for drop in (1, 0):
            c = rkmh_amd.Context(0, drop_last_window=drop)
            pol = orc.default_policy(drop_last_window=drop)
            c.set_references(rb, ro, [16], 1000)
            assert c.kmer_form()[0]
            sk, ln = c.get_reference_sketches()
            want = orc.classify_stream(qb, qo, [16], 1000, sk, ln, policy=pol, threads=T)
            got = c.classify(_pad(qb), qo)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert len(bad) == 0, (drop, len(bad), bad[:8], got[bad[:4]], want[bad[:4]])
            c.close()
    finally:
        os.environ.pop("RKMH_PRE_MAXKB", None)


def test_enumeration_finds_exactly_the_preimages(orc, pave):
    """k_enum_kmers against an independent enumeration by the oracle at k = 8 (65 536 k-mers): the number of strand pairs whose
    canonical hash is a key of the index (or 0) must be exactly what the GPU reports -- for sketched references and for imported
    sketches in which half the hashes were replaced by values no 8-mer produces."""
    import itertools
    import rkmh_amd
    _, rb, ro = pave
    k, S = 8, 300
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    canon_hash = {}
    for t in itertools.product(b"ACGT", repeat=k):
        s = bytes(t)
        r = s.translate(comp)[::-1]
        if s <= r:
            canon_hash[s] = orc.calc_hash(s)          # the oracle's canonical hash of the pair {s, revcomp(s)}
    assert len(canon_hash) == (4 ** k + 4 ** (k // 2)) // 2   # pairs + palindromes
    c = rkmh_amd.Context(0)
    try:
        c.set_references(rb, ro, [k], S)
        sk, ln = c.get_reference_sketches()
        keys = set(int(x) for i in range(len(ln)) for x in sk[i, : ln[i]])
        want = sum(1 for h in canon_hash.values() if h in keys or h == 0)
        active, found = c.kmer_form()
        assert active and found == want and want > 1000
        rng = np.random.default_rng(4)
        sk2 = sk.copy()
        for i in range(len(ln)):
            m = sk2[i, : ln[i]]
            m[::2] = rng.integers(1, 2**63, size=len(m[::2]), dtype=np.uint64)
            sk2[i, : ln[i]] = np.sort(m)
        c.set_reference_sketches(sk2, ln, [k], S)
        keys2 = set(int(x) for i in range(len(ln)) for x in sk2[i, : ln[i]])
        want2 = sum(1 for h in canon_hash.values() if h in keys2 or h == 0)
        active, found = c.kmer_form()
        assert active and found == want2 and 0 < want2 < want
    finally:
        c.close()


@pytest.mark.parametrize("slots", [1, 2, 3, 65537, 99999989, 1 << 20])
def test_depth_filter_with_unusual_table_sizes(orc, pave, slots):
    """-M end to end (count pass + keep bitmap + masked classify) for table sizes that stress hash % slots (mod_slots: Barrett
    reduction with a host-supplied reciprocal -- 1 slot, tiny, a Fermat prime, a large prime, a power of two), both masked kernel
    forms, against the oracle with the same table size."""
    import rkmh_amd
    from rkmh_amd import synth
    _, rb, ro = pave
    T = min(16, os.cpu_count() or 1)
    qb, qo = synth.generate_reads_fast(rb, ro, 31000, 31000 + 6000)
    c = rkmh_amd.Context(0)
    try:
        c.set_references(rb, ro, [16], 1000)
        sk, ln = c.get_reference_sketches()
        for min_occ in (2, 40):
            want = orc.classify_stream(qb, qo, [16], 1000, sk, ln, threads=T, min_kmer_occ=min_occ, counter_slots=slots)
            cnt = rkmh_amd.Counter(c, slots=slots)
            c.count_batch(_pad(qb), qo, cnt)
            c.set_depth_filter(cnt, min_occ)
            try:
                for force in ("0", "1"):
                    os.environ["RKMH_PRE_MASKED"] = force
                    got = c.classify(_pad(qb), qo)
                    bad = np.nonzero((got != want).any(axis=1))[0]
                    assert len(bad) == 0, (slots, min_occ, force, len(bad), got[bad[:3]], want[bad[:3]])
            finally:
                os.environ.pop("RKMH_PRE_MASKED", None)
                c.set_depth_filter(None, 0)
                cnt.destroy()
    finally:
        c.close()


def test_depth_filter_after_a_count_pass_on_another_stream(ctx, orc, pave):
    """rk_count_batch_device is asynchronous on the CALLER's stream; rk_set_depth_filter snapshots the table into a keep bitmap.
    The snapshot must see the finished pass 1 even when that ran on a stream the context does not own: the
    masked classification right after it equals the oracle's two-pass result, with the reference's 200 M-slot table so the
    count pass is long enough to still be running when the filter is set."""
    import torch
    import rkmh_amd
    from rkmh_amd import synth
    _, rb, ro = pave
    n = 300000
    qb, qo = synth.generate_reads_fast(rb, ro, 0, n)
    ctx.set_references(rb, ro, [20], 1000)     # k = 20: the masked hash-space kernels
    sk, ln = ctx.get_reference_sketches()
    want = orc.classify_stream(qb, qo, [20], 1000, sk, ln, threads=orc.max_threads(), min_kmer_occ=2, counter_slots=200000000)
    d_b = torch.from_numpy(qb).cuda()
    d_o = torch.from_numpy(qo.astype(np.int64)).to(torch.int32).cuda()
    d_out = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    for rep in range(3):
        cnt = rkmh_amd.Counter(ctx, slots=200000000)
        ctx.count_device(d_b.data_ptr(), d_o.data_ptr(), n, cnt, stream=side.cuda_stream)   # no synchronisation here, on purpose
        ctx.set_depth_filter(cnt, 2)
        try:
            ctx.classify_device_all(d_b.data_ptr(), d_o.data_ptr(), n, d_out.data_ptr(), max_read_len=150, stream=side.cuda_stream)
            side.synchronize()
            got = d_out.cpu().numpy()
        finally:
            ctx.set_depth_filter(None, 0)
            cnt.destroy()
        assert (got == want).all(), (rep, np.nonzero((got != want).any(axis=1))[0][:10])


def test_c4_filter_k20_s2000_against_megabase_references(orc, root, data_dir, tmp_path):
    """BASELINE config 4 in miniature (`filter`, k = 20, s = 2000, with and without -M 2, large references): 24
    synthetic 1.5 Mb sequences + the HPV16 variant genomes as references, 60 000 reads -- 90 % drawn from the synthetic genome,
    10 % HPV16 reads and reads that match nothing -- through bin/rkmh filter; stdout byte-identical to the oracle's restatement of
    classify_and_count_diff_filter (equiv.hpp:324-353) over the rows of the stream loop, 10 M-slot counters as rkmh.cpp:1187-1188."""
    from rkmh_amd import synth
    exe = os.path.join(root, "bin", "rkmh")
    rng = np.random.default_rng(44)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    chrom, nchrom, n = 1500000, 24, 60000
    refs = [(b"chr%d" % (c + 1), acgt[rng.integers(0, 4, size=chrom, dtype=np.uint8)].tobytes()) for c in range(nchrom)]
    hpv = [(r[0], r[1]) for r in orc.kseq_parse_file(os.path.join(data_dir, "hpv_16_allFasta.fa.gz"))]
    refs += hpv
    ref_fa = tmp_path / "genome.fa"
    with open(ref_fa, "wb") as f:
        for name, seq in refs:
            f.write(b">" + name + b"\n")
            for i in range(0, len(seq), 60000):     # multi-line FASTA records
                f.write(seq[i:i + 60000] + b"\n")
    gb, go = orc.pack([r[1] for r in refs[:nchrom]])
    hb, ho = orc.pack([orc.to_upper(r[1]) for r in hpv])
    nh = n // 10
    q1, _ = synth.generate_reads_fast(_pad(gb), go, 0, n - nh)
    q2, _ = synth.generate_reads_fast(_pad(hb), ho, 0, nh)
    seqs = [bytes(q1[i * 150:(i + 1) * 150]) for i in range(n - nh)] + [bytes(q2[i * 150:(i + 1) * 150]) for i in range(nh)]
    for i in range(0, n, 13):
        seqs[i] = rand_dna(rng, 150)              # reads that match nothing
    seqs[7] = seqs[7].lower()
    order = rng.permutation(n)
    seqs = [seqs[i] for i in order]
    names = [b"m%07d" % i for i in range(n)]
    q = b"I" * 150
    fq = tmp_path / "mixed.fq"
    fq.write_bytes(b"".join(b"@" + names[i] + b"\n" + seqs[i] + b"\n+\n" + q + b"\n" for i in range(n)))
    # the oracle: reference sketches once, then the stream rows with and without the depth mask
    rb, ro = orc.pack([orc.to_upper(x[1]) for x in refs])
    qb, qo = orc.pack(seqs)
    sk, ln = orc.sketch_refs(rb, ro, [20], 2000, threads=orc.max_threads())
    assert int(ln.min()) == 2000
    for flags, kw, mm in (([], {}, -1), (["-M", "2", "-N", "5"], dict(min_kmer_occ=2, counter_slots=10000000), 5)):
        rows = orc.classify_stream(qb, qo, [20], 2000, sk, ln, threads=orc.max_threads(), **kw)
        parts = [orc.filter_record(names[i], orc.to_upper(seqs[i]), q) for i in range(n) if orc.filter_decision(rows[i], mm, 0)[3]]
        assert n // 20 < len(parts) < n, (flags, len(parts))
        r = subprocess.run([exe, "filter", "-r", str(ref_fa), "-f", str(fq), "-k", "20", "-s", "2000"] + flags, capture_output=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout == b"".join(parts), (flags, len(r.stdout), sum(map(len, parts)))


def test_c3_sized_resident_shard(ctx, orc, data_dir):
    """BASELINE config 3, one GPU's share: 12.5 M synthetic 150 bp reads (a 1.9 GB resident shard) against every bundled
    reference (~270 viral genomes, k = 16, s = 1000) in ONE rk_classify_batch_device call; 60 000 rows sampled across the whole
    shard equal the oracle, no row is handed back, and the launch is repeatable."""
    import torch
    from rkmh_amd import synth
    seqs = []
    for f in ("all_pave_ref.fa.gz", "zika.refs.fa.gz", "dengue.fa.gz", "new_refs.fa.gz", "hpv_16.fa.gz",
              "zika.fa.gz", "yellow_fever.fa.gz", "hpv_16_allFasta.fa.gz"):
        seqs += [r[1] for r in orc.kseq_parse_file(os.path.join(data_dir, f))]
    rb, ro = orc.pack(seqs)
    rb = _pad(rb)
    n = 12500000
    qb, qo = synth.generate_reads_fast(rb, ro, 0, n, threads=min(16, os.cpu_count() or 1))
    ctx.set_references(rb, ro, [16], 1000)
    assert ctx.kmer_form()[0]
    sk, ln = ctx.get_reference_sketches()
    d_b = torch.from_numpy(qb).cuda()
    d_o = torch.from_numpy(qo.astype(np.int64)).to(torch.int32).cuda()
    d_out = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ctx.classify_device(d_b.data_ptr(), d_o.data_ptr(), n, d_out.data_ptr(), max_read_len=150, stream=st)
    torch.cuda.synchronize()
    first = d_out.cpu().numpy()
    assert not (first[:, 0] == -2).any()
    d_out.zero_()
    ctx.classify_device(d_b.data_ptr(), d_o.data_ptr(), n, d_out.data_ptr(), max_read_len=150, stream=st)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == first).all()
    rng = np.random.default_rng(12)
    blocks = np.sort(rng.choice(n // 1000, size=60, replace=False))          # sixty runs of 1000 consecutive reads
    for b in blocks:
        lo = int(b) * 1000
        sub_o = qo[lo:lo + 1001] - qo[lo]
        want = orc.classify_stream(qb[int(qo[lo]):int(qo[lo + 1000]) + 8], sub_o, [16], 1000, sk, ln, threads=orc.max_threads())
        assert (first[lo:lo + 1000] == want).all(), lo


def test_cli_devices_matches_single_device(orc, root, data_dir, tmp_path):
    """bin/rkmh --devices (several GPUs inside one process: one host thread + rk_ctx per device, sketches built once and imported,
    -M depth tables summed between the passes, batches written back in input order).  On a one-GPU box the same device is listed
    twice or three times: stdout must be byte-identical to the single-device run for stream, stream -M, filter -M and filter -I,
    on a FASTQ large enough for several parser batches."""
    from rkmh_amd import synth, api
    exe = os.path.join(root, "bin", "rkmh")
    n = 2300000          # > two parser batches of 2^20 records
    refs = orc.kseq_parse_file(os.path.join(data_dir, "all_pave_ref.fa.gz"))[:60]
    ref_fa = tmp_path / "refs.fa"
    ref_fa.write_bytes(b"".join(b">" + r[0] + b"\n" + r[1] + b"\n" for r in refs))
    R = api.parse_files([str(ref_fa)])
    qb, _ = synth.generate_reads_fast(R["bases"], R["offsets"], 0, n)
    rec = np.empty((n, 11 + 150 + 3 + 150 + 1), dtype=np.uint8)
    rec[:, 0] = ord("@"); rec[:, 1] = ord("r"); rec[:, 10] = 10; rec[:, 161] = 10
    idx = np.arange(n, dtype=np.int64)
    for d in range(8):
        rec[:, 9 - d] = 48 + (idx // 10 ** d) % 10
    rec[:, 2] = 48
    rec[:, 11:161] = qb[: n * 150].reshape(n, 150)
    rec[:, 162] = ord("+"); rec[:, 163] = 10; rec[:, 164:314] = ord("I"); rec[:, 314] = 10
    fq = tmp_path / "reads.fq"
    fq.write_bytes(rec.tobytes())
    small = tmp_path / "small.fq"
    small.write_bytes(rec[:200000].tobytes())

    def run(args):
        r = subprocess.run([exe] + args, capture_output=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout
    base = ["-r", str(ref_fa), "-k", "16", "-s", "1000"]
    one = run(["stream"] + base + ["-f", str(fq)])
    assert one.count(b"\n") == n
    assert run(["stream"] + base + ["-f", str(fq), "--devices", "0,0"]) == one
    assert run(["stream"] + base + ["-f", str(fq), "--devices", "0,0,0"]) == one
    for cmd, flags in (("stream", ["-M", "2"]), ("filter", ["-M", "2", "-N", "3"]), ("filter", ["-I", "2", "-D", "1"]), ("filter", [])):
        single = run([cmd] + base + ["-f", str(small)] + flags)
        assert len(single) > 0
        assert run([cmd] + base + ["-f", str(small)] + flags + ["--devices", "0,0"]) == single, (cmd, flags)
        assert run([cmd] + base + ["-f", str(small)] + flags + ["--devices", "0,0,0"]) == single, (cmd, flags)
