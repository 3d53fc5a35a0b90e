"""dedup=distinct against its multiset twin on config 2 (1 M synthetic 150 bp reads against the 182-genome panel, k = 16, s = 1000):
the DEDUP forms of k_classify_tile against the forms each policy runs without the key (k_classify_kmer, and k_classify_tile with the
k-mer-space form switched off), and the distinct bottom-S against the multiset one: set_references (block pre-select behind the
de-duplication pass) and rk_minhashes on 16 384 / 4 M hashes.  Usage: [N=1000000] python tools/bench_dedup.py"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import rkmh_amd
from rkmh_amd import api, synth
refs = api.parse_files([os.path.join(ROOT, "tests/golden/data/all_pave_ref.fa.gz")])
rb, ro = refs["bases"], refs["offsets"]
n = int(os.environ.get("N", "1000000"))
qb, qo = synth.generate_reads_fast(rb, ro, 0, n)
d_b = torch.from_numpy(qb).cuda(); d_o = torch.from_numpy(qo.astype(np.int64)).to(torch.int32).cuda()
st = torch.cuda.Stream()


def timed(f, reps=20):
    for _ in range(5):
        f()
    st.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(st):
        e0.record(st)
        for _ in range(reps):
            f()
        e1.record(st)
    st.synchronize()
    return e0.elapsed_time(e1) / reps


rng = np.random.default_rng(1)
arrays = {"16384 hashes, 2000 values": rng.integers(1, 2**63, 2000, dtype=np.uint64)[rng.integers(0, 2000, 16384)],
          "4 M hashes, 100 000 values": rng.integers(1, 2**63, 100000, dtype=np.uint64)[rng.integers(0, 100000, 4 << 20)]}
for spec, kmer_form in (("mash,canon=lexmin", True), ("mash,canon=lexmin", False), ("sourmash", False), ("default", False), ("dedup=distinct", False)):
    ctx = rkmh_amd.Context(0, policy_spec=spec)
    ctx.set_kmer_form(kmer_form)
    ctx.set_references(rb, ro, [16], 1000)
    t = time.perf_counter()
    for _ in range(3):
        ctx.set_references(rb, ro, [16], 1000)
    setup = (time.perf_counter() - t) / 3
    d_out = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    ms = timed(lambda: ctx.classify_device(d_b.data_ptr(), d_o.data_ptr(), n, d_out.data_ptr(), max_read_len=150, stream=st.cuda_stream))
    flagged = int((d_out[:, 0] == -2).sum())
    print("%-18s %-12s classify %.3f ms per %d reads (%d handed back); set_references %.1f ms" %
          (spec, "k-mer-space" if ctx.kmer_form()[0] else "hash-space", ms, n, flagged, setup * 1e3), flush=True)
    for name, h in arrays.items():
        ctx.minhashes(h, 1000)
        t = time.perf_counter()
        for _ in range(5):
            ctx.minhashes(h, 1000)
        print("    rk_minhashes, %-28s %.2f ms (host to host)" % (name, (time.perf_counter() - t) / 5 * 1e3), flush=True)
    ctx.close()
