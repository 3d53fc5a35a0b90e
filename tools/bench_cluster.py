#!/usr/bin/env python3
"""`rkmh cluster` next to what a user could do before it, and the clustering step alone (GPU box).

    python tools/bench_cluster.py command [--families 100] [--per 200] [--length 8000] [--rate 0.02] [--runs 5] [--dir /tmp]
    python tools/bench_cluster.py device  [the same collection options] [--runs 7]

The collection: --families base sequences of --length bases (synth.synthetic_panel), each with --per members that differ from it by
point substitutions at --rate; written as one FASTA.  At k = 21, --scaled 100 the members of a family share about a third of their
hashes and families share nothing, so the self-search has families * per^2 hits.

command: whole processes, wall clock, output into a file: `rkmh manysearch -r X` (the baseline: every hit downloaded and formatted)
and `rkmh cluster -r X`, the same -k, --scaled and --min-shared, alternating, one warm-up each, then --runs of each -> medians with
min .. max, the sizes of the two outputs, the number of clusters.  No ratio is asserted.

device: the collection's sketches (Context.sketch_scaled_batch), the self-search's hits resident (search_device), then
cluster_hits_device on them, timed with device events around the call (it synchronises once per round), two warm-ups, the median of
--runs; rk_cluster_hits_host on the same hits downloaded, wall clock, the same number of runs; the labels must be equal.  Prints one
JSON line per mode."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = ["-k", "21", "--scaled", "100", "--min-shared", "3", "--hash-policy", "sourmash"]


def collection(nfam, per, length, rate, seed=11):
    """-> (names, list of uint8 arrays): nfam * per sequences"""
    sys.path.insert(0, ROOT)
    from rkmh_amd import synth
    bases, offs = synth.synthetic_panel(nref=nfam, min_len=length, max_len=length)
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    names, seqs = [], []
    for f in range(nfam):
        row = bases[int(offs[f]):int(offs[f + 1])]
        m = np.tile(row, (per, 1))
        hit = rng.random(m.shape) < rate
        m[hit] = acgt[rng.integers(0, 4, int(hit.sum()))]
        for j in range(per):
            names.append(b"fam%04d_member%04d" % (f, j))
            seqs.append(m[j])
    return names, seqs


def write_fasta(path, names, seqs):
    with open(path, "wb") as f:
        for n, s in zip(names, seqs):
            f.write(b">" + n + b"\n" + s.tobytes() + b"\n")


def spread(times):
    times = sorted(times)
    return dict(median=times[len(times) // 2], min=times[0], max=times[-1], runs=len(times))


def command(o):
    names, seqs = collection(o.families, o.per, o.length, o.rate)
    fa = os.path.join(o.dir, "bench_cluster.fa")
    write_fasta(fa, names, seqs)
    rk = os.path.join(ROOT, "bin", "rkmh")
    outs = {"manysearch": os.path.join(o.dir, "bench_cluster.hits.tsv"), "cluster": os.path.join(o.dir, "bench_cluster.clusters.tsv")}
    walls = {"manysearch": [], "cluster": []}
    for r in range(o.runs + 1):
        for cmd in ("manysearch", "cluster"):
            with open(outs[cmd], "wb") as f:
                t0 = time.perf_counter()
                subprocess.run([rk, cmd, "-r", fa] + OPTS, stdout=f, check=True, timeout=600)
                dt = time.perf_counter() - t0
            if r:                                            # run 0 warms the file cache and the driver up
                walls[cmd].append(dt)
    lines = open(outs["cluster"]).read().splitlines()
    rec = {"bench": "cluster_command", "sketches": len(names), "families": o.families, "fasta_bytes": os.path.getsize(fa), "options": " ".join(OPTS),
           "manysearch_seconds": spread(walls["manysearch"]), "cluster_seconds": spread(walls["cluster"]),
           "manysearch_output_bytes": os.path.getsize(outs["manysearch"]), "cluster_output_bytes": os.path.getsize(outs["cluster"]),
           "hits": sum(1 for _ in open(outs["manysearch"], "rb")), "clusters": len(set(ln.split("\t")[0] for ln in lines)), "members": len(lines)}
    rec["manysearch_over_cluster"] = rec["manysearch_seconds"]["median"] / rec["cluster_seconds"]["median"]
    for p in [fa] + list(outs.values()):
        os.remove(p)
    print(json.dumps(rec), flush=True)


def device(o):
    sys.path.insert(0, ROOT)
    import torch
    import rkmh_amd
    from rkmh_amd import api
    names, seqs = collection(o.families, o.per, o.length, o.rate)
    ctx = rkmh_amd.Context(0, "sourmash")                                # no GPU: this raises, nothing is timed
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    values, vo = ctx.sketch_scaled_batch(np.concatenate(seqs), offs, [21], api.scaled_max_hash(100))
    n = len(vo) - 1
    d_v, d_o = (torch.from_numpy(x.view(np.int64)).cuda() for x in (values, vo))
    st = torch.cuda.Stream()
    idx = ctx.scaled_index_device(d_v.data_ptr(), d_o.data_ptr(), n, len(values), stream=st.cuda_stream)
    total = idx.search_device(d_v.data_ptr(), d_o.data_ptr(), n, len(values), 0, 0, min_shared=3, stream=st.cuda_stream)
    d_hits = torch.zeros((total, 3), dtype=torch.int32, device="cuda")
    idx.search_device(d_v.data_ptr(), d_o.data_ptr(), n, len(values), d_hits.data_ptr(), total, min_shared=3, stream=st.cuda_stream)
    d_lab = torch.zeros(n, dtype=torch.int32, device="cuda")
    rounds, times = 0, []
    for r in range(2 + max(5, o.runs)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        rounds = ctx.cluster_hits_device(d_hits.data_ptr(), total, d_o.data_ptr(), n, len(values), d_lab.data_ptr(), stream=st.cuda_stream)
        e1.record(st)
        e1.synchronize()
        if r >= 2:
            times.append(e0.elapsed_time(e1) * 1e-3)
    whole = []
    for r in range(1 + max(3, o.runs // 2)):
        d_all = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        idx.cluster_device(d_v.data_ptr(), d_o.data_ptr(), n, len(values), d_all.data_ptr(), min_shared=3, stream=st.cuda_stream)
        if r:
            whole.append(time.perf_counter() - t0)
    hits = d_hits.cpu().numpy()
    lens = np.diff(vo.astype(np.int64)).astype(np.uint64)
    host = []
    for r in range(max(5, o.runs)):
        t0 = time.perf_counter()
        want = api.cluster_hits_host(hits, lens)
        host.append(time.perf_counter() - t0)
    got = d_lab.cpu().numpy()
    equal = bool((got == want).all() and (d_all.cpu().numpy() == want).all())
    rec = {"bench": "cluster_device", "sketches": n, "values": int(len(values)), "hits": int(total), "hit_bytes": int(total) * 12, "hook_launches": rounds,
           "clusters": int(len(np.unique(want))), "cluster_hits_device_seconds": spread(times), "search_and_cluster_device_seconds": spread(whole),
           "cluster_hits_host_seconds_one_thread": spread(host), "equal": equal}
    print(json.dumps(rec), flush=True)
    idx.close()
    ctx.close()
    if not equal:
        sys.exit("the device labels and the host labels differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["command", "device"])
    ap.add_argument("--families", type=int, default=100)
    ap.add_argument("--per", type=int, default=200)
    ap.add_argument("--length", type=int, default=8000)
    ap.add_argument("--rate", type=float, default=0.02)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dir", default="/tmp")
    o = ap.parse_args()
    command(o) if o.mode == "command" else device(o)


if __name__ == "__main__":
    main()
