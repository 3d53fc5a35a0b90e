#!/usr/bin/env python3
"""All-pairs intersection of scaled sketches: k_scaled_pairs on the GPU, at every `lanes` value and at the automatic choice, against a
plain two-pointer loop on 16 host threads (GPU box).

    g++ -O3 -fopenmp -o tools/ubench/scaled_cpu tools/ubench/scaled_cpu.cpp      (built on first use when missing)
    python tools/bench_scaled.py [--n 2048] [--sizes 800,5000] [--runs 7] [--threads 16] [--cpu-runs 5]
    python tools/bench_scaled.py --abund [--n 2048] [--sizes 800,5000] [--runs 7] [--threads 16] [--cpu-runs 5]
                                               (the weighted form, k_scaled_pairs<L, PairsWeighted>, next to the plain launch at the same `lanes`; see below)
    python tools/bench_scaled.py --keep        (the keep step of the general path next to the hashing: RKMH_INDEX_TIMING lines on stderr)
    python tools/bench_scaled.py --keep [--abund] [--root <tree>]     (the same with abundances; --root: the tree whose package and library
                                               are loaded, this one by default -- for comparing two builds in one job)

Input: 2 x n sets of `size` values each, a tenth of every set drawn from a pool all sets share (planted overlap).  800 values: a viral
genome at scaled 10; 5 000: a bacterial genome at scaled 1000.  Device: the resident-input entry (rk_compare_scaled_device) on
torch's stream, timed with device events around one launch: two warm-up launches, then the median of --runs, at lanes = 1, 8, 64 and
0 (automatic).  Host: tools/ubench/scaled_cpu on --threads OpenMP threads, median of --cpu-runs, same box, same job.  All answers must
be equal.  Prints one JSON line per size; fails when the automatic choice does not beat the host threads, or is slower than the best
forced `lanes` by more than the spread (max - min) of that one's runs.

--abund: the same sets with abundances of 1 .. 500.  Per `lanes` value the weighted launch (rk_compare_scaled_abund_device) and the plain
one (rk_compare_scaled_device) are timed one after the other in the same way, in the same job; the host baseline is
rk_compare_scaled_abund_host on --threads threads (host clock, median of --cpu-runs).  All weighted answers must be equal to the
host's, and their `shared` to the plain launch's.  Prints one JSON line per size with the ratio weighted / plain per `lanes`; fails
when the automatic choice does not beat the host median by more than the larger of the two spreads.  Whether lanes = 0 is still the
best choice for the weighted kernel is reported (auto_over_best, best_spread_seconds), not enforced."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_input(n, size, seed=1):
    rng = np.random.default_rng(seed)
    tenth = size // 10
    pool = rng.integers(1, 1 << 64, size=2 * tenth + 2, dtype=np.uint64, endpoint=False)
    v = rng.integers(1, 1 << 64, size=(2 * n, size), dtype=np.uint64, endpoint=False)
    for i in range(2 * n):
        v[i, :tenth] = rng.choice(pool, size=tenth, replace=False)
    v.sort(axis=1)
    assert (v[:, 1:] > v[:, :-1]).all(), "a set holds a value twice"
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(size)
    return v[:n].reshape(-1).copy(), off, v[n:].reshape(-1).copy(), off.copy()


def bench_pairs(o):
    import torch
    import rkmh_amd
    ctx = rkmh_amd.Context(0)      # no GPU: this raises, nothing is timed
    exe = os.path.join(ROOT, "tools", "ubench", "scaled_cpu")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O3", "-fopenmp", "-o", exe, exe + ".cpp"])
    n, failures = o.n, []
    for size in [int(x) for x in o.sizes.split(",")]:
        av, ao, bv, bo = make_input(n, size)
        d_av, d_ao, d_bv, d_bo = (torch.from_numpy(x.view(np.int64)).cuda() for x in (av, ao, bv, bo))
        d_out = torch.empty((n, n), dtype=torch.int32, device="cuda")
        st = torch.cuda.Stream()
        res, answers = {}, {}
        for lanes in (1, 8, 64, 0):
            def launch():
                ctx.compare_scaled_device(d_av.data_ptr(), d_ao.data_ptr(), n, len(av), d_bv.data_ptr(), d_bo.data_ptr(), n, len(bv), d_out.data_ptr(),
                                          lanes=lanes, stream=st.cuda_stream)
            d_out.fill_(-1)
            torch.cuda.synchronize()
            for _ in range(2):
                launch()
            torch.cuda.synchronize()
            times = []
            for _ in range(max(5, o.runs)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                launch()
                e1.record(st)
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1e-3)
            times.sort()
            torch.cuda.synchronize()
            answers[lanes] = d_out.cpu().numpy().copy()
            res[lanes] = dict(median=times[len(times) // 2], min=times[0], max=times[-1], runs=len(times))
        with tempfile.TemporaryDirectory() as tmp:
            fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            with open(fin, "wb") as f:
                f.write(np.array([n, n], dtype=np.int64).tobytes())
                for x in (ao, bo, av, bv):
                    f.write(x.tobytes())
            r = subprocess.run([exe, fin, fout, str(o.threads), str(max(5, o.cpu_runs))], capture_output=True, check=True)
            cpu = [float(x) for x in r.stdout.split()[1:4]]
            want = np.fromfile(fout, dtype=np.int32).reshape(n, n)
        equal = all(bool((answers[l] == want).all()) for l in answers)
        best = min((1, 8, 64), key=lambda l: res[l]["median"])
        auto, spread = res[0]["median"], res[best]["max"] - res[best]["min"]
        bytes_per_pair = 2 * size * 8
        print(json.dumps({"bench": "scaled_pairs", "n": n, "size": size, "pairs": n * n, "device_seconds": {str(l): res[l] for l in res},
                          "best_forced_lanes": best, "auto_seconds_median": auto, "auto_over_best": auto / res[best]["median"], "best_spread_seconds": spread,
                          "auto_pairs_per_second": n * n / auto, "auto_row_bytes_per_second": n * n * bytes_per_pair / auto,
                          "cpu_threads": o.threads, "cpu_seconds_median": cpu[0], "cpu_seconds_min": cpu[1], "cpu_seconds_max": cpu[2],
                          "cpu_over_auto": cpu[0] / auto, "equal": equal, "shared_mean": float(want.mean())}), flush=True)
        if not equal:
            failures.append("size %d: device and host answers differ" % size)
        if not auto < cpu[0]:
            failures.append("size %d: the automatic choice is not faster than %d host threads" % (size, o.threads))
        if auto > res[best]["median"] + spread:
            failures.append("size %d: the automatic choice is slower than lanes = %d by more than that one's spread" % (size, best))
    ctx.close()
    if failures:
        sys.exit("; ".join(failures))


def _timed(launch, st, runs):
    import torch
    for _ in range(2):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(max(5, runs)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        launch()
        e1.record(st)
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    times.sort()
    torch.cuda.synchronize()
    return dict(median=times[len(times) // 2], min=times[0], max=times[-1], runs=len(times))


def bench_pairs_abund(o):
    import time
    import torch
    import rkmh_amd
    from rkmh_amd import api
    ctx = rkmh_amd.Context(0)      # no GPU: this raises, nothing is timed
    n, failures = o.n, []
    for size in [int(x) for x in o.sizes.split(",")]:
        av, ao, bv, bo = make_input(n, size)
        rng = np.random.default_rng(2)
        aw, bw = (rng.integers(1, 501, size=len(x), dtype=np.uint32) for x in (av, bv))
        d_av, d_ao, d_bv, d_bo = (torch.from_numpy(x.view(np.int64)).cuda() for x in (av, ao, bv, bo))
        d_aw, d_bw = (torch.from_numpy(x.view(np.int32)).cuda() for x in (aw, bw))
        d_out4 = torch.empty((n, n, 4), dtype=torch.int64, device="cuda")
        d_out = torch.empty((n, n), dtype=torch.int32, device="cuda")
        st = torch.cuda.Stream()
        cpu_times, want = [], None
        for _ in range(max(3, o.cpu_runs)):
            t0 = time.perf_counter()
            want = api.compare_scaled_abund_host(av, aw, ao, bv, bw, bo, threads=o.threads)
            cpu_times.append(time.perf_counter() - t0)
        cpu_times.sort()
        cpu = dict(median=cpu_times[len(cpu_times) // 2], min=cpu_times[0], max=cpu_times[-1], runs=len(cpu_times))
        res_w, res_p, equal = {}, {}, True
        for lanes in (1, 8, 64, 0):
            def weighted():
                ctx.compare_scaled_abund_device(d_av.data_ptr(), d_aw.data_ptr(), d_ao.data_ptr(), n, len(av), d_bv.data_ptr(), d_bw.data_ptr(), d_bo.data_ptr(),
                                                n, len(bv), d_out4.data_ptr(), lanes=lanes, stream=st.cuda_stream)

            def plain():
                ctx.compare_scaled_device(d_av.data_ptr(), d_ao.data_ptr(), n, len(av), d_bv.data_ptr(), d_bo.data_ptr(), n, len(bv), d_out.data_ptr(),
                                          lanes=lanes, stream=st.cuda_stream)
            d_out4.fill_(-1)
            d_out.fill_(-1)
            torch.cuda.synchronize()
            res_w[lanes] = _timed(weighted, st, o.runs)
            res_p[lanes] = _timed(plain, st, o.runs)
            got = d_out4.cpu().numpy().view(np.uint64)
            equal = equal and bool((got == want).all()) and bool((d_out.cpu().numpy().astype(np.uint64) == want[:, :, 0]).all())
        best = min((1, 8, 64), key=lambda l: res_w[l]["median"])
        auto, spread = res_w[0]["median"], res_w[best]["max"] - res_w[best]["min"]
        margin = max(cpu["max"] - cpu["min"], res_w[0]["max"] - res_w[0]["min"])
        print(json.dumps({"bench": "scaled_pairs_abund", "n": n, "size": size, "pairs": n * n, "weighted_seconds": {str(l): res_w[l] for l in res_w},
                          "plain_seconds": {str(l): res_p[l] for l in res_p}, "weighted_over_plain": {str(l): res_w[l]["median"] / res_p[l]["median"] for l in res_w},
                          "best_forced_lanes": best, "auto_seconds_median": auto, "auto_over_best": auto / res_w[best]["median"], "best_spread_seconds": spread,
                          "auto_within_best_spread": bool(auto <= res_w[best]["median"] + spread), "auto_pairs_per_second": n * n / auto,
                          "auto_row_bytes_per_second": n * n * 2 * size * 8 / auto, "auto_stored_bytes_per_second": n * n * 32 / auto,
                          "cpu_threads": o.threads, "cpu_seconds": cpu, "cpu_over_auto": cpu["median"] / auto, "larger_spread_seconds": margin, "equal": equal,
                          "shared_mean": float(want[:, :, 0].mean()), "dot_mean": float(want[:, :, 1].mean())}), flush=True)
        if not equal:
            failures.append("size %d: device and host answers differ" % size)
        if not cpu["median"] - auto > margin:
            failures.append("size %d: the automatic choice does not beat %d host threads by more than the larger spread" % (size, o.threads))
    ctx.close()
    if failures:
        sys.exit("; ".join(failures))


def bench_keep(abund):
    os.environ["RKMH_INDEX_TIMING"] = "1"      # read once, at the first batch of the general path
    import rkmh_amd
    from rkmh_amd import api, synth
    ctx = rkmh_amd.Context(0)
    rng = np.random.default_rng(77)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    one = acgt[rng.integers(0, 4, size=300_000, dtype=np.uint8)].tobytes()
    refs = api.parse_files([os.path.join(ROOT, "tests", "golden", "data", "all_pave_ref.fa.gz")])
    qb, qo = synth.generate_reads_fast(refs["bases"], refs["offsets"], 0, 3000)
    rb, ro = api.pack([one])
    for what, b, off, ks, scaled in (("one sequence of 300 000 bases, k = 21, scaled 1", rb, ro, [21], 1), ("3 000 reads of 150 bases, k = 16, scaled 1000", qb, qo, [16], 1000)):
        for rep in range(3):
            print("---- %s%s (run %d)" % (what, ", with abundances" if abund else "", rep), file=sys.stderr, flush=True)
            if abund:
                v, _, so = ctx.sketch_scaled_abund_batch(b, off, ks, api.scaled_max_hash(scaled))
            else:
                v, so = ctx.sketch_scaled_batch(b, off, ks, api.scaled_max_hash(scaled))
        print("---- kept %d values in %d sketches" % (len(v), len(so) - 1), file=sys.stderr, flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--sizes", default="800,5000")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--cpu-runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--keep", action="store_true")
    ap.add_argument("--abund", action="store_true")
    ap.add_argument("--root", default=ROOT)
    o = ap.parse_args()
    sys.path.insert(0, os.path.abspath(o.root))
    if o.keep:
        bench_keep(o.abund)
    elif o.abund:
        bench_pairs_abund(o)
    else:
        bench_pairs(o)


if __name__ == "__main__":
    main()
