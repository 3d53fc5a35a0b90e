#!/usr/bin/env python3
"""All-pairs sketch comparison: k_sketch_pairs on the GPU against a plain two-pointer loop on 16 host threads (GPU box).

    g++ -O3 -fopenmp -o tools/ubench/pairs_cpu tools/ubench/pairs_cpu.cpp      (built on first use when missing)
    python tools/bench_pairs.py [--n 2048] [--sketch 1000] [--runs 7] [--threads 16] [--cpu-runs 5]

Input: 2 x n random sketches of --sketch values, a tenth of each row drawn from a pool all rows share (planted overlap).  Device: the
resident-input entry (rk_compare_sketches_device) on torch's stream, timed with device events: two warm-up launches, then the median
of --runs.  Host: tools/ubench/pairs_cpu on --threads OpenMP threads, median of --cpu-runs, same box, same job.  Both answers must be
equal, all n x n x 4 integers.  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_input(n, S, seed=1):
    rng = np.random.default_rng(seed)
    pool = rng.integers(1, 1 << 64, size=2 * (S // 10) + 2, dtype=np.uint64, endpoint=False)
    sk = rng.integers(1, 1 << 64, size=(2 * n, S), dtype=np.uint64, endpoint=False)
    for i in range(2 * n):
        sk[i, : S // 10] = rng.choice(pool, size=S // 10, replace=False)
    sk.sort(axis=1)
    ln = np.full(2 * n, S, dtype=np.int32)
    return sk[:n].copy(), ln[:n].copy(), sk[n:].copy(), ln[n:].copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--sketch", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--cpu-runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    o = ap.parse_args()
    import torch
    import rkmh_amd
    n, S = o.n, o.sketch
    a, al, b, bl = make_input(n, S)
    ctx = rkmh_amd.Context(0)      # no GPU: this raises, nothing is timed
    d_a, d_b = (torch.from_numpy(x.view(np.int64)).cuda() for x in (a, b))
    d_al, d_bl = torch.from_numpy(al).cuda(), torch.from_numpy(bl).cuda()
    d_out = torch.empty((n, n, 4), dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()

    def launch():
        ctx.compare_sketches_device(d_a.data_ptr(), d_al.data_ptr(), n, d_b.data_ptr(), d_bl.data_ptr(), n, S, d_out.data_ptr(), stream=st.cuda_stream)

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
    got = d_out.cpu().numpy()
    ctx.close()
    exe = os.path.join(ROOT, "tools", "ubench", "pairs_cpu")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O3", "-fopenmp", "-o", exe, exe + ".cpp"])
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.array([n, n, S, 0], dtype=np.int32).tobytes())
            for x in (a, b, al, bl):
                f.write(x.tobytes())
        r = subprocess.run([exe, fin, fout, str(o.threads), str(max(5, o.cpu_runs))], capture_output=True, check=True)
        cpu = [float(x) for x in r.stdout.split()[1:4]]
        want = np.fromfile(fout, dtype=np.int32).reshape(n, n, 4)
    equal = bool((got == want).all())
    props = rkmh_amd.api.device_props(0)
    cus = int(props.get("compute_units", 256))
    dev = times[len(times) // 2]
    print(json.dumps({"bench": "pairs", "n": n, "sketch": S, "pairs": n * n,
                      "device_seconds_median": dev, "device_seconds_min": times[0], "device_seconds_max": times[-1], "device_runs": len(times),
                      "device_pairs_per_second": n * n / dev, "cpu_threads": o.threads, "cpu_seconds_median": cpu[0], "cpu_seconds_min": cpu[1],
                      "cpu_seconds_max": cpu[2], "cpu_over_device": cpu[0] / dev, "equal": equal, "compute_units": cus,
                      "shared_mean": float(want[:, :, 0].mean()), "common_mean": float(want[:, :, 2].mean())}))
    if not equal:
        sys.exit("device and host answers differ")
    if not dev < cpu[0]:
        sys.exit("the device is not faster than %d host threads" % o.threads)


if __name__ == "__main__":
    main()
