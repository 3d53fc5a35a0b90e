#!/usr/bin/env python3
"""The sample accumulator (rk_sample.hip, rkmh_sample.cpp) next to the route it replaces, in one job (GPU box).

    python tools/bench_sample.py device  [--reads 1000000] [--runs 7]
    python tools/bench_sample.py command [--reads 4000000] [--small 1000000] [--runs 5] [--dir /tmp]

device   --reads synthetic 150-base reads (rk_synth_reads on the bundled panel), resident; k = 21, policy sourmash, scaled 1 000, with
         abundances.  (a) Sample.add_device + finish, device events around both on a stream of its own, two warm-ups, the median of
         --runs; (b) the parent's route for the same reads: rk_sketch_scaled_abund_batch (host arrays, its upload included) and the
         host union rk_merge_scaled_abund, timed separately, the same number of runs.  The two sketches must be equal.
command  `rkmh sketch --scaled 1000 --abund -g` on one FASTQ file of --reads reads, plain and bgzip'd: RKMH_SAMPLE_DEVICE=1 against
         =0, alternating, the median wall of --runs each, and `rkmh stream` on the same file as the front end's ceiling.  Peak host
         RSS (the resource usage wait4 returns; one process, RKMH_FORK=0) of both routes at --small and --reads reads.  The outputs of the
         two routes must be equal.
Prints one JSON line per mode."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PANEL = os.path.join(ROOT, "tests", "golden", "data", "all_pave_ref.fa.gz")
EXE = os.path.join(ROOT, "bin", "rkmh")


def spread(times):
    times = sorted(times)
    return dict(median=times[len(times) // 2], min=times[0], max=times[-1], runs=len(times))


def device(args):
    import torch
    import rkmh_amd
    from bench_search import timed
    from rkmh_amd import api, synth
    refs = api.parse_files([PANEL])
    qb, qo = synth.generate_reads_fast(refs["bases"], refs["offsets"], 0, args.reads, read_len=150, threads=8)
    ctx = rkmh_amd.Context(0, policy_spec="sourmash")
    ks, mh = [21], api.scaled_max_hash(1000)
    d_b = torch.from_numpy(qb).cuda()
    d_o = torch.from_numpy(qo.astype(np.int64)).to(torch.int32).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = ctx.sample(ks, mh, abund=True)
    got = {}

    def feed():
        s.reset()
        s.add_device(d_b.data_ptr(), d_o.data_ptr(), args.reads, stream=st.cuda_stream)

    def feed_finish():
        feed()
        got["new"] = s.finish()
    res = dict(mode="device", reads=args.reads, k=21, policy="sourmash", scaled=1000)
    res["sample_add_device"] = timed(feed, st, args.runs)
    res["sample_add_device_finish"] = timed(feed_finish, st, args.runs)
    res["sample_stats"] = s.stats()
    sk, mg = [], []
    for i in range(args.runs + 2):
        t0 = time.perf_counter()
        v, a, off = ctx.sketch_scaled_abund_batch(qb, qo, ks, mh)
        t1 = time.perf_counter()
        got["old"] = api.merge_scaled_abund(v, a, off, mh)
        t2 = time.perf_counter()
        if i >= 2:
            sk.append(t1 - t0)
            mg.append(t2 - t1)
    res["parent_sketch_scaled_abund_batch"] = spread(sk)
    res["parent_merge_scaled_abund_host"] = spread(mg)
    res["equal"] = bool(np.array_equal(got["new"][0], got["old"][0]) and np.array_equal(got["new"][1], got["old"][1]))
    res["distinct"] = int(len(got["new"][0]))
    s.close()
    ctx.close()
    print(json.dumps(res), flush=True)
    return 0 if res["equal"] else 1


def write_fastq(path, n):
    """n reads of 150 bases as records of a fixed width, assembled in numpy"""
    from rkmh_amd import api, synth
    refs = api.parse_files([PANEL])
    with open(path, "wb") as f:
        for lo in range(0, n, 1 << 20):
            hi = min(n, lo + (1 << 20))
            qb, _ = synth.generate_reads_fast(refs["bases"], refs["offsets"], lo, hi, read_len=150, threads=8)
            m = hi - lo
            rec = np.empty((m, 316), dtype=np.uint8)  # @r<9 digits>\n, 150 bases\n, +\n, 150 qualities\n
            rec[:, 0] = ord("@"); rec[:, 1] = ord("r")
            num = np.arange(lo, hi, dtype=np.int64)
            for d in range(9):
                rec[:, 2 + d] = ord("0") + (num // 10 ** (8 - d)) % 10
            rec[:, 11] = ord("\n")
            rec[:, 12:162] = qb[: m * 150].reshape(m, 150)
            rec[:, 162] = ord("\n"); rec[:, 163] = ord("+"); rec[:, 164] = ord("\n")
            rec[:, 165:315] = ord("I")
            rec[:, 315] = ord("\n")
            f.write(rec.tobytes())


def run_cmd(argv, env_extra):
    """-> (wall seconds, stdout)"""
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    env.update(env_extra)
    t0 = time.perf_counter()
    p = subprocess.Popen(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    out, err = p.communicate()
    wall = time.perf_counter() - t0
    if p.returncode != 0:
        raise SystemExit("%s failed: %s" % (argv, err[-400:]))
    return wall, out


def run_rss(argv, env_extra):
    """peak resident set in MB of the command run as ONE process (RKMH_FORK=0), its output discarded: wait4's resource usage"""
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    env.update(env_extra)
    env["RKMH_FORK"] = "0"
    with open(os.devnull, "wb") as null:
        p = subprocess.Popen(argv, stdout=null, stderr=null, env=env)
        _, status, ru = os.wait4(p.pid, 0)
        p.returncode = os.waitstatus_to_exitcode(status) if hasattr(os, "waitstatus_to_exitcode") else status
    if p.returncode != 0:
        raise SystemExit("%s failed with status %s" % (argv, p.returncode))
    return ru.ru_maxrss // 1024


def command(args):
    from rkmh_amd import synth
    res = dict(mode="command", reads=args.reads, small=args.small, equal=True)
    files = {}
    for n in sorted({args.small, args.reads}):
        p = os.path.join(args.dir, "bench_sample_%d.fq" % n)
        write_fastq(p, n)
        files[n] = {"plain": p}
        z = p + ".gz"
        with open(z, "wb") as f:
            f.write(bytes(synth.bgzf_compress(open(p, "rb").read(), level=1, threads=16)))
        files[n]["bgzf"] = z
    sketch = [EXE, "sketch", "--scaled", "1000", "--abund", "-g", "-k", "21", "--hash-policy", "sourmash", "-f"]
    for form in ("plain", "bgzf"):
        path = files[args.reads][form]
        walls = {"1": [], "0": []}
        outs = {}
        for i in range(args.runs + 1):           # (the first pair warms the page cache and is dropped)
            for route in ("1", "0"):
                w, out = run_cmd(sketch + [path], {"RKMH_SAMPLE_DEVICE": route})
                outs[route] = out
                if i:
                    walls[route].append(w)
        res["equal"] = res["equal"] and outs["1"] == outs["0"]
        res[form] = dict(device=spread(walls["1"]), parsed_whole=spread(walls["0"]))
        st = []
        for i in range(3):
            w, _ = run_cmd([EXE, "stream", "-r", PANEL, "-f", path, "-k", "16", "-s", "1000"], {})
            st.append(w)
        res[form]["stream"] = spread(st)
        res[form]["rss_mb"] = {}
        for n in sorted(files):
            for route in ("1", "0"):
                res[form]["rss_mb"]["%s_reads_%d" % ("device" if route == "1" else "parsed_whole", n)] = run_rss(sketch + [files[n][form]], {"RKMH_SAMPLE_DEVICE": route})
        print(json.dumps({form: res[form]}), file=sys.stderr, flush=True)
    for n in files:
        for p in files[n].values():
            os.remove(p)
    print(json.dumps(res), flush=True)
    return 0 if res["equal"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["device", "command"])
    ap.add_argument("--reads", type=int, default=None)
    ap.add_argument("--small", type=int, default=1000000)
    ap.add_argument("--runs", type=int, default=None)
    ap.add_argument("--dir", default="/tmp")
    args = ap.parse_args()
    if args.reads is None:
        args.reads = 1000000 if args.mode == "device" else 4000000
    if args.runs is None:
        args.runs = 7 if args.mode == "device" else 5
    return device(args) if args.mode == "device" else command(args)


if __name__ == "__main__":
    sys.exit(main())
