#!/usr/bin/env python3
"""Bottom samples (rk_bottom.hip, rk_sample.hip, the bottom route of rkmh_sketches.cpp) next to the scaled sample and to the route
they replace, in one job (GPU box).

    python tools/bench_bottom.py device  [--reads 1000000] [--runs 7]
    python tools/bench_bottom.py command [--reads 4000000] [--small 200000] [--runs 5] [--dir /tmp]

device   --reads synthetic 150-base reads (rk_synth_reads on the bundled panel), resident; k = 21, policy sourmash, sketch size 1 000,
         min_copies 1 and 2: Sample.add_device + finish_bottom, device events around both on a stream of its own, two warm-ups, the
         median of --runs; the cuts and the candidates at the end.  Beside it the scaled sample (scaled 1 000, with abundances) on the
         same reads -- the same hashing kernel, so that is the floor.  At min_copies 1 the row must equal rk_sketch_batch +
         rk_merge_sketches on the first 20 000 reads fed alone.
command  `rkmh sketch -g -s 1000 -k 21` on one plain FASTQ file of --small reads: RKMH_SAMPLE_DEVICE=1 against =0, alternating, the
         first pair dropped, the median wall of --runs each, the peak host RSS of both (wait4's resource usage; one process,
         RKMH_FORK=0); the outputs must be equal.  Then the file of --reads reads: the device route as before; the old route once,
         under a time limit, when --small's time times reads / small stays below it -- else, or when it fails, exactly that is recorded.
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
from bench_sample import EXE, PANEL, run_cmd, spread, write_fastq  # noqa: E402

OLD_ROUTE_LIMIT_S = 240


def device(args):
    import torch
    import rkmh_amd
    from bench_search import timed
    from rkmh_amd import api, synth
    refs = api.parse_files([PANEL])
    qb, qo = synth.generate_reads_fast(refs["bases"], refs["offsets"], 0, args.reads, read_len=150, threads=8)
    ctx = rkmh_amd.Context(0, policy_spec="sourmash")
    ks, S = [21], 1000
    d_b = torch.from_numpy(qb).cuda()
    d_o = torch.from_numpy(qo.astype(np.int64)).to(torch.int32).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    res = dict(mode="device", reads=args.reads, k=21, policy="sourmash", sketch_size=S, equal=True)
    for m in (1, 2):
        s = ctx.sample_bottom(ks, S, m)
        got = {}

        def feed_finish():
            s.reset()
            s.add_device(d_b.data_ptr(), d_o.data_ptr(), args.reads, stream=st.cuda_stream)
            got["row"] = s.finish_bottom()
        r = dict(add_device_finish_bottom=timed(feed_finish, st, args.runs))
        r.update(state=s.bottom_state(), stats=s.stats(), length=got["row"][1])
        if m == 1:
            n = min(args.reads, 20000)
            s.reset()
            s.add_device(d_b.data_ptr(), d_o.data_ptr(), n, stream=st.cuda_stream)
            row, ln = s.finish_bottom()
            sk, lens = ctx.sketch_batch(qb, qo[:n + 1], ks, S)
            want, wl = api.merge_sketches(sk, lens, S, distinct=True)
            res["equal"] = bool(ln == wl and np.array_equal(row, want))
        res["min_copies_%d" % m] = r
        s.close()
    s = ctx.sample(ks, api.scaled_max_hash(1000), abund=True)

    def scaled():
        s.reset()
        s.add_device(d_b.data_ptr(), d_o.data_ptr(), args.reads, stream=st.cuda_stream)
        s.finish()
    res["scaled_sample_add_device_finish"] = timed(scaled, st, args.runs)
    s.close()
    ctx.close()
    print(json.dumps(res), flush=True)
    return 0 if res["equal"] else 1


def run_rss_limited(argv, env_extra, limit_s):
    """(wall seconds, peak resident set in MB, exit status or 'time limit') of the command as ONE process, its output discarded"""
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    env.update(env_extra)
    env["RKMH_FORK"] = "0"
    t0 = time.perf_counter()
    with open(os.devnull, "wb") as null:
        p = subprocess.Popen(argv, stdout=null, stderr=null, env=env)
        how = None
        while True:
            pid, status, ru = os.wait4(p.pid, os.WNOHANG)
            if pid:
                break
            if time.perf_counter() - t0 > limit_s and how is None:
                how = "time limit"
                p.kill()
            time.sleep(0.05)
        p.returncode = os.waitstatus_to_exitcode(status)
    return time.perf_counter() - t0, ru.ru_maxrss // 1024, how or p.returncode


def command(args):
    res = dict(mode="command", reads=args.reads, small=args.small, sketch_size=1000, k=21, equal=True)
    sketch = [EXE, "sketch", "-g", "-s", "1000", "-k", "21", "-f"]
    small = os.path.join(args.dir, "bench_bottom_%d.fq" % args.small)
    write_fastq(small, args.small)
    walls, outs = {"1": [], "0": []}, {}
    for i in range(args.runs + 1):           # (the first pair warms the page cache and is dropped)
        for route in ("1", "0"):
            w, outs[route] = run_cmd(sketch + [small], {"RKMH_SAMPLE_DEVICE": route})
            if i:
                walls[route].append(w)
    res["equal"] = outs["1"] == outs["0"]
    res["small"] = dict(device=spread(walls["1"]), parsed_whole=spread(walls["0"]), rss_mb={})
    for route, name in (("1", "device"), ("0", "parsed_whole")):
        res["small"]["rss_mb"][name] = run_rss_limited(sketch + [small], {"RKMH_SAMPLE_DEVICE": route}, 600)[1]
    two = [run_cmd(sketch[:-1] + ["--min-copies", "2", "-f", small], {"RKMH_SAMPLE_DEVICE": "1"})[0] for _ in range(3)]
    res["small"]["device_min_copies_2"] = spread(two)
    print(json.dumps({"small": res["small"], "equal": res["equal"]}), file=sys.stderr, flush=True)
    os.remove(small)
    big = os.path.join(args.dir, "bench_bottom_%d.fq" % args.reads)
    write_fastq(big, args.reads)
    w = [run_cmd(sketch + [big], {"RKMH_SAMPLE_DEVICE": "1"})[0] for _ in range(args.runs + 1)][1:]
    res["large"] = dict(device=spread(w), device_rss_mb=run_rss_limited(sketch + [big], {"RKMH_SAMPLE_DEVICE": "1"}, 600)[1])
    w2 = [run_cmd(sketch[:-1] + ["--min-copies", "2", "-f", big], {"RKMH_SAMPLE_DEVICE": "1"})[0] for _ in range(3)]
    res["large"]["device_min_copies_2"] = spread(w2)
    print(json.dumps({"large": res["large"]}), file=sys.stderr, flush=True)
    estimate = res["small"]["parsed_whole"]["median"] * args.reads / args.small
    if estimate < OLD_ROUTE_LIMIT_S:
        wall, rss, how = run_rss_limited(sketch + [big], {"RKMH_SAMPLE_DEVICE": "0"}, OLD_ROUTE_LIMIT_S)
        res["large"]["parsed_whole"] = dict(wall=wall, rss_mb=rss, ended=how, limit_s=OLD_ROUTE_LIMIT_S)
    else:
        res["large"]["parsed_whole"] = dict(not_run="%.0f s estimated from the small file, above the limit of %d s" % (estimate, OLD_ROUTE_LIMIT_S))
    os.remove(big)
    print(json.dumps(res), flush=True)
    return 0 if res["equal"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["device", "command"])
    ap.add_argument("--reads", type=int, default=None)
    ap.add_argument("--small", type=int, default=200000)
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
