#!/usr/bin/env python3
"""Screen (rk_screen.hip, rkmh_screen.cpp) next to the only exact route there was before it, in one job (GPU box).

    python tools/bench_screen.py device  [--reads 1000000] [--runs 7]
    python tools/bench_screen.py command [--reads 4000000] [--runs 5] [--dir /tmp]

device   the 182 HPV references as bottom-1000 sketches at k = 21 (policy mash); --reads synthetic 150-base reads (rk_synth_reads on the
         same panel), resident.  (a) Screen.add_device alone, (b) the route of the parent commit: Sample.add_device at max_hash = the
         largest reference value, with abundances, and the fold behind it (Sample.device), (c) Screen.rows_device.  Device events on a
         stream of its own, two warm-ups, then --runs rounds in which (a) and (b) ALTERNATE; medians with min .. max.  Device memory of
         both routes: the drop of the device's free memory from before the object is made to after its first feed (the arrays are
         kept between feeds, so this is what the route holds).  The two routes must agree on `shared` of every reference.
command  `rkmh screen -r <panel> -f <reads>` as a whole process on one FASTQ file of --reads reads, plain and bgzip'd, and beside it
         `rkmh sketch -g --scaled <N> --abund` on the same file, N chosen so that its max_hash is nearest the largest reference value:
         the baseline of the parent commit (which still lacks the comparison step), not a threshold.  One warm-up pair, then --runs
         alternating pairs; wall clock.
Prints one JSON line per mode."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PANEL = os.path.join(ROOT, "tests", "golden", "data", "all_pave_ref.fa.gz")
EXE = os.path.join(ROOT, "bin", "rkmh")
K, S, POLICY = 21, 1000, "mash"


def spread(times):
    times = sorted(times)
    return dict(median=times[len(times) // 2], min=times[0], max=times[-1], runs=len(times))


def reference_rows(ctx, refs):
    """-> (values, offsets) of the bottom-S rows as CSR, the rows collapsed, the largest value"""
    sk, lens = ctx.sketch_batch(refs["bases"], refs["offsets"], [K], S)
    rows = [sk[i, :int(lens[i])] for i in range(len(lens))]
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return np.concatenate(rows).astype(np.uint64), off, [np.unique(r) for r in rows], int(max(int(r.max()) for r in rows))


def device(args):
    import torch
    import rkmh_amd
    from bench_search import timed
    from rkmh_amd import api, synth
    refs = api.parse_files([PANEL])
    qb, qo = synth.generate_reads_fast(refs["bases"], refs["offsets"], 0, args.reads, read_len=150, threads=8)
    ctx = rkmh_amd.Context(0, policy_spec=POLICY)
    rv, ro, coll, max_key = reference_rows(ctx, refs)
    d_b = torch.from_numpy(qb).cuda()
    d_o = torch.from_numpy(qo.astype(np.int64)).to(torch.int32).cuda()
    st = torch.cuda.Stream()
    nref = len(ro) - 1
    d_out = torch.zeros(nref * 4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def free_mb():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0] / 2.0 ** 20

    f0 = free_mb()
    scr = ctx.screen([K], rv, ro)
    scr.add_device(d_b.data_ptr(), d_o.data_ptr(), args.reads, stream=st.cuda_stream)
    f1 = free_mb()
    smp = ctx.sample([K], max_key, abund=True)

    def sample_route():
        smp.reset()
        smp.add_device(d_b.data_ptr(), d_o.data_ptr(), args.reads, stream=st.cuda_stream)
        return smp.device()                                   # the fold

    sample_route()
    f2 = free_mb()

    def once(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        call()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    t_screen, t_sample = [], []
    for i in range(2 + args.runs):                            # the two routes alternate; two warm-up rounds
        a = once(lambda: scr.add_device(d_b.data_ptr(), d_o.data_ptr(), args.reads, stream=st.cuda_stream))
        b = once(sample_route)
        if i >= 2:
            t_screen.append(a)
            t_sample.append(b)
    res = dict(mode="device", reads=args.reads, k=K, sketch=S, policy=POLICY, references=nref, stats=None)
    res["screen_add_device"] = spread(t_screen)
    res["sample_add_device_and_fold"] = spread(t_sample)
    res["screen_over_sample"] = res["screen_add_device"]["median"] / res["sample_add_device_and_fold"]["median"]
    res["screen_rows_device"] = timed(lambda: scr.rows_device(d_out.data_ptr(), 1, st.cuda_stream), st, args.runs)
    res["device_memory_mb"] = dict(screen=f0 - f1, sample=f1 - f2)
    res["max_key"] = max_key
    res["max_key_fraction_of_hash_space"] = max_key / float(1 << 64)
    res["sample_stats"] = smp.stats()
    # the two routes agree: the sample against the collapsed rows, shared per reference
    scr.reset()
    scr.add_device(d_b.data_ptr(), d_o.data_ptr(), args.reads, stream=st.cuda_stream)
    torch.cuda.synchronize()
    res["stats"] = scr.stats()
    rows = scr.rows(1)
    v, a = smp.finish()
    cv = np.concatenate(coll).astype(np.uint64)
    co = np.zeros(nref + 1, dtype=np.uint64)
    co[1:] = np.cumsum([len(r) for r in coll])
    cmp4 = ctx.compare_scaled_abund(v, a, np.asarray([0, len(v)], np.uint64), cv, np.ones(len(cv), np.uint32), co)
    res["equal"] = bool((rows[:, 0].astype(np.uint64) == cmp4[0, :, 0]).all())
    res["references_with_shared"] = int((rows[:, 0] > 0).sum())
    scr.close()
    smp.close()
    ctx.close()
    print(json.dumps(res), flush=True)
    return 0 if res["equal"] else 1


def command(args):
    from bench_sample import run_cmd, write_fastq
    import rkmh_amd
    from rkmh_amd import api, synth
    ctx = rkmh_amd.Context(0, policy_spec=POLICY)
    max_key = reference_rows(ctx, api.parse_files([PANEL]))[3]
    ctx.close()
    scaled = max(1, int(round(float((1 << 64) - 1) / max_key)))
    res = dict(mode="command", reads=args.reads, k=K, sketch=S, policy=POLICY, baseline_scaled=scaled, max_key=max_key)
    plain = os.path.join(args.dir, "bench_screen_%d.fq" % args.reads)
    write_fastq(plain, args.reads)
    bgzf = plain + ".gz"
    with open(bgzf, "wb") as f:
        f.write(bytes(synth.bgzf_compress(open(plain, "rb").read(), level=1, threads=16)))
    opts = ["-k", str(K), "--hash-policy", POLICY]
    outs = {}
    for form, path in (("plain", plain), ("bgzf", bgzf)):
        walls = {"screen": [], "sketch": []}
        for i in range(args.runs + 1):                        # (the first pair warms the page cache and is dropped)
            for what, argv in (("screen", [EXE, "screen", "-r", PANEL, "-s", str(S), "-f", path] + opts),
                               ("sketch", [EXE, "sketch", "-g", "--scaled", str(scaled), "--abund", "-f", path] + opts)):
                w, out = run_cmd(argv, {})
                if what == "screen":
                    outs[form] = out.replace(path.encode(), b"X")
                if i:
                    walls[what].append(w)
        res[form] = dict(screen=spread(walls["screen"]), sketch_scaled_abund=spread(walls["sketch"]), file_bytes=os.path.getsize(path))
        print(json.dumps({form: res[form]}), file=sys.stderr, flush=True)
    res["screen_lines"] = outs["plain"].count(b"\n")
    res["equal"] = outs["plain"] == outs["bgzf"]
    for p in (plain, bgzf):
        os.remove(p)
    print(json.dumps(res), flush=True)
    return 0 if res["equal"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["device", "command"])
    ap.add_argument("--reads", type=int, default=None)
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
