#!/usr/bin/env python3
"""Gather of one large query against a resident database: rk_gather_scaled_device against two baselines (GPU box).

    python tools/bench_gather.py [--nref 4096] [--size 5000] [--parts 64] [--min-shared 50] [--runs 7] [--threads 16] [--base-runs 3]

Input: --nref sets of --size values each, a tenth of every set drawn from a pool of 20 000 values all sets share (planted overlap);
the query is the union of --parts of them plus as many foreign values.  The references are uploaded once.
  device    the resident-input entry on a stream of its own, device events around the whole call (it synchronises the stream): two
            warm-up calls, then the median of --runs with min and max; the same with max_rounds = 1 (the setup and one round), from
            which the cost of a later round follows
  host      rk_gather_scaled_host on --threads threads, host clock, one warm-up, median of --base-runs
  pairs     what the library offered before: the same loop driven from Python through compare_scaled_device (1 x nref per round,
            at the fastest of lanes = 1, 8, 64, tried once each), argmax on the host, the remaining query rebuilt on the host and
            uploaded again each round; host clock around the loop, one warm-up, median of --base-runs
All three answers must be equal.  Prints one JSON line; fails unless the device entry is faster than both baselines' medians by more
than the larger of their spreads (max - min).

    python tools/bench_gather.py --abund [--root <tree>]

The device entry alone on the same input, for comparing two builds in one job (run it once per build, alternating; --root: the tree
whose package and library are loaded, this one by default): rk_gather_scaled_device, and, where the library has it,
rk_gather_scaled_abund_device with abundances of 1 to 500 on the query -- the same rows, plus wunique.  One JSON line with the median,
min and max of --runs of each."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_input(nref, size, parts, seed=1):
    rng = np.random.default_rng(seed)
    tenth = size // 10
    pool = np.unique(rng.integers(1, 1 << 64, size=20000, dtype=np.uint64, endpoint=False))
    v = rng.integers(1, 1 << 64, size=(nref, size), dtype=np.uint64, endpoint=False)
    for i in range(nref):
        v[i, :tenth] = rng.choice(pool, size=tenth, replace=False)
    v.sort(axis=1)
    assert (v[:, 1:] > v[:, :-1]).all(), "a set holds a value twice"
    chosen = rng.choice(nref, size=parts, replace=False)
    u = np.unique(v[chosen].reshape(-1))
    foreign = rng.integers(1, 1 << 64, size=len(u), dtype=np.uint64, endpoint=False)
    q = np.unique(np.concatenate([u, foreign]))
    off = np.arange(nref + 1, dtype=np.uint64) * np.uint64(size)
    return q, v.reshape(-1).copy(), off, np.sort(chosen)


def stats(times):
    times = sorted(times)
    return dict(median=times[len(times) // 2], min=times[0], max=times[-1], runs=len(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nref", type=int, default=4096)
    ap.add_argument("--size", type=int, default=5000)
    ap.add_argument("--parts", type=int, default=64)
    ap.add_argument("--min-shared", type=int, default=50)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--base-runs", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--abund", action="store_true")
    ap.add_argument("--root", default=ROOT)
    o = ap.parse_args()
    sys.path.insert(0, os.path.abspath(o.root))
    import torch
    import rkmh_amd
    from rkmh_amd import api
    ctx = rkmh_amd.Context(0)      # no GPU: this raises, nothing is timed
    q, rv, ro, chosen = make_input(o.nref, o.size, o.parts)
    nref, nq = o.nref, len(q)
    d_q, d_rv, d_ro = (torch.from_numpy(x.view(np.int64)).cuda() for x in (q, rv, ro))
    d_out = torch.full((nref, 4), -1, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()

    # ---- the device entry
    def device(max_rounds):
        return ctx.gather_scaled_device(d_q.data_ptr(), nq, d_rv.data_ptr(), d_ro.data_ptr(), nref, len(rv), d_out.data_ptr(),
                                        min_shared=o.min_shared, max_rounds=max_rounds, stream=st.cuda_stream)

    def timed_device(max_rounds, device=device):
        for _ in range(2):
            n = device(max_rounds)
        torch.cuda.synchronize()
        times = []
        for _ in range(o.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            n = device(max_rounds)
            e1.record(st)
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3)
        torch.cuda.synchronize()
        return stats(times), d_out.cpu().numpy()[:n].copy()
    dev, rows_dev = timed_device(nref)
    if o.abund:
        res = {"bench": "gather_abund", "root": os.path.abspath(o.root), "nref": nref, "size": o.size, "query": nq, "rows": len(rows_dev),
               "plain_seconds": dev, "weighted_seconds": None}
        if hasattr(ctx, "gather_scaled_abund_device"):
            rng = np.random.default_rng(2)
            qa = rng.integers(1, 501, size=nq, dtype=np.uint32)
            d_qa = torch.from_numpy(qa.view(np.int32)).cuda()
            d_wu = torch.full((nref,), -1, dtype=torch.int64, device="cuda")

            def weighted(max_rounds):
                return ctx.gather_scaled_abund_device(d_q.data_ptr(), d_qa.data_ptr(), nq, d_rv.data_ptr(), d_ro.data_ptr(), nref, len(rv), d_out.data_ptr(),
                                                      d_wu.data_ptr(), min_shared=o.min_shared, max_rounds=max_rounds, stream=st.cuda_stream)
            wdev, rows_w = timed_device(nref, weighted)
            wu = d_wu.cpu().numpy()[:len(rows_w)]
            alive, want = np.ones(nq, dtype=bool), []
            for r in rows_w[:, 0].tolist():                      # the weights, recomputed from the rows
                hit = np.isin(q, rv[int(ro[r]):int(ro[r + 1])], assume_unique=True) & alive
                want.append(int(qa[hit].astype(np.uint64).sum()))
                alive &= ~hit
            res.update(weighted_seconds=wdev, weighted_over_plain=wdev["median"] / dev["median"],
                       equal=bool(rows_w.shape == rows_dev.shape and (rows_w == rows_dev).all() and wu.tolist() == want))
        print(json.dumps(res), flush=True)
        ctx.close()
        if res.get("equal") is False:
            sys.exit("the weighted call's rows or weights are wrong")
        return
    one, _ = timed_device(1)
    nrounds = len(rows_dev)

    # ---- baseline (a): the host entry
    def host():
        return api.gather_scaled_host(q, rv, ro, min_shared=o.min_shared, threads=o.threads)
    rows_host = host()
    times = []
    for _ in range(o.base_runs):
        t0 = time.perf_counter()
        rows_host = host()
        times.append(time.perf_counter() - t0)
    cpu = stats(times)

    # ---- baseline (b): all-pairs counts of the remaining query against every reference, once per round
    d_cnt = torch.empty((1, nref), dtype=torch.int32, device="cuda")
    one_off = np.zeros(2, dtype=np.uint64)

    def counts(rem, lanes):
        d_rem = torch.from_numpy(rem.view(np.int64)).cuda()
        one_off[1] = len(rem)
        d_off = torch.from_numpy(one_off.view(np.int64)).cuda()
        with torch.cuda.stream(st):
            ctx.compare_scaled_device(d_rem.data_ptr(), d_off.data_ptr(), 1, len(rem), d_rv.data_ptr(), d_ro.data_ptr(), nref, len(rv), d_cnt.data_ptr(),
                                      lanes=lanes, stream=st.cuda_stream)
            st.synchronize()
        return d_cnt.cpu().numpy()[0]
    trial = {}
    for lanes in (64, 8, 1):
        counts(q, lanes)
        t0 = time.perf_counter()
        counts(q, lanes)
        trial[lanes] = time.perf_counter() - t0
    best_lanes = min(trial, key=trial.get)

    def pairs():
        rem, rows = q, []
        total = counts(q, best_lanes).copy()
        cnt = total
        while len(rows) < nref:
            r = int(np.argmax(cnt))                              # the first of the largest
            if cnt[r] < o.min_shared:
                break
            ref = rv[int(ro[r]):int(ro[r + 1])]
            rem = rem[~np.isin(rem, ref, assume_unique=True)]
            rows.append((r, int(cnt[r]), int(total[r]), len(rem)))
            if len(rem) == 0:
                break
            cnt = counts(rem, best_lanes)
        return np.asarray(rows, dtype=np.int32).reshape(len(rows), 4)
    rows_pairs = pairs()
    times = []
    for _ in range(o.base_runs):
        t0 = time.perf_counter()
        rows_pairs = pairs()
        times.append(time.perf_counter() - t0)
    par = stats(times)

    equal = rows_dev.shape == rows_host.shape == rows_pairs.shape and bool((rows_dev == rows_host).all()) and bool((rows_dev == rows_pairs).all())
    spread = max(cpu["max"] - cpu["min"], par["max"] - par["min"])
    per_round = (dev["median"] - one["median"]) / max(nrounds - 1, 1)
    hits = int(rows_dev[:, 2].sum()) if nrounds else 0
    print(json.dumps({"bench": "gather", "nref": nref, "size": o.size, "query": nq, "parts": o.parts, "min_shared": o.min_shared, "rows": nrounds,
                      "picked_are_the_parts": bool(nrounds >= o.parts and (np.sort(rows_dev[:o.parts, 0]) == chosen).all()),
                      "device_seconds": dev, "device_setup_and_one_round_seconds": one, "device_seconds_per_later_round": per_round,
                      "launches_per_round": 3, "round_group": api.RK_GATHER_BATCH,
                      "host_threads": o.threads, "host_seconds": cpu, "pairs_lanes": best_lanes, "pairs_lanes_trial_seconds": {str(k): v for k, v in trial.items()},
                      "pairs_seconds": par, "host_over_device": cpu["median"] / dev["median"], "pairs_over_device": par["median"] / dev["median"],
                      "baseline_spread_seconds": spread, "total_of_picked": hits, "equal": equal}), flush=True)
    ctx.close()
    failures = []
    if not equal:
        failures.append("the three answers differ")
    if not dev["median"] + spread < cpu["median"]:
        failures.append("the device entry does not beat %d host threads by more than the baselines' spread" % o.threads)
    if not dev["median"] + spread < par["median"]:
        failures.append("the device entry does not beat the loop over compare_scaled_device by more than the baselines' spread")
    if failures:
        sys.exit("; ".join(failures))


if __name__ == "__main__":
    main()
