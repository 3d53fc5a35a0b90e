#!/usr/bin/env python3
"""Search through the resident inverted index (rk_search.hip) next to the dense all-pairs kernel (k_scaled_pairs) on the same arrays
(GPU box).

    python tools/bench_search.py [--refs 16384] [--queries 256] [--size 5000] [--runs 7]       the database shape
    python tools/bench_search.py --dense [--n 2048] [--sizes 800,5000] [--runs 7]              the dense shape of tools/bench_scaled.py

Database shape: --refs resident references and --queries queries of --size values each; every query takes a tenth of its values from
each of 8 chosen references (so it shares size / 10 values with each of them) and shares nothing deliberate with the rest.  Timed in
one job, each with device events on a stream of its own, two warm-ups, the median of --runs with min .. max:
  (a) build      the index build (rk_scaled_index_create_device)
  (b) search1    search_device at min_shared = 1
  (c) search50   search_device at min_shared = 50
      count1     search_device at min_shared = 1 with room for no hit: the counting pass and the scan alone
  (d) dense      compare_scaled_device at lanes = 0: the kernels the sketch-set layer had before the index
The answers of (b) and (d) are compared in full and must be equal.  Prints one JSON line; fails when (b) does not beat (d) by more than
the larger of the two spreads (max - min).  Also printed: build + search against (d), the number of searches of this size after which
the build has paid for itself, the index's stats and the number of hits.

--dense: the 2 x n sets of bench_scaled.make_input, where every pair shares: the same four timings and the same comparison, reported
whichever way it comes out."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def database(nref, nq, size, seed=1):
    rng = np.random.default_rng(seed)
    tenth = size // 10
    rv = rng.integers(1, 1 << 64, size=(nref, size), dtype=np.uint64, endpoint=False)
    rv.sort(axis=1)
    qv = rng.integers(1, 1 << 64, size=(nq, size), dtype=np.uint64, endpoint=False)
    chosen = np.zeros((nq, 8), dtype=np.int64)
    for i in range(nq):
        chosen[i] = rng.choice(nref, size=8, replace=False)
        for j, r in enumerate(chosen[i]):
            qv[i, j * tenth:(j + 1) * tenth] = rng.choice(rv[r], size=tenth, replace=False)
    qv.sort(axis=1)
    assert (rv[:, 1:] > rv[:, :-1]).all() and (qv[:, 1:] > qv[:, :-1]).all(), "a set holds a value twice"
    return (rv.reshape(-1), np.arange(nref + 1, dtype=np.uint64) * np.uint64(size), qv.reshape(-1), np.arange(nq + 1, dtype=np.uint64) * np.uint64(size), chosen)


def timed(launch, st, runs):
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


def run(ctx, name, rv, ro, qv, qo, runs, extra):
    """-> (the JSON record, whether the answers were equal, whether search1 beat dense by more than the larger spread)"""
    import torch
    nref, nq = len(ro) - 1, len(qo) - 1
    d_rv, d_ro, d_qv, d_qo = (torch.from_numpy(x.view(np.int64)).cuda() for x in (rv, ro, qv, qo))
    st = torch.cuda.Stream()
    made = []

    def build():
        while made:
            made.pop().close()
        made.append(ctx.scaled_index_device(d_rv.data_ptr(), d_ro.data_ptr(), nref, len(rv), stream=st.cuda_stream))
    res = {"build": timed(build, st, runs)}
    idx = made[0]
    stats = idx.stats()
    total1 = idx.search_device(d_qv.data_ptr(), d_qo.data_ptr(), nq, len(qv), 0, 0, min_shared=1, stream=st.cuda_stream)
    d_hits = torch.full((max(total1, 1), 3), -1, dtype=torch.int32, device="cuda")
    totals = {}
    for what, ms in (("search1", 1), ("search50", 50)):
        def search():
            totals[what] = idx.search_device(d_qv.data_ptr(), d_qo.data_ptr(), nq, len(qv), d_hits.data_ptr(), total1, min_shared=ms, stream=st.cuda_stream)
        res[what] = timed(search, st, runs)
        if ms == 1:
            hits = d_hits.cpu().numpy()[:totals[what]].copy()
    res["count1"] = timed(lambda: idx.search_device(d_qv.data_ptr(), d_qo.data_ptr(), nq, len(qv), 0, 0, min_shared=1, stream=st.cuda_stream), st, runs)
    d_out = torch.full((nq, nref), -1, dtype=torch.int32, device="cuda")

    def dense():
        ctx.compare_scaled_device(d_qv.data_ptr(), d_qo.data_ptr(), nq, len(qv), d_rv.data_ptr(), d_ro.data_ptr(), nref, len(rv), d_out.data_ptr(), lanes=0,
                                  stream=st.cuda_stream)
    res["dense"] = timed(dense, st, runs)
    want = d_out.cpu().numpy()
    i, j = np.nonzero(want)
    equal = bool(hits.shape == (len(i), 3) and (hits[:, 0] == i).all() and (hits[:, 1] == j).all() and (hits[:, 2] == want[i, j]).all())
    s1, d, b = res["search1"], res["dense"], res["build"]
    margin = max(s1["max"] - s1["min"], d["max"] - d["min"])
    faster = bool(d["median"] - s1["median"] > margin)
    saved = d["median"] - s1["median"]
    rec = {"bench": name, "nref": nref, "nq": nq, "pairs": nref * nq, "seconds": res, "larger_spread_seconds": margin, "dense_over_search1": d["median"] / s1["median"],
           "dense_over_build_plus_search1": d["median"] / (b["median"] + s1["median"]), "search1_faster_than_dense_beyond_spread": faster,
           "searches_of_this_size_until_the_build_is_paid": (int(np.ceil(b["median"] / saved)) if saved > 0 else None),
           "queries_until_the_build_is_paid": (int(np.ceil(b["median"] / saved * nq)) if saved > 0 else None),
           "index": stats, "hits_min_shared_1": int(totals["search1"]), "hits_min_shared_50": int(totals["search50"]),
           "hit_bytes": int(totals["search1"]) * 12, "pairs_per_second_search1": nref * nq / s1["median"], "equal": equal}
    rec.update(extra)
    idx.close()
    return rec, equal, faster


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=16384)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--size", type=int, default=5000)
    ap.add_argument("--dense", action="store_true")
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--sizes", default="800,5000")
    ap.add_argument("--runs", type=int, default=7)
    o = ap.parse_args()
    sys.path.insert(0, ROOT)
    import rkmh_amd
    ctx = rkmh_amd.Context(0)      # no GPU: this raises, nothing is timed
    failures = []
    if o.dense:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bench_scaled
        for size in [int(x) for x in o.sizes.split(",")]:
            av, ao, bv, bo = bench_scaled.make_input(o.n, size)
            rec, equal, _ = run(ctx, "search_dense_shape", bv, bo, av, ao, o.runs, {"size": size})
            print(json.dumps(rec), flush=True)
            if not equal:
                failures.append("size %d: the search and the dense comparison differ" % size)
    else:
        rv, ro, qv, qo, chosen = database(o.refs, o.queries, o.size)
        rec, equal, faster = run(ctx, "search_database_shape", rv, ro, qv, qo, o.runs, {"size": o.size, "planted_pairs": int(chosen.size)})
        print(json.dumps(rec), flush=True)
        if not equal:
            failures.append("the search and the dense comparison differ")
        if not faster:
            failures.append("search at min_shared = 1 does not beat the dense comparison by more than the larger spread")
    ctx.close()
    if failures:
        sys.exit("; ".join(failures))


if __name__ == "__main__":
    main()
