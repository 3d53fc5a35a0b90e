#!/usr/bin/env python3
"""Multigather (rk_multigather.hip) next to a loop of rk_gather_scaled_device over the same queries on the same resident arrays (GPU box).

    python tools/bench_multigather.py [--queries 64] [--parts 64] [--min-shared 50] [--runs 7] [--shape dense|sparse|both]

Two collections, the queries made the same way for both: every query is the union of --parts chosen references plus as many foreign
values.
  dense     the collection of tools/bench_gather.py: 4 096 references of 5 000 values, a tenth of each from a pool of 20 000 that all share
  sparse    the collection of tools/bench_search.py: 16 384 references of 5 000 random values, nothing shared by design
Timed in one job, each with device events around the whole entry on a stream of its own, two warm-ups, the median of --runs with min ..
max:
  (a) build          rk_scaled_index_create_device
  (b) multigather    ScaledIndex.multigather_device with room for every row; and the same at max_rounds = 1, from which the cost of one
                     pick-plus-remove round follows: (full - one) / (rounds - 1), rounds = the most rows of a query
  (c) gather loop    Context.gather_scaled_device for every query in turn: what the library offered before, its kernels unchanged
The answers of (b) and (c) are compared in full and must be equal: the tool fails otherwise.  Prints one JSON line per shape; whether
(b) beats (c) by more than the larger of the two spreads (max - min) is reported, not required."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def make_queries(rows, nq, parts, seed=3):
    """rows: uint64 [nref, size], every row ascending -> (values, offsets, chosen int64 [nq, parts])"""
    rng = np.random.default_rng(seed)
    out, chosen = [], np.zeros((nq, parts), dtype=np.int64)
    for i in range(nq):
        chosen[i] = np.sort(rng.choice(len(rows), size=parts, replace=False))
        u = np.unique(rows[chosen[i]].reshape(-1))
        out.append(np.unique(np.concatenate([u, rng.integers(1, 1 << 64, size=len(u), dtype=np.uint64, endpoint=False)])))
    off = np.zeros(nq + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(q) for q in out], dtype=np.uint64)
    return np.concatenate(out), off, chosen


def run(ctx, name, rv, ro, qv, qo, min_shared, runs, extra):
    import torch
    from bench_search import timed
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
    d_off = torch.full((nq + 1,), -1, dtype=torch.int64, device="cuda")
    total = idx.multigather_device(d_qv.data_ptr(), d_qo.data_ptr(), nq, len(qv), 0, d_off.data_ptr(), 0, min_shared=min_shared, stream=st.cuda_stream)
    d_rows = torch.full((max(total, 1), 4), -1, dtype=torch.int32, device="cuda")
    got = {}

    def multi(max_rounds):
        def f():
            got[max_rounds] = idx.multigather_device(d_qv.data_ptr(), d_qo.data_ptr(), nq, len(qv), d_rows.data_ptr(), d_off.data_ptr(), total, min_shared=min_shared,
                                                     max_rounds=max_rounds, stream=st.cuda_stream)
        return f
    res["multigather_one_round"] = timed(multi(1), st, runs)
    res["multigather"] = timed(multi(None), st, runs)
    rows = d_rows.cpu().numpy()[:total].copy()
    off = d_off.cpu().numpy().view(np.uint64).copy()
    per_query = np.diff(off.astype(np.int64))
    # (c) the queries one after the other through the existing entry, each at its place in the same resident array
    d_out = torch.full((nref, 4), -1, dtype=torch.int32, device="cuda")
    loop_rows = [None] * nq

    def loop(keep=False):
        for i in range(nq):
            a, b = int(qo[i]), int(qo[i + 1])
            n = ctx.gather_scaled_device(d_qv.data_ptr() + 8 * a, b - a, d_rv.data_ptr(), d_ro.data_ptr(), nref, len(rv), d_out.data_ptr(), min_shared=min_shared,
                                         stream=st.cuda_stream)
            if keep:
                loop_rows[i] = d_out.cpu().numpy()[:n].copy()
    loop(keep=True)
    res["gather_loop"] = timed(loop, st, max(3, runs // 2))
    equal = bool(got[None] == total and all(len(loop_rows[i]) == per_query[i] and (loop_rows[i] == rows[int(off[i]):int(off[i + 1])]).all() for i in range(nq)))
    m, g = res["multigather"], res["gather_loop"]
    margin = max(m["max"] - m["min"], g["max"] - g["min"])
    rounds = int(per_query.max()) if nq else 0
    rec = {"bench": name, "nref": nref, "nq": nq, "query_values": int(len(qv)), "min_shared": min_shared, "rows": int(total), "most_rows_of_a_query": rounds,
           "index": idx.stats(), "seconds": res, "larger_spread_seconds": margin, "gather_loop_over_multigather": g["median"] / m["median"],
           "multigather_faster_beyond_spread": bool(g["median"] - m["median"] > margin),
           "seconds_per_later_round": (m["median"] - res["multigather_one_round"]["median"]) / max(rounds - 1, 1), "launches_per_round": 2, "equal": equal}
    rec.update(extra)
    idx.close()
    return rec, equal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--parts", type=int, default=64)
    ap.add_argument("--min-shared", type=int, default=50)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--size", type=int, default=5000)
    ap.add_argument("--shape", default="both", choices=("dense", "sparse", "both"))
    o = ap.parse_args()
    sys.path.insert(0, ROOT)
    import rkmh_amd
    ctx = rkmh_amd.Context(0)      # no GPU: this raises, nothing is timed
    failures = []
    for shape in (("dense", "sparse") if o.shape == "both" else (o.shape,)):
        if shape == "dense":
            import bench_gather
            _, rv, ro, _ = bench_gather.make_input(4096, o.size, o.parts)
        else:
            import bench_search
            rv, ro, _, _, _ = bench_search.database(16384, 1, o.size)
        qv, qo, _ = make_queries(rv.reshape(len(ro) - 1, o.size), o.queries, o.parts)
        rec, equal = run(ctx, "multigather_" + shape, rv, ro, qv, qo, o.min_shared, o.runs, {"size": o.size, "parts": o.parts})
        print(json.dumps(rec), flush=True)
        if not equal:
            failures.append("%s: multigather and the loop over gather_scaled_device differ" % shape)
    ctx.close()
    if failures:
        sys.exit("; ".join(failures))


if __name__ == "__main__":
    main()
