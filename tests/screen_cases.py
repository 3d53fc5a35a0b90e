"""Shared inputs of the screen tests (rk_screen_*, include/rkmh_amd.h "SCREEN"): reads as bytes from seeded generators, reference rows
built FROM the window hashes of those reads and their neighbours +- 1, and random small (rows, counted set) pairs for the invariants.
Pure Python (screen_model / abund_model / sourmash_model; neither the library nor the oracle is called here).  What the cases hold is
shown on the model by tests/test_screen_cpu.py; tests/test_gpu_screen.py relies on it."""
import functools

import numpy as np

import sample_cases as sc
import screen_model as scm
import sourmash_model as sm

W = sc.HASH_TILE_WIN          # rk_kernels.hpp: window positions per tile of the walk
T = 256                       # rk_tile_walk.hpp: lanes of a workgroup
GRID_CAP = 4096               # rk_screen.hip, launch_count: at most this many workgroups
K = 21
POLICIES = sc.POLICIES
SAT = scm.SAT


def rand_read(rng, n):
    return sc.rand_read(rng, n)


def hashes(reads, ks=(K,), pol=sm.DEFAULT):
    """every non-zero window hash of the reads, one entry per window"""
    out = []
    for r in reads:
        h = sm.calc_hashes(r, list(ks), pol)
        out += [int(x) for x in h[h != 0].tolist()]
    return out


def rows_from(values, rng, nref, length, neighbours=True, repeats=False):
    """nref rows of about `length` values drawn from `values` (so that they are hit), their neighbours +- 1 and a few random ones (which
    are not); ascending; with `repeats` some values stand twice or three times"""
    values = sorted(set(values))
    rows = []
    for _ in range(nref):
        pick = set()
        if values:
            for i in rng.integers(0, len(values), size=length).tolist():
                v = values[i]
                pick.add(v)
                if neighbours and rng.integers(0, 4) == 0:
                    pick.add(v + 1 if v < scm.FULL else v)
                    if v > 1:
                        pick.add(v - 1)
        for v in rng.integers(1, 1 << 63, size=max(length // 8, 1), dtype=np.uint64).tolist():
            pick.add(int(v))
        row = sorted(pick)
        if repeats:
            row = sorted(row + row[::3] + row[::7])
        rows.append(row)
    return rows


# ---- totals of 1, k - 1, k, 2 047, 2 048, 2 049 and 3 x 2 048 + 5 positions as ONE read each, and as a batch of reads that start or end
# on, one before and one after a tile edge, with reads shorter than k, of one base and with N between them
TOTALS = (1, K - 1, K, W - 1, W, W + 1, 3 * W + 5)


@functools.lru_cache(maxsize=None)
def single_read(total):
    return (rand_read(np.random.default_rng(100 + total), total),)


@functools.lru_cache(maxsize=None)
def edge_batch():
    rng = np.random.default_rng(31)
    reads = []
    at = 0

    def add(n, with_n=False):
        nonlocal at
        r = bytearray(rand_read(rng, n))
        if with_n and n:
            r[n // 2] = ord("N")
        reads.append(bytes(r))
        at += n

    for edge_shift in (-1, 0, 1):                 # a read END (and the next read's START) at edge - 1, edge, edge + 1
        tile_end = (at // W + 1) * W
        add(150)
        add(1)
        add(K - 1)
        add(90, with_n=True)
        add(tile_end + edge_shift - at)           # ends at the edge (+ shift)
        add(K)                                    # starts there
        add(K + 1)
    add(5)                                        # the batch ends a few bases into a tile
    return tuple(reads)


def starts(reads):
    return sc.starts(reads)


# ---- a block of reads repeated R times: more tiles than the feed's grid in ONE batch; every count is R times the block's
@functools.lru_cache(maxsize=None)
def block():
    rng = np.random.default_rng(32)
    return tuple(rand_read(rng, int(n)) for n in rng.integers(120, 181, size=280))


def block_bases():
    return sum(len(r) for r in block())


def many_tiles_R():
    return GRID_CAP * W // block_bases() + 3      # ceil(R * block / 2048) > 4096


# ---- contention: 2 000 homopolymer reads whose one k-mer is a key
def homopolymers(n=2000, length=60):
    return tuple(b"A" * length for _ in range(n))


# ---- random small (rows, counted set) pairs for the invariants
def random_pair(seed, nref=6, universe=40, disjoint=False):
    rng = np.random.default_rng(seed)
    pool = [int(x) for x in rng.choice(np.arange(1, 10 * universe), size=universe, replace=False)]
    rows = []
    if disjoint:
        cuts = sorted(rng.choice(np.arange(1, universe), size=nref - 1, replace=False).tolist())
        parts = np.split(np.asarray(pool), cuts)
        rows = [sorted(int(x) for x in p) for p in parts]
    else:
        for _ in range(nref):
            n = int(rng.integers(0, universe // 2))
            row = sorted(int(x) for x in rng.choice(pool, size=n, replace=False))
            if rng.integers(0, 3) == 0:
                row = sorted(row + row[::2])
            rows.append(row)
    counts = {v: int(rng.integers(1, 6)) for v in pool if rng.integers(0, 3) != 0}
    for v in rng.integers(1, 10 * universe, size=5).tolist():   # values that may be no key at all
        counts.setdefault(int(v), int(rng.integers(1, 4)))
    return rows, counts


def counted_arrays(counts):
    vals = sorted(counts)
    return np.asarray(vals, dtype=np.uint64), np.asarray([counts[v] for v in vals], dtype=np.uint64)
