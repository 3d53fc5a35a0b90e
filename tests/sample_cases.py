"""Shared inputs of the sample-accumulator tests (rk_sample_*, include/rkmh_amd.h "SAMPLE SKETCHES"): reads as bytes from seeded numpy
generators, and the pure-Python expectation (abund_model / sourmash_model; neither the library nor the oracle is called here).  What
the cases hold -- enough kept windows to force folds and a retry, a run of more than 64 equal values, windows lost to each boundary
rule -- is shown on the model by tests/test_sample_cpu.py; tests/test_gpu_sample.py relies on it."""
import functools

import numpy as np

import abund_model as am
import dedup_model as dm
import scaled_model as scm
import sourmash_model as sm

HASH_TILE_WIN = 2048          # rk_kernels.hpp: window positions per tile of k_sample_keep
K = 16
FULL = am.FULL
POLICIES = {"default": sm.DEFAULT, "mash": sm.MASH, "sourmash": dm.SOURMASH}
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def rand_read(rng, n):
    return bytes(_ACGT[rng.integers(0, 4, size=n)])


def want(reads, ks=(K,), pol=sm.DEFAULT, mh=FULL):
    """the sample after `reads`: (values uint64, abund uint32), and kept = the unsaturated number of kept windows"""
    parts = [am.sketch(r, list(ks), pol, mh) for r in reads]
    v, a = am.merge(parts, mh)
    return v, a, sum(int(np.asarray(p[1], dtype=np.uint64).sum()) for p in parts)


def pack(reads):
    """-> (uint8 bases with slack behind them, uint64 offsets[n + 1])"""
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
    b = np.zeros(int(off[-1]) + 16, dtype=np.uint8)
    if int(off[-1]):
        b[: int(off[-1])] = np.frombuffer(b"".join(reads), dtype=np.uint8)
    return b, off


# ---- 300 reads for the fold, order and reset tests: lengths 100 .. 199 (odd and even: reads start at every byte alignment), a few N,
# a few lower-case stretches, and every tenth read a copy of an earlier one, so that abundances above 1 occur
@functools.lru_cache(maxsize=None)
def reads300():
    rng = np.random.default_rng(20)
    out = []
    for i in range(300):
        if i % 10 == 9:
            out.append(out[int(rng.integers(0, len(out)))])
            continue
        r = bytearray(rand_read(rng, int(rng.integers(100, 200))))
        if i % 7 == 0:
            r[int(rng.integers(0, len(r)))] = ord("N")
        if i % 11 == 0:
            a = int(rng.integers(0, len(r) - 20))
            r[a:a + 20] = bytes(r[a:a + 20]).lower()
        out.append(bytes(r))
    return tuple(out)


FOLD_CAPS = (1, 64, 1024, 0)  # pending_cap values of the fold test (0: the library's default)
FOLD_BATCH = 7                # reads per feed there
FOLD_MH = scm.max_hash(2)


def batches(reads, n):
    return [list(reads[i:i + n]) for i in range(0, len(reads), n)]


# ---- one batch whose kept windows exceed the capacity it is fed at
RETRY_CAP = 1024


@functools.lru_cache(maxsize=None)
def retry_batch():
    rng = np.random.default_rng(21)
    return tuple(rand_read(rng, 150) for _ in range(25))  # 25 x (150 - 16) = 3 350 windows, all kept at FULL


# ---- read edges at k = 16
def edge_reads(k=K):
    rng = np.random.default_rng(22)
    body = rand_read(rng, 64)
    lens = [0, 1, k - 1, k, k + 1, k + 2]
    out = [body[:n] for n in lens]
    for pos in (0, 20, 40):                      # an N at the first, middle and last base of a 41-base read
        r = bytearray(body[:41]); r[pos] = ord("N"); out.append(bytes(r))
    out.append(body[:50].lower())
    out += [rand_read(rng, n) for n in (17, 19, 21, 23, 33, 35, 37, 39)]   # odd lengths: every byte alignment of a start
    return out


# ---- tile edges: 40 reads of 150 bases and one of 5 000, plus the filler reads that put a read start exactly on a tile boundary and
# leave fewer than k bases in the last tile.  No sum of 150s and 5 000 is a multiple of 2 048 below 25 tiles, hence the fillers.
@functools.lru_cache(maxsize=None)
def tile_batch(k=K):
    rng = np.random.default_rng(23)
    short = [rand_read(rng, 150) for _ in range(40)]
    long_read = rand_read(rng, 5000)
    reads = short[:13]
    fill = HASH_TILE_WIN - sum(len(r) for r in reads)         # 98 bases: the next read starts at position 2 048 exactly
    reads.append(rand_read(rng, fill))
    on_boundary = len(reads)                                  # index of the read that starts on the boundary
    reads += short[13:20]                                     # 7 x 150: the 150-base read at 2 048 + 900 .. straddles nothing yet
    reads.append(long_read)                                   # 3 098 .. 8 098: straddles the boundaries at 4 096 and 6 144
    reads += short[20:]                                       # 20 x 150 up to 11 098: one of them straddles 8 192, one 10 240
    total = sum(len(r) for r in reads)
    tail = (-(total) % HASH_TILE_WIN) + 5                     # the batch ends 5 bases into its last tile
    if tail < k + 4:
        tail += HASH_TILE_WIN
    reads.append(rand_read(rng, tail))
    return tuple(reads), on_boundary


def starts(reads):
    return np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)


# ---- abundances
def homopolymer(n=3000):
    return b"A" * n


REPEAT_FEEDS = 70  # one read fed that often: a run of 70 equal values per window in the sorted pending array


# ---- FASTQ text for the slot tests
@functools.lru_cache(maxsize=None)
def fastq200():
    rng = np.random.default_rng(24)
    reads = [rand_read(rng, int(rng.integers(60, 180))) for _ in range(200)]
    text = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))
    return tuple(reads), text


def fastq_with_cr():
    reads, text = fastq200()
    lines = text.split(b"\n")
    lines[4 * 50 + 1] += b"\r"   # the sequence line of record 50 ends in CR LF
    return b"\n".join(lines)
