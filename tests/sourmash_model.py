"""A pure-Python / numpy model of the hashing policy, written from the published MurmurHash3_x64_128 algorithm and SURVEY.md's
statement of the rules -- it calls neither the library nor the oracle, so it can check the policy keys the oracle does not know
(canon=).  Policy = dict(fold 0|1|2, drop_last 0|1, canon 0|1, seed, mask_lt 0|1).

  murmur3_x64_128      scalar, Python ints (the form the known-answer vectors are checked against)
  window_hashes        every window of a sequence, numpy (one murmur per 16-byte block for all windows at once)
  kmer_hash            one k-mer, scalar
  bottom               minhashes: sorted ascending, zero-free, first S, repeats kept
  intersection_size    two-pointer merge, both sides advance on equality
  argmax_diff          rkmh.cpp:874-883
  classify             rows (ref, shared, diff, n_mins) of the stream loop, optionally under the -M mask (h % slots counter)
"""
import numpy as np

M64 = (1 << 64) - 1
C1, C2 = 0x87C37B91114253D5, 0x4CF5AD432745937F
DEFAULT = dict(fold=0, drop_last=1, canon=0, seed=42, mask_lt=1)
MASH = dict(DEFAULT, fold=1, drop_last=0)
LEXMIN = dict(MASH, canon=1)       # mash with the strand rule Mash and sourmash publish


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def _fmix(k):
    k ^= k >> 33
    k = (k * 0xFF51AFD7ED558CCD) & M64
    k ^= k >> 33
    k = (k * 0xC4CEB9FE1A85EC53) & M64
    return k ^ (k >> 33)


def murmur3_x64_128(key: bytes, seed: int):
    h1 = h2 = seed & 0xFFFFFFFF
    n = len(key)
    for b in range(n // 16):
        k1 = int.from_bytes(key[16 * b:16 * b + 8], "little")
        k2 = int.from_bytes(key[16 * b + 8:16 * b + 16], "little")
        k1 = (_rotl((k1 * C1) & M64, 31) * C2) & M64
        h1 = (_rotl(h1 ^ k1, 27) + h2) & M64
        h1 = (h1 * 5 + 0x52DCE729) & M64
        k2 = (_rotl((k2 * C2) & M64, 33) * C1) & M64
        h2 = (_rotl(h2 ^ k2, 31) + h1) & M64
        h2 = (h2 * 5 + 0x38495AB5) & M64
    tail = key[16 * (n // 16):]
    if len(tail) > 8:
        k2 = int.from_bytes(tail[8:], "little")
        h2 ^= (_rotl((k2 * C2) & M64, 33) * C1) & M64
    if tail:
        k1 = int.from_bytes(tail[:8], "little")
        h1 ^= (_rotl((k1 * C1) & M64, 31) * C2) & M64
    h1 ^= n
    h2 ^= n
    h1 = (h1 + h2) & M64
    h2 = (h2 + h1) & M64
    h1, h2 = _fmix(h1), _fmix(h2)
    h1 = (h1 + h2) & M64
    h2 = (h2 + h1) & M64
    return h1, h2


def fold128(h1, h2, fold):
    """U1: the 64 bits kept of the four 32-bit output words w0..w3 (h1 = w1:w0, h2 = w3:w2)."""
    if fold == 0:
        return ((h1 << 32) | (h1 >> 32)) & M64          # (w0 << 32) | w1
    if fold == 1:
        return h1                                        # the first 64 bits
    return ((h2 << 32) | (h1 >> 32)) & M64               # (w2 << 32) | w1


def to_upper(s: bytes) -> bytes:
    """Every (signed) char above 91 loses 32: lower-case letters become upper case, bytes >= 128 stay."""
    return bytes(c - 32 if 91 < c < 128 else c for c in s)


_COMP = {65: 84, 84: 65, 67: 71, 71: 67}


def revcomp(kmer: bytes) -> bytes:
    return bytes(_COMP[c] for c in reversed(kmer))


def lexmin_strand(kmer: bytes) -> bytes:
    r = revcomp(kmer)
    return kmer if kmer <= r else r


def kmer_hash(kmer: bytes, pol) -> int:
    """One k-mer: 0 when it holds a base that is not A/C/G/T after upper-casing."""
    k = to_upper(kmer)
    if any(c not in _COMP for c in k):
        return 0
    if pol["canon"]:
        return fold128(*murmur3_x64_128(lexmin_strand(k), pol["seed"]), pol["fold"])
    return min(fold128(*murmur3_x64_128(k, pol["seed"]), pol["fold"]),
               fold128(*murmur3_x64_128(revcomp(k), pol["seed"]), pol["fold"]))


# ---- numpy: all windows of a sequence at once ----
def _u(x):
    return np.uint64(x)


def _rotl_np(x, r):
    return (x << _u(r)) | (x >> _u(64 - r))


def _fmix_np(k):
    k = k ^ (k >> _u(33))
    k = k * _u(0xFF51AFD7ED558CCD)
    k = k ^ (k >> _u(33))
    k = k * _u(0xC4CEB9FE1A85EC53)
    return k ^ (k >> _u(33))


def _murmur_rows(rows: np.ndarray, seed: int, fold: int) -> np.ndarray:
    """rows: uint8 [n, k], one key per row -> folded hashes.  Zero padding of the tail block is exact: a zero k1 / k2 leaves
    h1 / h2 as the algorithm's skipped steps do."""
    n, k = rows.shape
    nb = (k + 15) // 16
    pad = np.zeros((n, nb * 16), dtype=np.uint8)
    pad[:, :k] = rows
    w = pad.view("<u8")
    h1 = np.full(n, seed, dtype=np.uint64)
    h2 = np.full(n, seed, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for b in range(nb):
            k1 = _rotl_np(w[:, 2 * b] * _u(C1), 31) * _u(C2)
            k2 = _rotl_np(w[:, 2 * b + 1] * _u(C2), 33) * _u(C1)
            if b < k // 16:
                h1 = (_rotl_np(h1 ^ k1, 27) + h2) * _u(5) + _u(0x52DCE729)
                h2 = (_rotl_np(h2 ^ k2, 31) + h1) * _u(5) + _u(0x38495AB5)
            else:
                h1 = h1 ^ k1
                h2 = h2 ^ k2
        h1 = h1 ^ _u(k)
        h2 = h2 ^ _u(k)
        h1 = h1 + h2
        h2 = h2 + h1
        h1, h2 = _fmix_np(h1), _fmix_np(h2)
        h1 = h1 + h2
        h2 = h2 + h1
    if fold == 0:
        return (h1 << _u(32)) | (h1 >> _u(32))
    if fold == 1:
        return h1
    return (h2 << _u(32)) | (h1 >> _u(32))


_COMP_NP = np.zeros(256, dtype=np.uint8)
for _a, _b in _COMP.items():
    _COMP_NP[_a] = _b
_VALID_NP = np.zeros(256, dtype=bool)
_VALID_NP[[65, 67, 71, 84]] = True


def window_hashes(seq: bytes, k: int, pol) -> np.ndarray:
    """calc_hashes for one k: len-k (drop_last) or len-k+1 windows, 0 for a window with a non-ACGT base."""
    s = np.frombuffer(to_upper(seq), dtype=np.uint8)
    nwin = len(s) - k + (0 if pol["drop_last"] else 1)
    if nwin <= 0:
        return np.zeros(0, dtype=np.uint64)
    W = np.lib.stride_tricks.sliding_window_view(s, k)[:nwin]
    ok = _VALID_NP[W].all(axis=1)
    out = np.zeros(nwin, dtype=np.uint64)
    F = np.ascontiguousarray(W[ok])
    if len(F) == 0:
        return out
    R = np.ascontiguousarray(_COMP_NP[F[:, ::-1]])
    if pol["canon"]:
        ne = F != R
        first = ne.argmax(axis=1)              # the first base where the strands differ (0 for a palindrome: equal there)
        rows = np.arange(len(F))
        take_f = F[rows, first] <= R[rows, first]
        out[ok] = _murmur_rows(np.where(take_f[:, None], F, R), pol["seed"], pol["fold"])
    else:
        out[ok] = np.minimum(_murmur_rows(F, pol["seed"], pol["fold"]), _murmur_rows(R, pol["seed"], pol["fold"]))
    return out


def calc_hashes(seq: bytes, ks, pol) -> np.ndarray:
    """Several k: the hashes of each size in turn, pooled in that order."""
    return np.concatenate([window_hashes(seq, k, pol) for k in ks]) if ks else np.zeros(0, dtype=np.uint64)


def lexmin_differs(seq: bytes, k: int, pol):
    """(windows that hash differently under the two canon rules, valid windows) -- the vacuity guard of the canon tests."""
    a = window_hashes(seq, k, dict(pol, canon=0))
    b = window_hashes(seq, k, dict(pol, canon=1))
    return int((a != b).sum()), int((a != 0).sum())


def bottom(h: np.ndarray, S: int) -> np.ndarray:
    h = np.sort(np.asarray(h, dtype=np.uint64))
    return h[h != 0][:S]


def intersection_size(a, b) -> int:
    i = j = n = 0
    while i < len(a) and a[i] == 0:
        i += 1
    while j < len(b) and b[j] == 0:
        j += 1
    while i < len(a) and j < len(b):
        if a[i] == b[j]:
            n += 1
            i += 1
            j += 1
        elif a[i] < b[j]:
            i += 1
        else:
            j += 1
    return n


def argmax_diff(shared):
    ms, mi, d = -1, 0, 0
    for j, v in enumerate(shared):
        if v > ms:
            d, ms, mi = v - ms, v, j
    return mi, ms, d


def sketch_refs(ref_seqs, ks, S, pol):
    return [bottom(calc_hashes(r, ks, pol), S) for r in ref_seqs]


def mask_by_frequency(h: np.ndarray, counter: np.ndarray, min_occ: int, pol) -> np.ndarray:
    """-M: a hash whose slot h % slots counted fewer than (mask_lt) / at most min_occ occurrences becomes 0."""
    c = counter[(h % _u(len(counter))).astype(np.int64)]
    drop = c < min_occ if pol["mask_lt"] else c <= min_occ
    return np.where(drop, _u(0), h)


def count_hashes(seqs, ks, slots: int, pol, counts_zero=True) -> np.ndarray:
    counter = np.zeros(slots, dtype=np.int64)
    for s in seqs:
        h = calc_hashes(s, ks, pol)
        if not counts_zero:
            h = h[h != 0]
        np.add.at(counter, (h % _u(slots)).astype(np.int64), 1)
    return counter


def classify(read_seqs, ref_sketches, ks, S, pol, counter=None, min_occ=0):
    """Rows (ref, shared, diff, n_mins) of the stream loop: every read against every reference, two-pointer semantics (the sum over
    values of min(multiplicity in the read sketch, multiplicity in the reference sketch))."""
    post = {}
    for j, sk in enumerate(ref_sketches):
        vals, cnt = np.unique(sk, return_counts=True)
        for v, c in zip(vals.tolist(), cnt.tolist()):
            post.setdefault(v, []).append((j, c))
    rows = np.zeros((len(read_seqs), 4), dtype=np.int32)
    for i, r in enumerate(read_seqs):
        h = calc_hashes(r, ks, pol)
        if counter is not None:
            h = mask_by_frequency(h, counter, min_occ, pol)
        mins = bottom(h, S)
        shared = [0] * len(ref_sketches)
        vals, cnt = np.unique(mins, return_counts=True)
        for v, c in zip(vals.tolist(), cnt.tolist()):
            for j, m in post.get(v, ()):
                shared[j] += min(c, m)
        mi, ms, d = argmax_diff(shared)
        rows[i] = (mi, ms, d, len(mins))
    return rows
