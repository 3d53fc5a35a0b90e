"""Inputs for classifying through the hash-space kernel (k_classify_tile, rk_classify.hip) at every k from 1 to 64, built from seeds
alone, with the conditions that keep a comparison against the oracle from passing vacuously.  tests/test_tile_cases_cpu.py checks
those conditions on the oracle and the model without a GPU; tests/test_gpu_tile_classify.py hands the same inputs to the device.

Sketch size S = 2000 everywhere: every reference of the catalogue is wholly sketched and no read of <= 1528 bases has more windows
than the sketch keeps, so bottom-S selection never acts and the fused kernel -- not the general path -- answers, provided also
that the panel has <= 16384 references (`assert_routed` states the three conditions).  The fused kernel still hands single reads
back on its own (row field 0 = -2, answered by the general path) where its per-read LDS structures would overflow; `may_hand_back`
restates those documented limits on the oracle's hashes, so the GPU test can hold the kernel to them: a read outside that set that
comes back flagged fails the test.

  panel            base_panel(): 12 references of 400 .. 900 bases (a 2 % diverged pair, an exact duplicate, a tandem repeat of a
                   7-base unit, one with lower case / N / IUPAC letters)
  read sets        ragged(k), uniform(k, L), counter_width(), prefetch_edges(L, k), panel_edges(nref)
  policies         Pol(fold, drop, canon, seed[, dedup]): the text for a Context, the oracle's struct, the model's dict
  expectations     want_rows / want_sketches: the oracle for canon=minhash, tests/sourmash_model.py for canon=lexmin

The DEDUP forms of the kernel (dedup=distinct: k_classify_tile<0, MODE, -1, PF, CANON, true>) have a catalogue of their own on the same
panel: Pol(..., dedup=1), the window hashes as above, the sketch rule from tests/dedup_model.py (want_rows / want_sketches dispatch on
pol.dedup), the kernel's limits under the key in `may_hand_back_distinct`.

  read sets        ragged(k), uniform(k, L), prefetch_edges(L, k) as above; set_ladder(W), stale_set(), several_k_limit(),
                   exactly_s(k, pol): what only the per-read set of distinct hashes can get wrong
"""
import collections
import functools

import numpy as np

import dedup_model as dm
import sourmash_model as sm

S = 2000
FUSED_MAXLEN = 1528          # longest read the fused kernel stages (rk_kernels.hpp)
MAX_REFS = 16384             # reference ids must fit the kernel's running (count, -ref) maximum
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
UNIT = b"ACGGTCA"            # the tandem repeat's unit (not its own reverse complement, no internal period)
TANDEM_COPIES = 20           # copies of UNIT in the tandem reference
TANDEM, DUP_OF, DUP, ANC, DIVERGED, MESSY = 4, 5, 9, 1, 6, 7   # places in the base panel

ALL_K = list(range(1, 65))
FULL_L_K = (7, 24, 48, 64)                      # every one of the 64 uniform lengths
CROSS_K = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
CROSS_SEEDS = (42, 7)
SINGLE_K = (12, 16, 20, 21, 31)                 # the KT-specialised instantiations
K_LISTS = ([12, 48], [20, 21], [16, 64], [31, 33, 63])   # the same sizes through KT = 0
MODE_K = (7, 33, 48, 64)
COUNT_SLOTS = 100003
PREFETCH_L = (504, 505, 760, 761, 1528, 1529)   # tile bytes <= 504 / 760 / 1528 choose PF = 2 / 3 / 6; 1529 is handed back
PANEL_NREF = (256, 257, 512, 513)               # dense | sparse rows: 512 | 513 with 8-bit fields, 256 | 257 with 16-bit


class Pol(collections.namedtuple("Pol", "fold drop canon seed dedup", defaults=(0,))):
    def spec(self):
        text = "fold=%s,windows=%s,canon=%s,seed=%d" % (("swap32", "h1", "w2w1")[self.fold], "len-k" if self.drop else "len-k+1",
                                                        "lexmin" if self.canon else "minhash", self.seed)
        return text + (",dedup=distinct" if self.dedup else "")

    def oracle(self, orc):
        assert not self.canon            # the oracle knows the minhash strand rule only
        return orc.default_policy(fold=self.fold, drop_last_window=self.drop, seed=self.seed)

    def model(self):
        return dict(sm.DEFAULT, fold=self.fold, drop_last=self.drop, canon=self.canon, seed=self.seed)

    def __str__(self):
        return self.spec()


DEFAULT = Pol(0, 1, 0, 42)
CROSS = [Pol(f, d, c, s) for f in (0, 1, 2) for d in (1, 0) for c in (0, 1) for s in CROSS_SEEDS]
DEDUP = (Pol(0, 1, 0, 42, dedup=1), Pol(0, 1, 1, 42, dedup=1))      # "both strand rules" of the DEDUP catalogue
DEDUP_CROSS = [Pol(f, d, c, 42, dedup=1) for f in (0, 1, 2) for d in (1, 0) for c in (0, 1)]
DEDUP_CROSS_K = (1, 8, 16, 17, 32, 33, 64)
DEDUP_MAX_WINDOWS = 2048     # half of the largest per-read set (DEDUP_MAX_SLOTS, rk_classify.hip)
LADDER_K = 24
LADDER_W = (32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025)   # windows of the longest read: uset = 64 | 128 | ... | 2048 | 4096
LIMIT_KS = [16, 64]          # 2 L - 80 windows under windows=len-k: 2048 at L = 1064
EXACT_S = 64                 # the sketch size of exactly_s()
EXACT_K = (16, 24)
EXACT_P = (63, 64, 65)


def nwin(length, k, pol=DEFAULT):
    return max(length - k + (0 if pol.drop else 1), 0)


def rand(rng, n):
    return bytes(rng.choice(ACGT, size=n).tolist())


def mutate(rng, s, rate):
    """substitutions at `rate` per base, each to one of the three other letters (upper-case A/C/G/T only)"""
    b = bytearray(s)
    for j in np.nonzero(rng.random(len(b)) < rate)[0].tolist():
        at = b"ACGT".find(bytes([b[j]]))
        if at >= 0:
            b[j] = b"ACGT"[(at + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(b)


@functools.lru_cache(maxsize=None)
def base_panel():
    rng = np.random.default_rng(20240)
    lens = [400, 520, 610, 700, 0, 640, 0, 760, 830, 0, 900, 455]
    refs = [rand(rng, n) if n else b"" for n in lens]
    refs[TANDEM] = rand(rng, 200) + UNIT * TANDEM_COPIES + rand(rng, 200)
    refs[DIVERGED] = mutate(rng, refs[ANC], 0.02)                  # shares an ancestor with refs[ANC]
    refs[DUP] = refs[DUP_OF]                                       # ties: the first wins
    m = bytearray(refs[MESSY])
    m[100:220] = bytes(m[100:220]).lower()
    for pos, c in ((40, b"N"), (300, b"n"), (301, b"N"), (420, b"R"), (500, b"Y"), (650, b"K"), (759, b"N")):
        m[pos] = c[0]
    refs[MESSY] = bytes(m)
    assert all(400 <= len(r) <= 900 for r in refs) and len(refs) == 12
    return tuple(refs)


def _cut(rng, panel, L, rate=0.01):
    """L bases cut from a panel member that is long enough, 1 % substitutions"""
    while True:
        r = panel[int(rng.integers(0, len(panel)))]
        if len(r) >= L:
            st = int(rng.integers(0, len(r) - L + 1))
            return mutate(rng, r[st:st + L], rate)


Ragged = collections.namedtuple("Ragged", "reads two_n tandem")


@functools.lru_cache(maxsize=None)
def ragged(k):
    """~120 reads for one k: the lengths around k and 2k, 150, 251 and random ones <= 400, two thirds cut from the panel; lower case;
    single N at the places where a window rule can be off by one; two N exactly k + 1 apart (one valid window, indices in
    .two_n); copies of the tandem repeat holding its k-mers less often and more often than the reference does (.tandem)."""
    rng = np.random.default_rng(1000 + k)
    P = base_panel()
    lens = [0, 1, k - 1, k, k + 1, k + 2, 2 * k - 1, 2 * k, 150, 251] + rng.integers(2, 401, 20).tolist()
    reads = []
    for rep in range(3):
        for L in lens:
            r = _cut(rng, P, L) if rep < 2 else rand(rng, L)
            reads.append(r.lower() if len(reads) % 5 == 3 else r)
    L = 3 * k + 5
    for pos in (0, L - 1, k - 1, k):                               # one N
        for rep in range(3):
            b = bytearray(_cut(rng, P, L, 0.0))
            b[pos] = ord("N")
            reads.append(bytes(b))
    two_n = []
    for a in sorted({0, min(1, k - 1), k // 2 if k > 1 else 0, k - 1}):   # N at a and a + k + 1 (the last base)
        for src in (DUP_OF, 10):
            st = int(rng.integers(0, len(P[src]) - (a + k + 2)))
            b = bytearray(P[src][st:st + a + k + 2])
            b[a] = b[a + k + 1] = ord("N")
            two_n.append(len(reads))
            reads.append(bytes(b))
    tandem = []
    for copies in (3, 10, TANDEM_COPIES, 25, 28, 40, 57):          # 25, 28: more often than the reference, and still counted in LDS
        tandem.append(len(reads))
        reads.append(UNIT * copies)
    tandem.append(len(reads))
    reads.append(P[TANDEM][150:150 + 251])                         # flank + the whole repeat + flank
    assert all(len(r) <= 400 for r in reads) and 100 <= len(reads) <= 130
    return Ragged(tuple(reads), tuple(two_n), tuple(tandem))


def uniform_lengths(k, every=1, start=0):
    """64 consecutive lengths from k + 1: whatever T make_geom picks, the tile's window count T * (L - k [+ 1]) takes every residue
    mod 64 (T <= 16 odd) or every residue of a coset that holds 0 and values on both sides of 32 (T even)"""
    return [k + 1 + j for j in range(start, 64, every)]


@functools.lru_cache(maxsize=None)
def uniform(k, L):
    """37 reads of one length cut from the panel: 37 is coprime to every T in 2 .. 16, so the last tile is partial"""
    rng = np.random.default_rng(7000000 + 1000 * k + L)
    return tuple(_cut(rng, base_panel(), L, 0.0 if L % 3 else 0.01) for _ in range(37))


@functools.lru_cache(maxsize=None)
def counter_width(k=24):
    """(panel with a 2000-base reference appended, {255: read, 256: read, 257: read}): reads cut verbatim, so every window hits that
    reference and max_shared is the window count -- the largest value an 8-bit field holds, and the first that needs 16 bits"""
    rng = np.random.default_rng(255)
    big = rand(rng, 2000)
    reads = {}
    for i, w in enumerate((255, 256, 257)):
        L = w + k - (0 if DEFAULT.drop else 1)
        reads[w] = big[100 + 300 * i: 100 + 300 * i + L]
        assert nwin(L, k) == w
    return base_panel() + (big,), reads


def counter_width_batches(k=24):
    """[(reads, window counts)]: each of the three reads in a batch whose longest read has 255 windows and in one whose longest has
    256 (the 257-window read only in batches of its own width: the maximum is then 257)"""
    _, r = counter_width(k)
    return [([r[255]], [255]), ([r[255], r[256]], [255, 256]), ([r[256], r[255]], [256, 255]), ([r[257], r[255], r[256]], [257, 255, 256])]


@functools.lru_cache(maxsize=None)
def prefetch_edges(L, k):
    """a batch whose longest read has L bases: random sequence around 250 bases of the panel (so the read's distinct hits fit the
    kernel's per-read hit set at any L), next to ten short panel reads"""
    rng = np.random.default_rng(50000 + L + k)
    P = base_panel()
    seg = P[10][300:550]
    cut = int(rng.integers(20, L - 270))
    long_read = rand(rng, cut) + seg + rand(rng, L - cut - len(seg))
    assert len(long_read) == L
    reads = [_cut(rng, P, 120) for _ in range(5)] + [long_read] + [_cut(rng, P, 64 + 7 * i) for i in range(5)]
    return tuple(reads), 5


PanelEdges = collections.namedtuple("PanelEdges", "refs family short long")


@functools.lru_cache(maxsize=None)
def panel_edges(nref):
    """nref references of 80 bases, mutated copies of four ancestors in a shuffled order (families of 40, 70 and two large ones; the
    first three members of each family are exact copies: ties among >= 3 references).  Reads: .short (<= 255 windows at k = 24 and 48)
    and .long (> 255), from single families and from families 0 + 1 together (<= 110 references hit: within the 128 a sparse row holds)
    and from the large families (more than 128 references hit: a sparse row overflows and the kernel hands the read back)."""
    rng = np.random.default_rng(80 + nref)
    anc = [rand(rng, 80) for _ in range(4)]
    sizes = [40, 70, (nref - 110) // 2, nref - 110 - (nref - 110) // 2]
    fam = np.repeat(np.arange(4), sizes)
    members = []
    seen = [0, 0, 0, 0]
    for f in fam.tolist():
        members.append(anc[f] if seen[f] < 3 else mutate(rng, anc[f], 0.02))
        seen[f] += 1
    order = rng.permutation(nref)
    refs = tuple(members[i] for i in order)
    family = tuple(int(fam[i]) for i in order)
    short = [anc[f] for f in range(4)] + [mutate(rng, anc[f], 0.03) for f in range(4)]
    short += [anc[0] + anc[1], anc[1][:60] + anc[0], anc[2] + anc[3]]
    short += [rand(rng, 100), anc[0][10:70].lower()]
    lng = [(anc[0] + anc[1]) * 2 + rand(rng, 40), anc[1] * 4 + anc[0][:50], rand(rng, 30) + anc[0] * 4,
           (anc[2] + anc[3]) * 2 + rand(rng, 40)]
    assert all(nwin(len(r), 24) <= 255 for r in short) and all(nwin(len(r), 48) > 255 for r in lng)
    return PanelEdges(refs, family, tuple(short), tuple(lng))


# ---- read sets for the DEDUP forms: what only the per-read set of distinct hashes can get wrong --------------------------------------
Ladder = collections.namedtuple("Ladder", "reads random periodic")


@functools.lru_cache(maxsize=None)
def set_ladder(W, k=LADDER_K):
    """a batch whose longest read has W windows under windows=len-k (the host sizes the set from it: the power of two >= 2 W): a random
    read of W windows around at most 250 panel bases (every hash distinct: at W = uset / 2 its set is exactly half full), three times in
    a row (.random: for any T >= 2 reads per tile two neighbours share a tile -- (5, 6) unless T is 2, 3 or 6, (6, 7) unless T is 7 -- so
    a set addressed by the wrong read of the tile shows as a read without distinct hashes), a read of W windows with period 11
    (.periodic), ten short panel reads"""
    rng = np.random.default_rng(90000 + W)
    P = base_panel()
    L = W + k
    seg = P[10][300:300 + min(250, L // 2)]
    cut = int(rng.integers(0, L - len(seg) + 1))
    rnd = rand(rng, cut) + seg + rand(rng, L - cut - len(seg))
    per = (rand(rng, 11) * (L // 11 + 1))[:L]
    short = [_cut(rng, P, min(L, 30 + 8 * i)) for i in range(10)]
    reads = short[:5] + [rnd, rnd, rnd, per] + short[5:]
    assert max(len(r) for r in reads) == L == len(rnd) == len(per) and nwin(L, k) == W
    return Ladder(tuple(reads), (5, 6, 7), 8)


def stale_set():
    """one 150-base panel read 37 times: whatever T is, some workgroup walks two tiles of it, and an entry left in a set by the first
    makes every window of the second a duplicate"""
    return (base_panel()[3][200:350],) * 37


@functools.lru_cache(maxsize=None)
def several_k_limit():
    """(batch at the limit, batch beyond it, place of the long read) for ks = LIMIT_KS under windows=len-k: X + X with X of 532 bases
    (250 of them from the panel) has 1048 + 1000 = 2048 windows -- only a list of k reaches that, a staged read has at most 1528 bases --
    and 2 * 532 distinct hashes; one base more makes 2050 windows"""
    rng = np.random.default_rng(2048)
    P = base_panel()
    X = rand(rng, 140) + P[10][300:550] + rand(rng, 142)
    short = [_cut(rng, P, 70 + 7 * i) for i in range(10)]
    return tuple(short[:5] + [X + X] + short[5:]), tuple(short[:5] + [X + X + b"A"] + short[5:]), 5


_EXACTLY_S = {}


def exactly_s(orc, k, pol):
    """reads for a sketch of EXACT_S = 64: three copies of a random unit of p = 63, 64, 65 bases (more windows than S, exactly p distinct
    hashes: the unit is redrawn until that holds), then ten panel reads of fewer windows than S"""
    if (k, pol) not in _EXACTLY_S:
        rng = np.random.default_rng(6400 + k)
        reads = []
        for p in EXACT_P:
            while True:
                r = rand(rng, p) * 3
                h = window_hashes(orc, r, [k], pol)
                if len(h) > EXACT_S and len(np.unique(h[h != 0])) == p:
                    break
            reads.append(r)
        reads += [_cut(rng, base_panel(), k + 6 + 5 * i) for i in range(10)]
        _EXACTLY_S[(k, pol)] = tuple(reads)
    return _EXACTLY_S[(k, pol)]


def sparse_rows(nref, max_windows):
    """the kernel's documented rule (make_geom): 8-bit count fields while no read of the batch has more than 255 windows, else 16-bit;
    a dense row of more than 128 words becomes a 128-entry map"""
    per_word = 4 if max_windows <= 255 else 2
    return (nref + per_word - 1) // per_word >= 129


# ---- expectations ----------------------------------------------------------------------------------------------------------------
def pack(seqs, pad=64):
    """(uint8 bases with `pad` readable bytes behind them, uint64 offsets)"""
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if seqs:
        offs[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    b = np.zeros(int(offs[-1]) + pad, dtype=np.uint8)
    b[: int(offs[-1])] = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    return b, offs


def assert_routed(refs, reads, ks, pol=DEFAULT, allow_long=()):
    """the routing guarantees: nothing here lets the host send a read to the general path (rk_classify_batch's general_only)"""
    assert 0 < len(refs) <= MAX_REFS
    for i, r in enumerate(reads):
        assert len(r) <= FUSED_MAXLEN or i in allow_long, (i, len(r))
        assert sum(nwin(len(r), k, pol) for k in ks) <= S or i in allow_long, (i, len(r))


def assert_wholly_sketched(refs, ks, pol=DEFAULT):
    assert all(sum(nwin(len(r), k, pol) for k in ks) <= S for r in refs), "a reference is not wholly sketched"


def window_hashes(orc, seq, ks, pol):
    if pol.canon:
        return sm.calc_hashes(seq, ks, pol.model())
    return orc.calc_hashes(orc.to_upper(seq), ks, pol.oracle(orc))


def want_sketches(orc, refs, ks, pol, sketch_size=S):
    """list of ascending arrays, one per reference"""
    if pol.dedup:
        return [dm.bottom_distinct(window_hashes(orc, r, ks, pol), sketch_size) for r in refs]
    assert sketch_size == S
    if pol.canon:
        return sm.sketch_refs(list(refs), ks, S, pol.model())
    rb, ro = pack(list(refs))
    sk, ln = orc.sketch_refs(rb, ro, ks, S, pol.oracle(orc), threads=8)
    return [sk[j, : int(ln[j])] for j in range(len(refs))]


def masked_hashes(orc, reads, ks, pol, min_occ=None, slots=COUNT_SLOTS):
    """every read's window hashes, all k pooled; min_occ: after mask_by_frequency against the counts of these very reads' windows
    (every window counts, a zero hash in slot 0, a repeated value each time: the count pass is the same under either sketch rule)"""
    hs = [window_hashes(orc, r, ks, pol) for r in reads]
    if min_occ is None:
        return hs
    counter = np.zeros(slots, dtype=np.int64)
    for h in hs:
        np.add.at(counter, (h % np.uint64(slots)).astype(np.int64), 1)
    return [sm.mask_by_frequency(h, counter, min_occ, pol.model()) for h in hs]


def rows_distinct(sketches, hs, sketch_size=S, bound=None):
    """the rule of tests/dedup_model.py on given hashes: sketch = bottom_distinct, shared = a set intersection, field 3 = len(sketch)
    (capped by `bound`: rk_set_min_num_bound), first maximum wins"""
    post = {}
    for j, sk in enumerate(sketches):
        for v in np.unique(sk).tolist():
            post.setdefault(v, []).append(j)
    rows = np.zeros((len(hs), 4), dtype=np.int32)
    for i, h in enumerate(hs):
        mins = dm.bottom_distinct(h, sketch_size)
        shared = [0] * len(sketches)
        for v in mins.tolist():
            for j in post.get(v, ()):
                shared[j] += 1
        mi, ms, d = sm.argmax_diff(shared)
        rows[i] = (mi, ms, d, len(mins) if bound is None or bound < 0 else min(len(mins), bound))
    return rows


def want_rows(orc, refs, reads, ks, pol, sketches=None, min_occ=None, slots=COUNT_SLOTS, bound=None, sketch_size=S):
    """int32 [n, 4] rows (max_id, max_shared, diff, min_num); min_occ: under the exact -M mask counted over these very reads;
    bound, sketch_size: for dedup=distinct policies only"""
    sketches = want_sketches(orc, refs, ks, pol, sketch_size) if sketches is None else sketches
    if pol.dedup:
        return rows_distinct(sketches, masked_hashes(orc, reads, ks, pol, min_occ, slots), sketch_size, bound)
    assert bound is None and sketch_size == S
    if pol.canon:
        counter = sm.count_hashes(list(reads), ks, slots, pol.model()) if min_occ is not None else None
        return sm.classify(list(reads), sketches, ks, S, pol.model(), counter=counter, min_occ=min_occ or 0)
    sk = np.zeros((len(refs), S), dtype=np.uint64)
    ln = np.zeros(len(refs), dtype=np.int32)
    for j, x in enumerate(sketches):
        sk[j, : len(x)] = x
        ln[j] = len(x)
    qb, qo = pack(list(reads))
    if min_occ is None:
        return orc.classify_stream(qb, qo, ks, S, sk, ln, pol.oracle(orc), threads=8)
    return orc.classify_stream(qb, qo, ks, S, sk, ln, pol.oracle(orc), threads=8, min_kmer_occ=min_occ, counter_slots=slots)


def shared_counts(sketches, h):
    """the merge of rkmh.cpp:869 for one read's window hashes against every sketch: sum over values of min(multiplicities);
    also the same with the reference's multiplicity ignored (how many of the read's windows find their hash in the sketch)"""
    v, c = np.unique(h[h != 0], return_counts=True)
    multi = np.zeros(len(sketches), dtype=np.int64)
    plain = np.zeros(len(sketches), dtype=np.int64)
    for j, sk in enumerate(sketches):
        sv, sc = np.unique(sk, return_counts=True)
        at = np.searchsorted(sv, v)
        at[at == len(sv)] = 0
        hit = sv[at] == v if len(sv) else np.zeros(len(v), dtype=bool)
        multi[j] = np.minimum(c[hit], sc[at[hit]]).sum()
        plain[j] = c[hit].sum()
    return multi, plain


def may_hand_back(sketches, h, length, sparse):
    """The documented limits of the kernel's per-read LDS structures: a read may come back flagged for the general path when it is
    longer than the kernel stages, when a sketch hash occurs in it more than 30 times (5-bit occurrence field of the hit set), when
    it hits more than 1024 distinct sketch hashes (largest hit set), or more references than a sparse counter row holds (128)."""
    if length > FUSED_MAXLEN:
        return True
    allv = np.unique(np.concatenate([np.asarray(s, dtype=np.uint64) for s in sketches]))
    v, c = np.unique(h[h != 0], return_counts=True)
    at = np.searchsorted(allv, v)
    at[at == len(allv)] = 0
    hit = allv[at] == v
    if (c[hit] > 30).any() or int(hit.sum()) > 1024:
        return True
    if sparse:
        multi, _ = shared_counts(sketches, h)
        return int((multi > 0).sum()) > 128
    return False


def may_hand_back_distinct(sketches, h, length, sparse, sketch_size=S):
    """The kernel's documented limits under dedup=distinct, on one read's (masked) window hashes of all k: it may come back flagged
    when it is longer than the kernel stages, has more windows than half the largest per-read set, more distinct non-zero hashes than
    the sketch keeps, hits more than 1024 distinct sketch hashes, or -- under a sparse row -- more than 128 references.  A duplicate
    is dropped before the look-up, so the hit set only ever sees rank 0: no limit on how often a sketch hash occurs."""
    if length > FUSED_MAXLEN or len(h) > DEDUP_MAX_WINDOWS:
        return True
    v = np.unique(h[h != 0])
    if len(v) > sketch_size:
        return True
    hit = [np.isin(v, np.asarray(s, dtype=np.uint64)) for s in sketches]
    if int(np.logical_or.reduce(hit).sum()) > 1024 if hit else False:
        return True
    return bool(sparse) and sum(1 for x in hit if x.any()) > 128


def row_from_shared(multi, h):
    ms, mi, d = -1, 0, 0
    for j, v in enumerate(multi.tolist()):
        if v > ms:
            d, ms, mi = v - ms, v, j
    return [mi, ms, d, int((h != 0).sum())]
