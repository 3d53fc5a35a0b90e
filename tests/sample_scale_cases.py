"""Inputs for the sample accumulator where one workgroup takes many tiles (tests/test_sample_scale_cpu.py, tests/test_gpu_sample_scale.py;
DESIGN.md section 21): the grid-stride of k_sample_keep under the device entry's "twice the batch before" grid rule, the cap of 4 096
workgroups, the piece cuts of rk_sample_add_batch, mixed runs in one wave of k_run_sums and saturation in its wave path.  Pure Python
and numpy on abund_model, sourmash_model and sample_cases: neither the library nor the oracle is called here.

A case is a list of feeds (host arrays for Sample.add, or arrays to upload for Sample.add_device) and the expected sample.  The small
cases keep their reads, so that the plain model (sample_cases.want) and the library's own per-read union answer them; the large ones are
emitted from np.tile / np.cumsum and answered by closed forms, which the CPU file checks against the plain model on miniatures.

THE REPLICAS.  grid_of, device_grids, tiles_of and pieces follow launch_keep, feed_locked, k_sample_keep's tile loop and
rk_sample_add_batch's piece loop (rkmh_amd/csrc/rk_sample.hip) BY READING: rk_sample_stats does not show a grid or a piece, so nothing
checks them against the library, and they must be changed with it."""
import functools
from dataclasses import dataclass, field

import numpy as np

import abund_model as am
import sample_cases as sc
import scaled_model as scm
import sourmash_model as sm

W = sc.HASH_TILE_WIN                  # rk_kernels.hpp: HASH_TILE_WIN
K = sc.K
FULL = sc.FULL
GRID_CAP = 4096                       # rk_sample.hip, launch_keep: min(max(ceil(bound_bases / 2048), 1), 4096)
SK_T = 256                            # rk_sample.hip: positions per round of a tile
SK_STAGE = 1024                       # rk_sample.hip: values a workgroup holds back; it flushes when more than SK_STAGE - SK_T wait
DEFAULT_PENDING = 1 << 22             # rk_sample.hip: SK_DEFAULT_PENDING
PIECE_BASES = 64 << 20                # rk_sample.hip: SK_PIECE_BASES
PIECE_SEQS = 1 << 22                  # rk_sample.hip, rk_sample_add_batch: i1 - i0 < 2^22
SCAN_FIRST_TRIP = 1 << 20             # rk_sets.hpp: 1 024 counts of 1 024 entries are the most k_scan_blocks scans at one count a thread
LANE_RUN = 16                         # rk_sample.hip, k_run_sums: a lane sums a run of up to 16 entries itself
UNKNOWN_BOUND = 0xFFFFFFFF            # rk_sample.hip, feed_locked: the bound of a first feed through the device entry


# ---- the replicas ----
def grid_of(bound_bases):
    return min(max((bound_bases + W - 1) // W, 1), GRID_CAP)


def device_grids(batch_bases):
    """the grid of every feed of a fresh (or reset) sample through the device entry, from the bases of each batch: twice the batch
    before, and the unknown bound where there is none (or it held no bases)"""
    out, last = [], 0
    for nb in batch_bases:
        out.append(grid_of(2 * last if last else UNKNOWN_BOUND))
        last = nb
    return out


def tiles_of(nbases, grid):
    """-> per workgroup that has any, the tiles it takes, in its order"""
    ntiles = (nbases + W - 1) // W
    return [list(range(w, ntiles, grid)) for w in range(min(grid, ntiles))]


def pieces(offsets, piece_bases=PIECE_BASES, piece_seqs=PIECE_SEQS):
    """rk_sample_add_batch's loop -> [(i0, i1)], pieces of whole sequences (the two limits are parameters for the miniatures)"""
    off = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    nseq, out, i0 = len(off) - 1, [], 0
    while i0 < nseq:
        # the largest i1 with off[i1] - off[i0] <= PIECE_BASES and i1 - i0 <= PIECE_SEQS, at least i0 + 1 (the while loop of the source, searched)
        by_bases = int(np.searchsorted(off, off[i0] + piece_bases, side="right")) - 1
        i1 = max(i0 + 1, min(by_bases, i0 + piece_seqs, nseq))
        out.append((i0, i1))
        i0 = i1
    return out


def pieces_plain(offsets, piece_bases=PIECE_BASES, piece_seqs=PIECE_SEQS):
    """the same loop written as the source writes it (for miniatures: it steps sequence by sequence)"""
    off = [int(x) for x in offsets]
    nseq, out, i0 = len(off) - 1, [], 0
    while i0 < nseq:
        i1 = i0 + 1
        while i1 < nseq and off[i1 + 1] - off[i0] <= piece_bases and i1 - i0 < piece_seqs:
            i1 += 1
        out.append((i0, i1))
        i0 = i1
    return out


# ---- the model by position ----
def window_table(reads, k, pol, mh):
    """the value kept at every position of the reads laid end to end (0: no window there, an invalid one, or one above mh)"""
    st = sc.starts(reads)
    t = np.zeros(int(st[-1]), dtype=np.uint64)
    for r, s in zip(reads, st.tolist()):
        h = sm.window_hashes(r, k, pol)
        t[s:s + len(h)] = np.where(h <= np.uint64(mh), h, np.uint64(0))
    return t


def union(parts):
    """abund_model.merge without its loop over values (shown equal to it by the CPU file); abundances saturate at 2^32 - 1"""
    parts = [(np.asarray(v, dtype=np.uint64), np.asarray(a, dtype=np.uint64)) for v, a in parts]
    v = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, np.uint64)
    a = np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, np.uint64)
    if len(v) == 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    order = np.argsort(v, kind="stable")
    v, a = v[order], a[order]
    first = np.flatnonzero(np.concatenate([[True], v[1:] != v[:-1]]))
    tot = np.add.reduceat(a, first)          # (below 2^64: the callers' totals are)
    return v[first], np.minimum(tot, am.SAT).astype(np.uint32)


def sketch_of_tables(tables):
    """(values, abund) of position tables, one per k and feed"""
    h = np.concatenate([t[t != 0] for t in tables]) if tables else np.zeros(0, np.uint64)
    return union([(h, np.ones(len(h), np.uint64))])


def staged_trace(tables_by_k, nbases, grid):
    """k_sample_keep's counter by reading: one launch (the k of one instantiation, in list order) over a batch of nbases positions.
    -> (per workgroup: [(tile, values staged when the tile ends)], flushes inside the tile loop, flushes in mid-tile)"""
    ends, flushes, mid = [], 0, 0
    for mine in tiles_of(nbases, grid):
        nstage, row = 0, []
        for tile in mine:
            a = tile * W
            nwin = min(nbases - a, W)
            for t in tables_by_k:
                for i0 in range(0, nwin, SK_T):
                    nstage += int(np.count_nonzero(t[a + i0: a + min(i0 + SK_T, nwin)]))
                    if nstage > SK_STAGE - SK_T:
                        flushes += 1
                        mid += 1 if (i0 + SK_T < nwin or t is not tables_by_k[-1]) else 0
                        nstage = 0
            row.append((tile, nstage))
        ends.append(row)
    return ends, flushes, mid


def launches(ks):
    """launch_keep: the k = 16 instantiation first, then the one for every other k of the list"""
    return [g for g in ([k for k in ks if k == 16], [k for k in ks if k != 16]) if g]


# ---- cases ----
@dataclass
class Feed:
    route: str                 # "host": Sample.add(bases, offsets);  "device": upload, then Sample.add_device with uint32 offsets
    bases: np.ndarray          # uint8, with slack behind the last base
    offsets: np.ndarray        # uint64[nseq + 1]; offsets[0] may be above 0
    reads: tuple = None        # the reads, where the case is small enough to keep them

    @property
    def nseq(self):
        return len(self.offsets) - 1

    @property
    def nbases(self):
        return int(self.offsets[-1]) - int(self.offsets[0])


@dataclass
class Case:
    name: str
    feeds: list
    values: np.ndarray         # expected
    abund: np.ndarray
    kept: int
    ks: tuple = (K,)
    policy: str = "default"
    mh: int = FULL
    pending_cap: int = 0
    retries: str = None        # None: not asserted; "none": == 0; "some": >= 1
    small: bool = False        # every feed keeps its reads: the plain model and the library's own union answer it
    note: dict = field(default_factory=dict)

    @property
    def nseq(self):
        return sum(f.nseq for f in self.feeds)

    @property
    def nbases(self):
        return sum(f.nbases for f in self.feeds)

    @property
    def reads(self):
        return [r for f in self.feeds for r in f.reads]

    @property
    def pol(self):
        return sc.POLICIES[self.policy]


def feed_of_reads(route, reads, lead=0, seed=0):
    """the reads packed behind `lead` random ACGT bases that belong to no read (offsets[0] = lead)"""
    b, off = sc.pack(list(reads))
    if lead:
        junk = np.frombuffer(sc.rand_read(np.random.default_rng(1000 + seed), lead), dtype=np.uint8)
        b = np.concatenate([junk, b])
        off = off + np.uint64(lead)
    b = np.concatenate([b, np.zeros(64, np.uint8)])
    return Feed(route, b, off, tuple(reads))


def small_case(name, feeds, **kw):
    ks, pol, mh = kw.get("ks", (K,)), sc.POLICIES[kw.get("policy", "default")], kw.get("mh", FULL)
    tables = [window_table(f.reads, k, pol, mh) for f in feeds for k in ks]
    v, a = sketch_of_tables(tables)
    return Case(name, feeds, v, a, int(sum(np.count_nonzero(t) for t in tables)), small=True, **kw)


@functools.lru_cache(maxsize=None)
def primer(nbases):
    return (sc.rand_read(np.random.default_rng(300 + nbases), nbases),)


def B():
    return sc.tile_batch()[0]


SPARSE_MH = scm.max_hash(50)      # each strand's hash is below it one time in 50: about one window in 25 is kept


def with_empties(where):
    """B with 3 000 empty reads between two real ones: "mid" -- in the middle of tile 0; "edge" -- exactly on the tile edge at 2 048"""
    reads, on_boundary = sc.tile_batch()
    at = {"mid": 4, "edge": on_boundary}[where]
    return tuple(reads[:at]) + (b"",) * 3000 + tuple(reads[at:])


THIRD_MH = scm.max_hash(3)        # a window's value is the smaller of two strands' hashes: 1 - (2/3)^2 = 5 in 9 are kept, about 140 a
                                  # round, so the flushes (every sixth round or so) fall out of step with the tiles' eight rounds


@functools.lru_cache(maxsize=None)
def stride_cases():
    """section A: name -> Case.  Every case but the host forms feeds a primer through the device entry first.  Each shape stands at
    FULL and, as <name>_third, at THIRD_MH.  At FULL every round of 256 positions of B keeps more than 192 values and at most 256,
    so the workgroup flushes after every fourth round, in mid-tile and at the tile's end: by the replica NOTHING waits across a
    tile edge there (test_sample_scale_cpu.py asserts that too).  At THIRD_MH it flushes in mid-tile AND carries values across the
    edges; at SPARSE_MH it only carries."""
    P100, P1025, P2049 = primer(100), primer(1025), primer(2049)
    dev = lambda reads, **kw: feed_of_reads("device", reads, **kw)
    out = [small_case("grid1_sparse", [dev(P100), dev(B())], mh=SPARSE_MH)]
    for tag, mh in (("", FULL), ("_third", THIRD_MH)):
        out += [
            small_case("grid1" + tag, [dev(P100), dev(B())], mh=mh),
            small_case("grid2" + tag, [dev(P1025), dev(B())], mh=mh),
            small_case("grid3" + tag, [dev(P2049), dev(B())], mh=mh),
            small_case("grid1_k12_16_retry" + tag, [dev(P100), dev(B())], mh=mh, ks=(12, 16), pending_cap=1024, retries="some"),
            small_case("grid1_k21" + tag, [dev(P100), dev(B())], mh=mh, ks=(21,)),
            small_case("grid1_mash" + tag, [dev(P100), dev(B())], mh=mh, policy="mash"),
            small_case("grid1_sourmash" + tag, [dev(P100), dev(B())], mh=mh, policy="sourmash"),
            small_case("grid1_first_4099" + tag, [dev(P100), dev(B(), lead=4099, seed=1)], mh=mh),
            small_case("host_first_5" + tag, [feed_of_reads("host", B(), lead=5, seed=2)], mh=mh),
            small_case("grid1_empties_mid" + tag, [dev(P100), dev(with_empties("mid"))], mh=mh),
            small_case("grid1_empties_edge" + tag, [dev(P100), dev(with_empties("edge"))], mh=mh),
            small_case("host_empties_mid" + tag, [feed_of_reads("host", with_empties("mid"))], mh=mh),
            small_case("host_empties_edge" + tag, [feed_of_reads("host", with_empties("edge"))], mh=mh),
            # three feeds for the reset test: grids 4 096, 1 and twice B's bases, on which three times B strides
            small_case("three_feeds" + tag, [dev(P100), dev(B()), dev(B() + B()[::-1] + B())], mh=mh),
            small_case("three_feeds_retry" + tag, [dev(P100), dev(B()), dev(B() + B()[::-1] + B())], mh=mh, pending_cap=1024, retries="some"),
        ]
    return {c.name: c for c in out}


def is_host_form(name):
    return name.startswith("host_")                 # host arrays: the grid equals the tiles, nothing strides


def case_grids(case):
    """the grid of every feed of the case: the device entry's rule from the batch before, the exact bases for host arrays (which are
    one piece each here)"""
    dev = iter(device_grids([f.nbases for f in case.feeds if f.route == "device"]))
    return [next(dev) if f.route == "device" else grid_of(f.nbases) for f in case.feeds]


# ---- B: past the cap of 4 096 workgroups ----
@functools.lru_cache(maxsize=None)
def block():
    """56 distinct reads of reads300 (no copies) whose total U is odd: the repeats then meet the tile edges at every phase"""
    src = [r for i, r in enumerate(sc.reads300()) if i % 10 != 9]
    assert len(set(src)) == len(src)
    reads, spare = src[:56], src[56:]
    while sum(len(r) for r in reads) % 2 == 0:
        reads[-1] = spare.pop(0)
    return tuple(reads)


def block_bases():
    return sum(len(r) for r in block())


def repeated_block(R, route="host"):
    """the block R times over as 56 R separate reads, from np.tile and np.cumsum"""
    one = np.frombuffer(b"".join(block()), dtype=np.uint8)
    lens = np.array([len(r) for r in block()], dtype=np.uint64)
    off = np.zeros(56 * R + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.tile(lens, R))
    return Feed(route, np.concatenate([np.tile(one, R), np.zeros(64, np.uint8)]), off)


def repeated_case(name, R, mh, **kw):
    """closed form: the block's values, its abundances and kept times R"""
    v, a, kept = sc.want(block(), mh=mh)
    assert R * int(a.max()) < am.SAT
    return Case(name, [repeated_block(R)], v, (a.astype(np.uint64) * np.uint64(R)).astype(np.uint32), kept * R, mh=mh, **kw)


def cap_R():
    U = block_bases()
    return -(-(GRID_CAP + 3) * W // U)


QUARTER_MH = scm.max_hash(4)      # keeps 1 - (3/4)^2 = 7 windows in 16
CAP_MH = {"quarter": QUARTER_MH, "fold": sc.FOLD_MH, "full": FULL}


def cap_case(which):
    """"quarter": the kept windows fit the default pending array, no retry.  "fold" (sample_cases.FOLD_MH keeps 3 windows in 4, the
    smaller of two hashes being under half the range that often) and "full": they do not, the batch retries and the array grows."""
    return repeated_case("cap_" + which, cap_R(), CAP_MH[which], retries="none" if which == "quarter" else "some", note=dict(R=cap_R()))


# ---- C: the piece cuts ----
CUT_MH = scm.max_hash(32)


def cut_by_bases_R():
    U = block_bases()
    return (PIECE_BASES + 2 * U) // U + 1


def cut_by_bases_case():
    return repeated_case("cut_by_bases", cut_by_bases_R(), CUT_MH, note=dict(R=cut_by_bases_R()))


PERIOD = 8400
LONG_L = PIECE_BASES + 5000


@functools.lru_cache(maxsize=None)
def period_string():
    return np.frombuffer(sc.rand_read(np.random.default_rng(31), PERIOD), dtype=np.uint8)


def periodic_read(L):
    S = period_string()
    return np.tile(S, -(-L // PERIOD))[:L]


def periodic_sketch(L, ks=(K,), pol=sm.DEFAULT, mh=FULL):
    """closed form of the periodic read of L bases: the window at each phase p of S, kept |{i = p mod 8400 : i + k + d <= L}| times
    (d = 1 when the policy drops the last window); phases that hash alike merged.  -> (values, abund, kept)"""
    S = period_string().tobytes()
    parts, kept = [], 0
    for k in ks:
        h = sm.window_hashes(S + S[:k], k, dict(pol, drop_last=0))[:PERIOD]
        last = L - k - (1 if pol["drop_last"] else 0)                 # the last position that is a window
        p = np.arange(PERIOD, dtype=np.int64)
        n = np.where(p <= last, (last - p) // PERIOD + 1, 0).astype(np.uint64)
        ok = (h != 0) & (h <= np.uint64(mh)) & (n > 0)
        parts.append((h[ok], n[ok]))
        kept += int(n[ok].sum())
    v, a = union(parts)
    return v, a, kept


def long_read_sides():
    r = sc.reads300()
    return tuple(r[100:110]), tuple(r[200:210])


def long_read_case(alone=False):
    """ONE read of 64 MiB + 5 000 bases between ten reads300 reads and ten more (three pieces), or alone for the device entry"""
    body = periodic_read(LONG_L)
    lv, la, lkept = periodic_sketch(LONG_L)
    if alone:
        off = np.array([0, LONG_L], dtype=np.uint64)
        return Case("long_read_alone", [Feed("device", np.concatenate([body, np.zeros(64, np.uint8)]), off)], lv, la, lkept, retries="some")
    front, back = long_read_sides()
    fb, fo = sc.pack(list(front))
    bb, bo = sc.pack(list(back))
    nf, nbk = int(fo[-1]), int(bo[-1])
    off = np.concatenate([fo, np.uint64(nf + LONG_L) + bo]).astype(np.uint64)
    bases = np.concatenate([fb[:nf], body, bb[:nbk], np.zeros(64, np.uint8)])
    sv, sa, skept = sc.want(front + back)
    v, a = union([(lv, la), (sv, sa)])
    return Case("long_read", [Feed("host", bases, off)], v, a, lkept + skept, retries="some", note=dict(long_index=len(front)))


COUNT_NSEQ = PIECE_SEQS + 3
COUNT_REAL_AT = (0, PIECE_SEQS - 1, PIECE_SEQS, PIECE_SEQS + 2)


def count_reals():
    r = sc.reads300()
    return (r[1], r[2], r[3], r[4])


def cut_by_count_feed(nseq=COUNT_NSEQ, real_at=COUNT_REAL_AT):
    reals = count_reals()
    lens = np.ones(nseq, dtype=np.uint64)
    lens[list(real_at)] = [len(r) for r in reals]
    off = np.zeros(nseq + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    bases = np.full(int(off[-1]) + 64, ord("A"), dtype=np.uint8)
    bases[int(off[-1]):] = 0
    for i, r in zip(real_at, reals):
        bases[int(off[i]): int(off[i + 1])] = np.frombuffer(r, dtype=np.uint8)
    return Feed("host", bases, off)


def cut_by_count_case():
    v, a, kept = sc.want(count_reals())
    return Case("cut_by_count", [cut_by_count_feed()], v, a, kept)


# ---- D: k_run_sums ----
MIX_MULT = (1, 2, 16, 17, 63, 64, 65, 300)


@functools.lru_cache(maxsize=None)
def mixed_reads():
    """eight distinct reads of about 120 bases with the multiplicities of MIX_MULT, interleaved by one fixed permutation"""
    rng = np.random.default_rng(41)
    distinct = [sc.rand_read(rng, int(n)) for n in rng.integers(112, 129, size=len(MIX_MULT))]
    idx = np.repeat(np.arange(len(MIX_MULT)), MIX_MULT)
    return tuple(distinct), tuple(distinct[i] for i in rng.permutation(idx))


MIX_CAP_WHOLE = 1 << 16
MIX_GROUP = 8          # reads per feed of the grouped form: about 830 kept windows, under a pending_cap of 1 000


def mixed_cases():
    """one batch at a pending_cap that holds everything; one batch at 1 000 (a retry that grows the array: again one fold over whole
    runs); and feeds of eight reads at 1 000, where folds meet resident counts with pending ones behind them"""
    _, reads = mixed_reads()
    return [small_case("mixed_whole", [feed_of_reads("host", reads)], pending_cap=MIX_CAP_WHOLE, retries="none"),
            small_case("mixed_cap_1000", [feed_of_reads("host", reads)], pending_cap=1000, retries="some"),
            small_case("mixed_grouped_1000", [feed_of_reads("host", g) for g in sc.batches(reads, MIX_GROUP)], pending_cap=1000, retries="none")]


SAT_FEEDS = 17
SAT_START = am.SAT - 10


def saturation_case():
    """-> (x, read): x a value of the read kept once; add_sketch([x], [2^32 - 1 - 10]), then the read 17 times in one batch"""
    read = sc.reads300()[1]
    v, a, _ = sc.want([read])
    j = len(v) // 2
    assert int(a[j]) == 1
    return int(v[j]), read
