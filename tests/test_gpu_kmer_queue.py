"""The candidate queue of the k-mer-space kernel (k_classify_kmer, rk_kmer.hip): 16-bit entries P | read << 12, 640 of them, drained
when the next step of 256 windows might not fit and once after a tile's last step.  A tile of reads drawn from the panel at the usual
key density (about one window in eight) makes one drain call; the cases here are about the other tiles: so many candidates that the
window loop must stop, drain whole waves of 64 mid-tile and carry the remainder forward, several times per tile.

Every case classifies through rk_classify_batch_device (max_read_len = 0: the geometry follows the batch's longest read) and compares
the rows bit for bit with oracle.classify_stream on the oracle's reference sketches.  A row of -2 would be answered elsewhere and hide
the kernel, so every case also asserts that no row comes back -2.

Density.  The dense references are random sequences no longer than S + k - 1 bases (S = 2000), so their sketches hold every k-mer and
EVERY window of an error-free read drawn from them is a key: 84 / 134 / 234 / 484 candidates per read of 100 / 150 / 250 / 500 bases
(a read of L bases has L - k windows; density 1.0; up to 8 x 84, 6 x 134, 4 x 234, 2 x 484 per tile against a queue of 640).  The
per-read hit multiset is sized from that density (three slots per expected hit, at most 1024), so these reads are the kernel's own:
the parent build answers every row of every case here.  Thinned cases: the 1200-base reads
(NQ = 2) are 700 bases of a reference followed by 500 bases of random text (684 of 1184 windows are keys, density 0.58: a fully dense
read of that length has more hits than the 1024-slot multiset holds and is handed back by design) and the 1010-base reads take 600
dense bases (density 0.59).  The references of the two-size run (k = 12 and 16 together) are 1000 bases long, so that the k-mers of
both sizes fit the sketch.  With density 1.0 in the panel the launch uses the large LDS layout; the queue and the drain are the same
code in both layouts."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S = 2000
GLEN = 1500                      # <= S + k - 1 for every k used here: the sketch of such a reference holds all its k-mers
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
THREADS = min(16, os.cpu_count() or 1)


def _rand(rng, n):
    return bytes(rng.choice(ACGT, size=n))


def _pad(b):
    out = np.zeros(len(b) + 16, dtype=np.uint8)
    out[: len(b)] = b
    return out


def _device_rows(c, qb, qo):
    import torch
    n = len(qo) - 1
    d_b = torch.from_numpy(qb).cuda()
    d_o = torch.from_numpy(qo.astype(np.int64)).to(torch.int32).cuda()
    d_out = torch.full((n, 4), -7, dtype=torch.int32, device="cuda")
    c.classify_device(d_b.data_ptr(), d_o.data_ptr(), n, d_out.data_ptr(), max_read_len=0, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


class _Panel:
    """one context per panel: references set once, sketches checked against the oracle's once, any number of batches"""

    def __init__(self, orc, refs, ks, seed):
        import rkmh_amd
        self.orc, self.refs, self.ks = orc, refs, list(ks)
        self.rng = np.random.default_rng(seed)
        rb, ro = orc.pack(refs)
        rb = _pad(rb)
        self.wsk, self.wln = orc.sketch_refs(rb, ro, self.ks, S, threads=THREADS)
        self.c = rkmh_amd.Context(0)
        try:
            self.c.set_references(rb, ro, self.ks, S)
            assert self.c.kmer_form()[0], "the k-mer-space kernel must be the one that answers"
            sk, ln = self.c.get_reference_sketches()
            assert (sk == self.wsk).all() and (ln == self.wln).all(), "reference sketches differ from the oracle's"
        except BaseException:
            self.c.close()
            raise

    def close(self):
        self.c.close()

    def dense(self, L, keep=None, ref=None):
        """an error-free read of L bases: the first `keep` (default: all) from a reference (default: any), the rest random text"""
        keep = L if keep is None else keep
        g = self.refs[int(self.rng.integers(0, len(self.refs))) if ref is None else ref]
        p = int(self.rng.integers(0, len(g) - keep + 1))
        return g[p: p + keep] + _rand(self.rng, L - keep)

    def text(self, L):
        return _rand(self.rng, L)

    def tiles(self, T, L, keep=None, counts=None):
        """tiles of T reads of L bases: `nd` dense reads first, then last, for every nd in counts (default 0 .. T); the two
        alternating tiles; a short last tile of dense reads"""
        reads = []
        for nd in (range(T + 1) if counts is None else counts):
            for first in (True, False):
                for t in range(T):
                    d = t < nd if first else t >= T - nd
                    reads.append(self.dense(L, keep) if d else self.text(L))
        for odd in (0, 1):
            if T > 1:
                reads += [self.dense(L, keep) if t % 2 == odd else self.text(L) for t in range(T)]
        reads += [self.dense(L, keep) for _ in range(max(1, T // 2))]
        return reads

    def check(self, reads, what):
        qb, qo = self.orc.pack(reads)
        qb = _pad(qb)
        want = self.orc.classify_stream(qb, qo, self.ks, S, self.wsk, self.wln, threads=THREADS)
        raw = _device_rows(self.c, qb, qo)
        assert raw.shape == want.shape == (len(reads), 4)
        back = np.nonzero(raw[:, 0] == -2)[0]
        assert len(back) == 0, "%s: %d rows handed back (first: read %d of %d bases)" % (what, len(back), back[0], len(reads[back[0]]))
        bad = np.nonzero((raw != want).any(axis=1))[0]
        assert len(bad) == 0, "%s: %d rows differ; read %d of %d bases: got %s, want %s" % (
            what, len(bad), bad[0], len(reads[bad[0]]), raw[bad[0]].tolist(), want[bad[0]].tolist())
        return raw


def _random_refs(seed, n, glen=GLEN):
    rng = np.random.default_rng(seed)
    return [_rand(rng, glen) for _ in range(n)]


@pytest.fixture(scope="module")
def k16(orc):
    p = _Panel(orc, _random_refs(11, 10), [16], 101)
    yield p
    p.close()


@pytest.fixture(scope="module")
def two_k(orc):
    p = _Panel(orc, _random_refs(12, 10, glen=1000), [12, 16], 102)    # 988 + 984 k-mers per reference <= S
    yield p
    p.close()


@pytest.fixture(scope="module")
def wide(orc):
    p = _Panel(orc, _random_refs(13, 10), [17], 103)
    yield p
    p.close()


@pytest.fixture(scope="module")
def family(orc):
    """twelve near-identical references (a handful of substitutions each) beside four unrelated ones: every hit of a family read has a
    posting list of twelve, stored as (base, exceptions) -- the FAM instantiations"""
    rng = np.random.default_rng(14)
    anc = rng.choice(ACGT, size=GLEN)
    refs = []
    for m in range(12):
        g = anc.copy()
        if m % 4 != 0:
            pos = rng.integers(0, GLEN, size=3)
            g[pos] = rng.choice(ACGT, size=3)
        refs.append(bytes(g))
    refs += _random_refs(15, 4)
    p = _Panel(orc, refs, [16], 104)
    assert p.c.index_stats()["bases_kept"] > 0, "the panel was meant to switch the (base, exceptions) lists on"
    yield p
    p.close()


# ---- 1. dense tiles at every tile geometry: 0 .. T dense reads per tile, first / last / alternating, random text between them ---------
@pytest.mark.parametrize("L,T", [(100, 8), (150, 6), (250, 4), (500, 2)])
def test_dense_tiles(k16, L, T):
    assert min((1024 - 15) // L, 8) == T
    raw = k16.check(k16.tiles(T, L), "dense tiles, %d bases" % L)
    assert raw[:, 1].max() == L - 16                 # a dense read scores every one of its L - k windows


def test_dense_tiles_two_quads_per_lane(k16):
    """1200 bases: NQ = 2, one read per tile, positions up to 1199 + the padding's 2048 (entries up to 0x8803); thinned to 700 dense
    bases (see the module's docstring)"""
    raw = k16.check(k16.tiles(1, 1200, keep=700), "1200 bases")
    assert raw[:, 1].max() >= 700 - 16
    raw = k16.check(k16.tiles(2, 1010, keep=600), "1010 bases")      # NQ = 2 with two reads per tile
    assert raw[:, 1].max() >= 600 - 16


def test_unequal_lengths_and_invalid_bases(k16):
    """tiles of unequal reads (the searched group -> read mapping) and dense reads holding an N (the has_invalid copy of the window
    code), in uniform and in unequal tiles"""
    rng = k16.rng
    uneven = []
    for i in range(60):
        L = 150 if i % 6 == 0 else int(rng.integers(16, 151))
        uneven.append(k16.dense(L) if i % 5 != 4 else k16.text(L))
    k16.check(uneven, "unequal lengths")

    def with_n(s, at):
        return s[:at] + b"N" + s[at + 1:]
    reads = [k16.dense(150) for _ in range(24)]
    for i, at in ((1, 0), (4, 75), (8, 149), (9, 15), (15, 134), (22, 60)):
        reads[i] = with_n(reads[i], at)
    raw = k16.check(reads, "dense reads with an N")
    assert raw[4, 1] == 134 - 16 and raw[0, 1] == 134 and raw[1, 1] == 133     # an N spoils the windows that hold it
    for i, at in ((3, 10), (17, 40), (31, 5), (44, 0)):
        if len(uneven[i]) > at:
            uneven[i] = with_n(uneven[i], at)
    k16.check(uneven, "unequal lengths with an N")


# ---- 2. the other instantiations that share the queue: their smallest dense and mixed case ---------------------------------------------
def _dense_and_mixed(p, T, L, keep=None):
    return p.tiles(T, L, keep, counts=(T, T // 2))


def test_several_k(two_k):
    """KT = 0: one pass over the tile's windows per k-mer size, the queue starts empty for each; 138 + 134 windows per read"""
    raw = two_k.check(_dense_and_mixed(two_k, 4, 150), "k = 12 and 16")
    assert raw[:, 1].max() == (150 - 12) + (150 - 16)


def test_wide_k(wide):
    """KT = 32: k = 17, 64-bit k-mers"""
    raw = wide.check(_dense_and_mixed(wide, 6, 150), "k = 17")
    assert raw[:, 1].max() == 150 - 17


def test_family_panel(family):
    """FAM on: a dense read of the family defers or expands 134 posting lists of twelve"""
    raw = family.check(_dense_and_mixed(family, 6, 150), "family panel")
    assert raw[:, 1].max() == 134


@pytest.mark.parametrize("nref,L,glen", [(512, 150, 200), (513, 150, 200), (256, 300, 400), (257, 300, 400)])
def test_sparse_counters(orc, nref, L, glen):
    """Both sides of both switches of the per-read counter form (the launcher's rule: 8-bit fields while no read has more than 255
    windows, else 16-bit; a 128-entry sparse map from 129 words per row up):
        512 references, 150 bases: 134 windows, 8-bit fields, 128 words -- the largest dense row;  513: 129 words, sparse
        256 references, 300 bases: 284 windows, 16-bit fields, 128 words -- dense;                  257: sparse
    The references are `glen` bases long, so a dense read lies inside one of them.  One read is drawn from the last reference and one
    from the first: at the dense boundary the arg-max of the former reads the last field of the row's last word."""
    p = _Panel(orc, _random_refs(16, nref, glen=glen), [16], 105)
    try:
        T = min((1024 - 15) // L, 8)
        reads = _dense_and_mixed(p, T, L) + [p.dense(L, ref=nref - 1), p.dense(L, ref=0)]
        raw = p.check(reads, "%d references, %d bases" % (nref, L))
    finally:
        p.close()
    assert raw[:, 1].max() == L - 16
    assert raw[-2, :2].tolist() == [nref - 1, L - 16] and raw[-1, :2].tolist() == [0, L - 16]
