"""The per-read reference counters of the k-mer-space kernel (rk_kmer.hip): with dense counters a posting is one add, and phase 2
derives the maximum, its FIRST reference (rkmh.cpp:878) and the best earlier score from the finished row.  Every row must equal
the oracle's: ties between references far apart in id order, reads that hit nothing, repeated k-mers against keys of multiplicity
above one, reads long enough for 16-bit counters, panels whose last counter word is partly used, and a config-3-sized family panel."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _pad(b):
    out = np.zeros(len(b) + 16, dtype=np.uint8)
    out[: len(b)] = b
    return out


def _panel(rng, nref, glen=4000):
    """random genomes; a few are exact copies placed far apart in id order (their reads tie), one holds a tandem repeat"""
    refs = [bytes(rng.choice(ACGT, size=glen)) for _ in range(nref)]
    for a, b in ((1, nref - 1), (3, nref // 2), (0, nref - 2)):
        refs[b] = refs[a]
    unit = bytes(rng.choice(ACGT, size=23))
    g = bytearray(refs[5])
    g[1000:1000 + 23 * 40] = (unit * 40)[: 23 * 40]  # k-mers of the repeat occur many times: sketch multiplicity > 1
    refs[5] = bytes(g)
    refs[nref - 3] = bytes(g)  # ... and tie with a reference far away
    return refs


def _reads(rng, refs, n, L):
    seqs = []
    for i in range(n):
        r = rng.random()
        if r < 0.1:  # no hit at all
            seqs.append(bytes(rng.choice(ACGT, size=L)))
            continue
        g = refs[int(rng.integers(0, len(refs)))]
        if r < 0.3:  # from the tandem repeat: the same k-mers many times in one read
            g = refs[5]
            p = int(rng.integers(900, 1100))
        else:
            p = int(rng.integers(0, len(g) - L))
        s = bytearray(g[p: p + L])
        if r > 0.8:  # a few substitutions: counts below the read's maximum for the other references
            for q in rng.integers(0, L, size=4):
                s[int(q)] = int(rng.choice(ACGT))
        seqs.append(bytes(s))
    return seqs


def _check(orc, refs, seqs, ks, S):
    import rkmh_amd
    rb, ro = orc.pack(refs)
    rb = _pad(rb)
    qb, qo = orc.pack(seqs)
    qb = _pad(qb)
    T = min(16, os.cpu_count() or 1)
    c = rkmh_amd.Context(0)
    try:
        c.set_references(rb, ro, ks, S)
        assert c.kmer_form()[0]
        sk, ln = c.get_reference_sketches()
        want = orc.classify_stream(qb, qo, ks, S, sk, ln, threads=T)
        got = c.classify(qb, qo)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (len(bad), got[bad[:5]], want[bad[:5]])
        return got
    finally:
        c.close()


@pytest.mark.parametrize("nref", [181, 182, 183, 184])
def test_ties_misses_and_partial_counter_words(orc, nref):
    """4 n + {1, 2, 3, 0} references: the last counter word holds 1, 2, 3 or 4 of them"""
    rng = np.random.default_rng(100 + nref)
    refs = _panel(rng, nref)
    got = _check(orc, refs, _reads(rng, refs, 12000, 150), [16], 1000)
    assert (got[:, 0] == 0).any() and (got[:, 0] > nref // 2).any()  # misses and far winners both occur


@pytest.mark.parametrize("L", [300, 600])
def test_long_reads_sixteen_bit_counters(orc, L):
    """more than 255 windows per read: 16-bit counters"""
    rng = np.random.default_rng(7 + L)
    refs = _panel(rng, 45, glen=6000)
    _check(orc, refs, _reads(rng, refs, 6000, L), [16], 2000)


def test_config3_sized_family_panel(orc):
    """266 references, families of near-identical genomes: postings stored as (base, exceptions), expanded in phase 2"""
    rng = np.random.default_rng(266)
    refs = []
    for n in (61, 21, 10):
        anc = rng.choice(ACGT, size=5000)
        for m in range(n):
            g = anc.copy()
            if m % 4:
                pos = rng.integers(0, len(g), size=8 * (m % 4))
                g[pos] = rng.choice(ACGT, size=len(pos))
            refs.append(bytes(g))
        refs.extend(bytes(rng.choice(ACGT, size=5000)) for _ in range(58))
    assert len(refs) == 266
    _check(orc, refs, _reads(rng, refs, 12000, 150), [16], 1000)
