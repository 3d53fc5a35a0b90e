"""The general path (rk_general.hip) on the two branches no other test reaches: a classified read that needs the multi-block
select, and a batch that is planned as two chunks.  Both against the CPU oracle, value for value."""
import os

import numpy as np
import pytest

from helpers import rand_dna

pytestmark = pytest.mark.gpu

T = min(16, os.cpu_count() or 1)


def _pad(b):
    out = np.zeros(len(b) + 16, dtype=np.uint8)
    out[: len(b)] = b
    return out


def _three_reads(text):
    """One read per route of the general path's sort step, cut from `text` so that the shorter two lie inside the longest (every
    k-mer of theirs occurs at least twice in the batch: a depth filter of 2 keeps some hashes and drops others)."""
    big = bytes(text[1000:301000])       # 299 985 windows at k = 16: more than 2^18, the multi-block select
    mid = bytes(text[50000:80000])       # 29 985 windows: more than the in-LDS sorter holds, the block pre-select
    short = bytes(text[60005:60155])     # 135 windows: the fused kernel where the panel and the sketch allow it
    return [big, mid, short]


def _pave_panel(orc, data_dir):
    recs = orc.kseq_parse_file(os.path.join(data_dir, "all_pave_ref.fa.gz"))
    rb, ro = orc.pack([r[1] for r in recs])
    return rb, ro, 1000, _three_reads(rb)


def _many_refs_panel(orc, data_dir):
    # the panel of test_panel_too_large_for_lds_counters: 45 000 references, neighbours overlap by 30 bases
    rng = np.random.default_rng(77)
    nref = 45000
    genome = rand_dna(rng, 60 * nref + 200, b"ACGT")
    rb, ro = orc.pack([genome[60 * i: 60 * i + 90] for i in range(nref)])
    return rb, ro, 16, _three_reads(genome)


@pytest.mark.parametrize("panel,min_occ", [(_pave_panel, None), (_pave_panel, 2), (_many_refs_panel, None)],
                         ids=["pave", "pave-depth2", "45000refs"])
def test_multi_block_select_feeds_the_intersect(orc, data_dir, panel, min_occ):
    """A classified read with more than 2^18 hashes: bottom-S by multi-block radix select, then sort + intersect of the selection
    (so far only sketches took that route).  Beside it a read for the block pre-select and a short one; every row against the
    oracle.  With a depth filter the selection itself masks by the counter.  The third case counts in global rows
    (SortArgs::gcount): 200 references of 400 bases would not -- sort_intersect_global_rows(1024, 200) is 0, their counter row
    (800 bytes) fits the LDS beside the sort buffer -- so it takes the 45 000 references that are known to need them."""
    import rkmh_amd
    rb, ro, S, reads = panel(orc, data_dir)
    assert [len(r) for r in reads] == [300000, 30000, 150]
    qb, qo = orc.pack(reads)
    wsk, wln = orc.sketch_refs(rb, ro, [16], S, threads=T)
    kw = dict(min_kmer_occ=min_occ, counter_slots=1000003) if min_occ else {}
    want = orc.classify_stream(qb, qo, [16], S, wsk, wln, threads=T, **kw)
    c = rkmh_amd.Context(0)
    try:
        c.set_references(_pad(rb), ro, [16], S)
        cnt = None
        if min_occ:
            cnt = rkmh_amd.Counter(c, slots=1000003)
            c.count_batch(_pad(qb), qo, cnt)
            c.set_depth_filter(cnt, min_occ)
        try:
            got = c.classify(_pad(qb), qo)
        finally:
            if cnt is not None:
                c.set_depth_filter(None, 0)
                cnt.destroy()
    finally:
        c.close()
    for i in range(len(reads)):
        assert (got[i] == want[i]).all(), (i, got[i], want[i])
    assert (want[:, 1] > 0).all()  # the reads come from the panel: every one shares hashes with its best reference


def test_batch_planned_as_two_chunks(ctx, orc):
    """sketch_batch over a batch whose hashes do not fit one chunk of the general path (2^26): the first two sequences make
    chunk one, the third opens chunk two, whose bases, tiles and output rows start past those of the first."""
    ks, S = [9, 10, 11, 12, 13, 14, 15, 16], 16
    lens = [4200000, 1000, 4200000, 150]
    nh = [sum(L - k for k in ks) for L in lens]                      # the default policy drops the last window
    assert nh[0] + nh[1] <= 2 ** 26 < nh[0] + nh[1] + nh[2]
    rng = np.random.default_rng(2026)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=sum(lens))]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    want_sk, want_ln = orc.sketch_refs(bases, offs, ks, S, threads=4)
    sk, ln = ctx.sketch_batch(_pad(bases), offs, ks, S)
    assert (ln == want_ln).all(), (ln, want_ln)
    assert (sk == want_sk).all()
    assert (want_ln == S).all()
