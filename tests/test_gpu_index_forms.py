"""Every value form of the resident index at its boundary, read through all three readers (panels and read sets: tests/index_cases.py,
checked without a GPU by tests/test_index_cases_cpu.py).

For each panel two contexts take the same sketch rows through Context.set_reference_sketches: one with the k-mer-space form allowed
(k_classify_kmer answers the short reads) and one with it forbidden (k_classify_tile does).  In each:

  stats     Context.index_stats() equals the counts of the labels, form by form: the device says which form every key took, nothing
            is inferred from rows that happen to agree -- and the restated bucket fill (buckets, overflow flags, chain length, wrap)
  short     rows of classify equal the oracle's plain merge; rows of classify_device (flags left in place) equal it wherever they are
            not flagged, and are flagged -2 only where the kernel's documented limits allow (tile_cases.may_hand_back for
            k_classify_tile, index_cases.may_hand_back_kmer for k_classify_kmer); batches of <= 255 windows (8-bit counter fields)
            and of more (16-bit)
  long      the reads of 1600 .. 2400 bases through classify: accumulate_posting on the general path
  -M        the short reads counted into a depth map, set_depth_filter(map, 2), min_num bounds 0 and -1: the key ids that
            build_key_mask bakes into the masked map copies and the masked key array

All comparisons are exact integer equality."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import index_cases as ic  # noqa: E402
import tile_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu

FORMS = ("kmer", "hash")
BASES = {"forms": (0, 1), "wide_ids": (4, 0), "families": (8, 0), "chains": (0, 0)}    # (bases kept, cleared by the 5 % rule)


@pytest.fixture(scope="module")
def contexts(orc):
    """(panel, form) -> a context holding the panel's rows, made on first use and closed with the module"""
    import rkmh_amd
    made = {}

    def get(name, form):
        if (name, form) not in made:
            P = ic.panel(orc, name)
            c = rkmh_amd.Context(0, policy_spec=ic.POL.spec())
            made[(name, form)] = c
            c.set_kmer_form(form == "kmer")
            c.set_reference_sketches(P.sk, P.ln, ic.KS, P.S)
            assert c.kmer_form()[0] is (form == "kmer"), (name, form)
        return made[(name, form)]
    yield get
    for c in made.values():
        c.close()


@functools.lru_cache(maxsize=None)
def _want(orc, name, which, min_occ=None):
    P, rd = ic.panel(orc, name), ic.reads(orc, name)
    rows = ic.want_rows(orc, P, ic.short(rd) if which == "short" else rd.long, min_occ)
    rows.setflags(write=False)
    return rows


def _report(P, seqs, what, got, want):
    bad = np.nonzero((got != want).any(axis=1))[0]
    if len(bad):
        i = int(bad[0])
        raise AssertionError("%s, %s: %d rows differ; read %d of %d bases (%r...): got %s, want %s"
                             % (P.name, what, len(bad), i, len(seqs[i]), seqs[i][:40], got[i].tolist(), want[i].tolist()))


def _device_rows(c, qb, qo):
    import torch
    n = len(qo) - 1
    d_b = torch.from_numpy(qb).cuda()
    d_o = torch.from_numpy(qo.astype(np.int64)).to(torch.int32).cuda()
    d_out = torch.full((n, 4), -7, dtype=torch.int32, device="cuda")
    c.classify_device(d_b.data_ptr(), d_o.data_ptr(), n, d_out.data_ptr(), max_read_len=0, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ic.PANELS)
def test_index_stats_equal_the_labels(orc, contexts, name, form):
    P = ic.panel(orc, name)
    st = contexts(name, form).index_stats()
    hs, kv, fill = P.counts("hs"), P.counts("kv"), ic.bucket_fill(P.post)
    lists = [len(p) for h, p in P.post.items() if P.hs[h] == "list"]
    want = dict(keys=len(P.post), buckets=fill.nb, buckets_overflowed=fill.overflowed, longest_chain=fill.longest_chain, chain_wrapped=fill.wrapped,
                single_once=hs["single_once"], single_multi=hs["single_multi"], pair=hs["pair"], list=hs["list"],
                list_longest=max(lists + [0]), post_words=1 + sum(1 + 2 * n for n in lists))
    if form == "kmer":
        want.update(kmer_form=1, bases_kept=BASES[name][0], bases_dropped_by_share_rule=BASES[name][1], kv_reference=kv["reference"],
                    kv_single_multi=kv["single_multi"], kv_pair=kv["pair"], kv_inline_list=kv["inline"], kv_base_inline=kv["base_inline"],
                    kv_base_list=kv["base_list"], kv_plain_list=kv["plain"])
    else:                                                                               # not built: every k-mer-space counter reads 0
        want.update({k: 0 for k in st if k.startswith(("kv_", "bases_", "kmer_form"))})
        want.update(km1_bits=[0], km1_longest_hop=[0], kf4_sectors=[0], found=[0])
    print("index_stats", name, form, st)
    assert {k: st[k] for k in want} == want
    if form == "kmer":
        assert st["found"][0] >= len(P.post) and st["km1_bits"][0] >= 12 and st["kf4_sectors"][0] >= 256 and st["km1_longest_hop"][0] <= 7
    if name == "chains":
        assert st["buckets"] == 256 and st["chain_wrapped"] == 1 and st["longest_chain"] >= 4
    if name == "families" and form == "kmer":
        labels = {P.label[h]: h for h in P.boundary}
        near = sum(1 for h in P.post if P.kv[h].startswith("base") and min(len(set(P.post[h]) ^ set(b)) for b in ic.kmer_forms(P).bases) <= 8)
        assert st["kv_base_inline"] == near and st["kv_base_list"] == 2 == sum(P.kv[labels[x]] == "base_list" for x in ("A+5-4", "A+6-5"))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ic.PANELS)
def test_short_reads_through_the_fused_kernel(orc, contexts, name, form):
    P, rd, c = ic.panel(orc, name), ic.reads(orc, name), contexts(name, form)
    s, want = ic.short(rd), _want(orc, name, "short")
    hand_back = ic.may_hand_back_kmer if form == "kmer" else tc.may_hand_back
    for ids in ic.batches(rd):
        seqs = [s[i] for i in ids]
        qb, qo = tc.pack(seqs)
        what = "%s form, batch of %d short reads" % (form, len(ids))
        _report(P, seqs, what, c.classify(qb, qo), want[ids])
        raw = _device_rows(c, qb, qo)
        flagged = raw[:, 0] == -2
        keep = np.nonzero(~flagged)[0]
        _report(P, [seqs[i] for i in keep], what + ", resident input", raw[keep], want[ids][keep])
        sparse = tc.sparse_rows(P.nref, max(tc.nwin(len(r), ic.K) for r in seqs))
        for i in np.nonzero(flagged)[0].tolist():
            h = tc.window_hashes(orc, seqs[i], ic.KS, ic.POL)
            assert hand_back(P.hit_rows(h), h, len(seqs[i]), sparse), "%s: read %d (%r...) handed back without cause" % (what, i, seqs[i][:40])
        if form == "kmer":
            assert not flagged.any(), (what, int(flagged.sum()))       # (none of these reads is near k_classify_kmer's limits)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ic.PANELS)
def test_long_reads_through_the_general_path(orc, contexts, name, form):
    P, rd, c = ic.panel(orc, name), ic.reads(orc, name), contexts(name, form)
    qb, qo = tc.pack(list(rd.long))
    _report(P, rd.long, "%s form, long reads" % form, c.classify(qb, qo), _want(orc, name, "long"))


def test_a_refused_setter_changes_nothing(orc, data_dir):
    """rk_set_reference_sketches refuses a sketch length beyond S and a k beyond RK_MAX_K before anything in the context changes: the
    rows of classify, index_stats() and get_reference_sketches() are those of the set before; on a fresh context nothing is set"""
    import rkmh_amd
    from rkmh_amd import api
    refs = api.parse_files([os.path.join(data_dir, "all_pave_ref.fa.gz")])
    rb, ro = refs["bases"], refs["offsets"]
    two = [bytes(rb[int(ro[r]): int(ro[r]) + 3000]) for r in (0, 1)]
    reads = [two[0][100:250], two[0][1500:1650], two[1][7:157], two[1][2000:2150]]
    sk, ln = orc.sketch_refs(*orc.pack(two), [16], 1000, threads=1)
    qb, qo = tc.pack(reads)
    c = rkmh_amd.Context(0)
    try:
        c.set_reference_sketches(sk, ln, [16], 1000)
        A, stats = c.classify(qb, qo), c.index_stats()
        assert (A == orc.classify_stream(qb, qo, [16], 1000, sk, ln, threads=1)).all() and (A[:, 1] > 0).all()
        ln500 = np.minimum(ln, 500)
        long_ln = ln500.copy()
        long_ln[0] = 501
        for bad_ks, bad_ln in (([12], long_ln), ([65], ln500)):
            with pytest.raises(rkmh_amd.RkmhError):
                c.set_reference_sketches(sk[:, :500].copy(), bad_ln, bad_ks, 500)
            assert (c.classify(qb, qo) == A).all()
            assert c.index_stats() == stats
            gsk, gln = c.get_reference_sketches()
            assert gsk.shape == sk.shape and (gsk == sk).all() and (gln == ln).all()
    finally:
        c.close()
    c = rkmh_amd.Context(0)
    try:
        with pytest.raises(rkmh_amd.RkmhError):
            c.set_reference_sketches(sk[:, :500].copy(), long_ln, [12], 500)
        with pytest.raises(rkmh_amd.RkmhError, match="rk_set_references"):
            c.classify(qb, qo)
    finally:
        c.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ic.PANELS)
def test_depth_filter_by_key(orc, contexts, name, form):
    import rkmh_amd
    P, rd, c = ic.panel(orc, name), ic.reads(orc, name), contexts(name, form)
    s = ic.short(rd)
    want = _want(orc, name, "short", 2)
    assert (want != _want(orc, name, "short")).any()                   # the mask drops something ...
    assert (want[:, 1] > 0).sum() >= len(s) // 2                        # ... and leaves most hits
    qb, qo = tc.pack(list(s))
    cnt = rkmh_amd.Counter(c, slots=ic.COUNT_SLOTS)
    try:
        c.count_batch(qb, qo, cnt)
        for bound in (0, -1):
            c.set_min_num_bound(bound)
            c.set_depth_filter(cnt, 2)
            w = want.copy()
            if bound >= 0:
                w[:, 3] = np.minimum(w[:, 3], bound)
            _report(P, s, "%s form, -M 2 with min_num bound %d" % (form, bound), c.classify(qb, qo), w)
    finally:
        c.set_depth_filter(None, 0)
        c.set_min_num_bound(-1)
        cnt.destroy()
