"""The policy key dedup= (U6) and the `sourmash` preset at the host layer, the pure-Python model of the key (tests/dedup_model.py)
against hand-checked vectors, and the non-vacuity conditions of the GPU inputs (tests/dedup_cases.py).  No GPU."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import dedup_cases as dc  # noqa: E402
import dedup_model as dm  # noqa: E402
import sourmash_model as sm  # noqa: E402
import test_policy_canon_cpu as canon_cpu  # noqa: E402  (the literals every earlier policy text must still equal)
from rkmh_amd import api  # noqa: E402

SOURMASH_TEXT = "fold=h1,windows=len-k+1,zero=count,mask=lt,freqmax=incl,canon=lexmin,dedup=distinct,seed=42"
DISTINCT = 0x100


# ---- the model ----
def test_model_known_answers():
    vec = json.load(open(os.path.join(HERE, "golden", "dedup_kat.json")))["vectors"]
    assert len(vec) >= 20
    names = " | ".join(v["name"] for v in vec)
    for must in ("empty", "all zeros", "all equal", "fewer than S distinct", "across rank S", "zeros mixed in"):
        assert must in names, must
    for v in vec:
        h = np.array(v["hashes"], dtype=np.uint64)
        assert dm.bottom_distinct(h, v["S"]).tolist() == v["sketch"], v["name"]
        assert dm.bottom_distinct(h[::-1], v["S"]).tolist() == v["sketch"], v["name"]      # order of the input does not matter


def test_model_equals_the_multiset_rule_without_repeats():
    rng = np.random.default_rng(2)
    for n in (0, 1, 5, 64, 1000):
        h = rng.permutation(np.arange(1, n + 1, dtype=np.uint64) * np.uint64(2654435761))
        for S in (1, 16, 64, 2000):
            assert dm.bottom_distinct(h, S).tolist() == sm.bottom(h, S).tolist()
    refs = dc.references()[:12]                           # random sequences: no repeated k-mer
    reads = [r[10:90] for r in refs]
    want = sm.classify(reads, sm.sketch_refs(refs, [16], 64, sm.MASH), [16], 64, sm.MASH)
    assert (dm.classify(reads, dm.sketch_refs(refs, [16], 64, sm.MASH), [16], 64, sm.MASH) == want).all()


def test_model_rows_are_set_intersections():
    refs = [np.array([3, 5, 9], dtype=np.uint64), np.array([5, 7], dtype=np.uint64)]
    post = dm.classify([b""], refs, [4], 4, sm.DEFAULT)
    assert post.tolist() == [[0, 0, 1, 0]]
    assert dm.frequency_filter([4, 6, 0, 8], np.array([1, 3], dtype=np.int32), 1, 1).tolist() == [4, 6, 0, 8]
    assert dm.frequency_filter([4, 5], np.array([1, 3], dtype=np.int32), 1, 1).tolist() == [4, 0]


# ---- rk_policy_parse / describe / same_hashes ----
def test_sourmash_preset():
    p = api.parse_policy("sourmash")
    assert (p.fold, p.drop_last_window, p.seed, p.canon) == (1, 0, 42, 1 | DISTINCT)
    assert (p.strand, p.dedup) == (1, 1)
    assert api.describe_policy(p) == SOURMASH_TEXT
    assert bytes(api.parse_policy("mash,canon=lexmin,dedup=distinct")) == bytes(p)
    assert bytes(api.parse_policy(SOURMASH_TEXT)) == bytes(p)
    assert C.sizeof(api.Policy) == 28


def test_mash_and_default_leave_the_bit_alone():
    assert api.parse_policy("mash").dedup == 0 and api.parse_policy("default").dedup == 0 and api.parse_policy(None).dedup == 0
    assert api.parse_policy("dedup=distinct,mash").canon == DISTINCT
    assert api.describe_policy(api.parse_policy("dedup=distinct,mash")) == canon_cpu.MASH_TEXT.replace(",seed", ",dedup=distinct,seed")
    assert api.describe_policy(api.parse_policy("dedup=distinct,default")) == canon_cpu.DEFAULT_TEXT.replace(",seed", ",dedup=distinct,seed")
    assert api.describe_policy(api.parse_policy("sourmash,default")) == canon_cpu.DEFAULT_TEXT.replace(",seed", ",dedup=distinct,seed")
    assert api.describe_policy(api.parse_policy("sourmash,dedup=multiset")) == canon_cpu.LEXMIN_TEXT
    assert api.describe_policy(api.parse_policy("sourmash,canon=minhash")) == canon_cpu.MASH_TEXT.replace(",seed", ",dedup=distinct,seed")


def test_texts_without_the_key_are_what_they_were():
    assert api.describe_policy(api.parse_policy(None)) == canon_cpu.DEFAULT_TEXT
    assert api.describe_policy(api.parse_policy("default")) == canon_cpu.DEFAULT_TEXT
    assert api.describe_policy(api.parse_policy("mash")) == canon_cpu.MASH_TEXT
    assert api.describe_policy(api.parse_policy("mash,canon=lexmin")) == canon_cpu.LEXMIN_TEXT
    assert api.describe_policy(api.parse_policy("dedup=multiset")) == canon_cpu.DEFAULT_TEXT
    assert api.describe_policy(api.parse_policy("mash,dedup=multiset")) == canon_cpu.MASH_TEXT


def test_round_trip_fold_canon_dedup():
    for fold in ("swap32", "h1", "w2w1"):
        for canon in ("minhash", "lexmin"):
            for dedup in ("multiset", "distinct"):
                spec = "fold=%s,windows=len-k+1,zero=skip,mask=le,freqmax=excl,canon=%s,dedup=%s,seed=9" % (fold, canon, dedup)
                p = api.parse_policy(spec)
                assert (p.strand, p.dedup) == (canon == "lexmin", dedup == "distinct")
                text = api.describe_policy(p)
                q = api.parse_policy(text)
                assert bytes(p) == bytes(q) and api.describe_policy(q) == text, spec
                assert ("dedup=distinct" in text) == (dedup == "distinct") and "dedup=multiset" not in text
                assert ("canon=lexmin" in text) == (canon == "lexmin")
                if canon == "lexmin" and dedup == "distinct":
                    assert text.index("canon=") < text.index("dedup=") < text.index("seed=")
                if dedup == "multiset":     # byte-identical to the text the parent of this key printed
                    want = "fold=%s,windows=len-k+1,zero=skip,mask=le,freqmax=excl,%sseed=9" % (fold, "canon=lexmin," if canon == "lexmin" else "")
                    assert text == want


def test_policy_properties_are_properties():
    assert [f[0] for f in api.Policy._fields_] == ["fold", "drop_last_window", "counter_counts_zero", "mask_strict_less", "freq_max_inclusive", "seed", "canon"]
    assert isinstance(api.Policy.strand, property) and isinstance(api.Policy.dedup, property)
    p = api.parse_policy("mash")
    p.dedup = 1
    assert p.canon == DISTINCT and p.strand == 0
    p.strand = 1
    assert p.canon == DISTINCT | 1 and api.describe_policy(p) == SOURMASH_TEXT
    p.dedup = 0
    assert p.canon == 1 and api.describe_policy(p) == canon_cpu.LEXMIN_TEXT
    p.canon = 0x200                                   # no known rule
    with pytest.raises(api.RkmhError):
        api.describe_policy(p)


def test_same_hashes_separates_the_two_values():
    lib = api.load_library()
    same = lambda a, b: lib.rk_policy_same_hashes(C.byref(api.parse_policy(a)), C.byref(api.parse_policy(b)))  # noqa: E731
    assert same("sourmash", "mash,canon=lexmin,dedup=distinct,zero=skip") == 1
    assert same("sourmash", "mash,canon=lexmin") == 0
    assert same("dedup=distinct", "default") == 0
    assert same("dedup=multiset", "default") == 1


@pytest.mark.parametrize("spec", ["dedup=", "dedup=1", "dedup=Distinct", "dedup", "sourmash=1", "Sourmash"])
def test_refusals(spec):
    with pytest.raises(api.RkmhError):
        api.parse_policy(spec)


def test_messages_list_the_key():
    with pytest.raises(api.RkmhError) as e:
        api.parse_policy("distinct=yes")
    assert "dedup" in str(e.value) and "canon" in str(e.value)
    with pytest.raises(api.RkmhError) as e:
        api.parse_policy("dedup=set")
    assert "multiset|distinct" in str(e.value)
    with pytest.raises(api.RkmhError) as e:
        api.parse_policy("sourmesh")
    assert "sourmash" in str(e.value)


# ---- the inputs of tests/test_gpu_dedup.py mean something ----
def test_raw_arrays_are_not_vacuous():
    dc.raw_conditions(dc.raw_arrays())


def test_reference_sketches_are_not_vacuous():
    refs = dc.references()
    for _, pol in dc.SPECS:
        multi = sm.sketch_refs(refs, [16], dc.S_SEQ, pol)
        dist = dm.sketch_refs(refs, [16], dc.S_SEQ, pol)
        assert len(dist[12]) < 8 and len(multi[12]) == dc.S_SEQ              # the tandem repeat: a handful of distinct k-mers
        assert len(np.unique(multi[13])) < dc.S_SEQ == len(dist[13])        # the container sketches reference 0's hashes twice
        assert all(d.tolist() == m.tolist() for d, m in zip(dist[:12], multi[:12]))


@pytest.mark.parametrize("k", dc.ROW_K)
@pytest.mark.parametrize("spec", [s for s, _ in dc.SPECS])
def test_rows_are_not_vacuous(k, spec):
    dc.row_conditions(k, dict(dc.SPECS)[spec])
