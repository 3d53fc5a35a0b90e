"""The policy key canon= (U2) at the host layer, and the pure-Python model the GPU tests
of that key are checked against (tests/sourmash_model.py) pinned by known-answer vectors that come from outside this repository.
No GPU."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import sourmash_model as sm  # noqa: E402
from rkmh_amd import api  # noqa: E402

DEFAULT_TEXT = "fold=swap32,windows=len-k,zero=count,mask=lt,freqmax=incl,seed=42"
MASH_TEXT = "fold=h1,windows=len-k+1,zero=count,mask=lt,freqmax=incl,seed=42"
LEXMIN_TEXT = "fold=h1,windows=len-k+1,zero=count,mask=lt,freqmax=incl,canon=lexmin,seed=42"


def _golden(name):
    return json.load(open(os.path.join(HERE, "golden", name)))["vectors"]


# ---- the model against vectors from an independent murmur ----
def test_model_murmur_known_answers():
    vec = _golden("murmur3_kat.json")
    assert len(vec) >= 50
    for v in vec:
        assert sm.murmur3_x64_128(bytes.fromhex(v["key_hex"]), v["seed"]) == (v["h1"], v["h2"]), v


def test_model_lexmin_known_answers():
    vec = _golden("lexmin_kat.json")
    assert len(vec) >= 50
    ks = {v["k"] for v in vec}
    assert set(range(8, 33)) | {40, 64} <= ks
    assert sum(v["kmer"] == sm.revcomp(v["kmer"].encode()).decode() for v in vec) >= 5     # palindromes
    assert sum(v["kmer"] != v["lexmin_strand"] for v in vec) >= 10                          # the reverse strand wins
    for v in vec:
        km = v["kmer"].encode()
        assert sm.lexmin_strand(km).decode() == v["lexmin_strand"], v
        for fold in (0, 1, 2):
            want = sm.fold128(v["h1"], v["h2"], fold)
            pol = dict(sm.LEXMIN, fold=fold)
            assert sm.kmer_hash(km, pol) == want, v
            assert sm.kmer_hash(km.lower(), pol) == want, v
            got = sm.window_hashes(km, v["k"], pol)         # the numpy form: one window
            assert got.tolist() == [want], v


def test_model_numpy_form_equals_scalar_form():
    rng = np.random.default_rng(7)
    seq = bytes(rng.choice(np.frombuffer(b"ACGTACGTACGTacgtNR", dtype=np.uint8), 300).tolist())
    for k in (8, 15, 16, 17, 31, 32, 33, 48, 64):
        for canon in (0, 1):
            for fold in (0, 1, 2):
                for drop in (0, 1):
                    pol = dict(sm.DEFAULT, canon=canon, fold=fold, drop_last=drop)
                    got = sm.window_hashes(seq, k, pol)
                    want = [sm.kmer_hash(seq[i:i + k], pol) for i in range(len(seq) - k + (0 if drop else 1))]
                    assert got.tolist() == want, (k, pol)
    d, n = sm.lexmin_differs(seq, 16, sm.MASH)
    assert n > 0 and d * 4 >= n      # about half of all k-mers hash differently under the two rules


def test_model_bottom_and_merge():
    h = np.array([5, 0, 3, 3, 9, 0, 3, 7, 7], dtype=np.uint64)
    assert sm.bottom(h, 4).tolist() == [3, 3, 3, 5]
    assert sm.bottom(h, 40).tolist() == [3, 3, 3, 5, 7, 7, 9]
    assert sm.intersection_size([0, 0, 3, 3, 3, 5], [3, 3, 4, 5, 5]) == 3
    assert sm.argmax_diff([0, 4, 4, 6, 2]) == (3, 6, 2)
    assert sm.argmax_diff([0, 0]) == (0, 0, 1)
    rng = np.random.default_rng(3)
    refs = [np.sort(rng.integers(1, 40, 30).astype(np.uint64)) for _ in range(5)]
    # classify()'s per-value min(multiplicity) equals the two-pointer merge
    for _ in range(20):
        a = np.sort(rng.integers(1, 40, 25).astype(np.uint64))
        vals, cnt = np.unique(a, return_counts=True)
        for r in refs:
            rv, rc = np.unique(r, return_counts=True)
            m = dict(zip(rv.tolist(), rc.tolist()))
            assert sum(min(c, m.get(v, 0)) for v, c in zip(vals.tolist(), cnt.tolist())) == sm.intersection_size(a, r)


# ---- rk_policy_parse / describe / same_hashes ----
def test_default_and_mash_describe_as_before():
    assert api.describe_policy(api.parse_policy(None)) == DEFAULT_TEXT
    assert api.describe_policy(api.parse_policy("default")) == DEFAULT_TEXT
    assert api.describe_policy(api.parse_policy("mash")) == MASH_TEXT
    assert api.describe_policy(api.parse_policy("canon=minhash")) == DEFAULT_TEXT
    assert api.parse_policy("mash").canon == 0          # `mash` keeps its meaning: fold, windows, seed only
    assert api.parse_policy(None).canon == 0


def test_canon_key():
    p = api.parse_policy("mash,canon=lexmin")
    assert (p.fold, p.drop_last_window, p.canon, p.seed) == (1, 0, 1, 42)
    assert api.describe_policy(p) == LEXMIN_TEXT
    assert api.describe_policy(api.parse_policy("mash,canon=lexmin,canon=minhash")) == MASH_TEXT
    assert api.describe_policy(api.parse_policy("canon=lexmin")) == DEFAULT_TEXT.replace(",seed", ",canon=lexmin,seed")
    assert api.describe_policy(api.parse_policy("canon=lexmin,default")) == DEFAULT_TEXT
    assert api.describe_policy(api.parse_policy("canon=lexmin,mash")) == LEXMIN_TEXT      # the preset leaves the strand rule alone


def test_describe_parse_round_trip():
    for fold in ("swap32", "h1", "w2w1"):
        for canon in ("minhash", "lexmin"):
            for windows in ("len-k", "len-k+1"):
                spec = "fold=%s,windows=%s,zero=skip,mask=le,freqmax=excl,canon=%s,seed=9" % (fold, windows, canon)
                p = api.parse_policy(spec)
                text = api.describe_policy(p)
                q = api.parse_policy(text)
                assert bytes(p) == bytes(q), spec
                assert api.describe_policy(q) == text
                assert ("canon=" in text) == (canon == "lexmin")


def test_same_hashes_tells_the_key_apart():
    lib = api.load_library()
    same = lambda a, b: lib.rk_policy_same_hashes(C.byref(api.parse_policy(a)), C.byref(api.parse_policy(b)))  # noqa: E731
    assert same("mash,canon=lexmin", "fold=h1,windows=len-k+1,canon=lexmin") == 1
    assert same("mash,canon=lexmin", "mash,canon=lexmin,zero=skip,mask=le,freqmax=excl") == 1    # counter keys do not change hashes
    assert same("mash,canon=lexmin", "mash") == 0
    assert same("canon=lexmin", "default") == 0
    assert same("default", "canon=minhash") == 1


@pytest.mark.parametrize("spec", ["canon=", "canon=LEXMIN", "canon=lex", "canon=1", "canon", "canon=lexmin;mash"])
def test_refusals(spec):
    with pytest.raises(api.RkmhError):
        api.parse_policy(spec)


def test_unknown_key_message_lists_the_new_key():
    with pytest.raises(api.RkmhError) as e:
        api.parse_policy("strand=lexmin")
    assert "canon" in str(e.value)
    with pytest.raises(api.RkmhError) as e:
        api.parse_policy("canon=lex")
    assert "minhash|lexmin" in str(e.value)


def test_struct_layout():
    assert C.sizeof(api.Policy) == 7 * 4            # one int32 appended after seed
    names = [f[0] for f in api.Policy._fields_]
    assert names == ["fold", "drop_last_window", "counter_counts_zero", "mask_strict_less", "freq_max_inclusive", "seed", "canon"]
    for i, n in enumerate(names):
        assert getattr(api.Policy, n).offset == 4 * i
