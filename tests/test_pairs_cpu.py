"""Sketch comparison without a GPU: the model (tests/pairs_model.py) against the hand-checked vectors, the host half of the feature
(rk_merge_sketches, rk_mash_distance), everything `rkmh dist` refuses before it creates a context, and -- on the model's output --
that the panel inputs of tests/test_gpu_pairs.py exercise every count they compare."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import dedup_model as dm
import pairs_cases as pc
import pairs_model as pm
import sourmash_model as sm
from rkmh_amd import api


# ---- the model against the vectors ----
@pytest.mark.parametrize("i", range(len(pc.kat())))
def test_model_matches_hand_checked_vectors(i):
    v = pc.kat()[i]
    assert list(pm.pair_counts(v["a"], v["b"], v["S"])) == v["want"], v["name"]
    assert list(pm.pair_counts(v["b"], v["a"], v["S"])) == v["want"], v["name"]        # every count is symmetric
    sk, ln = pm.rows([v["a"], v["b"]], v["S"])                                           # and as padded rows
    out = pm.all_pairs(sk[:1], ln[:1], sk[1:], ln[1:])
    assert out[0, 0].tolist() == v["want"], v["name"]
    j, d = pm.mash_distance(v["want"][2], v["want"][3], v["k"])
    assert j == v["jaccard"] and abs(d - v["distance"]) < 1e-15, v["name"]


def test_vectors_cover_what_they_must():
    names = " | ".join(v["name"] for v in pc.kat())
    assert len(pc.kat()) >= 20
    for v in pc.kat():
        assert len(v["a"]) <= v["S"] and len(v["b"]) <= v["S"] and v["a"] == sorted(v["a"]) and v["b"] == sorted(v["b"]) and 0 not in v["a"] + v["b"]
    assert any(not v["a"] and not v["b"] for v in pc.kat()) and any(bool(v["a"]) != bool(v["b"]) for v in pc.kat())
    assert any(v["a"] == v["b"] and v["a"] for v in pc.kat())
    assert any(len(v["a"]) >= v["S"] and v["b"] and max(v["a"]) < min(v["b"]) and v["want"][2:] == [0, v["S"]] for v in pc.kat())
    assert any(v["a"] == [5, 5, 5] and v["b"] == [5, 5] and v["want"] == [2, 1, 1, 1] for v in pc.kat())
    assert any(x >= 1 << 63 for v in pc.kat() for x in v["a"] + v["b"])
    assert any(v["want"][1] > v["want"][2] for v in pc.kat())                  # a common value past the S-th union value
    assert any(v["want"][0] > v["want"][1] for v in pc.kat())                  # repeats
    assert "low 32 bits" in names and "high 32 bits" in names and "padding" in names and "straddles" in names
    zero = [v for v in pc.kat() if v["want"][2] == v["want"][3] > 0]
    assert zero and all(v["distance"] == 0 and pm.distance_text(v["distance"]) == "0" for v in zero)


# ---- rk_mash_distance ----
def test_mash_distance_vectors_and_refusals():
    for v in pc.kat():
        j, d = api.mash_distance(v["want"][2], v["want"][3], v["k"])
        assert j == v["jaccard"] and abs(d - v["distance"]) < 1e-15, v["name"]
        assert not math.copysign(1.0, d) < 0, v["name"]                       # never -0
    assert api.mash_distance(1000, 1000, 21) == (1.0, 0.0) and math.copysign(1.0, api.mash_distance(7, 7, 1)[1]) == 1.0
    assert api.mash_distance(0, 0, 16) == (0.0, 1.0)
    assert api.mash_distance(1, 1000, 1)[1] == 1.0                            # clamped: -ln(2 / 1001) > 1
    j, d = api.mash_distance(500, 1000, 21)
    assert j == 0.5 and abs(d - math.log(1.5) / 21) < 1e-15
    for bad in ((-1, 5, 16), (1, -5, 16), (6, 5, 16), (1, 5, 0), (1, 5, -3)):
        with pytest.raises(api.RkmhError) as e:
            api.mash_distance(*bad)
        assert e.value.code == -1


# ---- rk_merge_sketches ----
def _parts(rng, n, S, pool):
    """n sketches of S, some empty, some short; values repeat inside a part and across parts"""
    parts = []
    for i in range(n):
        ln = (0, 1, S, S // 2)[i % 4] if n > 1 else S - 1
        parts.append(np.sort(rng.choice(pool, size=ln, replace=True)))
    return parts


@pytest.mark.parametrize("n", [1, 2, 17])
@pytest.mark.parametrize("S", [1, 5, 64, 1000])
def test_merge_sketches_is_the_bottom_of_the_concatenation(n, S):
    rng = np.random.default_rng(100 * n + S)
    pool = rng.integers(1, 1 << 64, size=max(3, S + S // 2), dtype=np.uint64, endpoint=False)
    parts = _parts(rng, n, S, pool)
    sk, ln = pm.rows([p.tolist() for p in parts], S)
    cat = np.concatenate(parts) if parts else np.zeros(0, np.uint64)
    if n == 17 and S >= 5:
        assert len(np.unique(cat)) < len(cat) and len(cat) > S and (ln == 0).any() and ((ln > 0) & (ln < S)).any()
        assert len(np.intersect1d(parts[2], parts[6])) > 0                   # repeats across parts
    for distinct, want in ((False, sm.bottom(cat, S)), (True, dm.bottom_distinct(cat, S))):
        got, m = api.merge_sketches(sk, ln, S, distinct=distinct)
        assert m == len(want) and got[:m].tolist() == want.tolist() and (got[m:] == 0).all() and len(got) == S, (n, S, distinct)


def test_merge_sketches_edges_and_refusals():
    got, m = api.merge_sketches(np.zeros((0, 4), np.uint64), np.zeros(0, np.int32), 4)
    assert m == 0 and got.tolist() == [0, 0, 0, 0]
    sk, ln = pm.rows([[5, 5, 9], [5, 7]], 3)
    assert api.merge_sketches(sk, ln, 3)[0].tolist() == [5, 5, 5] and api.merge_sketches(sk, ln, 3, distinct=True)[0].tolist() == [5, 7, 9]
    sk[0, 0] = 0                                                             # a zero inside the length is padding, not a value
    got, m = api.merge_sketches(sk, ln, 3)
    assert (got.tolist(), m) == ([5, 5, 7], 3)
    for lens in ([4, 1], [-1, 1]):
        with pytest.raises(api.RkmhError):
            api.merge_sketches(sk, np.array(lens, np.int32), 3)
    with pytest.raises(api.RkmhError):
        api.merge_sketches(np.zeros((1, 16385), np.uint64), np.zeros(1, np.int32), 16385)


# ---- rkmh dist: everything it refuses, before a context exists (so it runs without a GPU) ----
def _run(root, *args):
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    return subprocess.run([os.path.join(root, "bin", "rkmh")] + list(args), capture_output=True, env=env)


def _sketch_file(path, policy="fold=swap32,windows=len-k,zero=count,mask=lt,freqmax=incl,seed=42", kmer="16", length=4, n=2):
    doc = [{"alphabet": "ATGC", "canonical": "true", "hashBits": 64, "hashPolicy": policy, "hashSeed": 42, "hashType": "MurmurHash3_x64_128",
            "kmer": kmer, "name": "s%d" % i, "preserveCase": "false", "seqLen": 100,
            "sketches": {"comment": "", "hashes": [3 + i, 9, 20], "length": length, "name": "s%d" % i}} for i in range(n)]
    path.write_text(json.dumps(doc, separators=(",", ":")))
    return str(path)


def test_dist_help(root):
    r = _run(root, "dist")
    assert r.returncode == 1 and r.stdout == b"" and b"rkmh dist (-r" in r.stderr and b"-Q" in r.stderr
    r = _run(root)
    assert r.returncode == 1 and b"  dist " in r.stderr


def test_dist_refusals(root, data_dir, tmp_path):
    fa = os.path.join(data_dir, "zika.refs.fa.gz")
    ok = _sketch_file(tmp_path / "ok.json")
    MASH = "fold=h1,windows=len-k+1,zero=count,mask=lt,freqmax=incl,seed=42"
    cases = {
        "two -k": ["-r", fa, "-k", "12", "-k", "16"],
        "S above the limit": ["-r", fa, "-s", "16385"],
        "no references": ["-f", fa],
        "-r and -R": ["-r", fa, "-R", ok],
        "policy: -Q differs from -R": ["-R", ok, "-Q", _sketch_file(tmp_path / "q_mash.json", policy=MASH)],
        "policy: -R differs from the run": ["-R", _sketch_file(tmp_path / "r_mash.json", policy=MASH)],
        "policy: the run differs from -R": ["-R", ok, "--hash-policy", "sourmash"],
        "kmer: -Q differs from -R": ["-R", ok, "-Q", _sketch_file(tmp_path / "q_k21.json", kmer="21")],
        "kmer: -k differs from -R": ["-R", ok, "-k", "21"],
        "kmer: two sizes in one sketch": ["-R", _sketch_file(tmp_path / "r_k2.json", kmer="12 16")],
        "length: -Q differs from -R": ["-R", ok, "-Q", _sketch_file(tmp_path / "q_s8.json", length=8)],
        "length: -s differs from -R": ["-R", ok, "-s", "8"],
        "length: two -R files differ": ["-R", ok, "-R", _sketch_file(tmp_path / "r_s8.json", length=8)],
        "unreadable": ["-R", str(tmp_path / "missing.json")],
        "length: beyond the limit, nothing of that size allocated": ["-R", _sketch_file(tmp_path / "r_huge.json", length=2000000000)],
        "-g with loaded sketches only": ["-R", ok, "-g"],
    }
    for what, args in cases.items():
        r = _run(root, "dist", *args)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"rkmh dist: "), (what, r)
    r = _run(root, "dist", "-R", _sketch_file(tmp_path / "r_mash2.json", policy=MASH))
    assert b"--hash-policy " + MASH.encode() in r.stderr


# ---- the panel inputs of the GPU tests are not vacuous (on the model's output) ----
def test_panel_subset_exercises_every_count():
    """Over the pairs i < j of the three settings on the panel subset: repeats that matter (shared != shared_distinct), common values
    past the S-th union value (common != shared_distinct), pairs that share nothing and pairs that share something."""
    rows = np.concatenate([pc.unordered(pc.panel(n)["out"]) for n in ("default-k12", "mash-k16", "sourmash-k21")])
    assert int((rows[:, 0] != rows[:, 1]).sum()) >= 20
    assert int((rows[:, 2] != rows[:, 1]).sum()) >= 500
    assert int((rows[:, 0] == 0).sum()) >= 500 and int((rows[:, 0] > 0).sum()) >= 500
    z = pc.unordered(pc.panel("zika-k16")["out"])
    assert len(z) == 1770 and (z[:, 0] > 0).all() and int((z[:, 2] != z[:, 0]).sum()) >= 1000
    d = pc.panel("sourmash-k21")
    assert (d["out"][:, :, 0] == d["out"][:, :, 1]).all()                    # distinct sketches: the multiset count is the set count
    for name in pc.PANEL:                                                    # and the model agrees with itself where it must
        p = pc.panel(name)
        n = len(p["ln"])
        assert (p["out"] == p["out"].transpose(1, 0, 2)).all()
        assert (p["out"][np.arange(n), np.arange(n), 0] == p["ln"]).all()
