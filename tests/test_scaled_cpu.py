"""Scaled sketches without a GPU: the model (tests/scaled_model.py) against the hand-checked vectors, the host-only calls
(rk_scaled_max_hash, rk_merge_scaled, rk_scaled_distance) against the model, what the shared inputs of tests/test_gpu_scaled.py
exercise (shown on the model's output), the help texts, and everything `rkmh dist --scaled` and the other readers of sketch files
refuse before a context exists."""
import json
import os
import subprocess

import numpy as np
import pytest

import scaled_cases as sc
import scaled_model as scm
from rkmh_amd import api


# ---- the model against the vectors ----
def test_there_are_enough_vectors():
    names = [v["name"] for v in sc.kat()]
    assert len(names) >= 20 and len(set(names)) == len(names)


@pytest.mark.parametrize("i", range(len(sc.kat())))
def test_model_matches_hand_checked_vectors(i):
    v = sc.kat()[i]
    assert scm.shared(v["a"], v["b"]) == v["want"] and scm.shared(v["b"], v["a"]) == v["want"], v["name"]
    assert scm.shared(v["a"], v["a"]) == len(v["a"])


# ---- host-only calls ----
def test_scaled_max_hash():
    full = (1 << 64) - 1
    for s in (1, 2, 3, 1000, 1 << 32, full):
        assert api.scaled_max_hash(s) == full // s == scm.max_hash(s), s
    assert api.scaled_max_hash(1) == full and api.scaled_max_hash(full) == 1 and api.scaled_max_hash(1 << 32) == (1 << 32) - 1
    with pytest.raises(api.RkmhError) as e:
        api.scaled_max_hash(0)
    assert e.value.code == -1


@pytest.mark.parametrize("parts", [1, 2, 17])
def test_merge_scaled_against_the_model(parts):
    rng = np.random.default_rng(parts)
    pl = sc.pool(rng, 3000)
    sets = sc.random_sets(rng, parts, pl, lengths=[0, 1, 65, 1000])
    sets[0] = np.sort(rng.choice(pl, size=1500, replace=False))               # one part is never empty
    v, off = scm.csr(sets)
    for mh in (scm.FULL, int(np.sort(pl)[len(pl) // 3]), int(np.sort(pl)[len(pl) // 3]) - 1, 1):
        want = scm.merge(sets, mh)
        got = api.merge_scaled(v, off, mh)
        assert got.dtype == np.uint64 and got.tolist() == want.tolist(), (parts, mh)
    assert len(scm.merge(sets)) > 0 and len(scm.merge(sets, 1)) == 0
    if parts > 1:
        assert len(scm.merge(sets)) < sum(len(s) for s in sets)             # the parts overlap: the union drops repeats
    # unsorted parts with repeats and zeros are a union all the same
    messy = np.concatenate([v[::-1], v[:10], np.zeros(3, dtype=np.uint64)])
    assert api.merge_scaled(messy, np.array([0, len(messy)], dtype=np.uint64)).tolist() == scm.merge(sets).tolist()


def test_merge_scaled_is_downsampling():
    rng = np.random.default_rng(3)
    s = np.sort(sc.pool(rng, 5000))
    for scaled in (1, 2, 10, 1000):
        got = api.merge_scaled(s, np.array([0, len(s)], dtype=np.uint64), scm.max_hash(scaled))
        assert got.tolist() == scm.downsample(s, scaled).tolist() == s[:len(got)].tolist()        # a prefix
    assert 0 < len(scm.downsample(s, 10)) < len(scm.downsample(s, 2)) < len(s)


def test_merge_scaled_refusals():
    lib = api.load_library()
    v = np.arange(1, 9, dtype=np.uint64)
    with pytest.raises(api.RkmhError) as e:
        api.merge_scaled(v, np.array([0, 5, 3], dtype=np.uint64))
    assert e.value.code == -1
    with pytest.raises(ValueError):
        api.merge_scaled(v, np.array([0, 9], dtype=np.uint64))
    assert lib.rk_merge_scaled(None, None, 1, 5, None, None) == -1
    assert api.merge_scaled(v, np.array([0], dtype=np.uint64)).tolist() == []       # no sketches: the empty union


def test_scaled_distance():
    for sh, la, lb, k in ((0, 0, 0, 21), (0, 5, 0, 21), (0, 5, 9, 21), (5, 5, 5, 21), (3, 5, 9, 16), (1, 1000, 1000, 12), (1, 100000, 100000, 1),
                          (700, 800, 829, 21), (2 ** 31, 2 ** 32, 2 ** 33, 31)):
        j, d = api.scaled_distance(sh, la, lb, k)
        wj, wd = scm.distance(sh, la, lb, k)
        assert j == pytest.approx(wj, rel=1e-15, abs=0) and d == pytest.approx(wd, rel=1e-14, abs=0), (sh, la, lb, k)
        assert 0.0 <= d <= 1.0 and str(d) != "-0.0"
    assert api.scaled_distance(0, 0, 0, 21) == (0.0, 1.0) and api.scaled_distance(4, 4, 4, 21) == (1.0, 0.0)
    assert api.scaled_distance(1, 100000, 100000, 1)[1] == 1.0                # clamped
    for bad in ((-1, 5, 5, 21), (2, -1, 5, 21), (2, 5, -1, 21), (6, 5, 9, 21), (6, 9, 5, 21), (1, 5, 5, 0)):
        with pytest.raises(api.RkmhError) as e:
            api.scaled_distance(*bad)
        assert e.value.code == -1


def test_compare_scaled_refuses_offsets_past_the_values():
    """checked in the binding, before a context is needed"""
    class NoContext(api.Context):
        def __init__(self):
            pass

        def __del__(self):
            pass
    with pytest.raises(ValueError):
        NoContext().compare_scaled(np.arange(1, 5, dtype=np.uint64), np.array([0, 2, 9], dtype=np.uint64))


# ---- what the shared inputs exercise (the model's output only) ----
def test_floors_sourmash_k21():
    sh = sc.unordered(sc.panel_shared("sourmash-k21", 10))
    print("sourmash k=21 scaled 10: shared > 0:", int((sh > 0).sum()), " shared = 0:", int((sh == 0).sum()),
          " lengths:", min(map(len, sc.sketches("sourmash-k21", 10))), max(map(len, sc.sketches("sourmash-k21", 10))))
    assert (sh > 0).sum() >= 150 and (sh == 0).sum() >= 500
    p = sc.panel("sourmash-k21")
    removed = p["nonzero"] - sum(len(f) for f in p["full"])
    print("sourmash k=21 scaled 1: repeats removed:", removed)
    assert removed >= 200


def test_floors_default_k12():
    sh = sc.unordered(sc.panel_shared("default-k12", 100))
    print("default k=12 scaled 100: shared > 0:", int((sh > 0).sum()), " shared = 0:", int((sh == 0).sum()))
    assert (sh > 0).sum() >= 450 and (sh == 0).sum() >= 150


def test_floors_zika_k16():
    sks = sc.sketches("zika-k16", 100)
    sh = sc.unordered(sc.panel_shared("zika-k16", 100))
    lens = [len(s) for s in sks]
    print("default k=16 zika scaled 100: pairs:", len(sh), " smallest shared:", int(sh.min()), " lengths:", min(lens), max(lens))
    assert len(sks) == 60 and len(sh) == 1770 and (sh > 0).all()
    assert 167 <= min(lens) and max(lens) <= 219


# ---- the commands, as far as they go without a GPU ----
def _run(root, *args):
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    return subprocess.run([os.path.join(root, "bin", "rkmh")] + list(args), capture_output=True, env=env)


DEFAULT_POLICY = "fold=swap32,windows=len-k,zero=count,mask=lt,freqmax=incl,seed=42"


def _sketch_file(path, scaled=None, hashes=(3, 9, 20), n=2, length=None, max_hash=None, per_object_scaled=None):
    doc = []
    for i in range(n):
        h = [int(x) for x in hashes]
        d = {"alphabet": "ATGC", "canonical": "true", "hashBits": 64, "hashPolicy": DEFAULT_POLICY, "hashSeed": 42, "hashType": "MurmurHash3_x64_128",
             "kmer": "16", "name": "s%d" % i, "preserveCase": "false", "seqLen": 100,
             "sketches": {"comment": "", "hashes": h, "length": len(h) if length is None else length, "name": "s%d" % i}}
        s = per_object_scaled[i] if per_object_scaled else scaled
        if s:
            d["scaled"] = s
            d["maxHash"] = scm.max_hash(s) if max_hash is None else max_hash
        doc.append(d)
    path.write_text(json.dumps(doc, separators=(",", ":"), sort_keys=True))
    return str(path)


def test_help_texts_mention_scaled(root):
    for cmd in ("dist", "sketch"):
        r = _run(root, cmd)
        assert r.returncode == 1 and r.stdout == b"" and b"--scaled" in r.stderr, cmd
    assert b"--scaled" in _run(root).stderr


def _refused(r, *words):
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"rkmh dist: "), r.stderr[-300:]
    for w in words:
        assert w.encode() in r.stderr, (w, r.stderr[-300:])


def test_dist_scaled_refusals(root, tmp_path):
    fa = tmp_path / "x.fa"
    fa.write_text(">x\nACGTACGTACGTACGTACGTACGT\n")
    fa = str(fa)
    sc10 = _sketch_file(tmp_path / "sc10.json", scaled=10)
    sc100 = _sketch_file(tmp_path / "sc100.json", scaled=100)
    bottom = _sketch_file(tmp_path / "bottom.json", length=4)
    _refused(_run(root, "dist", "--scaled", "0", "-r", fa), "--scaled")
    _refused(_run(root, "dist", "--scaled", "ten", "-r", fa), "--scaled")
    _refused(_run(root, "dist", "--scaled", "10x", "-r", fa), "--scaled")
    _refused(_run(root, "dist", "--scaled", "-5", "-r", fa), "--scaled")
    _refused(_run(root, "dist", "--scaled", "10", "-s", "100", "-r", fa), "--scaled", "-s")
    _refused(_run(root, "dist", "-R", sc10, "-Q", bottom), "bottom")                    # scaled and bottom-S files in one run
    _refused(_run(root, "dist", "-R", bottom, "-Q", sc10), "bottom")
    _refused(_run(root, "dist", "--scaled", "10", "-R", bottom), "bottom")
    _refused(_run(root, "dist", "-R", sc10, "-s", "4"), "-s")                           # a scaled file next to -s
    _refused(_run(root, "dist", "--scaled", "10", "-R", sc100), "scaled = 100")         # cannot be made finer
    _refused(_run(root, "dist", "--scaled", "50", "-R", sc10, "-Q", sc100), "scaled = 100")
    mixed = _sketch_file(tmp_path / "mixed.json", per_object_scaled=[10, 100])
    _refused(_run(root, "dist", "-R", mixed), "disagree in scaled")
    half = _sketch_file(tmp_path / "half.json", per_object_scaled=[10, 0])
    _refused(_run(root, "dist", "-R", half), "disagree in scaled")
    for name, hashes in (("unsorted", (9, 3, 20)), ("repeat", (3, 9, 9)), ("zero", (0, 3, 9))):
        _refused(_run(root, "dist", "-R", _sketch_file(tmp_path / (name + ".json"), scaled=10, hashes=hashes)), "ascending")
    above = _sketch_file(tmp_path / "above.json", scaled=10, hashes=(3, 9, scm.max_hash(10) + 1))
    _refused(_run(root, "dist", "-R", above), "maxHash")
    at = _sketch_file(tmp_path / "wrongmax.json", scaled=10, max_hash=12345)
    _refused(_run(root, "dist", "-R", at), "maxHash")


def test_other_readers_refuse_scaled_files(root, tmp_path, data_dir):
    sc10 = _sketch_file(tmp_path / "sc10.json", scaled=10)
    r = _run(root, "stream", "-R", sc10, "-f", os.path.join(data_dir, "z1.fq.gz"), "-k", "16")
    assert r.returncode == 1 and r.stdout == b"" and b"scaled" in r.stderr and b"rkmh dist" in r.stderr, r.stderr[-300:]


def test_sketch_scaled_refusals(root, tmp_path):
    fa = tmp_path / "x.fa"
    fa.write_text(">x\nACGTACGTACGTACGTACGTACGT\n")
    for args in (("--scaled", "0"), ("--scaled", "x"), ("--scaled", "10", "-s", "5"), ("--scaled", "10", "--kmer-cache", str(tmp_path / "c.rkkc"))):
        r = _run(root, "sketch", "-f", str(fa), "-k", "16", *args)
        assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"rkmh sketch: "), (args, r.stderr[-300:])
