"""`rkmh sketch -g -s 500` and `rkmh dist -g -s 500` with the file's sketch built on the device as a bottom sample (rkmh_sample.cpp,
rkmh_sketches.cpp), and --min-copies: for a 2 000-read file as plain FASTQ, BGZF, gzip and multi-line FASTA, standard output equals
the RKMH_SAMPLE_DEVICE=0 run (the route that parses the file whole and unites per-read sketches on the host) byte for byte, and
tests/bottom_model.py.  Blocks and BGZF jobs are cut at toy size, so every file is many of them."""
import functools
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import bottom_model as bm
import pairs_model as pm
import scaled_cases as sc
import sourmash_model as sm

pytestmark = pytest.mark.gpu

K, S, NREADS = 16, 500, 2000
FORMS = ["plain", "bgzf", "gzip", "fasta"]
REFS = os.path.join(sc.DATA, "zika.refs.fa.gz")


@functools.lru_cache(maxsize=None)
def _ref_seqs():
    from rkmh_amd import api
    refs = api.parse_files([REFS])
    b, o = refs["bases"], refs["offsets"]
    return tuple(bytes(b[int(o[i]):int(o[i + 1])]) for i in range(len(o) - 1))


@functools.lru_cache(maxsize=None)
def _reads():
    from rkmh_amd import api, synth
    refs = api.parse_files([REFS])
    qb, qo = synth.generate_reads_fast(refs["bases"], refs["offsets"], 0, NREADS, read_len=150, threads=4)
    return tuple(bytes(qb[int(qo[i]):int(qo[i + 1])]) for i in range(NREADS))


@functools.lru_cache(maxsize=None)
def _want(m, refs=False):
    """the sketch of the reads (or of the reference file as one sketch) under the default policy: a list of values"""
    return tuple(bm.direct(_ref_seqs() if refs else _reads(), (K,), sm.DEFAULT, S, m, False))


def _fastq(reads):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))


def _write(tmp_path, form):
    from rkmh_amd import synth
    reads = _reads()
    if form == "fasta":
        p = tmp_path / "reads.fa"
        p.write_bytes(b"".join(b">r%d\n" % i + b"".join(r[j:j + 60] + b"\n" for j in range(0, len(r), 60)) for i, r in enumerate(reads)))
        return str(p)
    text = _fastq(reads)
    p = tmp_path / {"plain": "reads.fq", "bgzf": "reads.bgzf.fq.gz", "gzip": "reads.fq.gz"}[form]
    p.write_bytes(text if form == "plain" else gzip.compress(text, 1) if form == "gzip" else bytes(synth.bgzf_compress(text, level=1, block=20000)))
    return str(p)


def _env(device_route, timing=False):
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    env.update(RKMH_SAMPLE_DEVICE="1" if device_route else "0", RKMH_RAW_BLOCK_KB="64", RKMH_BGZF_JOB_KB="64")
    if timing:
        env["RKMH_TIMING"] = "1"
    return env


def _run(root, args, device_route, timing=False):
    r = subprocess.run([os.path.join(root, "bin", "rkmh")] + list(args), capture_output=True, env=_env(device_route, timing))
    assert r.returncode == 0, (args, r.stderr[-600:])
    return r.stdout, r.stderr.decode()


def _check_sketch(out, path, m):
    doc = json.loads(out)
    want = list(_want(m))
    assert len(doc) == 1 and doc[0]["name"] == path and doc[0]["seqLen"] == NREADS * 150 and "scaled" not in doc[0]
    assert doc[0]["sketches"]["hashes"] == want and doc[0]["sketches"]["length"] == S and len(want) == S
    assert doc[0].get("minCopies", 1) == m and ("minCopies" in doc[0]) == (m > 1)
    if m > 1:
        assert out.index(b'"kmer"') < out.index(b'"minCopies":%d,' % m) < out.index(b'"name"')       # its alphabetical place


def _dist_line(path, m):
    a, b = np.asarray(_want(m), np.uint64), np.asarray(_want(m, refs=True), np.uint64)
    shared, _, common, denom = pm.pair_counts(a, b, S)
    _, d = pm.mash_distance(common, denom, K)
    return ("%s\t%s\t%s\t%d/%d\t%d\n" % (REFS, path, pm.distance_text(d), common, denom, shared)).encode()


@pytest.mark.parametrize("form", FORMS)
def test_sketch_equals_the_old_route_and_the_model(root, tmp_path, form):
    path = _write(tmp_path, form)
    sketch = ["sketch", "-g", "-s", str(S), "-k", str(K), "-f", path]
    new, err = _run(root, sketch, True, timing=True)
    old, _ = _run(root, sketch, False)
    assert new == old
    _check_sketch(new, path, 1)
    route = {"plain": "plain route", "bgzf": "bgzf route", "gzip": "reader route", "fasta": "reader route"}[form]
    assert route in err and "scanner takes over" not in err, err[-600:]
    if form in ("plain", "bgzf"):
        assert int(err.split(route + ", ")[1].split(" blocks")[0]) >= 5, err[-600:]      # cut at toy size: the file is many blocks
    line = [x for x in err.split("\n") if "bottom sample" in x]
    assert len(line) == 1 and "sketch size %d, min copies 1" % S in line[0] and int(line[0].split(", ")[-1].split(" cuts")[0]) >= 1, err[-600:]
    two, _ = _run(root, sketch + ["--min-copies", "2"], True)
    _check_sketch(two, path, 2)
    assert _want(2) != _want(1)


@pytest.mark.parametrize("form", FORMS)
def test_dist_equals_the_old_route_and_the_model(root, tmp_path, form):
    path = _write(tmp_path, form)
    dist = ["dist", "-g", "-s", str(S), "-k", str(K), "-r", REFS, "-f", path]
    new, _ = _run(root, dist, True)
    old, _ = _run(root, dist, False)
    assert new == old == _dist_line(path, 1)
    # --min-copies is for the read set: the reference file beside it is sketched as it is
    two, _ = _run(root, dist + ["--min-copies", "2"], True)
    a, b = np.asarray(_want(2), np.uint64), np.asarray(_want(1, refs=True), np.uint64)
    shared, _, common, denom = pm.pair_counts(a, b, S)
    assert two == ("%s\t%s\t%s\t%d/%d\t%d\n" % (REFS, path, pm.distance_text(pm.mash_distance(common, denom, K)[1]), common, denom, shared)).encode()


def test_a_file_sketched_with_min_copies_loads(root, tmp_path):
    path = _write(tmp_path, "plain")
    q, r = str(tmp_path / "reads.json"), str(tmp_path / "refs.json")
    _run(root, ["sketch", "-g", "-s", str(S), "-k", str(K), "-f", path, "--min-copies", "2", "-o", q], True)
    _run(root, ["sketch", "-g", "-s", str(S), "-k", str(K), "-f", REFS, "-o", r], True)
    assert b'"minCopies":2' in open(q, "rb").read() and b"minCopies" not in open(r, "rb").read()
    out, _ = _run(root, ["dist", "-R", r, "-Q", q], True)
    a, b = np.asarray(_want(2), np.uint64), np.asarray(_want(1, refs=True), np.uint64)
    shared, _, common, denom = pm.pair_counts(a, b, S)
    assert out == ("%s\t%s\t%s\t%d/%d\t%d\n" % (REFS, path, pm.distance_text(pm.mash_distance(common, denom, K)[1]), common, denom, shared)).encode()


def test_min_copies_refusals(root, tmp_path):
    path = _write(tmp_path, "plain")
    rkmh = os.path.join(root, "bin", "rkmh")
    cases = [
        (["sketch", "-s", str(S), "-f", path, "--min-copies", "2"], True, "needs -g"),
        (["sketch", "-g", "--scaled", "10", "-f", path, "--min-copies", "2"], True, "scaled"),
        (["sketch", "-g", "-s", str(S), "-f", path, "--min-copies", "2"], False, "RKMH_SAMPLE_DEVICE=0"),
        (["dist", "-s", str(S), "-r", REFS, "-f", path, "--min-copies", "2"], True, "needs -g"),
        (["dist", "-g", "--scaled", "10", "-r", REFS, "-f", path, "--min-copies", "2"], True, "scaled"),
        (["dist", "-g", "-s", str(S), "-r", REFS, "-f", path, "--min-copies", "2"], False, "RKMH_SAMPLE_DEVICE=0"),
        (["sketch", "-g", "-s", str(S), "-f", path, "--min-copies", "0"], True, "--min-copies takes a number"),
        (["sketch", "-g", "-s", str(S), "-f", path, "--min-copies", "4294967296"], True, "--min-copies takes a number"),
    ]
    for args, device_route, word in cases:
        r = subprocess.run([rkmh] + args + ["-k", str(K)], capture_output=True, env=_env(device_route))
        err = r.stderr.decode()
        assert r.returncode != 0 and r.stdout == b"" and word in err and err.count("\n") == 1 and err.startswith("rkmh " + args[0] + ": --min-copies"), (args, err)
    # --min-copies 1 is the default and asks for nothing
    out, _ = _run(root, ["sketch", "-s", str(S), "-k", str(K), "-f", path, "--min-copies", "1"], False)
    assert b"minCopies" not in out
