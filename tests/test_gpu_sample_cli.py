"""`rkmh sketch --scaled 10 --abund -g` and `rkmh gather --abund` with the sample sketch built on the device (rkmh_sample.cpp): for a
2 000-read file as plain FASTQ, BGZF, gzip and multi-line FASTA, standard output equals the RKMH_SAMPLE_DEVICE=0 run (the route that
parses the file whole) byte for byte, and tests/abund_model.py.  Blocks and BGZF jobs are cut at toy size, so every file is many of
them; one plain file turns irregular in its second block and is handed to the scanner mid-file."""
import functools
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import abund_model as am
import scaled_cases as sc
import scaled_model as scm
import sourmash_model as sm

pytestmark = pytest.mark.gpu

K, SCALED, NREADS = 16, 10, 2000
FORMS = ["plain", "bgzf", "gzip", "fasta"]


@functools.lru_cache(maxsize=None)
def _reads():
    from rkmh_amd import api, synth
    refs = api.parse_files([os.path.join(sc.DATA, "zika.refs.fa.gz")])
    qb, qo = synth.generate_reads_fast(refs["bases"], refs["offsets"], 0, NREADS, read_len=150, threads=4)
    return tuple(bytes(qb[int(qo[i]):int(qo[i + 1])]) for i in range(NREADS))


@functools.lru_cache(maxsize=None)
def _want():
    """the sample sketch of the reads at scaled 10: (values, abund)"""
    mh = scm.max_hash(SCALED)
    return am.merge([am.sketch(r, [K], sm.DEFAULT, mh) for r in _reads()], mh)


def _fastq(reads, cr_at=None):
    return b"".join(b"@r%d%s\n%s\n+\n%s\n" % (i, b"\r" if i == cr_at else b"", r, b"I" * len(r)) for i, r in enumerate(reads))


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


def _run(root, args, device_route, timing=False):
    env = dict(os.environ)
    env.pop("RKMH_POLICY", None)
    env.update(RKMH_SAMPLE_DEVICE="1" if device_route else "0", RKMH_RAW_BLOCK_KB="64", RKMH_BGZF_JOB_KB="64")
    if timing:
        env["RKMH_TIMING"] = "1"
    r = subprocess.run([os.path.join(root, "bin", "rkmh")] + list(args), capture_output=True, env=env)
    assert r.returncode == 0, (args, r.stderr[-600:])
    return r.stdout, r.stderr.decode()


def _check_sketch(out, path):
    doc = json.loads(out)
    v, a = _want()
    assert len(doc) == 1 and doc[0]["name"] == path and doc[0]["seqLen"] == NREADS * 150 and doc[0]["scaled"] == SCALED
    assert doc[0]["sketches"]["hashes"] == v.tolist() and doc[0]["sketches"]["abundances"] == a.tolist()


def _gather_want(path):
    names = [n.decode() for n in sc.panel("zika-k16")["names"]]
    return am.gather_text([path], [_want()], names, sc.sketches("zika-k16", SCALED)).encode()


@pytest.mark.parametrize("form", FORMS)
def test_sketch_and_gather_equal_the_old_route(root, tmp_path, form):
    path = _write(tmp_path, form)
    refs = os.path.join(sc.DATA, "zika.refs.fa.gz")
    sketch = ["sketch", "--scaled", str(SCALED), "--abund", "-g", "-k", str(K), "-f", path]
    gather = ["gather", "--abund", "--scaled", str(SCALED), "-k", str(K), "-r", refs, "-f", path]
    new, err = _run(root, sketch, True, timing=True)
    old, _ = _run(root, sketch, False)
    assert new == old
    _check_sketch(new, path)
    route = {"plain": "plain route", "bgzf": "bgzf route", "gzip": "reader route", "fasta": "reader route"}[form]
    assert route in err and "scanner takes over" not in err, err[-600:]
    if form in ("plain", "bgzf"):
        blocks = int(err.split(route + ", ")[1].split(" blocks")[0])
        assert blocks >= 5, err[-600:]                                     # cut at toy size: the file is many blocks
    new, _ = _run(root, gather, True)
    old, _ = _run(root, gather, False)
    assert new == old == _gather_want(path) and len(new.split(b"\n")) > 3


def test_hand_over_in_the_second_block(root, tmp_path):
    """a carriage return behind a record name some 100 KB into the file: the device refuses that block, which has added nothing; the
    scanner takes the file over from the block's first byte and the sketch is the same"""
    reads = _reads()
    text = _fastq(reads, cr_at=300)
    assert 65536 < text.index(b"\r") < 2 * 65536 - 4096
    p = tmp_path / "cr.fq"
    p.write_bytes(text)
    sketch = ["sketch", "--scaled", str(SCALED), "--abund", "-g", "-k", str(K), "-f", str(p)]
    new, err = _run(root, sketch, True, timing=True)
    old, _ = _run(root, sketch, False)
    assert new == old
    _check_sketch(new, str(p))
    assert "scanner takes over" in err, err[-600:]
    at = int(err.split("stops at byte ")[1].split(" ")[0])
    assert 0 < at <= text.index(b"\r") and text[at:at + 2] == b"@r"          # mid-file, at a record start
