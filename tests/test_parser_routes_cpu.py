"""The routes of the host read parser that tests/test_parser_parallel.py does not reach (it writes plain regular files, so the
mapped-file branch alone): gzip input -- the pipe-block branch of the block front end (rk_parse_blocks.cpp) fed by the inflater
thread of the gzip source (rk_parse.cpp), and the sequential scanner over gzread -- the byte-range reader that the multi-rank
command line reads through (rk_reader_open_range, rk_reader_strict, api.parse_file_range), small exact batches and readers that
drop the quality strings.  CPU only: the parser is host code."""
import gzip
import os
import zlib

import numpy as np
import pytest

from rkmh_amd import api
from test_parser_parallel import CASES, _fasta, _fastq, _oracle_records, _records

# files of exactly four lines per record: the only text on which a byte range has exact boundaries
FOUR_LINE = ("fastq_plain", "fastq_at_quals", "fastq_crlf", "fastq_no_final_newline", "fastq_empty_seq")


def _data(name):
    return CASES[name](np.random.default_rng(zlib.crc32(name.encode())))   # the seed test_parser_parallel uses


def _write(tmp_path, fname, data):
    path = str(tmp_path / fname)
    with open(path, "wb") as f:
        f.write(data)
    return path


def _with_env(env, fn):
    """fn() with the parser's knobs set, and deleted again afterwards (as test_parser_parallel._parse does)"""
    for k, v in env.items():
        os.environ[k] = str(v)
    try:
        return fn()
    finally:
        for k in env:
            del os.environ[k]


def _knobs(threads, block_kb, **more):
    return dict(RKMH_PARSE_THREADS=threads, RKMH_PARSE_BLOCK_KB=block_kb, **more)


def _read_all(path, max_records=1 << 16, max_bases=1 << 28, keep_quals=True):
    rd = api.Reader(path, keep_quals=keep_quals)
    batches = []
    while True:
        b = rd.next_batch(max_records=max_records, max_bases=max_bases)
        if b is None:
            break
        batches.append(b)
    rd.close()
    return batches


@pytest.mark.parametrize("name", sorted(CASES))
def test_gzip_route_matches_kseq_grammar(orc, tmp_path, name):
    """RKMH_GZ_BLOCKS=0: the sequential scanner reads through gzread; =2: the inflater thread and the block front end's pipe branch
    (blocks topped up from the thread's queue, the unfinished tail carried to the next block), even for files this small."""
    data = _data(name)
    path = _write(tmp_path, name + ".txt.gz", gzip.compress(data, 1))
    want = _oracle_records(orc, data)
    for gz_blocks in (0, 2):
        for threads, block_kb in ((4, 4), (8, 200)):
            env = _knobs(threads, block_kb, RKMH_GZ_BLOCKS=gz_blocks)
            whole = _with_env(env, lambda: _records(api.parse_files([path])))
            batched = _with_env(env, lambda: [r for b in _read_all(path) for r in _records(b)])
            assert whole == want, (name, gz_blocks, threads, block_kb, "parse_files")
            # quality strings are all-or-nothing per batch (rk_seqset.quals), so batches compare names + bases
            assert [r[:2] for r in batched] == [r[:2] for r in want], (name, gz_blocks, threads, block_kb, "reader")


@pytest.mark.parametrize("name", FOUR_LINE)
def test_byte_ranges_partition_the_file(tmp_path, name):
    """Four ranges [c[i], c[i+1]) that cover the file, wherever the bounds fall, hold every record exactly once and in order."""
    data = _data(name)
    size = len(data)
    path = _write(tmp_path, name + ".fq", data)
    rng = np.random.default_rng(zlib.crc32(name.encode()) ^ 0x52616e67)
    draws = []
    for d in range(40):
        cuts = sorted(int(x) for x in rng.integers(0, size + 1, 3))
        if d == 7:
            cuts[1] = cuts[0]                                  # an empty range
        last = size + int(rng.integers(1, 1 << 20)) if d % 2 else size   # past the end of the file in half the draws
        draws.append([0] + cuts + [last])
    for threads, block_kb in ((4, 4), (8, 64)):
        def run():
            whole = _records(api.parse_files([path]))
            assert len(whole) > 0
            for c in draws:
                got = []
                for lo, hi in zip(c, c[1:]):
                    part = api.parse_file_range(path, lo, hi)
                    assert part["strict"] is True, (name, threads, block_kb, c, lo, hi)
                    got.extend(_records(part))
                assert got == whole, (name, threads, block_kb, c)
        _with_env(_knobs(threads, block_kb), run)


def test_byte_ranges_non_strict_and_refusals(tmp_path):
    """A record of more than four lines makes the reader fall back to the sequential scanner: strict is False and the caller must
    parse the whole file.  FASTA and gzip cannot be split by byte ranges at all."""
    data = _data("fastq_multiline")
    path = _write(tmp_path, "multiline.fq", data)
    part = _with_env(_knobs(4, 64), lambda: api.parse_file_range(path, 0, len(data)))
    assert part["strict"] is False
    fa = _write(tmp_path, "refs.fa", _fasta(np.random.default_rng(3), 50))
    with pytest.raises(api.RkmhError):
        api.parse_file_range(fa, 0, 1000)
    gz = _write(tmp_path, "reads.fq.gz", gzip.compress(_fastq(np.random.default_rng(4), 200), 1))
    with pytest.raises(api.RkmhError):
        api.parse_file_range(gz, 0, 1000)


def test_small_exact_batches(orc, tmp_path):
    """max_records below 65536 hands the file to the sequential scanner, whose limits are exact: 7 records per batch."""
    data = _data("fastq_at_quals")
    path = _write(tmp_path, "small.fq", data)
    want = _oracle_records(orc, data)
    for threads, block_kb in ((4, 4), (8, 64)):
        batches = _with_env(_knobs(threads, block_kb), lambda: _read_all(path, max_records=7, max_bases=0))
        assert all(b["nseq"] == 7 for b in batches[:-1]) and 1 <= batches[-1]["nseq"] <= 7, (threads, block_kb)
        assert [r for b in batches for r in _records(b)] == want, (threads, block_kb)


def test_reader_without_quals(orc, tmp_path):
    data = _data("fastq_at_quals")
    path = _write(tmp_path, "noquals.fq", data)
    gz = _write(tmp_path, "noquals.fq.gz", gzip.compress(data, 1))
    want = [r[:2] for r in _oracle_records(orc, data)]
    for p, env in ((path, _knobs(4, 4)), (path, _knobs(8, 64)), (gz, _knobs(4, 4, RKMH_GZ_BLOCKS=2)), (gz, _knobs(4, 4, RKMH_GZ_BLOCKS=0))):
        batches = _with_env(env, lambda: _read_all(p, keep_quals=False))
        assert len(batches) > 0 and all(b["quals"] is None for b in batches), env
        assert [r[:2] for b in batches for r in _records(b)] == want, env
