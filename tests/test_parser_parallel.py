"""Block-parallel FASTA/FASTQ front end (rk_parse_blocks.cpp next_block) against the kseq-grammar restatement in
oracle/oracle.py (kseq.hpp:170-208) and against the sequential scanner, on well-formed and hostile inputs.
CPU only: the parser is host code."""
import os

import zlib

import numpy as np
import pytest

from rkmh_amd import api


def _records(ss):
    out = []
    for i in range(len(ss["names"])):
        s = bytes(ss["bases"][int(ss["offsets"][i]):int(ss["offsets"][i + 1])])
        q = ss["quals"][i] if ss.get("quals") is not None else None
        out.append((ss["names"][i], s, q))
    return out


def _oracle_records(orc, data):
    recs = orc.kseq_parse_bytes(data)
    have_q = len(recs) > 0 and all(r[2] is not None for r in recs)
    return [(r[0], r[1], r[2] if have_q else None) for r in recs]


def _parse(path, threads, block_kb):
    os.environ["RKMH_PARSE_THREADS"] = str(threads)
    os.environ["RKMH_PARSE_BLOCK_KB"] = str(block_kb)
    try:
        whole = _records(api.parse_files([path]))
        rd = api.Reader(path)
        batched = []
        while True:
            b = rd.next_batch(max_records=1 << 16, max_bases=1 << 28)
            if b is None:
                break
            batched.extend(_records(b))
        rd.close()
        return whole, batched
    finally:
        del os.environ["RKMH_PARSE_THREADS"]
        del os.environ["RKMH_PARSE_BLOCK_KB"]


def _fastq(rng, n, crlf=False, at_quals=False, lens=(20, 200)):
    nl = b"\r\n" if crlf else b"\n"
    out = []
    for i in range(n):
        L = int(rng.integers(lens[0], lens[1]))
        seq = bytes(rng.choice(np.frombuffer(b"ACGTNacgt", np.uint8), L))
        q = bytearray(rng.integers(33, 127, L, dtype=np.uint8).tobytes())
        if at_quals and L and i % 3 == 0:
            q[0] = ord("@")
        if at_quals and L > 1 and i % 5 == 0:
            q[0] = ord("+")
        out.append(b"@r%d some comment" % i + nl + seq + nl + b"+" + nl + bytes(q) + nl)
    return b"".join(out)


def _fasta(rng, n, width=60):
    out = []
    for i in range(n):
        L = int(rng.integers(0, 3000))
        seq = bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), L))
        out.append(b">ref%d desc\n" % i)
        for j in range(0, L, width):
            out.append(seq[j:j + width] + b"\n")
        if i % 7 == 0:
            out.append(b"\n")
    return b"".join(out)


CASES = {
    "fastq_plain": lambda r: _fastq(r, 4000),
    "fastq_at_quals": lambda r: _fastq(r, 4000, at_quals=True),
    "fastq_crlf": lambda r: _fastq(r, 3000, crlf=True, at_quals=True),
    "fastq_no_final_newline": lambda r: _fastq(r, 3000)[:-1],
    "fastq_truncated_qual": lambda r: _fastq(r, 3000)[:-40],
    "fastq_truncated_in_header": lambda r: _fastq(r, 2000) + b"@last",
    "fastq_multiline": lambda r: _fastq(r, 1500) + b"@ml\nACGT\nACGT\n+\nIIIIIIII\n" + _fastq(r, 1500),
    "fastq_junk_between": lambda r: _fastq(r, 1500) + b"junk line\n" + _fastq(r, 1500),
    "fastq_spaces_in_seq": lambda r: _fastq(r, 1500) + b"@sp\nAC GT\n+\nIIII\n" + _fastq(r, 1500),
    "fastq_short_qual": lambda r: _fastq(r, 1500) + b"@sq\nACGTACGT\n+\nIII\n" + _fastq(r, 1500, at_quals=True),
    "fastq_long_qual": lambda r: _fastq(r, 1500) + b"@lq\nACGT\n+\nIIII@II\n" + _fastq(r, 1500),
    "fastq_empty_seq": lambda r: _fastq(r, 1000) + b"@e\n\n+\n\n" + _fastq(r, 1000),
    "fasta_multiline": lambda r: _fasta(r, 400),
    "fasta_plus_inside": lambda r: _fasta(r, 200) + b">odd\nACGT+ACGT\nACGT\n" + _fasta(r, 200),
    "fasta_gt_inside": lambda r: _fasta(r, 200) + b">odd\nACGT>x\nACGT\n" + _fasta(r, 200),
    "mixed_fasta_fastq": lambda r: _fasta(r, 150) + _fastq(r, 1500) + _fasta(r, 100),
    "leading_blank_lines": lambda r: b"\n\n" + _fastq(r, 2000),
    "leading_junk": lambda r: b"# comment\n" + _fastq(r, 2000),
    "fasta_giant_single_line_records": lambda r: b"".join(b">chr%d some description\n" % i + bytes(r.choice(np.frombuffer(b"ACGTN", np.uint8), int(r.integers(1000, 300000)))) + b"\n" for i in range(7)),
    "fasta_giant_wrapped_crlf": lambda r: _fasta(r, 40, width=70).replace(b"\n", b"\r\n"),
    "fasta_long_headers": lambda r: b"".join(b">" + b"h" * int(r.integers(1, 9000)) + b" x\n" + b"ACGT" * int(r.integers(0, 3000)) + b"\n" for _ in range(60)),
    "fasta_ends_in_header": lambda r: _fasta(r, 100) + b">last_header_without_newline",
    "fasta_lone_gt": lambda r: _fasta(r, 100) + b">\n" + _fasta(r, 20),
    "fasta_no_final_newline": lambda r: _fasta(r, 120)[:-1],
    "fasta_plus_in_giant_record": lambda r: b">a\n" + b"ACGT" * 40000 + b"+" + b"ACGT" * 40000 + b"\n>b\nAC\n",
    "fasta_junk_first": lambda r: b"junk\n" + _fasta(r, 100),
    "empty": lambda r: b"",
    "only_newlines": lambda r: b"\n\n\n",
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_parallel_parser_matches_kseq_grammar(orc, tmp_path, name):
    rng = np.random.default_rng(zlib.crc32(name.encode()))   # a STABLE seed: hash(str) is randomised per process
    data = CASES[name](rng)
    path = str(tmp_path / (name + ".txt"))
    with open(path, "wb") as f:
        f.write(data)
    want = _oracle_records(orc, data)
    for threads, block_kb in ((1, 64), (4, 64), (8, 200), (8, 1 << 20)):
        whole, batched = _parse(path, threads, block_kb)
        assert whole == want, (name, threads, block_kb, "parse_files")
        # quality strings are all-or-nothing per batch (rk_seqset.quals), so batches compare names + bases
        assert [r[:2] for r in batched] == [r[:2] for r in want], (name, threads, block_kb, "reader")


def test_parallel_parser_big_default_settings(orc, tmp_path):
    """Default knobs (8 threads, large blocks) on a file big enough to split across every worker."""
    rng = np.random.default_rng(5)
    data = _fastq(rng, 60000, at_quals=True, lens=(100, 200))
    path = str(tmp_path / "big.fq")
    with open(path, "wb") as f:
        f.write(data)
    got = _records(api.parse_files([path]))
    assert got == _oracle_records(orc, data)


def test_parallel_parser_fuzz(orc, tmp_path):
    """Well-formed FASTQ/FASTA files with a few random structural mutations (inserted/deleted/overwritten '@', '>', '+',
    newlines, CRLF, blanks, arbitrary bytes, truncation), tiny blocks so that cuts and fallbacks land everywhere;
    RKMH_TEST_FUZZ=12000 for a soak (12 400 inputs x 3 settings passed when this was written)."""
    rng = np.random.default_rng(2024)
    tokens = [b"@", b">", b"+", b"\n", b"\r\n", b" ", b"\t", b"\n\n"]

    def mutate(data, k):
        b = bytearray(data)
        for _ in range(k):
            if not b:
                break
            op, pos = int(rng.integers(0, 4)), int(rng.integers(0, len(b)))
            tok = tokens[int(rng.integers(0, len(tokens)))] if rng.random() < 0.7 else bytes([int(rng.integers(0, 256))])
            if op == 0:
                b[pos:pos] = tok
            elif op == 1:
                del b[pos:pos + int(rng.integers(1, 8))]
            elif op == 2:
                b[pos:pos + len(tok)] = tok
            else:
                b = b[:pos]
        return bytes(b)

    path = str(tmp_path / "fuzz.txt")
    for it in range(int(os.environ.get("RKMH_TEST_FUZZ", "120"))):
        base = _fastq(rng, int(rng.integers(50, 500)), lens=(0, 120), at_quals=bool(it % 2)) if rng.random() < 0.6 \
            else _fasta(rng, int(rng.integers(20, 150)))
        data = mutate(base, int(rng.integers(0, 6)))
        with open(path, "wb") as f:
            f.write(data)
        want = [r[:2] for r in _oracle_records(orc, data)]
        for threads, block_kb in ((4, 4), (8, 16), (3, 64)):
            whole, _ = _parse(path, threads, block_kb)
            assert [r[:2] for r in whole] == want, (it, threads, block_kb)


@pytest.mark.parametrize("seed", [23, 27, 57])
def test_reader_survives_more_workers_in_a_later_block(orc, tmp_path, seed):
    """Regression: a FASTA of a few giant single-line records read in 200 KB blocks by 8 workers uses more workers for a later
    block than for an earlier one; std::vector<Piece>::resize then relocated live pieces through a shallow copy and the next
    reserve() double-freed (a rare abort of the parser tests, whose inputs were seeded from the per-process hash() of the case
    name; found with AddressSanitizer).  These three inputs aborted every time before the fix."""
    rng = np.random.default_rng(seed)
    data = CASES["fasta_giant_single_line_records"](rng)
    path = str(tmp_path / "giant.fa")
    with open(path, "wb") as f:
        f.write(data)
    want = _oracle_records(orc, data)
    for threads, block_kb in ((8, 200), (4, 64), (8, 64)):
        whole, batched = _parse(path, threads, block_kb)
        assert whole == want and [r[:2] for r in batched] == [r[:2] for r in want], (threads, block_kb)
