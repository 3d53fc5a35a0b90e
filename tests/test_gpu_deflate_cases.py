"""The device inflater (rk_inflate.hip, rk_gunzip.hip) on the catalogue of tests/deflate_cases.py: DEFLATE streams written bit by bit,
with the shapes that zlib's encoder never produces (tests/test_gpu_inflate.py and tests/test_gpu_gunzip.py feed it zlib's output
only).  BGZF form: for jobs of one member, a few members and the whole file rk_fastq_slot_load_bgzf returns the status the case's
expectation states, and for status 0 the slot's text, length and offset equal the host route's.  Single-stream form: every stretch
through a device-text slot, with chunks of 1 KB and 32 KB.  FASTA cases through the reference loader, a command-line run over
several cases, and the refused members: status 1, never text.  No case is skipped; "the device handed it over" passes only where
the expectation says so."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import deflate_cases as dc
from helpers import _through_device

pytestmark = pytest.mark.gpu

LEGAL = dc.legal_cases()
REFUSED = dc.refused_cases()
BGZF_FASTQ = [c for c in LEGAL if c.containers["bgzf"] is not None and c.kind == "fastq"]
GZIP_FASTQ = [c for c in LEGAL if c.containers["gzip"] is not None and c.kind == "fastq"]
FASTA = [c for c in LEGAL if c.kind == "fasta"]
EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "rkmh")


@pytest.fixture(scope="module")
def gctx(orc, data_dir):
    import rkmh_amd
    recs = orc.kseq_parse_file(os.path.join(data_dir, "hpv_16.fa.gz"))
    rb, ro = orc.pack([r[1] for r in recs])
    c = rkmh_amd.Context(0)
    c.set_references(np.concatenate([rb, np.zeros(16, np.uint8)]), ro, [16], 1000)
    yield c
    c.close()


@pytest.fixture(scope="module")
def slot(gctx):
    from rkmh_amd import api
    s = api.FastqSlot(gctx, max_bytes=1 << 20)
    yield s
    s.destroy()


@pytest.mark.parametrize("case", BGZF_FASTQ, ids=[c.name for c in BGZF_FASTQ])
def test_bgzf_form_device_equals_host(slot, tmp_path, case):
    from rkmh_amd import api
    path = tmp_path / "c.fq.gz"
    path.write_bytes(case.containers["bgzf"])
    z = api.Bgzf.open(str(path))
    assert z is not None and z.text_bytes == len(case.text)
    cap = 1 << 20
    host = C.create_string_buffer(cap + 64)
    try:
        for target in (1, 150000, 1 << 30):
            first = z.plan(target)
            got_all = b""
            for b0, b1 in zip(first, first[1:]):
                st, n, off = z.fastq_records(b0, b1, host, cap)
                assert st == 0
                got_all += host.raw[:n]
                dst, dn, doff = slot.load_bgzf(z, b0, b1)
                if case.expectation == "handover":
                    # (the one member with more than LONG_CAP long codes is the first of its file: every job inflates it)
                    assert dst == 1 if b0 == 0 else (dst == 1 or dn == 0), (case.name, b0, b1, dst)
                    continue
                assert dst == 0, (case.name, target, b0, b1)
                assert (dn, doff) == (n, off) or n == 0, (b0, b1, dn, n, doff, off)
                if dn:
                    res = slot.classify_raw(dn)       # (waits for the text's way back to the host; the device front end accepts it)
                    assert res.status == 0
                    assert bytes(slot.text_buffer()[:dn]) == host.raw[:n], (case.name, target, b0, b1)
            assert got_all == case.text
        if "halves" in case.facts:                    # cat a.fq.gz b.fq.gz: jobs that begin at, in front of and behind the empty member
            na, (la, lb) = case.facts["empty_member_at"], case.facts["halves"]
            assert z.text_offset(na) == z.text_offset(na + 1) == la
            for first in ([0, na + 1, z.members], [0, na, z.members], [0, na - 1, na + 1, na + 2, z.members]):
                got = b""
                for b0, b1 in zip(first, first[1:]):
                    dst, dn, doff = slot.load_bgzf(z, b0, b1)
                    assert dst == 0 and (dn == 0 or doff == len(got)), (first, b0, b1, dst, doff, len(got))
                    if dn:
                        assert slot.classify_raw(dn).status == 0
                        got += bytes(slot.text_buffer()[:dn])
                assert got == case.text and len(got) == la + lb, first
    finally:
        z.close()


@pytest.mark.parametrize("chunk_kb", [1, 32])
@pytest.mark.parametrize("case", GZIP_FASTQ, ids=[c.name for c in GZIP_FASTQ])
def test_single_stream_form(gctx, tmp_path, case, chunk_kb):
    path = tmp_path / "c.fq.gz"
    path.write_bytes(case.containers["gzip"])
    st = _through_device(gctx, path, case.text, 1 << 20, {"RKMH_GZIP_CHUNK_KB": str(chunk_kb)})
    if case.expectation == "handover":
        assert st and st[-1] == 1, (case.name, st)
    else:
        assert st and all(s == 0 for s in st), (case.name, chunk_kb, st)


LIBDEFLATE_LENIENT = {"repeat_past_hlit_plus_hdist", "bit_pattern_with_no_code"}      # (see tests/test_deflate_cases_cpu.py)


@pytest.mark.parametrize("bad", REFUSED, ids=[r.name for r in REFUSED])
def test_refused_member_is_never_text(slot, tmp_path, bad):
    """status 1 from the device (the branch that refuses it: bad.why), for all 22.  The host route then reports an error -- except
    that libdeflate, where it is the host inflater, takes the two classes of LIBDEFLATE_LENIENT and gives the footer's text"""
    from rkmh_amd import api
    p = tmp_path / "bad.gz"
    p.write_bytes(dc.bgzf_file([bad.member]))
    z = api.Bgzf.open(str(p))
    assert z is not None
    try:
        st, n, _ = slot.load_bgzf(z, 0, z.members)
        assert st == 1 and n == 0, (bad.name, bad.why, st, n)
        host = C.create_string_buffer(1 << 16)
        if api.load_library().rk_bgzf_inflater() == b"libdeflate" and bad.name in LIBDEFLATE_LENIENT:
            hs, hn, _ = z.fastq_records(0, z.members, host, 1 << 16)
            assert hs == 0 and host.raw[:hn] == bad.text
        else:
            with pytest.raises(api.RkmhError):
                z.fastq_records(0, z.members, host, 1 << 16)
    finally:
        z.close()


def _reads_from(tmp_path, fa_text, n=3000):
    from rkmh_amd import api, synth
    fa = tmp_path / "g.fa"
    fa.write_bytes(fa_text)
    refs = api.parse_files([str(fa)])
    qb, qo = synth.generate_reads_fast(refs["bases"], refs["offsets"], 0, n, read_len=100, threads=4)
    fq = tmp_path / "r.fq"
    fq.write_bytes(b"".join(b"@q%06d\n" % i + bytes(qb[int(qo[i]):int(qo[i + 1])]) + b"\n+\n" + b"I" * 100 + b"\n" for i in range(n)))
    return fa, fq


@pytest.mark.parametrize("case", FASTA, ids=[c.name for c in FASTA])
def test_reference_loader_takes_the_fasta_cases(tmp_path, case):
    """-r case.fa.gz with RKMH_RAW_REFS=1: rk_fasta_load_put_bgzf / _gzip inflate the references' text on the device; the same
    lines as with the host parser on the plain file"""
    fa, fq = _reads_from(tmp_path, case.text)
    form = "bgzf" if case.containers["bgzf"] is not None else "gzip"
    gz = tmp_path / ("g.%s.fa.gz" % form)
    gz.write_bytes(case.containers[form])

    def run(ref, env):
        r = subprocess.run([EXE, "stream", "-k", "16", "-s", "1000", "-f", str(fq), "-r", str(ref)], capture_output=True, env=dict(os.environ, RKMH_TIMING="1", **env))
        assert r.returncode == 0, r.stderr[-500:]
        return r.stdout, r.stderr
    want, _ = run(fa, {"RKMH_RAW_REFS": "0"})
    assert want.count(b"\n") == 3000
    got, err = run(gz, {"RKMH_RAW_REFS": "1", "RKMH_GZIP_CHUNK_KB": "1"})
    assert got == want
    assert b"references through the device: 6 sequences" in err, err[-600:]
    got, _ = run(gz, {"RKMH_RAW_REFS": "0"})
    assert got == want


def test_cli_stream_on_a_file_of_several_cases(tmp_path, data_dir):
    """bin/rkmh stream on a BGZF file made of the members of several cases, and on the single-stream case, prints what it prints
    for the plain text; the diagnostics show the device inflated them"""
    names = ("repeat16_crosses_hlit", "repeat16_after_18", "repeat16_after_17", "long_codes_128_of_cap_128", "hlit286_hdist30_all_thirty_distances_twenty_long",
             "hundreds_of_one_symbol_blocks", "literal_runs_254_to_511_between_matches", "long_read_of_distance_1_matches_of_258",
             "distance_32768_length_258_in_a_65536_byte_member", "self_overlapping_matches_of_258_at_distances_2_to_17", "member_of_512_entries")
    by = {c.name: c for c in LEGAL}
    members, text = [], b""
    for nm in names:
        for raw, t in by[nm].raws:
            members.append(dc.bgzf_member(raw, t))
            text += t
    fq = tmp_path / "cases.fq"
    fq.write_bytes(text)
    bz = tmp_path / "cases.bgzf.fq.gz"
    bz.write_bytes(dc.bgzf_file(members))
    one = by["stream_of_the_catalogue_token_shapes"]
    fq1 = tmp_path / "one.fq"
    fq1.write_bytes(one.text)
    gz1 = tmp_path / "one.fq.gz"
    gz1.write_bytes(one.containers["gzip"])
    base = ["-r", os.path.join(data_dir, "hpv_16.fa.gz"), "-k", "16", "-s", "1000"]

    def run(f, env=None):
        r = subprocess.run([EXE, "stream"] + base + ["-f", str(f)], capture_output=True, env=dict(os.environ, RKMH_BGZF_TIMING="1", RKMH_TIMING="1", **(env or {})))
        assert r.returncode == 0, r.stderr[-600:]
        return r.stdout, r.stderr
    want, _ = run(fq)
    assert want.count(b"\n") == text.count(b"\n") // 4
    got, err = run(bz)
    assert got == want and b"[bgzf device]" in err and b"handed to the host" not in err, err[-800:]
    got, _ = run(bz, {"RKMH_BGZF_DEVICE": "0"})
    assert got == want
    want1, _ = run(fq1)
    for env in ({}, {"RKMH_GZIP_CHUNK_KB": "1"}):
        got1, err1 = run(gz1, env)
        assert got1 == want1 and b"[gzip device]" in err1 and b"stops at byte" not in err1, err1[-800:]


CHUNK_COUNTS = [c for c in LEGAL if c.name.startswith("stream_every_block_with_a_crossing") or c.name == "stream_of_fixed_and_stored_blocks_no_chunk_start"]


@pytest.mark.parametrize("case", CHUNK_COUNTS, ids=[c.name for c in CHUNK_COUNTS])
def test_chunk_starts_found_behind_crossing_headers(tmp_path, data_dir, case):
    """gz_header_ok's verdict, seen through the number of chunks the device route forms with chunk boundaries every 1 KB.  A stream
    whose every block (< 1 KB of compressed bytes each) begins with a header that carries a crossing repeat has a header behind
    every boundary: all but the last few boundaries (gz_header_maybe leaves the last 4 096 bits to the chunk in front) must
    yield a chunk, and every chunk must lie in the chain.  A stream of fixed and stored blocks has no chunk start: one chunk."""
    import re
    fq = tmp_path / "c.fq"
    fq.write_bytes(case.text)
    gz = tmp_path / "c.fq.gz"
    gz.write_bytes(case.containers["gzip"])
    base = ["-r", os.path.join(data_dir, "hpv_16.fa.gz"), "-k", "16", "-s", "1000"]

    def run(f):
        r = subprocess.run([EXE, "stream"] + base + ["-f", str(f)], capture_output=True, env=dict(os.environ, RKMH_BGZF_TIMING="1", RKMH_TIMING="1", RKMH_GZIP_CHUNK_KB="1", RKMH_GZIP_STRETCH_KB="1024"))      # (one call for the whole file)
        assert r.returncode == 0, r.stderr[-600:]
        return r.stdout, r.stderr
    want, _ = run(fq)
    got, err = run(gz)
    assert got == want and b"stops at byte" not in err
    m = re.findall(rb"\[gzip device\] .* call 1 of 1: (\d+) chunks \((\d+) in the chain\)", err)
    assert len(m) == 1, err[-800:]
    chunks, chain = int(m[0][0]), int(m[0][1])
    nbound = (8 * (len(case.containers["gzip"]) - 8) - 80 - 1) // 8192      # boundaries every 8 192 bits behind the gzip header's 80
    if case.facts["blocks"]["dynamic"] == 0:
        assert nbound > 100 and (chunks, chain) == (1, 1)
    else:
        assert nbound >= 20 and chunks == chain and chunks >= nbound - 1, (chunks, chain, nbound)
