"""The catalogue of tests/deflate_cases.py, without a GPU: every legal case inflates under zlib -- the arbiter, because it is what the
reference's gzopen runs -- to exactly its text; every case's `facts` show the property its name claims; every refused case raises
under zlib (gzip, for ISIZE and CRC-32); and the HOST routes of this library (rk_bgzf_fastq_records with libdeflate and with zlib,
the sequential gzip reader) give the same text -- and, for the refused members, an error: all 22 with zlib, 20 with libdeflate, whose
two lenient classes are named (LIBDEFLATE_LENIENT)."""
import ctypes as C
import gzip
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import deflate_cases as dc

LEGAL = dc.legal_cases()
REFUSED = dc.refused_cases()


@pytest.mark.parametrize("case", LEGAL, ids=[c.name for c in LEGAL])
def test_legal_case_is_its_text_under_zlib(case):
    for raw, text in case.raws:
        assert zlib.decompress(raw, -15) == text
    assert case.raws or case.containers["bgzf"]
    for form, img in case.containers.items():
        if img is not None:
            assert gzip.decompress(img) == case.text, form
    assert case.kind == ("fasta" if case.text[:1] == b">" else "fastq")
    if case.kind == "fastq":                    # four-line records, as the loaders cut them
        lines = case.text.split(b"\n")
        assert lines[-1] == b"" and len(lines) % 4 == 1
        for i in range(0, len(lines) - 1, 4):
            assert lines[i][:1] == b"@" and lines[i + 2][:1] == b"+" and len(lines[i + 1]) == len(lines[i + 3]) > 0, (case.name, i)


# what every case exists for, as a property of the facts its writer recorded
CLAIMS = {
    "repeat16_crosses_hlit": lambda f: f["repeat_crossed"] == [16] and f["long_dl_max"] == 5,
    "repeat18_crosses_hlit": lambda f: f["repeat_crossed"] == [18],
    "repeat17_crosses_hlit": lambda f: f["repeat_crossed"] == [17],
    "repeat16_after_18": lambda f: f["rep16_after"] == [18] and f["repeat_crossed"] == [18],
    "repeat16_after_17": lambda f: f["rep16_after"] == [17],
    "repeat18_crosses_into_incomplete_distance_code": lambda f: f["repeat_crossed"] == [18] and f["incomplete_dist"] == 1,
    "stream_every_block_with_a_crossing_16": lambda f: f["repeat_crossed"] == [16] * 40 and f["blocks"]["dynamic"] == 40 and _headers_in_every_kb(f),
    "stream_every_block_with_a_crossing_18": lambda f: f["repeat_crossed"] == [18] * 40 and f["incomplete_dist"] == 0 and _headers_in_every_kb(f),
    "stream_every_block_with_a_crossing_18_into_an_incomplete_distance_code": lambda f: f["repeat_crossed"] == [18] * 40 and f["incomplete_dist"] == 40 and _headers_in_every_kb(f),
    "stream_of_fixed_and_stored_blocks_no_chunk_start": lambda f: f["blocks"]["dynamic"] == 0 and f["blocks"]["fixed"] >= 30 and f["blocks"]["stored"] >= 15 and f["out_len"] > 150000,
    "hlit257_no_length_symbols_no_distance_code": lambda f: f["hlit"] == {257} and f["hdist"] == {1} and f["no_dist_code"] == 1 and not f["matches"],
    "dynamic_blocks_with_only_the_end_of_block_code": lambda f: f["empty_blocks"]["dynamic"] == 2 and f["first_block"] == "dynamic" and f["final_empty"],
    "hclen5_the_least_a_legal_header_has": lambda f: f["hclen"] == {5},
    "long_codes_128_of_cap_128": lambda f: f["long_ll_max"] == 128 and f["hlit"] == {286} and f["high_literals"] >= 128,
    "long_codes_129_of_cap_128": lambda f: f["long_ll_max"] == 129 and f["hlit"] == {286} and f["high_literals"] >= 128,
    "hlit286_hdist30_all_thirty_distances_twenty_long": lambda f: f["hlit"] == {286} and f["hdist"] == {30} and f["dist_syms"] == set(range(30)) and f["long_dl_max"] == 20
                                                        and f["max_dist"] == 32768 and f["longest_dl"] > dc.DT,
    "fixed_code_literals_128_to_255": lambda f: f["blocks"] == {"stored": 0, "fixed": 1, "dynamic": 0} and f["high_literals"] > 200,
    "empty_stored_block_first_and_final": lambda f: f["first_block"] == "stored" and f["final_block"] == "stored" and f["final_empty"] and min(f["empty_blocks"].values()) >= 1,
    "empty_fixed_block_first_and_final": lambda f: f["first_block"] == "fixed" and f["final_block"] == "fixed" and f["final_empty"] and min(f["empty_blocks"].values()) >= 1,
    "empty_dynamic_block_first_and_final": lambda f: f["first_block"] == "dynamic" and f["final_block"] == "dynamic" and f["final_empty"] and min(f["empty_blocks"].values()) >= 1,
    "hundreds_of_one_symbol_blocks": lambda f: min(f["blocks"].values()) >= 190 and sum(f["blocks"].values()) == f["out_len"],
    "stored_block_behind_every_bit_offset": lambda f: f["stored_hdr_bit_offsets"] == set(range(8)),
    "literal_runs_254_to_511_between_matches": lambda f: _runs_between(f) >= {254, 255, 256, 509, 510, 511, 765},
    "long_read_of_distance_1_matches_of_258": lambda f: f["literals"] == 2 + 10 and f["len258"] >= 246 and 245 <= f["entries"] <= 255 and f["out_len"] > 64000,
    "distance_32768_length_258_in_a_65536_byte_member": lambda f: f["max_dist"] == 32768 and (258, 32768) in f["matches"] and f["len258_as_284"] >= 1,
    "distance_32767_length_258_in_a_65536_byte_member": lambda f: f["max_dist"] == 32767 and (258, 32767) in f["matches"],
    "self_overlapping_matches_of_258_at_distances_2_to_17": lambda f: {m for m in f["matches"]} == {(258, d) for d in range(2, 18)},
    "chain_of_400_matches_each_copying_the_one_before": lambda f: f["matches"].count((5, 5)) == 800,
    "member_of_511_entries": lambda f: f["entries_per_member"] == [511],
    "member_of_512_entries": lambda f: f["entries_per_member"] == [512],
    "member_of_513_entries": lambda f: f["entries_per_member"] == [513],
    "members_of_0_1_2_65535_65536_bytes": lambda f: f["member_text_sizes"][:5] == [1, 2, 65535, 0, 65536] and f["empty_members_in_the_middle"] == 1,
    "cat_of_two_bgzf_files_empty_member_mid_file": lambda f: f["empty_member_at"] > 0 and min(f["halves"]) > 30000,
    "stream_every_block_with_an_incomplete_one_code_distance_tree": lambda f: f["incomplete_dist"] == f["blocks"]["dynamic"] == 60 and f["max_dist"] == 1,
    "stream_of_the_catalogue_token_shapes": lambda f: f["final_dynamic_bits_from_end"] < 4096 and f["max_dist"] == 32768 and (20, 32767) in f["matches"]
                                            and min(f["blocks"].values()) >= 14 and min(f["empty_blocks"].values()) >= 14 and {255, 1, 0} <= set(f["lit_runs"]),
    "fasta_members_with_zero_run_repeats": lambda f: f["rep16_after_zero_run"] >= 2 and len(f["entries_per_member"]) == 2,
    "fasta_stream_fixed_stored_dynamic": lambda f: min(f["blocks"].values()) >= 1,
}
for _R in (254, 255, 256, 509, 510, 511):
    CLAIMS["literal_tail_of_%d" % _R] = (lambda R: lambda f: _tail(f) == R and isinstance(f["matches"][-1], tuple))(_R)
for _m in range(4):
    CLAIMS["literal_total_%d_mod_4" % _m] = (lambda m: lambda f: f["literals"] % 4 == m)(_m)


def _headers_in_every_kb(f):
    bits = f["dynamic_header_bits"]
    return max(b - a for a, b in zip(bits, bits[1:])) < 8192


def _whole_runs(f):
    """the literal runs in front of every match and at the tail.  lit_runs holds one number per entry of pass 1; a run reaches 255
    only as a carry entry (the 255th literal makes one at once, the match behind it then has a run of 0), so the 255s add up"""
    out, acc = [], 0
    for r in f["lit_runs"]:
        acc += r
        if r != 255:
            out.append(acc)
            acc = 0
    return out + ([acc] if acc else [])


def _runs_between(f):
    return set(_whole_runs(f)[:-1])


def _tail(f):
    return _whole_runs(f)[-1]


@pytest.mark.parametrize("case", LEGAL, ids=[c.name for c in LEGAL])
def test_facts_show_what_the_name_claims(case):
    assert case.name in CLAIMS, "a case without a stated claim"
    assert CLAIMS[case.name](case.facts), {k: v for k, v in case.facts.items() if k not in ("matches", "lit_runs")}
    assert case.expectation in ("device", "handover")
    for n in case.facts.get("entries_per_member", []):
        assert n <= 0x7FFF                      # (status[nmem + m] keeps the entries in 15 bits)


def test_the_catalogue_covers_every_residue_and_both_sides_of_the_cap():
    names = {c.name for c in LEGAL}
    assert len(names) == len(LEGAL) >= 40
    assert sorted(c.name for c in LEGAL if c.expectation == "handover") == ["long_codes_129_of_cap_128"]      # (the one reason the source names)
    assert all(c.facts["long_ll_max"] <= 128 for c in LEGAL if c.expectation == "device")
    assert {c.facts["literals"] % 4 for c in LEGAL if c.name.startswith("literal_total_")} == {0, 1, 2, 3}


@pytest.mark.parametrize("bad", REFUSED, ids=[r.name for r in REFUSED])
def test_refused_case_raises_under_zlib(bad):
    if bad.arbiter == "zlib":
        with pytest.raises(zlib.error):
            zlib.decompress(bad.raw, -15)
    with pytest.raises((zlib.error, gzip.BadGzipFile, EOFError)):
        gzip.decompress(bad.member + dc.BGZF_EOF)


def _host_bgzf_text(api, path, text, kind):
    z = api.Bgzf.open(str(path))
    assert z is not None and z.text_bytes == len(text)
    cap = len(text) + 64
    dst = C.create_string_buffer(cap)
    try:
        for target in (1, 70000, 1 << 30):
            first = z.plan(target)
            got = b""
            for b0, b1 in zip(first, first[1:]):
                st, n, off = z.fastq_records(b0, b1, dst, cap)
                assert st == 0 and (n == 0 or off == len(got)), (b0, b1, st, off, len(got))
                got += dst.raw[:n]
            assert got == text, target
    finally:
        z.close()


def _same_sequences(api, a, b):
    ra, rb = api.parse_files([str(a)]), api.parse_files([str(b)])
    assert len(ra["names"]) == len(rb["names"]) > 0 and list(ra["names"]) == list(rb["names"])
    assert np.array_equal(ra["offsets"], rb["offsets"]) and np.array_equal(ra["bases"], rb["bases"])


def _inflater(api):
    return api.load_library().rk_bgzf_inflater().decode()


@pytest.mark.parametrize("nolibdeflate", [False, True])
def test_host_routes_give_the_text(tmp_path, nolibdeflate):
    """rk_bgzf_fastq_records over every job of the BGZF form -- with libdeflate where the machine has it, and with zlib
    (RKMH_NO_LIBDEFLATE=1 in a fresh interpreter: the inflater is chosen when the library is first used) -- and the sequential gzip
    reader (rk_parse_files) over the single-stream form: every legal case, the one the device hands over included.  The run prints
    which inflater it was (rk_bgzf_inflater)"""
    if nolibdeflate and not os.environ.get("RKMH_NO_LIBDEFLATE"):
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", __file__, "-k", "test_host_routes_give_the_text and True"],
                           env=dict(os.environ, RKMH_NO_LIBDEFLATE="1"), capture_output=True)
        assert r.returncode == 0 and b"host inflater: zlib" in r.stdout, r.stdout.decode()[-3000:]
        return
    from rkmh_amd import api
    print("host inflater:", _inflater(api))
    assert _inflater(api) == "zlib" if os.environ.get("RKMH_NO_LIBDEFLATE") else _inflater(api) in ("libdeflate", "zlib")
    for case in LEGAL:
        plain = tmp_path / (case.name + (".fa" if case.kind == "fasta" else ".fq"))
        plain.write_bytes(case.text)
        if case.containers["bgzf"] is not None:
            p = tmp_path / (case.name + ".bgzf.gz")
            p.write_bytes(case.containers["bgzf"])
            if case.kind == "fastq":
                _host_bgzf_text(api, p, case.text, case.kind)
            _same_sequences(api, p, plain)
        if case.containers["gzip"] is not None:
            p = tmp_path / (case.name + ".gz")
            p.write_bytes(case.containers["gzip"])
            assert api.Bgzf.open(str(p)) is None
            _same_sequences(api, p, plain)


# the members libdeflate takes although zlib refuses them (it then delivers the text the footer's CRC-32 and ISIZE vouch for): it lets
# the last code-length repeat run past HLIT + HDIST, and decodes either bit as the one symbol of an incomplete one-code tree
LIBDEFLATE_LENIENT = {"repeat_past_hlit_plus_hdist", "bit_pattern_with_no_code"}


@pytest.mark.parametrize("bad", REFUSED, ids=[r.name for r in REFUSED])
def test_host_route_reports_the_refused_member(tmp_path, bad):
    """rk_bgzf_fastq_records on every refused member, by the inflater this process runs (rk_bgzf_inflater).  zlib: an error for all
    22.  libdeflate: an error for 20; for the two classes of LIBDEFLATE_LENIENT, the footer's text and nothing else."""
    from rkmh_amd import api
    dst = C.create_string_buffer(1 << 16)
    p = tmp_path / (bad.name + ".gz")
    p.write_bytes(dc.bgzf_file([bad.member]))
    z = api.Bgzf.open(str(p))
    assert z is not None, bad.name
    try:
        if _inflater(api) == "libdeflate" and bad.name in LIBDEFLATE_LENIENT:
            st, n, off = z.fastq_records(0, z.members, dst, 1 << 16)
            assert (st, off) == (0, 0) and dst.raw[:n] == bad.text and zlib.crc32(bad.text) == int.from_bytes(bad.member[-8:-4], "little")
        else:
            with pytest.raises(api.RkmhError):
                z.fastq_records(0, z.members, dst, 1 << 16)
    finally:
        z.close()


def test_host_route_with_zlib_reports_all_refused_members():
    """the same in a fresh interpreter with RKMH_NO_LIBDEFLATE=1: the inflater is zlib there, and all 22 are errors"""
    from rkmh_amd import api
    if os.environ.get("RKMH_NO_LIBDEFLATE"):
        assert _inflater(api) == "zlib"
        return
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", __file__, "-k", "test_host_route_reports_the_refused_member or test_host_route_with_zlib"],
                       env=dict(os.environ, RKMH_NO_LIBDEFLATE="1"), capture_output=True)
    assert r.returncode == 0 and b"23 passed" in r.stdout, r.stdout.decode()[-3000:]
