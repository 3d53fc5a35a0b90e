"""`call` on the device, record by record: Context.call against the oracle as multisets of whole records (the device appends
through an atomicAdd, so order is not part of the contract), bin/rkmh call against CALL_HEADER + call_rows.  Exact equality.
The inputs and the property each exists for live in tests/call_cases.py; tests/test_call_cpu.py checks them without a GPU."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import call_cases as cc
from call_cases import WL, _SEEDS, wl_name

pytestmark = pytest.mark.gpu

# seeds of the randomized generator that once failed (kept forever), each with what it showed: none so far
_REGRESSION_SEEDS = []


def _pad(b):
    out = np.zeros(len(b) + 16, dtype=np.uint8)
    out[: len(b)] = b
    return out


def _device(orc, case, calls=1, spec=None):
    """The device's sorted records for a case, `calls` times on one context built for the case's policy (as keyword fields, or
    as the text form when `spec` is given)."""
    import rkmh_amd
    rb, ro = orc.pack(case.ref_seqs)
    qb, qo = orc.pack(case.reads)
    c = rkmh_amd.Context(0, policy_spec=spec) if spec else rkmh_amd.Context(0, **case.policy)
    try:
        want = case.pol(orc)
        assert (c.policy.fold, c.policy.drop_last_window, c.policy.seed) == (want.fold, want.drop_last_window, want.seed)
        return [cc.device_records(c.call(_pad(rb), ro, _pad(qb), qo, case.k, case.w)) for _ in range(calls)]
    finally:
        c.close()


def _same(got, want, what):
    if got != want:
        a, b = set(got), set(want)
        raise AssertionError("%s: %d device records, %d oracle records; device only %s; oracle only %s"
                             % (what, len(got), len(want), sorted(a - b)[:8], sorted(b - a)[:8]))


def _run(orc, name, **kw):
    case, want = cc.checked_oracle(orc, name)          # the case's non-vacuity check passes before the device is asked
    for got in _device(orc, case, **kw):
        _same(got, want, name)
    return case, want


def _spec(policy):
    return "fold=%s,windows=%s,seed=%d" % (("swap32", "h1", "w2w1")[policy.get("fold", 0)],
                                           "len-k" if policy.get("drop_last_window", 1) else "len-k+1", policy.get("seed", 42))


@pytest.mark.parametrize("k", cc.K_SWEEP)
def test_k_sweep(orc, k):
    """one to four trips of the 64-lane candidate loop; canonical_bytes across 32 bases"""
    _run(orc, "ksweep_k%d" % k)


def test_limits_are_refused(orc):
    import rkmh_amd
    case = cc.get_case(orc, "panel_one")
    rb, ro = orc.pack(case.ref_seqs)
    qb, qo = orc.pack(case.reads)
    c = rkmh_amd.Context(0)
    try:
        for k, w, code in ((65, 100, -5), (0, 100, -5), (16, 0, -1), (16, -3, -1)):     # RK_ERR_LIMIT, RK_ERR_ARG
            with pytest.raises(rkmh_amd.api.RkmhError) as e:
                c.call(_pad(rb), ro, _pad(qb), qo, k, w)
            assert e.value.code == code, (k, w, e.value.code)
        # wtot >= 2^30 is refused too, but only a reference of a gigabase reaches that check through rk_call: not asserted here
        _same(cc.device_records(c.call(_pad(rb), ro, _pad(qb), qo, 64, 100)),
              sorted(orc.call_records(case.ref_names, case.ref_seqs, case.reads, 64, 100)), "k=64 after the refusals")
    finally:
        c.close()


@pytest.mark.parametrize("fold,drop,seed", cc.POLICIES)
def test_policies(orc, fold, drop, seed):
    """every fold x window rule x two seeds; a reference of exactly k bases (one window under len-k+1) and one of k - 1"""
    name = "policy_f%d_d%d_s%d" % (fold, drop, seed)
    case, want = _run(orc, name)
    for got in _device(orc, case, spec=_spec(case.policy)):        # the same policy given as text
        _same(got, want, name + " by policy_spec")


def test_non_acgt(orc):
    """N runs, IUPAC codes, lower case: hash 0 as a populated key, as reference depth and as candidate; snp_alt without answer"""
    _run(orc, "non_acgt")


@pytest.mark.parametrize("which", cc.PANELS)
def test_panels(orc, which):
    """1, 2, 3 and 40 references; references without a window first, in the middle, last, adjacent, alone; dips within
    window_len of a reference's start, so the mean reaches back across one and two reference boundaries"""
    case, want = _run(orc, "panel_" + which)
    if which == "only_short":
        assert want == []


@pytest.mark.parametrize("label", WL)
def test_window_lengths(orc, label):
    case, want = _run(orc, wl_name(orc, label))
    if label == "1":
        assert want == []


def test_more_than_a_million_windows(orc):
    """two second-level scan blocks (both k_scan_add launches): SNPs and deletions on first-level block boundaries, on window
    2^20 and in the last windows of a 1.3 Mb reference, then a second reference"""
    _run(orc, "million_windows")


def test_record_overflow(orc):
    """more records than the first buffer holds: complete after the re-run, and the same on a second call"""
    case, want = _run(orc, "record_overflow", calls=2)
    assert len(want) > cc.RCAP0


def test_depth_table_homopolymers(orc):
    _run(orc, "homopolymer")


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_depth_table_capacity_doubles(orc, delta):
    _run(orc, "cap_%+d" % delta)


def test_depth_table_probe_chain_wraps(orc):
    _run(orc, "probe_wrap")


@pytest.mark.parametrize("name", ["no_reads", "short_reads"])
def test_no_read_windows(orc, name):
    case, want = _run(orc, name)
    assert want == []


@pytest.mark.parametrize("seed", _SEEDS + _REGRESSION_SEEDS)
def test_randomized_call_differential(orc, seed):
    """random k, window length, policy, panel (copies, low complexity, N runs, lower case, lengths around k and 0) and ragged
    reads from mutated copies (SNPs, 1-bp deletions and insertions, noise, both strands) against the literal loop"""
    _run(orc, "random_%d" % seed)


# ---- the command line ------------------------------------------------------------------------------------------------------
def _cli(orc, root, tmp_path, case, nfiles, extra=()):
    exe = os.path.join(root, "bin", "rkmh")
    per = (len(case.refs) + nfiles - 1) // nfiles
    fas = []
    for f in range(nfiles):
        p = tmp_path / ("refs%d.fa" % f)
        p.write_bytes(b"".join(b">" + n + b"\n" + s + b"\n" for n, s in case.refs[f * per:(f + 1) * per]))
        fas.append(str(p))
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(case.reads)))
    gz = tmp_path / "reads.fq.gz"
    with gzip.open(gz, "wb") as f:
        f.write(fq.read_bytes())
    # what the files hold, read back by the restated record grammar, is what the oracle is given
    refs = [x for p in fas for x in orc.kseq_parse_file(p)]
    reads = [x[1] for x in orc.kseq_parse_file(str(fq))]
    assert [(n, s) for n, s, _ in refs] == list(case.refs) and reads == list(case.reads)
    want = orc.CALL_HEADER % fas[0] + "".join(orc.rows_from_records(case.ref_names, cc.oracle_records(orc, case)))
    args = [exe, "call"] + [a for p in fas for a in ("-r", p)]
    outs = []
    for reads_path in (fq, gz):
        r = subprocess.run(args + ["-f", str(reads_path), "-k", str(case.k), "-w", str(case.w)] + list(extra), capture_output=True)
        assert r.returncode == 0, r.stderr
        assert (b"WARNING: more than one ref provided" in r.stderr) == (len(case.refs) > 1)
        assert r.stdout.decode() == want, (case.name, str(reads_path))
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    return want


@pytest.mark.parametrize("name,nfiles", [("non_acgt", 2), ("panel_three", 3), ("panel_short_adjacent", 6), ("panel_forty", 2),
                                         ("panel_only_short", 2)])
def test_cli_rows(orc, root, tmp_path, name, nfiles):
    case, recs = cc.checked_oracle(orc, name)
    want = _cli(orc, root, tmp_path, case, nfiles)
    assert (want.count("\tPASS\t") > 0) == (len(recs) > 0)


def test_cli_rows_randomized_with_policy(orc, root, tmp_path):
    """one seed of the randomized generator through --hash-policy (the first with several references and records)"""
    for seed in range(200):
        case = cc.get_case(orc, "random_%d" % seed)
        if len(case.refs) >= 2 and len(cc.oracle_records(orc, case)) > 50 and case.policy != dict(fold=0, drop_last_window=1, seed=42):
            break
    else:
        raise AssertionError("no seed with several references and records")
    _cli(orc, root, tmp_path, case, len(case.refs), extra=["--hash-policy", _spec(case.policy)])


def test_cli_hash_policy_mash(orc, root, tmp_path):
    """--hash-policy mash = fold h1, windows len-k+1, seed 42"""
    case, _ = cc.checked_oracle(orc, "policy_f1_d0_s42")
    _cli(orc, root, tmp_path, case, 4, extra=["--hash-policy", "mash"])
