"""`call` on the CPU alone: the record-level oracle against its second formulation and against the rows it printed before it was
split, and the non-vacuity condition of every input tests/test_gpu_call.py hands to the device (tests/call_cases.py)."""
import json
import os

import pytest

import call_cases as cc
from helpers import _call_fixture

from call_cases import WL, _SEEDS, wl_name


def test_call_rows_unchanged_by_the_split(orc, data_dir, golden_dir):
    """call_rows, now rows_from_records(call_records), gives the rows recorded from the one-piece call_rows."""
    g = json.load(open(os.path.join(golden_dir, "call_rows_hpv16.json")))
    rec, reads, _, _ = _call_fixture(orc, data_dir, None)
    assert rec[0].decode() == g["ref_name"] and [(c["k"], c["window_len"]) for c in g["cases"]] == [(12, 100), (16, 30)]
    for c in g["cases"]:
        names = [rec[0].decode()]
        recs = orc.call_records(names, [rec[1]], reads, c["k"], c["window_len"])
        assert orc.rows_from_records(names, recs) == c["rows"]
        assert orc.call_rows(names, [rec[1]], reads, c["k"], c["window_len"]) == c["rows"]
        assert sorted(orc.call_records_fast(names, [rec[1]], reads, c["k"], c["window_len"])) == sorted(recs)
        assert sum(int(r.split("KC=")[1].split(";")[0]) for r in c["rows"]) == len(recs)


def _both(orc, name):
    """non-vacuity of the case on the oracle's records, and fast == literal"""
    case, recs = cc.checked_oracle(orc, name)
    other = cc.oracle_records(orc, case, fast=not case.fast)
    assert other == recs, (name, len(other), len(recs), sorted(set(other) ^ set(recs))[:6])
    return case, recs


@pytest.mark.parametrize("name", list(cc.SMALL))
def test_small_case(orc, name):
    _both(orc, name)


@pytest.mark.parametrize("label", WL)
def test_window_len_case(orc, label):
    _both(orc, wl_name(orc, label))


@pytest.mark.parametrize("name", list(cc.LARGE))
def test_large_case(orc, name):
    _both(orc, name)


def test_records_carry_what_rows_hide(orc):
    """The gap the record-level comparison closes: records whose avg_d / depth the aggregated row (maxima per site) drops."""
    case, recs = cc.checked_oracle(orc, "panel_three")
    rows = orc.rows_from_records(case.ref_names, recs)
    assert len(rows) < len(recs)
    cc.check_avg_varies_within_site(orc, case, recs)


@pytest.mark.parametrize("seed", _SEEDS)
def test_randomized_fast_equals_literal(orc, seed):
    _both(orc, "random_%d" % seed)


def test_randomized_inputs_are_not_all_empty(orc):
    """the generator's seeds call something: records of both kinds in a good share of them, references without windows in some"""
    n_rec = n_both = n_empty_ref = 0
    for seed in _SEEDS:
        case = cc.get_case(orc, "random_%d" % seed)
        recs = cc.oracle_records(orc, case)
        n_rec += bool(recs)
        n_both += any(r[4] == 0 for r in recs) and any(r[4] == 1 for r in recs)
        n_empty_ref += 0 in case.nwin(orc)
    assert n_rec * 2 >= len(_SEEDS) and n_both * 4 >= len(_SEEDS) and n_empty_ref * 6 >= len(_SEEDS), (n_rec, n_both, n_empty_ref)
