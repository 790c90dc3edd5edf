"""CPU (no GPU): what the level-weighted decoders refuse, and in which order -- tests/golden/level_decoder_refusals.tsv was recorded (tools/gen_level_decoder_refusals.py)
from the public entry points as they were before their host paths were merged; every row of tests/level_refusal_cases.py is replayed here and must raise the same
exception type with the same message, or, for the four C entry points, return the same status.  A row with two faults pins which of them is refused first; a `host` row
with valid arguments must get as far as the device check and no further; a `device` row with valid arguments must arrive at the recorded symbol of the library."""
import collections
import csv
import os

import pytest
import torch

from conftest import ROOT

import level_refusal_cases as L

TABLE = os.path.join(ROOT, "tests", "golden", "level_decoder_refusals.tsv")


@pytest.fixture(scope="module")
def table():
    with open(TABLE, newline="") as f:
        rows = list(csv.DictReader(f, delimiter="\t", quoting=csv.QUOTE_NONE))
    return {(r["entry"], r["tag"]): r for r in rows}


def test_the_table_and_the_cases_name_the_same_rows(table):
    names = [c[:2] for c in L.CASES] + [c[:2] for c in L.C_CASES]
    assert len(names) == len(table) and set(names) == set(table)
    for entry, tag, where, _ in L.CASES:
        assert table[(entry, tag)]["where"] == where
    for symbol, tag, made_up, _ in L.C_CASES:
        assert table[(symbol, tag)]["where"] == ("made_up" if made_up else "null") and table[(symbol, tag)]["outcome"] == "status"


def test_the_table_covers_what_it_is_for(table):
    by_entry = collections.defaultdict(list)
    for (entry, tag), r in table.items():
        by_entry[entry.split("/")[0]].append((tag, r))
    assert set(by_entry) == {"codec.extract_soft", "codec.extract_soft_l", "codec.level_pack", "codec.level_pack_l", "soft.extract_soft", "soft.extract_soft_l",
                             "trace.trace_latents_keyed_soft", "trace.trace_latents_keyed_soft_l", "detect.detect_latents", "detect.detect_latents_soft_l",
                             "detect.detect_latents_aligned_soft", "align.search_keys", "align.search_keys_soft", "align.extract_aligned_soft",
                             "gsw_extract_soft", "gsw_extract_soft_l", "gsw_level_pack", "gsw_level_pack_l"}
    for entry, rows in by_entry.items():
        assert sum(tag.startswith("two_") for tag, _ in rows) >= 1, entry                       # the order of two faults
        if entry.startswith("gsw_"):
            assert {r["message"] for _, r in rows} >= {"1", "2"}, entry                         # GSW_ERR_BAD_ARG and GSW_ERR_UNSUPPORTED; no row is accepted
            assert "0" not in {r["message"] for _, r in rows} and "4" not in {r["message"] for _, r in rows}, entry
            assert all(r["message"] == "1" for _, r in rows if r["where"] == "null"), entry
        else:
            host = [r for tag, r in rows if tag.split("/")[0] in ("host", "host_table")]
            assert host and all(r["outcome"] == "RuntimeError" and "HIP device" in r["message"] for r in host), entry
            assert any(r["outcome"] == "Reached" for _, r in rows), entry
    assert {r["message"] for r in table.values() if r["outcome"] == "Reached"} >= {"gsw_extract_soft", "gsw_extract_soft_l", "gsw_level_pack", "gsw_level_pack_l"}


@pytest.mark.parametrize("entry", sorted({c[0] for c in L.CASES}))
def test_python_entries_refuse_as_recorded(table, entry):
    wrong = []
    for e, tag, where, thunk in L.CASES:
        if e == entry:
            want = table[(e, tag)]
            got = L.outcome(thunk, where)
            if got != (want["outcome"], want["message"]):
                wrong.append((tag, got, (want["outcome"], want["message"])))
    assert not wrong, wrong
    assert "is_cuda" not in vars(torch.Tensor) and not torch.zeros(1).is_cuda                  # the stand-in for the device is gone again


@pytest.mark.parametrize("symbol", sorted({c[0] for c in L.C_CASES}))
def test_c_entries_return_as_recorded(table, symbol):
    """Rows with a null pointer everywhere; the rows whose pointers are made up only where no device could ever see them"""
    device = torch.cuda.is_available()
    wrong, ran = [], 0
    for s, tag, made_up, args in L.C_CASES:
        if s == symbol and not (made_up and device):
            got, ran = L.c_outcome(s, args), ran + 1
            if str(got) != table[(s, tag)]["message"]:
                wrong.append((tag, got, table[(s, tag)]["message"]))
    assert ran >= 10 and not wrong, wrong
