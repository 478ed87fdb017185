"""Every refusing path of the C ABI layer keeps its return code, its message and its precedence: the table of tests/abi_refusals.py
against the one recorded from the library before the layer was split into files (no device is reached: runs anywhere)."""
import json
import os

import abi_refusals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_refusals_match_the_recorded_table():
    with open(os.path.join(ROOT, "tests", "golden", "abi_refusals.json")) as f:
        want = json.load(f)
    got = abi_refusals.collect()
    assert len(want) >= 730
    for g, w in zip(got, want):
        assert g == w      # (the first difference, readably)
    assert len(got) == len(want)
