"""The effect kinds' front end without a GPU, byte for byte against tests/golden/fx_front_end.json: the dumped line of a
mid-range script line, the last_error() of script lines with one fault each (and of a few with several), and the TermdawError of
the same value faults through Graph.add_<kind> and <kind>_params -- for every one of the thirteen kinds.  The file was recorded
by tests/golden/make_fx_front_end.py on the parent of the commit that declares a kind's parameters once (csrc/fx_params.h); the
lines and faults are that generator's tables."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_fx_front_end as M  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(M.PATH))["kinds"]


@pytest.fixture(scope="module")
def now(api):
    return M.front_end(api)


def test_the_record_holds_every_kind_and_every_fault(recorded):
    assert list(M.KINDS) == ["add_compressor", "add_eq", "add_delay", "add_saturator", "add_chorus", "add_reverb", "add_gate", "add_phaser",
                             "add_vocoder", "add_filter", "add_limiter", "add_multiband", "add_convolution"]
    assert sorted(recorded) == sorted(M.KINDS)
    for call in M.KINDS:
        f = M.faults(call)
        assert sorted(recorded[call]["script"]) == sorted(label for label, _, _ in f), call
        assert sorted(recorded[call]["graph"]) == sorted(label for label, _, value in f if value), call
        assert sorted(recorded[call]["params"]) == (sorted(recorded[call]["graph"]) if call in M.PARAMS else []), call
        for n, t, _, lo, hi in M.KINDS[call]:   # every parameter has a fault of its own
            assert t == M.S or any(label.startswith(n + " ") for label in recorded[call]["script"]), (call, n)


@pytest.mark.parametrize("call", list(M.KINDS))
def test_the_front_end_says_what_it_said(recorded, now, call):
    want, got = recorded[call], now[call]
    assert got["dump"] == want["dump"] and got["replay"] == want["replay"] and got["passes"] == want["passes"]
    for path in ("script", "graph", "params"):
        for label in want[path]:
            assert got[path][label] == want[path][label], (call, path, label)
        assert sorted(got[path]) == sorted(want[path])
