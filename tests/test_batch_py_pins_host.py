"""The host behaviour of gpscore.batch's wrappers and gpscore.experiment's run_*_batch runners
against tests/golden/batch_py_pins.json (no GPU, no library call): every refusal's class
and full message, which of two broken checks reports, the entry name and every slot of a
well-formed call, where each returned array comes from, the order in which the runners consume
their generator, and what they return or raise for failed replicates.  The fixture was written by
tests/golden/make_batch_py_pins.py before the Python layer was folded; this replays the same
list."""
import json
import os
import sys

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import make_batch_py_pins as M  # noqa: E402


def test_batch_python_layer_matches_the_pins():
    with open(os.path.join(GOLDEN, "batch_py_pins.json")) as f:
        text = f.read()
    want = json.loads(text)
    got = json.loads(M.dumps(M.collect()))
    assert set(got) == set(want)
    for part in sorted(want):
        if isinstance(want[part], list) and want[part] and isinstance(want[part][0], dict):
            assert len(got[part]) == len(want[part]), part
            for g, w in zip(got[part], want[part]):
                assert g == w, (part, w.get("call"), w.get("case"))
        else:
            assert got[part] == want[part], part
    assert M.dumps(M.collect()) == text  # and the generator rewrites the file byte for byte
    # the refusals cover every wrapper and runner, and nothing reached the library
    calls = {r["call"] for r in want["wrapper_refusals"]}
    assert calls == set(M.WRAPPERS)
    assert {r["call"] for r in want["runner_refusals"]} == set(M.RUNNERS)
    assert all(r["calls"] == 0 for r in want["wrapper_refusals"] if r["type"] is not None)
    assert all(r["calls"] == 0 for r in want["runner_refusals"])
