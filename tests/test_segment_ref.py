"""CPU: the numpy statement of the main-segment finder and the cut
(tests/segment_ref.py) against the goldens the reference scripts produced
(tools/make_segment_goldens.py): levels as float32 bits, noise floor and
threshold as float64 bits, stdout as text, the exceptions, the written array."""
import json

import numpy as np
import pytest

from tests import segment_ref as sg
from tests.golden.segment_cases import CUT_CASES, SEGMENT_CASES


@pytest.mark.parametrize("case", SEGMENT_CASES, ids=lambda c: c["name"])
def test_statement_matches_reference(case):
    fx = sg.fixture(case["name"])
    assert json.loads(str(fx["meta"])) == json.loads(json.dumps(case))
    x = sg.build_input(case["name"])
    assert sg.sha(x) == str(fx["in_sha"])
    exc = str(fx["exc_type"])
    if exc:
        with pytest.raises(Exception) as ei:
            sg.statement(x, case["sr"], **case["params"])
        assert type(ei.value).__name__ == exc and str(ei.value) == str(fx["exc_text"])
        return
    r = sg.statement(x, case["sr"], **case["params"])
    assert np.array_equal(r["levels"].view(np.uint32), fx["levels_bits"])
    assert np.float64(r["noise_floor"]).view(np.uint64) == fx["noise_floor_bits"]
    assert np.float64(r["thr"]).view(np.uint64) == fx["thr_bits"]
    assert r["stdout"] == str(fx["stdout"])


def test_cases_cover_the_branches():
    out = {c["name"]: str(sg.fixture(c["name"])["stdout"]) for c in SEGMENT_CASES}
    assert sum(o.startswith("====") for o in out.values()) == 4
    assert sum(o.startswith("未找到") for o in out.values()) == 1
    assert sum(o.startswith("最长段只有") for o in out.values()) == 1
    assert sum(o == "" for o in out.values()) == 2
    assert "start=0.000s" in out["seg_44k_pad0"] and "end=6.000s" in out["seg_44k_odd_end"]
    # window lengths: 4800 / 2400, 4410 / 2205, 12000 / 6000, 1653 / 551
    wins = {(int(c["sr"] * c["params"].get("win_ms", 100.0) / 1000.0),
             int(c["sr"] * c["params"].get("hop_ms", 50.0) / 1000.0)) for c in SEGMENT_CASES}
    assert wins == {(4800, 2400), (4410, 2205), (12000, 6000), (1653, 551)}


@pytest.mark.parametrize("case", CUT_CASES, ids=lambda c: c["name"])
def test_cut_statement_matches_reference(case):
    fx = sg.fixture(case["name"])
    x = sg.build_input(case["name"])
    assert sg.sha(x) == str(fx["in_sha"])
    secs = 16.0 if case["cut_seconds"] is None else case["cut_seconds"]
    y, text = sg.cut_statement(x, case["sr"], secs)
    assert len(y) == int(fx["out_len"])
    # the script hands libsndfile a 1-D array for a mono file: the same bytes
    assert sg.sha(y) == str(fx["out_sha"])
    assert text == str(fx["stdout"])
    # the inputs are PCM_24 values below half scale: the file round trip is lossless
    k = x.astype(np.float64) * 2.0 ** 23
    assert np.array_equal(k, np.rint(k)) and np.max(np.abs(k)) < 2 ** 22
    assert np.array_equal(sg.pcm24(x), k.astype(np.int32))
