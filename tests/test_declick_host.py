"""De-click stage, host side (no GPU): the test-local numpy statement
(tests/declick_ref.py) reproduces every golden the reference produced, exactly;
the module's host-side surface (merge_runs, CLI flags, argument guards) holds."""
import os
import re

import numpy as np
import pytest

from tests import declick_ref as ref
from tests.golden.declick_cases import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def results():
    out = {}
    for c in CASES:
        x = ref.build_input(c)
        out[c["name"]] = (x, ref.declick(x, c["sr"], **c["params"]))
    return out


def test_case_set_covers_the_paths():
    fx = [ref.load_golden(n) for n in NAMES]
    st = [(f["meta"]["N"], int(f["hits"]), int(f["raw"]), len(f["segs"])) for f in fx]
    assert any(k >= 4 and raw - k >= 1 for _, _, raw, k in st)
    assert any(k == 0 and h > 0 for _, h, _, k in st)
    assert any(h == 0 for _, h, _, _ in st)
    assert any(n > 1 and (n - 1) % 2 == 0 for n, *_ in st)
    assert any((n - 1) % 2 == 1 for n, *_ in st)
    assert sum(os.path.getsize(os.path.join(ref.GOLDEN_DIR, n + ".npz")) for n in NAMES) < 65536


@pytest.mark.parametrize("name", NAMES)
def test_numpy_statement_reproduces_golden(results, name):
    fx = ref.load_golden(name)
    c = fx["meta"]
    x, r = results[name]
    assert ref.sha(x) == str(fx["in_sha"])
    assert ref.sha(r["y"]) == str(fx["out_sha"])
    assert r["y"].dtype == np.float32
    np.testing.assert_array_equal(r["segs"], fx["segs"])
    assert (r["raw"], r["hits"]) == (int(fx["raw"]), int(fx["hits"]))
    assert ref.f64_bits(r["sigma"]) == int(fx["sigma_bits"])
    assert ref.f64_bits(r["thr"]) == int(fx["thr_bits"])
    if r["hits"]:
        assert ref.report_text(r["segs"], c["sr"]) == str(fx["report_csv"])
    m = re.search(r"MAD-sigma=(\S+), thr=(\S+), hits=(\d+)", str(fx["stdout"]))
    assert m.group(1) == f"{r['sigma']:.6g}" and m.group(2) == f"{r['thr']:.6g}"


def test_golden_landmarks():
    fx = ref.load_golden("declick_zero")
    assert "MAD-sigma=1.48258e-12" in str(fx["stdout"]) and int(fx["hits"]) == 0
    fx = ref.load_golden("declick_square")
    assert str(fx["out_sha"]) == str(fx["in_sha"]) and int(fx["hits"]) == 30000
    fx = ref.load_golden("declick_stereo24")
    assert (int(fx["raw"]), len(fx["segs"])) == (5, 4)
    assert fx["segs"][0, 0] == 0 and fx["segs"][-1, 1] == 200001
    fx = ref.load_golden("declick_one")
    assert "MAD-sigma=nan, thr=nan, hits=0" in str(fx["stdout"])


def _mask_of(hit_idx, n, pad):
    mask = np.zeros(n, bool)
    for i in hit_idx:
        mask[max(0, i - pad):min(n, i + 1 + pad)] = True
    return mask


def test_merge_runs_matches_closed_form_cluster_rule():
    from tomatis_audio_processor_amd.declick_inpaint import merge_runs
    rng = np.random.default_rng(5)
    for trial in range(200):
        n = int(rng.integers(2, 400))
        pad, gap = int(rng.integers(0, 6)), int(rng.integers(0, 6))
        dens = rng.choice([0.0, 0.02, 0.2, 0.9, 1.0])
        hit_idx = np.flatnonzero(rng.random(n - 1) < dens)
        got = merge_runs(_mask_of(hit_idx, n, pad), gap=gap)
        want = ref.clusters(hit_idx, n, pad, gap)
        assert got.dtype == np.int64 and got.shape == want.shape, (trial, got, want)
        np.testing.assert_array_equal(got, want)
    assert merge_runs(np.zeros(7, bool)).shape == (0, 2)
    np.testing.assert_array_equal(merge_runs(np.array([1, 1, 0, 1, 0, 0, 1], bool)),
                                  [[0, 2], [3, 4], [6, 7]])
    np.testing.assert_array_equal(merge_runs(np.array([1, 1, 0, 1, 0, 0, 1], bool), gap=1),
                                  [[0, 4], [6, 7]])


def test_cli_flags_and_defaults():
    from tomatis_audio_processor_amd import declick_inpaint as dc
    a = dc.build_parser().parse_args(["-i", "in.flac", "-o", "out.flac"])
    assert vars(a) == dict(input="in.flac", output="out.flac", k=12.0, pad_ms=1.5,
                           merge_gap_ms=0.5, max_fix_ms=8.0, report_csv=None)
    a = dc.build_parser().parse_args(["--input", "a", "--output", "b", "--k", "6", "--pad_ms", "0",
                                      "--merge_gap_ms", "2", "--max_fix_ms", "4",
                                      "--report_csv", "r.csv"])
    assert (a.k, a.pad_ms, a.merge_gap_ms, a.max_fix_ms, a.report_csv) == (6.0, 0.0, 2.0, 4.0,
                                                                         "r.csv")
    with pytest.raises(SystemExit):
        dc.build_parser().parse_args(["-i", "only-input"])
    import inspect
    sig = inspect.signature(dc.declick)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[2:]] == [
        ("k", 12.0), ("pad_ms", 1.5), ("merge_gap_ms", 0.5), ("max_fix_ms", 8.0)]


def test_negative_windows_raise_before_the_gpu(tmp_path):
    from tomatis_audio_processor_amd import declick_inpaint as dc
    x = np.zeros((10, 2), np.float32)
    with pytest.raises(ValueError, match="pad_ms"):
        dc.declick(x, 48000, pad_ms=-0.1)
    with pytest.raises(ValueError, match="merge_gap_ms"):
        dc.declick(x, 48000, merge_gap_ms=-1.0)
    missing = str(tmp_path / "missing.flac")
    with pytest.raises(ValueError, match="pad_ms"):
        dc.main(["-i", missing, "-o", str(tmp_path / "o.flac"), "--pad_ms", "-1"])
    with pytest.raises(ValueError, match="merge_gap_ms"):
        dc.main(["-i", missing, "-o", str(tmp_path / "o.flac"), "--merge_gap_ms", "-1"])


def test_declick_symbols_are_bound():
    from tomatis_audio_processor_amd import _lib
    names = [n for n in _lib.EXPORTS if n.startswith("tomatis_declick_")]
    assert sorted(names) == ["tomatis_declick_dmax", "tomatis_declick_hits",
                             "tomatis_declick_inpaint", "tomatis_declick_segments",
                             "tomatis_declick_select", "tomatis_declick_work_words"]
    header = open(os.path.join(ROOT, "include", "tomatis_hip.h")).read()
    assert all(n + "(" in header for n in names)
    assert _lib.ABI_VERSION == 11
