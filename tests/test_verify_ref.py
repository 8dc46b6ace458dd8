"""CPU: the numpy statement of the two acceptance validators (tests/verify_ref.py)
against the fixtures recorded from the reference's own ``main`` runs
(tests/golden/verify_*.npz, tools/make_verify_goldens.py), and the host side of
the device modules: header, binding, argparse defaults."""
import json
import os
import re

import numpy as np
import pytest

from tests import verify_ref as vr
from tests.golden import verify_cases as vc
from tests.golden_util import load_fixture, sha

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["tomatis_an_anchored_ratio", "tomatis_an_pair_band_energy", "tomatis_an_verify_pair",
       "tomatis_sum_f64"]


def _inputs(c, fx):
    x, y, rows = vc.make_pair(c)
    assert sha(x) == str(fx["x_sha"]), "the regenerated input differs from the fixture's"
    assert len(y) == int(fx["y_len"])
    d = np.abs(y[::vc.DECIM].astype(np.float64) - fx["y_dec"].astype(np.float64))
    assert float(d.max(initial=0)) <= 1e-6, "the regenerated output differs from the fixture's"
    return x, y, rows


@pytest.mark.parametrize("name", [c["name"] for c in vc.V2_CASES])
def test_v2_statement_equals_fixture(name):
    c, fx = vc.BY_NAME[name], load_fixture(name)
    x, y, _ = _inputs(c, fx)
    R = vr.run_v2(x, y, vc.SR, vc.v2_args(c))
    assert sha(R["levels"]) == str(fx["levels_sha"]) and len(R["levels"]) == int(fx["n_levels"])
    assert R["T"] == float(fx["T"]) and R["ratio"] == float(fx["ratio"])
    assert vr.state_sha(R["codes"]) == str(fx["state_sha"])
    assert R["switch_count"] == int(fx["switch_count"])
    assert [len(v) for v in vr.stable(R["codes"])] == fx["stable"].tolist()
    assert [R["c1_n"], R["c2_n"]] == fx["used"].tolist()
    assert np.float32(R["peak"]).view(np.uint32) == fx["peak_bits"]
    keys = ("input", "output", "c1", "c2")
    assert [len(R["ti_data"][k]) for k in keys] == fx["ti_n"].tolist()
    # every verdict word and printed number of the report, and the exit code
    assert vr.report_v2(R) == str(fx["report"])
    assert int(not R["ok"]) == int(fx["exit_code"])
    assert np.array_equal(vr.csv_columns(R).astype(np.float32), fx["cols"])


def _l1_words(text):
    return re.findall(r"^  (工程检查|Gate复算|条件频谱): (PASS|FAIL)$", text, flags=re.M)


@pytest.mark.parametrize("name", [c["name"] for c in vc.L1_CASES])
def test_l1_statement_equals_fixture(name):
    c, fx = vc.BY_NAME[name], load_fixture(name)
    x, y, rows = _inputs(c, fx)
    R = vr.run_l1(x, y, vc.SR, rows, vc.l1_args(c))
    assert sha(R["levels"]) == str(fx["levels_sha"])
    assert vr.state_sha(R["sim"]) == str(fx["state_sha"])
    assert (R["mismatch"], R["total"], R["csv_switches"], R["sim_switches"]) == \
        (int(fx["mismatch"]), int(fx["total"]), int(fx["csv_switches"]), int(fx["sim_switches"]))
    assert R["level_max_diff"] == float(fx["level_max_diff"])
    assert [R["c1_n"], R["c2_n"]] == fx["used"].tolist()
    assert np.float32(R["peak"]).view(np.uint32) == fx["peak_bits"]
    w = lambda b: "PASS" if b else "FAIL"  # noqa: E731
    assert _l1_words(str(fx["stdout"])) == [("工程检查", w(R["eng_pass"])),
                                            ("Gate复算", w(R["gate_ok"])),
                                            ("条件频谱", w(R["spectrum_ok"]))]
    assert int(not R["ok"]) == int(fx["exit_code"])
    assert np.array_equal(vr.csv_columns(R).astype(np.float32), fx["cols"])


def test_fixture_verdicts_are_the_issues():
    """PASS on the three shapes for both validators; the failing cases fail on
    the line they were built to fail; every verdict is ten tolerances clear."""
    want = {"verify_v2_st_4096": 0, "verify_v2_mono_2048": 0, "verify_v2_st_3000": 0,
            "verify_v2_dc": 1, "verify_v2_short": 1, "verify_v2_silent": 1,
            "verify_v2_delay100": 0, "verify_v2_loud": 1, "verify_l1_st_4096": 0,
            "verify_l1_mono_2048": 0, "verify_l1_st_3000": 0, "verify_l1_3db": 1,
            "verify_l1_delayed": 1}
    for name, rc in want.items():
        fx = load_fixture(name)
        assert int(fx["exit_code"]) == rc, name
        for k, (v, thr, tol) in zip(json.loads(str(fx["margin_keys"])), fx["margins"].tolist()):
            assert abs(v - thr) >= 10 * tol and v != thr, (name, k)
    out = {n: str(load_fixture(n)["stdout"]) for n in want}
    assert re.search(r"DC偏移: 0\.00\d+ FAIL", out["verify_v2_dc"])
    assert "(diff=-1) FAIL" in out["verify_v2_short"]
    assert "最优阈值 T: -120.00 dBFS" in out["verify_v2_silent"]
    assert "有效帧: C1=277, C2=0" in out["verify_v2_silent"]
    assert re.search(r"峰值: 0\.99\d+ \(-0\.0\d dBFS\) FAIL", out["verify_v2_loud"])
    assert "Gate复算: FAIL" in out["verify_l1_delayed"]
    assert "条件频谱: FAIL" in out["verify_l1_3db"]
    assert "Layer1 验证: PASS" in out["verify_l1_st_4096"]
    assert "验证结果: PASS" in out["verify_v2_st_4096"]


# ---------------------------------------------------------------------------
# header, binding, modules
# ---------------------------------------------------------------------------

def test_new_entry_points_are_declared_and_bound():
    from tomatis_audio_processor_amd import _lib
    src = open(os.path.join(ROOT, "include", "tomatis_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(tomatis_[a-z0-9_]+)\s*\(", code))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and name in _lib._SIGS
    assert set(_lib.EXPORTS) == declared
    defs = dict(re.findall(r"#define (TOMATIS_[A-Z0-9_]+) \(?(-?\d+)u?\)?", src))
    assert int(defs["TOMATIS_ABI_VERSION"]) == _lib.ABI_VERSION == 11
    assert int(defs["TOMATIS_SUM_DOUBLES"]) == _lib.SUM_DOUBLES == 1025
    # every entry point cites the reference lines it replaces
    for cite in ("verify_tomatis_15db_v2.py:307-354", "verify_tomatis_15db_v2.py:451-470",
                 "verify_tomatis_15db_v2.py:90"):
        assert cite in src, cite
    assert len(_lib._SIGS["tomatis_an_anchored_ratio"][1]) == 11
    assert len(_lib._SIGS["tomatis_an_pair_band_energy"][1]) == 13
    assert len(_lib._SIGS["tomatis_an_verify_pair"][1]) == 16
    assert len(_lib._SIGS["tomatis_sum_f64"][1]) == 4


def test_library_exports_the_new_symbols():
    import ctypes
    from tomatis_audio_processor_amd import _lib
    path = _lib.lib_path()
    if not os.path.exists(path):
        pytest.fail(f"{path} missing: run __graft_entry__.build() first")
    h = ctypes.CDLL(path)
    assert all(hasattr(h, n) for n in NEW)
    assert h.tomatis_abi_version() == 11


def _defaults(parser):
    return {a.dest: a.default for a in parser._actions
            if a.dest not in ("help", "input", "output", "state_csv")}


def test_modules_import_without_a_gpu_and_keep_the_reference_defaults():
    from tomatis_audio_processor_amd import validate_layer1 as l1
    from tomatis_audio_processor_amd import verify_tomatis_15db_v2 as v2
    assert _defaults(v2.build_parser()) == vc.V2_DEFAULTS
    assert _defaults(l1.build_parser()) == vc.L1_DEFAULTS
    for a, b in ((_defaults(v2.build_parser()), vc.V2_DEFAULTS),
                 (_defaults(l1.build_parser()), vc.L1_DEFAULTS)):
        assert {k: type(v) for k, v in a.items()} == {k: type(v) for k, v in b.items()}
    for name in ("check_engineering", "compute_frame_levels", "simulate_gate_with_threshold",
                 "find_optimal_threshold", "analyze_gate_stats", "compute_conditional_spectrum_v2",
                 "compute_spectrum_metrics_v2", "compute_tilt_index", "analyze_tilt_index",
                 "verify", "main", "find_stable_frames", "build_tilt_gain_db"):
        assert callable(getattr(v2, name)), name
    for name in ("check_engineering", "load_state_csv", "simulate_gate", "compare_gate_states",
                 "analyze_gate_stats", "compute_spectrum_rmse", "main", "find_stable_frames",
                 "compute_conditional_spectrum", "build_tilt_gain_db"):
        assert callable(getattr(l1, name)), name
    required = {a.dest for a in l1.build_parser()._actions if a.required}
    assert required == {"input", "output", "state_csv"}


def test_host_statistics_match_the_statement():
    """The per-frame list logic the modules keep on the host, on a crafted state
    sequence: run lengths, switches, stable classes, the float32 thresholds."""
    from tomatis_audio_processor_amd import analysis
    from tomatis_audio_processor_amd import validate_layer1 as l1
    from tomatis_audio_processor_amd import verify_tomatis_15db_v2 as v2
    rng = np.random.default_rng(5)
    codes = np.repeat(rng.integers(1, 3, 60), rng.integers(1, 7, 60)).astype(np.int8)
    names = analysis.state_names(codes)
    assert np.array_equal(analysis.state_codes(names), codes)
    levels = rng.normal(-40, 8, len(codes)).astype(np.float32).astype(np.float64)
    s = v2.analyze_gate_stats(names, levels, 48000, 2048)
    runs = vr.run_lengths(codes)
    assert s["switch_count"] == vr.switches(codes) == len(runs) - 1
    assert (s["run_min"], s["run_max"], s["short_runs"]) == \
        (runs.min(), runs.max(), int(np.count_nonzero(runs <= 3)))
    assert s["c2_count"] == int(np.count_nonzero(codes == 2))
    assert s["c1_level_mean"] == np.mean(levels[codes == 1])
    s1 = l1.analyze_gate_stats(names)
    assert s1["run_count"] == len(runs) and s1["run_median"] == np.median(runs)
    c1, c2 = vr.stable(codes)
    cls = analysis.stable_classes(codes)
    assert np.array_equal(np.nonzero(cls == 1)[0], c1) and np.array_equal(np.nonzero(cls == 2)[0], c2)
    assert analysis.find_stable_frames(names) == (c1.tolist(), c2.tolist())
    cmp = l1.compare_gate_states(names, names[3:] + names[:3], levels, levels + 0.05)
    assert cmp["mismatch_count"] == int(np.count_nonzero(codes != np.roll(codes, -3)))
    assert abs(cmp["level_max_diff"] - 0.05) < 1e-12
    # the smallest float32 >= Ton and the largest <= Toff decide as float64 does
    for T in (-34.94140625, -40.0 + 1e-9, -39.98, 0.1):
        up, dn = analysis._f32_at_least(T), analysis._f32_at_most(T)
        assert float(up) >= T >= float(dn)
        assert float(np.nextafter(up, np.float32(-np.inf))) < T or float(up) == T
        assert float(np.nextafter(dn, np.float32(np.inf))) > T or float(dn) == T
