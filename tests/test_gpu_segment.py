"""GPU: the main-segment finder (``find_main_segment`` over
``tomatis_an_frame_power_mean``) against the goldens the reference script
produced (tools/make_segment_goldens.py), from an array, a resident tensor and a
file: levels as float32 bits, noise floor and threshold as float64 bits, the
stdout of ``main()`` as text, the recorded exception where the reference raised;
and the entry point alone against ``np.mean`` per window, as bits."""
import contextlib
import io

import numpy as np
import pytest

from tests import segment_ref as sg
from tests.golden.segment_cases import SEGMENT_CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fms():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tomatis_audio_processor_amd import _lib, find_main_segment
    _lib.lib()
    yield find_main_segment
    sg.build_input.cache_clear()


def _check(r, fx):
    assert r["levels"].dtype == np.float32
    assert np.array_equal(r["levels"].view(np.uint32), fx["levels_bits"])
    assert np.float64(r["noise_floor"]).view(np.uint64) == fx["noise_floor_bits"]
    assert np.float64(r["thr"]).view(np.uint64) == fx["thr_bits"]
    first = str(fx["stdout"])[:3]
    assert r["status"] == {"===": "ok", "未找到": "none", "最长段": "short"}[first]


@pytest.mark.parametrize("case", SEGMENT_CASES, ids=lambda c: c["name"])
def test_against_reference(fms, case, tmp_path):
    import torch
    from tomatis_audio_processor_amd import audio_io
    fx = sg.fixture(case["name"])
    x, sr, p = sg.build_input(case["name"]), case["sr"], case["params"]
    path = str(tmp_path / "in.flac")
    audio_io.write(path, x, sr)
    exc = str(fx["exc_type"])
    if exc:
        for src, rate in ((x, sr), (torch.from_numpy(np.array(x)).cuda(), sr), (path, None)):
            with pytest.raises(Exception) as ei:
                fms.find_main_segment(src, rate, **p)
            assert type(ei.value).__name__ == exc and str(ei.value) == str(fx["exc_text"])
        with pytest.raises(Exception) as ei:
            fms.main(["-i", path] + sg.cli_args(p))
        assert type(ei.value).__name__ == exc and str(ei.value) == str(fx["exc_text"])
        return
    _check(fms.find_main_segment(x, sr, **p), fx)
    _check(fms.find_main_segment(torch.from_numpy(np.array(x)).cuda(), sr, **p), fx)
    r = fms.find_main_segment(path, **p)
    _check(r, fx)
    assert r["sr"] == sr and r["dur"] == len(x) / sr
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        fms.main(["-i", path] + sg.cli_args(p))
    assert buf.getvalue() == str(fx["stdout"])


WINS = [1, 7, 8, 9, 128, 129, 2205, 4410, 4800, 65536]


@pytest.mark.parametrize("win", WINS)
def test_frame_power_mean_is_np_mean(fms, win):
    import torch
    n = 3 * win + 5
    rng = np.random.default_rng(300 + win)
    x = (rng.uniform(-1.0, 1.0, (n, 2)) * 0.7).astype(np.float32)
    xd = torch.from_numpy(x).cuda().reshape(-1)
    for hop in sorted({1, max(1, win // 2), win, win + 3}):
        if win > 4800 and hop == 1:
            hop = 7919          # a few windows at odd offsets, not 131 078 of them
        got = fms.frame_power_mean(xd, n, win, hop).cpu().numpy()
        starts = range(0, n - win + 1, hop)
        assert got.shape == (len(starts),) == (1 + (n - win) // hop,)
        want = np.empty(len(starts), np.float32)
        for f, s in enumerate(starts):
            w = x[s:s + win]
            p = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) * 0.5
            want[f] = np.mean(p)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (win, hop)


def test_frame_power_mean_guards(fms):
    import torch
    from tomatis_audio_processor_amd import _lib
    L, hs, p = _lib.lib(), _lib.stream_handle(), _lib.ptr
    x = torch.zeros(200, dtype=torch.float32, device="cuda")
    out = torch.full((100,), 5.0, dtype=torch.float32, device="cuda")
    assert L.tomatis_an_frame_power_mean(p(x), 100, 0, 1, p(out), hs) == _lib.E_ARG
    assert L.tomatis_an_frame_power_mean(p(x), 100, 10, 0, p(out), hs) == _lib.E_ARG
    assert L.tomatis_an_frame_power_mean(None, 100, 10, 5, p(out), hs) == _lib.E_ARG
    assert L.tomatis_an_frame_power_mean(p(x), 100, 65537, 5, p(out), hs) == _lib.E_UNSUPPORTED
    assert L.tomatis_an_frame_power_mean(p(x), 9, 10, 5, p(out), hs) == 0    # no window fits
    assert L.tomatis_an_frame_power_mean(p(x), 100, 10, 5, p(out), hs) == 0
    got = out.cpu().numpy()
    assert not np.any(got[:19]) and np.all(got[19:] == 5.0)
    assert fms.frame_power_mean(x, 9, 10, 5).numel() == 0
    with pytest.raises(ValueError):
        fms.frame_power_mean(x, 100, 65537, 5)
