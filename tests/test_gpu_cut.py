"""GPU: ``cut_tomatis_d.cut_audio`` file to file.

* The two cut goldens (tools/make_segment_goldens.py): the decoded output file
  holds the PCM_24 quantisation of the array the reference wrote, as integers,
  and the prints are the reference's.
* A 24-bit FLAC cut with no resample is lossless.  The inputs are PCM_24 values
  k / 2^23 with |k| < 2^22 (tests/segment_ref.build_input): libsndfile's
  float -> int rule rint(x (2^23 - 1)) = rint(k - k / 2^23) returns k exactly
  there, so the integers of the output are the integers of ``input[cut:]``.
* ``duration_seconds`` and ``target_sr``: 44.1 kHz stereo, cut 0.25 s, keep
  0.5 s, to 48 kHz: 24 000 frames, the integers of ``fileio.requantize_device``
  of ``resample_to`` over the same range.
* The three ``sys.argv`` forms and the two extra positionals.
"""
import contextlib
import io
import os

import numpy as np
import pytest

from tests import segment_ref as sg
from tests.golden.segment_cases import CUT_CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cut():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tomatis_audio_processor_amd import _lib, cut_tomatis_d
    _lib.lib()
    yield cut_tomatis_d
    sg.build_input.cache_clear()


def _ints(path):
    from tomatis_audio_processor_amd import audio_io
    with open(path, "rb") as f:
        pcm, sr, bps = audio_io.flac_decode_int(f.read())
    assert bps == 24
    return pcm, sr


def _run(fn, *a, **k):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        fn(*a, **k)
    return buf.getvalue()


@pytest.mark.parametrize("case", CUT_CASES, ids=lambda c: c["name"])
def test_cut_goldens(cut, case, tmp_path):
    from tomatis_audio_processor_amd import audio_io
    fx = sg.fixture(case["name"])
    x, sr = sg.build_input(case["name"]), case["sr"]
    inp, out = str(tmp_path / "in.flac"), str(tmp_path / "out.flac")
    audio_io.write(inp, x, sr)
    args = (inp, out) if case["cut_seconds"] is None else (inp, out, case["cut_seconds"])
    text = _run(cut.cut_audio, *args)
    assert text == str(fx["stdout"]).replace("{in}", inp).replace("{out}", out)
    # the array the reference wrote is x[cut:] (its hash is the fixture's)
    secs = 16.0 if case["cut_seconds"] is None else case["cut_seconds"]
    y = x[int(secs * sr):]
    assert sg.sha(y if x.shape[1] > 1 else y[:, 0]) == str(fx["out_sha"])
    assert len(y) == int(fx["out_len"])
    pcm, got_sr = _ints(out)
    assert got_sr == sr and np.array_equal(pcm, sg.pcm24(y))
    # lossless: the integers of the input file past the cut
    src, _ = _ints(inp)
    assert np.array_equal(pcm, src[int(secs * sr):])


def test_cut_keep_and_resample(cut, tmp_path):
    import torch
    from tomatis_audio_processor_amd import audio_io, fileio, resample
    sr = 44100
    x = sg.build_input("seg_44k_pad0")[:sr]          # one second, stereo
    inp, out = str(tmp_path / "in.flac"), str(tmp_path / "out.flac")
    audio_io.write(inp, x, sr)
    text = _run(cut.cut_audio, inp, out, cut_seconds=0.25, duration_seconds=0.5, target_sr=48000)
    base = _run(cut.cut_audio, inp, str(tmp_path / "plain.flac"), cut_seconds=0.25)
    assert len(text.splitlines()) == len(base.splitlines()) + 2     # one extra line each
    assert "22050" in text and "48000 Hz" in text and "24000" in text
    pcm, got_sr = _ints(out)
    assert got_sr == 48000 and pcm.shape == (24000, 2)
    y = resample.resample_to(x, sr, 48000, start=11025, stop=33075)
    assert y.shape == (24000, 2)
    q = fileio.requantize_device(y.reshape(-1), 24000, 2).cpu().numpy().reshape(24000, 2)
    assert np.array_equal(pcm, np.rint(q.astype(np.float64) * 2.0 ** 23).astype(np.int32))
    # the resident path saw the frames around the range; the result is that of the range alone
    alone = resample.resample_poly(np.ascontiguousarray(x[11025:33075]), 160, 147)
    assert torch.equal(y, alone)
    # duration alone, running past the end of the file: what is left
    _run(cut.cut_audio, inp, out, cut_seconds=0.75, duration_seconds=5.0)
    pcm, got_sr = _ints(out)
    src, _ = _ints(inp)
    assert got_sr == sr and np.array_equal(pcm, src[33075:])


def test_resampler_overshoot_clips(cut, tmp_path):
    from tomatis_audio_processor_amd import audio_io
    # a full-scale square wave at 8 kHz rings above full scale when resampled
    sr = 8000
    x = np.where((np.arange(4000) // 7) % 2 == 0, 1.0, -1.0).astype(np.float32)
    x = np.stack([x, -x], axis=1)
    inp, out = str(tmp_path / "in.flac"), str(tmp_path / "out.flac")
    audio_io.write(inp, x, sr)
    _run(cut.cut_audio, inp, out, cut_seconds=0.0, target_sr=48000)
    pcm, got_sr = _ints(out)
    assert got_sr == 48000 and pcm.shape == (24000, 2)
    assert pcm.max() == 2 ** 23 - 1 and pcm.min() == -2 ** 23


def test_argv_forms(cut, tmp_path, monkeypatch):
    from tomatis_audio_processor_amd import audio_io
    sr = 48000
    x = sg.build_input("cut_48k_st")
    calls = []
    monkeypatch.setattr(cut, "cut_audio", lambda *a: calls.append(a))
    cut.main(["cut_tomatis_d.py"])
    cut.main(["cut_tomatis_d.py", "a.flac"])
    cut.main(["cut_tomatis_d.py", "a.flac", "b.flac"])
    cut.main(["cut_tomatis_d.py", "a.flac", "b.flac", "1.5"])
    cut.main(["cut_tomatis_d.py", "a.flac", "b.flac", "16.8", "1800", "48000"])
    assert calls == [("Tomatis_D.flac", "Tomatis_D_cut16s.flac", 16.0, None, None),
                     ("a.flac", "a_cut16s.flac", 16.0, None, None),
                     ("a.flac", "b.flac", 16.0, None, None),
                     ("a.flac", "b.flac", 1.5, None, None),
                     ("a.flac", "b.flac", 16.8, 1800.0, 48000)]
    monkeypatch.undo()
    # and one of them for real: the third form with a cut
    inp, out = str(tmp_path / "in.flac"), str(tmp_path / "out.flac")
    audio_io.write(inp, x, sr)
    _run(cut.main, ["cut_tomatis_d.py", inp, out, "1.3"])
    pcm, _ = _ints(out)
    assert np.array_equal(pcm, sg.pcm24(x[62400:]))
    assert os.path.exists(out)
