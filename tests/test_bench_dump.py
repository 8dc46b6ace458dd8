"""CPU: bench.py's --dump-outputs writer (dump_outputs / _dump_array) on host
tensors: float32 .npy files named after the arrays, small arrays whole, large
ones as the same seeded sample in every call, chunk peaks as the floats their
bits encode."""
import os

import numpy as np
import pytest

import bench


def _result(torch, n_y, n_frames, n_chunks, seed):
    from tomatis_audio_processor_amd.engine import Result
    g = torch.Generator().manual_seed(seed)
    y = torch.rand(n_y, generator=g, dtype=torch.float32) - 0.5
    states = torch.randint(0, 3, (n_frames,), generator=g, dtype=torch.uint8)
    pk = torch.rand(n_chunks, generator=g, dtype=torch.float32)
    return Result(y=y, out_offs=[0], out_lens=[n_y // 2], ch=2, frame_base=[0],
                  n_frames=[n_frames], first_start=[0], hop=512, states=states,
                  chunk_peaks=pk.view(torch.int32), chunk_base=[0], n_chunks=[n_chunks]), pk


def test_dump_outputs_whole_arrays(tmp_path):
    torch = pytest.importorskip("torch")
    res, pk = _result(torch, 4096, 37, 5, 1)
    d = str(tmp_path / "out")
    bench.dump_outputs(d, res)
    assert sorted(os.listdir(d)) == ["chunk_peaks.npy", "states.npy", "y.npy"]
    y, st, p = (np.load(os.path.join(d, f + ".npy")) for f in ("y", "states", "chunk_peaks"))
    assert y.dtype == st.dtype == p.dtype == np.float32
    assert y.tobytes() == res.y.numpy().tobytes()
    assert np.array_equal(st, res.states.numpy().astype(np.float32))
    assert p.tobytes() == pk.numpy().tobytes()


def test_dump_outputs_samples_large_arrays(tmp_path, monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(bench, "DUMP_MAX_SAMPLES", 1000)
    monkeypatch.setattr(bench, "DUMP_MAX_FRAMES", 100)
    res, _ = _result(torch, 50000, 3000, 7, 2)
    res2, _ = _result(torch, 50000, 3000, 7, 2)
    bench.dump_outputs(str(tmp_path / "a"), res, stage2=res2)
    bench.dump_outputs(str(tmp_path / "b"), res2, stage2=res)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["chunk_peaks.npy", "chunk_peaks_stage2.npy", "states.npy", "y.npy",
                     "y_stage2.npy"]
    for f in names:  # same inputs -> same files
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes()
    y = np.load(tmp_path / "a" / "y.npy")
    assert y.shape == (1000,) and np.load(tmp_path / "a" / "states.npy").shape == (100,)
    idx = np.sort(np.random.default_rng(1).integers(0, 50000, 1000, dtype=np.int64))
    assert y.tobytes() == res.y.numpy()[idx].tobytes()
    assert np.load(tmp_path / "a" / "chunk_peaks.npy").shape == (7,)


def test_dump_caps_stay_under_64_mb():
    assert 4 * (2 * bench.DUMP_MAX_SAMPLES + 3 * bench.DUMP_MAX_FRAMES) <= 64 * 10 ** 6
