"""Parameter recovery on the device: the per-frame dB
difference rows of k_an_pair_tilt against the float64 statement, its band means
and k_an_pair_diff_mean's frame means against the device's own rows, and the two
host mirrors (reverse_engineer_params, verify_tilt_amplitude) against fixtures
recorded from the reference's own scripts (tools/make_reverse_goldens.py).

Tolerances.  Rows and tilts: the project's rule, err <= 8 * max(e32, floor) with
e32 the float32 numpy statement's own error on the same input and the floor one
float32 ulp of the logarithm's argument in dB (20 / ln 10 * 2^-23); absolute, in
dB, over the bins whose |A| and |B| reach 1e-4 of their frame's largest (a power
mono's DC bin dominates its spectrum), at most 1e-3 of all bins left out.  Band
means against the returned rows: 1e-9 dB, a bound on the rounding of a float64
sum of <= 8193 values below 400 (4e-10).  Frame means against the returned
rows: bit for bit in the documented order.  Fixtures: integers and levels
exactly, tilts and printed dB values within one unit of their last digit."""
import contextlib
import functools
import io
import re

import numpy as np
import pytest

from tests import reverse_ref as rr
from tests.golden import reverse_cases as rc
from tests.golden import verify_cases as vc
from tests.golden_util import load_fixture, sha

pytestmark = pytest.mark.gpu
SR = 48000


def _mods():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tomatis_audio_processor_amd import analysis, reverse_engineer_params, verify_tilt_amplitude
    return torch, analysis, reverse_engineer_params, verify_tilt_amplitude


# name -> (n_fft, hop, n)
SHAPES = {
    "256_64": (256, 64, 256 + 64 * 40 + 5),          # one-bin low band, F = 41
    "64_16": (64, 16, 64 + 16 * 36 + 3),             # no low-band bin at 48 kHz
    "3000_750": (3000, 750, 4 * SR + 7),             # Bluestein
    "4096_2048": (4096, 2048, 4 * SR + 11),          # the two scripts' own framing
    "16384_4096": (16384, 4096, 4 * SR),             # the LDS ceiling, 33 bins per thread
    "one_frame": (4096, 2048, 4096 + 100),           # F = 1
}


@functools.lru_cache(maxsize=None)
def _signal(n):
    """x: enveloped noise (verify_cases "env", seed 311, stereo); y: x through a
    first difference, so that the rows are far from flat.  Read-only."""
    x = np.ascontiguousarray(vc.make_x(dict(x="env", seed=311, ch=2))[:n])
    y = x.copy()
    y[1:] -= np.float32(0.9) * x[:-1]
    for a in (x, y):
        a.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def _statement(shape):
    """The float64 and float32 statements of a shape, computed once."""
    n_fft, hop, n = SHAPES[shape]
    x, y = _signal(n)
    d64, A64, B64 = rr.diff_rows(x, y, n_fft, hop, np.float64)
    d32, _, _ = rr.diff_rows(x, y, n_fft, hop, np.float32)
    for a in (d64, A64, B64, d32):
        a.setflags(write=False)
    return d64, A64, B64, d32


def _bands(n_fft):
    freqs = np.fft.rfftfreq(n_fft, 1 / SR)
    return rr.band_range(freqs, 200, 500), rr.band_range(freqs, 2000, 6000)


@functools.lru_cache(maxsize=None)
def _device(shape):
    """(band means [F, 2] float64, rows [F, nb] float32) of a shape as numpy,
    with the resident pair; one launch shared by the tests below."""
    torch, A, _, _ = _mods()
    n_fft, hop, n = SHAPES[shape]
    x, y = _signal(n)
    xd, yd = A.pair_on_device(x.copy(), y.copy(), 0)
    lo, hi = _bands(n_fft)
    means, rows = A.pair_tilt(xd, yd, n_fft, hop, lo, hi, want_rows=True)
    torch.cuda.synchronize()
    return xd, yd, means, rows


# ---------------------------------------------------------------------------
# 1. rows against float64
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(SHAPES))
def test_rows_against_float64(shape):
    n_fft, hop, n = SHAPES[shape]
    d64, A64, B64, d32 = _statement(shape)
    _, _, _, rows = _device(shape)
    F = rr.n_frames(n, n_fft, hop)
    assert tuple(rows.shape) == (F, n_fft // 2 + 1) == d64.shape
    if shape == "one_frame":
        assert F == 1
    rows = rows.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(rows))
    ok = (A64 >= 1e-4 * A64.max(axis=1, keepdims=True)) & \
         (B64 >= 1e-4 * B64.max(axis=1, keepdims=True))
    assert np.count_nonzero(~ok) <= 1e-3 * ok.size, np.count_nonzero(~ok)
    e32 = float(np.max(np.abs(d32.astype(np.float64) - d64)[ok]))
    err = float(np.max(np.abs(rows - d64)[ok]))
    # the two real bins on their own: the float64 sums keep them at the floor
    real = [0] + ([n_fft // 2] if n_fft % 2 == 0 else [])
    err_real = float(np.max(np.abs(rows - d64)[:, real]))
    print(f"{shape}: rows err {err:.2e} dB, e32 {e32:.2e} dB, real bins {err_real:.2e} dB, "
          f"left out {np.count_nonzero(~ok)}/{ok.size}")
    assert err <= rr.rule_bound_db(e32), (err, e32)


# ---------------------------------------------------------------------------
# 2. band means against the device's own rows
# ---------------------------------------------------------------------------

def _row_means(rows, r):
    with np.errstate(invalid="ignore", divide="ignore"):
        return rows[:, r[0]:r[1]].astype(np.float64).sum(axis=1) / (r[1] - r[0])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_band_means_against_the_rows(shape):
    torch, A, _, _ = _mods()
    n_fft, hop, n = SHAPES[shape]
    lo, hi = _bands(n_fft)
    if shape == "256_64":
        assert lo[1] - lo[0] == 1
    xd, yd, means, rows = _device(shape)
    means2, rows2 = A.pair_tilt(xd, yd, n_fft, hop, lo, hi, want_rows=True)
    means3, none = A.pair_tilt(xd, yd, n_fft, hop, lo, hi)
    torch.cuda.synchronize()
    assert none is None
    # two calls, and a call without the rows: the same bits (NaN included)
    assert torch.equal(rows, rows2)
    for m in (means2, means3):
        assert torch.equal(means.view(torch.int64), m.view(torch.int64))
    m, r = means.cpu().numpy(), rows.cpu().numpy()
    for j, band in enumerate((lo, hi)):
        if band[0] == band[1]:
            assert np.all(np.isnan(m[:, j]))        # numpy's mean of an empty slice
        else:
            assert float(np.max(np.abs(m[:, j] - _row_means(r, band)))) <= 1e-9
    if lo[0] == lo[1]:
        assert shape == "64_16"
        return
    d64, _, _, d32 = _statement(shape)
    t64, t32 = rr.tilts(d64, lo, hi), rr.tilts(d32, lo, hi).astype(np.float64)
    e32 = float(np.max(np.abs(t32 - t64)))
    err = float(np.max(np.abs((m[:, 1] - m[:, 0]) - t64)))
    print(f"{shape}: tilt err {err:.2e} dB, e32 {e32:.2e} dB")
    assert err <= rr.rule_bound_db(e32), (err, e32)


def test_overlapping_empty_and_full_ranges():
    torch, A, _, _ = _mods()
    n_fft, hop, _ = SHAPES["256_64"]
    xd, yd, _, rows = _device("256_64")
    r = rows.cpu().numpy()
    nb = n_fft // 2 + 1
    for lo, hi in (((2, 20), (10, 30)), ((0, nb), (0, nb)), ((5, 5), (0, 1)), ((nb, nb), (nb - 1, nb))):
        m, _ = A.pair_tilt(xd, yd, n_fft, hop, lo, hi)
        m = m.cpu().numpy()
        for j, band in enumerate((lo, hi)):
            if band[0] == band[1]:
                assert np.all(np.isnan(m[:, j])), (lo, hi)
            else:
                assert float(np.max(np.abs(m[:, j] - _row_means(r, band)))) <= 1e-9, (lo, hi)


def test_an_odd_cut_gives_the_rows_of_the_cut_arrays():
    """The frames of x[d:], y[d:] for an odd d start off 16-byte alignment: the
    resident slices give the bits of freshly uploaded copies."""
    torch, A, _, _ = _mods()
    n_fft, hop, n = SHAPES["256_64"]
    x, y = _signal(n)
    xd, yd = A.pair_on_device(x, y, 0)
    lo, hi = _bands(n_fft)
    for d in (1, 3):
        assert xd[d:].data_ptr() % 16 == 8
        m1, r1 = A.pair_tilt(xd[d:], yd[d:], n_fft, hop, lo, hi, want_rows=True)
        xc, yc = A.pair_on_device(np.ascontiguousarray(x[d:]), np.ascontiguousarray(y[d:]), 0)
        m2, r2 = A.pair_tilt(xc, yc, n_fft, hop, lo, hi, want_rows=True)
        assert torch.equal(r1, r2) and torch.equal(m1, m2)
        a1 = A.pair_diff_mean(xd[d:], yd[d:], n_fft, hop)
        assert np.array_equal(a1.cpu().numpy(), rr.slab_mean(r1.cpu().numpy()))


# ---------------------------------------------------------------------------
# 3. frame means against the device's own rows, bit for bit
# ---------------------------------------------------------------------------

def test_frame_means_bit_for_bit():
    torch, A, _, _ = _mods()
    n_fft, hop, n = SHAPES["256_64"]
    xd, yd, _, rows = _device("256_64")
    r = rows.cpu().numpy()
    F = len(r)
    assert F == 41
    rng = np.random.default_rng(7)
    lists = [np.sort(rng.choice(F, k, replace=False)) for k in (1, 15, 16, 17, 33)]
    lists += [np.arange(F), np.arange(0, F, 3), np.array([F - 1])]
    for fl in lists:
        got = A.pair_diff_mean(xd, yd, n_fft, hop, fl).cpu().numpy()
        assert np.array_equal(got, rr.slab_mean(r, fl)), len(fl)
    # frames = NULL is the full list, and two calls give the same bits
    full = A.pair_diff_mean(xd, yd, n_fft, hop)
    assert torch.equal(full, A.pair_diff_mean(xd, yd, n_fft, hop, np.arange(F)))
    assert torch.equal(full, A.pair_diff_mean(xd, yd, n_fft, hop))
    # no frame: NaN everywhere
    none = A.pair_diff_mean(xd, yd, n_fft, hop, []).cpu().numpy()
    assert none.shape == (n_fft // 2 + 1,) and np.all(np.isnan(none))
    # a descending list, a repeated and an out-of-range index: TOMATIS_E_ARG
    for bad in ([3, 2], [0, 5, 5], [-1, 0], [0, F]):
        with pytest.raises(RuntimeError, match=r"status -1"):
            A.pair_diff_mean(xd, yd, n_fft, hop, bad)


@pytest.mark.parametrize("shape", ["64_16", "3000_750", "4096_2048", "16384_4096", "one_frame"])
def test_frame_means_at_every_size(shape):
    torch, A, _, _ = _mods()
    n_fft, hop, n = SHAPES[shape]
    xd, yd, _, rows = _device(shape)
    r = rows.cpu().numpy()
    F = len(r)
    got = A.pair_diff_mean(xd, yd, n_fft, hop).cpu().numpy()
    assert np.array_equal(got, rr.slab_mean(r))
    third = np.arange(0, F, 3)
    got = A.pair_diff_mean(xd, yd, n_fft, hop, third).cpu().numpy()
    assert np.array_equal(got, rr.slab_mean(r, third))


# ---------------------------------------------------------------------------
# 4. fixtures recorded from the reference
# ---------------------------------------------------------------------------

_NUM = re.compile(r"(-?\d+(?:\.\d+)?)")
# lines made of exact quantities only (the delay, lengths, the bit-exact levels)
_EXACT = re.compile(r"延迟|对齐后长度|分析帧数|最大电平|最小电平|估计 Gate 阈值|^Delay|frames \(level")


def _same_text(got, want):
    """Line for line: words and integers exactly; each decimal within one unit
    of its last printed digit, or exactly on a line of _EXACT."""
    g, w = got.splitlines(), want.splitlines()
    assert len(g) == len(w), (len(g), len(w), got, want)
    for a, b in zip(g, w):
        if _EXACT.search(b):
            assert a == b, (a, b)
            continue
        pa, pb = _NUM.split(a), _NUM.split(b)
        assert pa[0::2] == pb[0::2], (a, b)
        for u, v in zip(pa[1::2], pb[1::2]):
            if "." in v:
                k = len(v.split(".")[1])
                assert "." in u and abs(float(u) - float(v)) <= 10.0 ** -k + 1e-12, (a, b)
            else:
                assert u == v, (a, b)


def _run(fn, *args, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn(*args, **kw)
    return out, buf.getvalue()


def _same_csv(got, want):
    g, w = got.split("\r\n"), want.split("\r\n")
    assert len(g) == len(w) and g[0] == w[0] and g[-1] == w[-1] == ""
    worst = 0.0
    for a, b in zip(g[1:-1], w[1:-1]):
        ca, cb = a.split(","), b.split(",")
        assert ca[:3] == cb[:3], (a, b)               # frame, time and level: the text
        worst = max(worst, abs(float(ca[3]) - float(cb[3])))
        assert re.fullmatch(r"-?\d+\.\d\d", ca[3]), a
    assert worst <= 0.01 + 1e-12, worst
    return worst


@pytest.mark.parametrize("name", [c["name"] for c in rc.CASES])
def test_reverse_fixture(name, tmp_path):
    torch, _, rev, _ = _mods()
    c, fx = rc.BY_NAME[name], load_fixture(name)
    x, y = rc.make_pair(c)
    assert sha(x) == str(fx["x_sha"])
    T, text = _run(rev.analyze, x, y)
    assert T["delay"] == int(fx["delay"])
    k = rr.reverse_counts(T["inp_level"], T["tilt"])
    assert k["level_bins"] == fx["level_bins"].tolist()
    assert [k["c1"], k["c2"]] == fx["tilt_classes"].tolist()
    assert k["hist"] == fx["hist"].tolist()
    _same_text(text, str(fx["reverse_stdout"]))
    path = str(tmp_path / "frames.csv")
    rev.write_csv(path, T)
    with open(path, encoding="utf-8", newline="") as f:
        worst = _same_csv(f.read(), str(fx["csv"]))
    # the levels are the float32 statement's bits, the tilts follow the rule
    want = rr.reverse_table(x, y, T["delay"], dtype=np.float64)
    assert np.array_equal(T["inp_level"], want["levels"])
    err = float(np.max(np.abs(T["tilt"].astype(np.float64) - want["tilts"])))
    print(f"{name}: tilt column worst text difference {worst:.2f}, against float64 {err:.2e} dB")


@pytest.mark.parametrize("name", [c["name"] for c in rc.CASES])
def test_amplitude_fixture(name):
    torch, _, _, amp = _mods()
    c, fx = rc.BY_NAME[name], load_fixture(name)
    x, y = rc.make_pair(c)
    R, text = _run(amp.analyze, x, y)
    assert R["delay"] == int(fx["delay"])
    assert [R["n_c1"], R["n_c2"]] == fx["amp_classes"].tolist()
    assert ("c1_avg" in R) == (min(fx["amp_classes"]) > 10)
    want_text = str(fx["amp_stdout"])
    _same_text(text, want_text[want_text.index("Delay:"):])
    if "c1_avg" in R:
        # for the record: each class mean against the float64 statement (every
        # bin, the weakest included; the printed values above are the check)
        W64 = rr.amplitude(x, y, R["delay"], dtype=np.float64)
        for key in ("c1_avg", "c2_avg"):
            assert R[key].shape == W64[key].shape and np.all(np.isfinite(R[key]))
            print(f"{name}: {key} worst bin {float(np.max(np.abs(R[key] - W64[key]))):.2e} dB")


# ---------------------------------------------------------------------------
# 5. tensors, arrays and the CLIs
# ---------------------------------------------------------------------------

def test_resident_tensors_give_the_arrays_result():
    torch, _, rev, amp = _mods()
    x, y = rc.make_pair(rc.BY_NAME["reverse_m5003"])
    xt, yt = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(y.copy()).cuda()
    T1, t1 = _run(rev.analyze, x, y)
    T2, t2 = _run(rev.analyze, xt, yt)
    assert t1 == t2 and np.array_equal(T1["tilt"], T2["tilt"])
    assert np.array_equal(T1["inp_level"], T2["inp_level"])
    R1, u1 = _run(amp.analyze, x, y)
    R2, u2 = _run(amp.analyze, xt, yt)
    assert u1 == u2 and np.array_equal(R1["c1_avg"], R2["c1_avg"])
    assert np.array_equal(R1["c2_avg"], R2["c2_avg"])


def test_cli_end_to_end(tmp_path, monkeypatch):
    torch, _, rev, amp = _mods()
    from tomatis_audio_processor_amd import audio_io
    monkeypatch.chdir(tmp_path)
    c = rc.BY_NAME["reverse_p1201"]
    fx = load_fixture(c["name"])
    x, y = rc.make_pair(c)
    audio_io.write("in.flac", x, SR, "FLAC")
    audio_io.write("out.flac", y, SR, "FLAC")
    _, text = _run(rev.main, ["-i", "in.flac", "-o", "out.flac", "--csv", "frames.csv"])
    assert "Tomatis 设备参数反推分析" in text and "输入文件: in.flac" in text
    assert f"延迟: {int(fx['delay'])} samples" in text and "估计 Gate 阈值" in text
    assert "详细数据已保存: frames.csv" in text
    with open("frames.csv", encoding="utf-8", newline="") as f:
        lines = f.read().split("\r\n")
    assert lines[0] == "frame,time_sec,inp_level_dbfs,tilt_db"
    assert len(lines) == len(str(fx["csv"]).split("\r\n"))
    # 24-bit files: the tilts move by far less than the classes' distance
    got = np.array([float(s.split(",")[3]) for s in lines[1:-1]])
    want = np.array([float(s.split(",")[3]) for s in str(fx["csv"]).split("\r\n")[1:-1]])
    assert float(np.max(np.abs(got - want))) < 0.5
    _, text = _run(amp.main, ["in.flac", "out.flac"])
    assert "倾斜滤波器增益幅度验证" in text and f"Delay: {int(fx['delay'])} samples" in text
    assert "总结:" in text and "C1-C2 差异" in text
    _, text = _run(rev.main, ["-i", "in.flac", "-o", "in.flac"])
    assert "延迟: 0 samples" in text and "无法估计Gate阈值" in text
