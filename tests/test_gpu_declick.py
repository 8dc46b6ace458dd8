"""De-click stage on the GPU: everything is asked for
exactly — output hashes, segments, counts and the bit patterns of sigma and thr
against the goldens the reference produced, selection against np.partition, and
seeded random configurations against the numpy statement in tests/declick_ref.py."""
import io
import contextlib

import numpy as np
import pytest

from tests import declick_ref as ref
from tests.golden.declick_cases import BY_NAME, CASES

pytestmark = pytest.mark.gpu


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _check(res, want_y_sha, segs, raw, hits, sigma_bits, thr_bits, shape):
    y = res.y.cpu().numpy()
    assert y.dtype == np.float32 and y.shape == shape
    assert (res.hits, res.raw) == (hits, raw)
    np.testing.assert_array_equal(res.segs, segs)
    assert res.segs.dtype == np.int64
    assert ref.f64_bits(res.sigma) == sigma_bits
    assert ref.f64_bits(res.thr) == thr_bits
    assert ref.sha(y) == want_y_sha


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_declick_matches_reference_golden(name):
    torch = _torch()
    from tomatis_audio_processor_amd.declick_inpaint import declick
    fx = ref.load_golden(name)
    c = fx["meta"]
    x = ref.build_input(c)
    assert ref.sha(x) == str(fx["in_sha"])
    as_tensor = c["N"] % 2 == 0  # both kinds of input
    res = declick(torch.from_numpy(x).cuda() if as_tensor else x, c["sr"], **c["params"])
    _check(res, str(fx["out_sha"]), fx["segs"], int(fx["raw"]), int(fx["hits"]),
           int(fx["sigma_bits"]), int(fx["thr_bits"]), x.shape)


def _select(torch, v, lo, hi, center=None):
    from tomatis_audio_processor_amd._lib import check, lib, ptr, stream_handle
    n = v.numel()
    work = torch.empty(int(lib().tomatis_declick_work_words(n)), dtype=torch.int32, device="cuda")
    out = torch.empty(2, dtype=torch.int32, device="cuda")
    check(lib().tomatis_declick_select(ptr(v), n, int(center is not None),
                                       float(center or 0.0), lo, hi, ptr(work), ptr(out),
                                       stream_handle()), "declick_select")
    return out.cpu().numpy().view(np.uint32)


def _select_arrays():
    rng = np.random.default_rng(11)
    out = {}
    for n in (1, 2, 63, 64, 65, 1023, 1025):
        out[f"random_{n}"] = rng.random(n, dtype=np.float32)
    # more than three workgroups' worth (1024 values each) plus a ragged tail
    out["ragged_3589"] = (rng.random(3589, dtype=np.float32) * np.float32(1e-3))
    # heavy ties: six distinct values; 16-bit steps; all equal; all zero
    out["ties_6"] = (rng.integers(0, 6, 50001) / 8.0).astype(np.float32)
    out["ties_16bit"] = (np.abs(rng.integers(-300, 300, 70002)) / 32768.0).astype(np.float32)
    out["equal"] = np.full(4099, 0.25, np.float32)
    out["zeros"] = np.zeros(2050, np.float32)
    # longer than one sweep of the grid, wide dynamic range (every digit pass matters)
    out["wide_2500001"] = np.exp(rng.uniform(-40, 2, 2_500_001)).astype(np.float32)
    return out


@pytest.fixture(scope="module")
def select_arrays():
    return _select_arrays()


SELECT_KEYS = ["random_1", "random_2", "random_63", "random_64", "random_65", "random_1023",
               "random_1025", "ragged_3589", "ties_6", "ties_16bit", "equal", "zeros",
               "wide_2500001"]


@pytest.mark.parametrize("key", SELECT_KEYS)
def test_select_matches_partition(select_arrays, key):
    torch = _torch()
    a = select_arrays[key]
    n = len(a)
    v = torch.from_numpy(a).cuda()
    s = np.sort(a)
    ranks = [((n - 1) // 2, n // 2), (0, n - 1), (n // 3, n // 3)]
    for lo, hi in ranks:
        got = _select(torch, v, lo, hi)
        part = np.partition(a, [lo, hi])
        assert got[0] == part[lo].view(np.uint32) == s[lo].view(np.uint32), (key, lo)
        assert got[1] == part[hi].view(np.uint32), (key, hi)
    # the MAD's keys |v - center|, formed on the fly
    center = s[n // 2]
    dev = np.abs(a - center)
    lo, hi = (n - 1) // 2, n // 2
    got = _select(torch, v, lo, hi, center=center)
    part = np.partition(dev, [lo, hi])
    assert (got[0], got[1]) == (part[lo].view(np.uint32), part[hi].view(np.uint32)), key


def test_select_unaligned_pointer(select_arrays):
    torch = _torch()
    a = select_arrays["ties_16bit"]
    v = torch.from_numpy(a).cuda()[1:]          # 4 bytes past a 16-byte boundary
    b = a[1:]
    n = len(b)
    got = _select(torch, v, (n - 1) // 2, n // 2)
    part = np.partition(b, [(n - 1) // 2, n // 2])
    assert (got[0], got[1]) == (part[(n - 1) // 2].view(np.uint32), part[n // 2].view(np.uint32))


def _random_configs():
    rng = np.random.default_rng(2024)
    sizes = [2, 3, 5, 64, 4096, 4097, 4098, 8193, 65537, 300000]
    cfgs = []
    for i in range(20):
        n = sizes[i] if i < len(sizes) else int(rng.integers(2, 300001))
        cfgs.append(dict(
            seed=500 + i, n=n, ch=int(rng.integers(1, 4)),
            sr=int(rng.choice([44100, 48000, 96000])), bits=int(rng.choice([16, 24])),
            k=float(rng.choice([6.0, 8.0, 10.0, 12.0, 14.0])),
            pad_ms=float(rng.choice([0.0, 0.25, 1.5, 3.0])),
            merge_gap_ms=float(rng.choice([0.0, 0.5, 2.0])),
            max_fix_ms=float(rng.choice([0.0, 2.0, 8.0, 20.0])),
            n_random=int(min(n, rng.integers(0, 40))),
            burst=bool(rng.integers(2)) and n > 5000))
    return cfgs


@pytest.mark.parametrize("cfg", _random_configs(), ids=lambda c: f"n{c['n']}_c{c['ch']}_s{c['seed']}")
def test_random_configurations_match_numpy_statement(cfg):
    torch = _torch()
    from tomatis_audio_processor_amd.declick_inpaint import declick
    n = cfg["n"]
    bursts = [(n // 3, min(1500, n // 8))] if cfg["burst"] else []
    _, x = ref.noise_clicks(cfg["seed"], n, cfg["ch"], cfg["sr"], cfg["bits"],
                            clicks=[0, n - 1] if cfg["seed"] % 3 == 0 else [],
                            n_random=cfg["n_random"], bursts=bursts)
    kw = {k: cfg[k] for k in ("k", "pad_ms", "merge_gap_ms", "max_fix_ms")}
    want = ref.declick(x, cfg["sr"], **kw)
    res = declick(x, cfg["sr"], **kw)
    _check(res, ref.sha(want["y"]), want["segs"], want["raw"], want["hits"],
           ref.f64_bits(want["sigma"]), ref.f64_bits(want["thr"]), x.shape)


def test_more_tiles_than_one_scan_round():
    """More than 1024 tiles of 4096 differences: the one-workgroup scans over
    the tiles take a second round, with clicks on both sides of its boundary."""
    _torch()
    from tomatis_audio_processor_amd.declick_inpaint import declick
    edge = 4096 * 1024
    n = edge + 4096 * 2 + 19
    _, x = ref.noise_clicks(601, n, 1, 48000, 16, clicks=[0, edge - 40, edge, edge + 1, n - 1],
                            n_random=30)
    want = ref.declick(x, 48000)
    assert want["raw"] >= 30 and len(want["segs"]) >= 30
    res = declick(x, 48000)
    _check(res, ref.sha(want["y"]), want["segs"], want["raw"], want["hits"],
           ref.f64_bits(want["sigma"]), ref.f64_bits(want["thr"]), x.shape)


def test_thousands_of_short_segments():
    """pad = gap = 0 and a pair of hits every eight differences: thousands of
    raw segments, many per tile, all kept and inpainted."""
    torch = _torch()
    from tomatis_audio_processor_amd.declick_inpaint import declick
    n = 20001
    x = np.zeros((n, 1), np.float32)
    x[1::8] = 0.5          # steps at differences 0, 1, 8, 9, 16, 17, ...
    x[::64] += np.float32(2.0 ** -10)
    want = ref.declick(x, 48000, k=12.0, pad_ms=0.0, merge_gap_ms=0.0, max_fix_ms=1.0)
    assert want["raw"] > 2000 and len(want["segs"]) == want["raw"]
    res = declick(x, 48000, k=12.0, pad_ms=0.0, merge_gap_ms=0.0, max_fix_ms=1.0)
    _check(res, ref.sha(want["y"]), want["segs"], want["raw"], want["hits"],
           ref.f64_bits(want["sigma"]), ref.f64_bits(want["thr"]), x.shape)


def test_module_surface_on_device():
    torch = _torch()
    from tomatis_audio_processor_amd import declick_inpaint as dc
    c = BY_NAME["declick_mono16"]
    x = ref.build_input(c)
    d = ref.detection_statistic(x)
    assert ref.f64_bits(dc.mad_sigma(d)) == ref.f64_bits(ref.robust_sigma(d))
    assert ref.f64_bits(dc.mad_sigma(torch.from_numpy(d[:-1]).cuda())) == \
        ref.f64_bits(ref.robust_sigma(d[:-1]))
    segs = np.array([[0, 7], [100, 101], [5000, 5300], [len(x) - 3, len(x)]], np.int64)
    y = dc.inpaint_linear(x, segs).cpu().numpy()
    np.testing.assert_array_equal(y.view(np.uint32), ref.inpaint(x, segs).view(np.uint32))


def _run_cli(argv):
    from tomatis_audio_processor_amd import declick_inpaint as dc
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        dc.main(argv)
    return buf.getvalue()


def test_cli_file_to_file(tmp_path):
    _torch()
    from tomatis_audio_processor_amd import audio_io
    fx = ref.load_golden("declick_stereo24")
    c = fx["meta"]
    pcm, x = ref.build_input_pcm(c)
    inp, out, rep = (str(tmp_path / n) for n in ("in.flac", "out.flac", "report.csv"))
    with open(inp, "wb") as f:
        f.write(audio_io.flac_encode_int(pcm, c["sr"], c["bits"]))
    text = _run_cli(["-i", inp, "-o", out, "--report_csv", rep])
    assert text.replace(rep, "{report}").replace(out, "{out}") == str(fx["stdout"])
    with open(rep, newline="", encoding="utf-8") as f:
        assert f.read() == str(fx["report_csv"])
    want = ref.declick(x, c["sr"])
    assert ref.sha(want["y"]) == str(fx["out_sha"])
    got, sr, bps = audio_io.flac_decode_int(open(out, "rb").read())
    assert (sr, bps) == (c["sr"], 24)
    np.testing.assert_array_equal(got, ref.pcm24_of(want["y"]))


def test_cli_no_hit_file_is_the_input(tmp_path):
    _torch()
    from tomatis_audio_processor_amd import audio_io
    fx = ref.load_golden("declick_zero")
    c = fx["meta"]
    pcm, x = ref.build_input_pcm(c)
    inp, out = str(tmp_path / "in.flac"), str(tmp_path / "out.flac")
    with open(inp, "wb") as f:
        f.write(audio_io.flac_encode_int(pcm, c["sr"], c["bits"]))
    text = _run_cli(["-i", inp, "-o", out])
    assert text == str(fx["stdout"])
    got, sr, bps = audio_io.flac_decode_int(open(out, "rb").read())
    assert (sr, bps) == (c["sr"], 24)
    np.testing.assert_array_equal(got, pcm)
