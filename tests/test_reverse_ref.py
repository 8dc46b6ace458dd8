"""CPU checks of the parameter-recovery tools: the numpy
restatement (tests/reverse_ref.py) in float32 reproduces every fixture recorded
from the reference's own scripts, and the two entry points' argument checks
return the documented codes before anything is launched or read."""
import ctypes as C

import numpy as np
import pytest

from tests import reverse_ref as rr
from tests.golden import reverse_cases as rc
from tests.golden_util import load_fixture, sha

E_ARG, E_UNSUPPORTED = -1, -2
NAMES = [c["name"] for c in rc.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_float32_restatement_reproduces_the_fixture(name):
    c, fx = rc.BY_NAME[name], load_fixture(name)
    assert fx["meta"] == c
    x, y = rc.make_pair(c)
    assert sha(x) == str(fx["x_sha"])
    assert len(y) == int(fx["y_len"]) and np.array_equal(y[::rc.DECIM], fx["y_dec"])
    delay = rr.find_delay(x, y)
    assert delay == int(fx["delay"])
    assert float(fx["margin64"]) >= 1e-3      # the correlation's top stands clear in float64
    T = rr.reverse_table(x, y, delay)
    assert T["n"] == int(fx["n_aligned"])
    assert rr.reverse_csv(T["levels"], T["tilts"]) == str(fx["csv"])
    assert rr.reverse_text(delay, T["n"], T["levels"], T["tilts"]) == str(fx["reverse_stdout"])
    k = rr.reverse_counts(T["levels"], T["tilts"])
    assert k["level_bins"] == fx["level_bins"].tolist()
    assert [k["c1"], k["c2"]] == fx["tilt_classes"].tolist()
    assert k["hist"] == fx["hist"].tolist()
    A = rr.amplitude(x, y, delay)
    assert [A["n_c1"], A["n_c2"]] == fx["amp_classes"].tolist()
    assert str(fx["amp_stdout"]).endswith(rr.amplitude_text(A))


def test_the_cases_reach_every_branch():
    fx = {n: load_fixture(n) for n in NAMES}
    assert int(fx["reverse_p1201"]["delay"]) > 0 > int(fx["reverse_m5003"]["delay"])
    assert min(fx["reverse_p1201"]["tilt_classes"]) > 0            # clear separation
    assert "估计 Gate 阈值" in str(fx["reverse_p1201"]["reverse_stdout"])
    assert fx["reverse_flat"]["tilt_classes"].tolist() == [0, 0]
    assert "无法估计Gate阈值" in str(fx["reverse_flat"]["reverse_stdout"])
    assert min(fx["reverse_p1201"]["amp_classes"]) > 10            # both curves printed
    assert "总结:" in str(fx["reverse_p1201"]["amp_stdout"])
    assert min(fx["reverse_one_class"]["amp_classes"]) <= 10       # the two count lines only
    assert "总结:" not in str(fx["reverse_one_class"]["amp_stdout"])
    assert all(0 in f["level_bins"] for f in fx.values())          # an empty level bin


def test_slab_mean_is_the_plain_mean_up_to_rounding():
    r = np.random.default_rng(5).standard_normal((37, 9)).astype(np.float32)
    assert np.allclose(rr.slab_mean(r), r.astype(np.float64).mean(axis=0), rtol=0, atol=1e-14)
    assert np.all(np.isnan(rr.slab_mean(r, [])))
    assert np.array_equal(rr.slab_mean(r, [3]), r[3].astype(np.float64))


# ---------------------------------------------------------------------------
# argument checks: no launch, no read (the pointers below are never followed)
# ---------------------------------------------------------------------------

def _lib():
    from tomatis_audio_processor_amd._lib import lib
    return lib()


P = C.c_void_p(4096)      # a non-null pointer that must not be read
NULL = C.c_void_p(0)


def _tilt(L, x=P, y=P, n=10000, n_fft=256, hop=64, lo=(1, 3), hi=(10, 40), win=P, means=P):
    return L.tomatis_an_pair_tilt(x, y, n, n_fft, hop, *lo, *hi, win, NULL, means, NULL)


def test_pair_tilt_argument_checks():
    L = _lib()
    for kw in (dict(x=NULL), dict(y=NULL), dict(win=NULL), dict(means=NULL), dict(hop=0),
               dict(lo=(-1, 3)), dict(lo=(3, 2)), dict(hi=(10, 130)), dict(hi=(129, 128)),
               dict(n_fft=0)):
        assert _tilt(L, **kw) == E_ARG, kw
    for n_fft in (8, 15, 32768, 8193, 12000):
        assert _tilt(L, n_fft=n_fft, lo=(0, 1), hi=(0, 1)) == E_UNSUPPORTED, n_fft
    # the full range and empty ranges are in order; n < n_fft writes nothing
    assert _tilt(L, n=255, lo=(0, 129), hi=(129, 129)) == 0


def _mean(L, x=P, y=P, n=10000, n_fft=256, hop=64, win=P, frames=None, n_sel=None, work=P,
          out=P):
    fl = None if frames is None else np.asarray(frames, np.int32)
    n_sel = (0 if fl is None else len(fl)) if n_sel is None else n_sel
    fp = NULL if fl is None else fl.ctypes.data_as(C.c_void_p)
    return L.tomatis_an_pair_diff_mean(x, y, n, n_fft, hop, win, fp, n_sel, work, out, NULL)


def test_pair_diff_mean_argument_checks():
    L = _lib()
    F = 1 + (10000 - 256) // 64
    for kw in (dict(x=NULL), dict(y=NULL), dict(win=NULL), dict(out=NULL), dict(hop=0),
               dict(n_fft=0), dict(frames=[0, 1], work=NULL), dict(frames=[0], n_sel=-1)):
        assert _mean(L, frames=kw.pop("frames", [0, 1]), **kw) == E_ARG, kw
    for n_fft in (8, 32768, 8193):
        assert _mean(L, frames=[0], n_fft=n_fft) == E_UNSUPPORTED, n_fft
    # the list: checked on the host before any launch
    for frames in ([3, 2], [0, 5, 5], [-1, 2], [0, F], [5, 4, 3, 2, 1]):
        assert _mean(L, frames=frames) == E_ARG, frames
    assert _mean(L, frames=None, n_sel=F - 1) == E_ARG       # NULL means all F frames
    assert _mean(L, n=255, frames=[0]) == 0                  # n < n_fft: nothing is written
    W = L.tomatis_an_pair_diff_mean_work_doubles
    assert W(0, 129) == 0 and W(1, 129) == 129 + 1 and W(16, 129) == 129 + 8
    assert W(17, 129) == 2 * 129 + 9 and W(5, 0) == 0 and W(2 ** 31, 129) == 0
