"""The pipelined pass hand-off of engine._Pipelined on its own (no GPU): a stub
pipeline with small CPU tensors, whose pipelined launch and whose library (the
limiter and the unpipelined transform) are fakes that record every call in one
log and return a scripted status.  Which pass a launch limits, which buffer it
writes, what is flushed and when, for every path the GPU tests
(test_gpu_handoffs.py, test_gpu_pipelined.py) pin end to end.
"""
import importlib.util
import types

import pytest

torch = pytest.importorskip("torch")

from tomatis_audio_processor_amd import _lib, engine  # noqa: E402
from tomatis_audio_processor_amd._lib import E_UNSUPPORTED  # noqa: E402

CUR = object()   # the current stream, and every stub's: no wait between them


def _boom(*a, **k):
    raise AssertionError("device or library touched")


def test_engine_imports_without_device_or_library(monkeypatch):
    """The module body (the base class included) loads no library and asks
    torch for no device."""
    monkeypatch.setattr(_lib, "lib", _boom)
    monkeypatch.setattr(_lib, "stream_handle", _boom)
    for name in ("is_available", "current_stream", "init", "Stream", "Event"):
        monkeypatch.setattr(torch.cuda, name, _boom)
    spec = importlib.util.find_spec("tomatis_audio_processor_amd.engine")
    fresh = importlib.util.module_from_spec(spec)   # (a second copy: sys.modules keeps the first)
    spec.loader.exec_module(fresh)
    assert issubclass(fresh.GatePipeline, fresh._Pipelined)
    assert issubclass(fresh.AdaptivePipeline, fresh._Pipelined)


class _FakeLib:
    """tomatis_apply_limiter / tomatis_stft_ola_limited: recorded, status 0."""

    def __init__(self, log):
        self.log = log

    def tomatis_apply_limiter(self, plan, y, peaks, limit, hs):
        self.log.append(("limiter", plan, y.value, peaks.value))
        return 0

    def tomatis_stft_ola_limited(self, plan, x, gains, n_rows, rows, y, peaks, limit, hs):
        self.log.append(("limited", plan, y.value, peaks.value))
        return 0


@pytest.fixture
def log(monkeypatch):
    log = []
    fake = _FakeLib(log)
    monkeypatch.setattr(engine, "lib", lambda: fake)
    monkeypatch.setattr(engine, "stream_handle", lambda: None)
    for name in ("is_available", "current_stream", "stream"):
        monkeypatch.setattr(torch.cuda, name, _boom)
    return log


class Stub(engine._Pipelined):
    """``script``: the statuses of its pipelined launches, in order (an
    exception instance is raised)."""

    def __init__(self, name, log, script=(), pipelined=True, second_buffer=True):
        self.name, self.log, self.script = name, log, list(script)
        self.plan = types.SimpleNamespace(h=name)
        self.ss = types.SimpleNamespace(x=torch.zeros(4))
        self.gains, self.n_rows = torch.ones(3), 1
        self.rows = torch.zeros(2, dtype=torch.int16)
        self.y = torch.zeros(6)
        self.peaks = torch.zeros(2, dtype=torch.int32)
        self._init_pipelined(pipelined, second_buffer)

    def _rows_call(self, nxt, pplan, prev_y, prev_pk):
        rc = self.script.pop(0)
        self.log.append(("launch", self.name, nxt, pplan, prev_y, prev_pk, rc))
        if isinstance(rc, Exception):
            raise rc
        return rc

    def run(self, prev_pipe=None):
        prev, = self._take_prev(prev_pipe, CUR, CUR)
        self._after_prev(prev, self._transform)


def _launches(log, name):
    return [e for e in log if e[0] == "launch" and e[1] == name]


def _limiter(p, slot=None):
    """The log entry of p.flush() (of buffer ``slot``; default the current one)."""
    y, pk = (p.y, p.peaks) if slot is None else (p._ys[slot], p._pks[slot])
    return ("limiter", p.plan.h, y.data_ptr(), pk.data_ptr())


def test_own_passes_alternate_and_limit_the_previous_slot(log):
    p = Stub("p", log, [0, 0, 0])
    assert p._ys[1] is not None and p._pks[1] is not None
    assert not p._pks[1].any()
    ys, pks = list(p._ys), list(p._pks)
    for k in range(3):
        p.run()
        assert p.pending and p.pipelined
        assert p.y is ys[k % 2] and p.peaks is pks[k % 2] and p._cur == k % 2
    assert all(a is b for a, b in zip(p._ys + p._pks, ys + pks))
    got = [(e[2], e[3], e[4], e[5]) for e in log]
    assert [g[0] for g in got] == [0, 1, 0]
    assert got[0][1:] == (None, None, None)
    assert got[1][1] is p.plan and got[1][2] is ys[0] and got[1][3] is pks[0]
    assert got[2][1] is p.plan and got[2][2] is ys[1] and got[2][3] is pks[1]
    del log[:]
    want = _limiter(p, 0)
    p.flush()
    assert log == [want] and not p.pending
    p.flush()
    assert log == [want]


def test_second_buffer_on_first_need(log):
    p = Stub("p", log, [0, 0], second_buffer=False)
    p.run()
    assert p._ys[1] is None and p.y is p._ys[0]
    p.run()
    assert p._ys[1] is not None and p._ys[1] is not p._ys[0]
    assert p._ys[1].data_ptr() != p._ys[0].data_ptr() and p._ys[1].shape == p._ys[0].shape
    assert p.y is p._ys[1] and p.peaks is p._pks[1] and not p._pks[1].any()


def test_unpipelined_never_gets_a_second_buffer(log):
    p = Stub("p", log, pipelined=False)
    p.run()
    p.run()
    assert p._ys[1] is None and not p.pending
    assert log == [("limited", "p", p.y.data_ptr(), p.peaks.data_ptr())] * 2


def test_foreign_predecessor_limited_inside_the_launch(log):
    prev, p = Stub("prev", log, [0]), Stub("p", log, [0])
    prev.run()
    del log[:]
    p.run(prev_pipe=prev)
    (e,) = log   # one launch, no limiter call
    assert e[2] == 0 and e[3] is prev.plan and e[4] is prev.y and e[5] is prev.peaks
    assert not prev.pending and p.pending and p.pipelined and p._after is None


def test_foreign_predecessor_declined_is_flushed_once(log):
    prev, p = Stub("prev", log, [0]), Stub("p", log, [E_UNSUPPORTED, 0])
    prev.run()
    del log[:]
    p.run(prev_pipe=prev)
    first, flushed, second = log
    assert first[3] is prev.plan and first[6] == E_UNSUPPORTED
    assert flushed == _limiter(prev)
    assert second[2:] == (0, None, None, None, 0)
    assert not prev.pending and p.pending and p.pipelined and p._after is None


def test_own_shape_declined(log):
    p = Stub("p", log, [E_UNSUPPORTED])
    assert p._pipelined_launch(p._rows_call) is False
    assert not p.pipelined and not p.pending
    assert [e[6] for e in _launches(log, "p")] == [E_UNSUPPORTED]   # nothing launched
    # the wrapper: what was pending is flushed, then the unpipelined transform
    q = Stub("q", log, [0, E_UNSUPPORTED])
    q.run()
    del log[:]
    q.run()
    declined, flushed, limited = log
    assert declined[3] is q.plan and declined[6] == E_UNSUPPORTED
    assert flushed == _limiter(q, 0)
    assert limited == ("limited", "q", q.y.data_ptr(), q.peaks.data_ptr())
    assert not q.pipelined and not q.pending
    q.run()      # pipelining stays off: no further launch attempt
    assert len(_launches(log, "q")) == 1 and log[-1] == limited


def test_own_shape_declined_with_foreign_predecessor(log):
    """(a successor without a frame) the predecessor is flushed once, on the
    first decline."""
    prev, p = Stub("prev", log, [0]), Stub("p", log, [E_UNSUPPORTED, E_UNSUPPORTED])
    prev.run()
    del log[:]
    p.run(prev_pipe=prev)
    assert [e[0] for e in log] == ["launch", "limiter", "launch", "limited"]
    assert log[1] == _limiter(prev) and log[2][3] is None
    assert not prev.pending and not p.pending and not p.pipelined


def test_both_pending_own_pass_flushed_first(log):
    prev, p = Stub("prev", log, [0]), Stub("p", log, [0, 0])
    prev.run()
    p.run()
    del log[:]
    own = _limiter(p)
    p.run(prev_pipe=prev)
    flushed, launch = log
    assert flushed == own
    assert launch[2] == 0 and launch[3] is prev.plan and launch[4] is prev.y
    assert p.pending and not prev.pending


def test_unpipelined_successor_flushes_predecessor_after_its_pass(log):
    prev, p = Stub("prev", log, [0]), Stub("p", log, pipelined=False)
    prev.run()
    del log[:]
    p.run(prev_pipe=prev)
    assert log == [("limited", "p", p.y.data_ptr(), p.peaks.data_ptr()), _limiter(prev)]
    assert not prev.pending and not p.pending


def test_group_predecessor_one_partner_per_launch(log):
    a, idle, b = Stub("a", log, [0]), Stub("idle", log), Stub("b", log, [0])
    a.run()
    b.run()
    groups = types.SimpleNamespace(pipes=[a, idle, b])
    del log[:]
    p = Stub("p", log, [0])
    p.run(prev_pipe=groups)
    flushed, launch = log
    assert flushed == _limiter(b)
    assert launch[3] is a.plan and launch[4] is a.y
    assert not (a.pending or b.pending or idle.pending)


def test_take_prev_partners_and_waits(log):
    class Stream:
        def __init__(self):
            self.waited = []

        def wait_stream(self, s):
            self.waited.append(s)

    a, idle, b, c = (Stub(n, log, [0]) for n in ("a", "idle", "b", "c"))
    for q in (a, b, c):
        q.run()
    a.stream, idle.stream, b.stream = Stream(), Stream(), Stream()
    groups = types.SimpleNamespace(pipes=[a, idle, b, c])
    del log[:]
    strm, cur = Stream(), Stream()
    assert engine._Pipelined._take_prev(None, strm, cur, 2) == [None, None]
    # two launches: two partners, the third pending member flushed
    assert engine._Pipelined._take_prev(groups, strm, cur, 2) == [a, b]
    assert log == [_limiter(c)]
    assert strm.waited == [a.stream, idle.stream, b.stream, cur]
    # more launches than pending members; no wait for strm itself
    assert engine._Pipelined._take_prev(groups, a.stream, cur, 3) == [a, b, None]
    assert a.stream.waited == [idle.stream, b.stream, cur] and len(log) == 1


def test_launch_raises_nothing_more_is_launched(log):
    err = RuntimeError("launch failed")
    prev, p = Stub("prev", log, [0]), Stub("p", log, [err])
    prev.run()
    del log[:]
    with pytest.raises(RuntimeError, match="launch failed"):
        p.run(prev_pipe=prev)
    assert len(log) == 1 and log[0][0] == "launch" and log[0][3] is prev.plan
    assert prev.pending and p._after is None and not p.pending
