"""Main-segment and cut golden cases (tests/golden/seg_*.npz, cut_*.npz): seeds
and parameters only.  ``tests/segment_ref.build_input`` turns a case into its
samples: seeded uniform noise at ``quiet`` peak with the spans of ``loud``
(seconds) at ``amp`` peak, quantised to 24 bits below half scale so that a
PCM_24 file round trip returns the same float32 values.

``params`` are the CLI flags of find_main_segment that differ from the
defaults; a cut case carries ``cut_seconds`` (None: the default of 16 s).
"""

SEGMENT_CASES = [
    # one clear segment, 48 kHz, the default 100 / 50 ms (4800 / 2400)
    dict(name="seg_48k_one", seed=201, sr=48000, ch=2, dur=12.0, loud=[(3.0, 9.0)],
         params={"min_seg_sec": 2.0}),
    # two segments of equal length, the first wins; 96 kHz, 125 / 62.5 ms (12000 / 6000):
    # every window time is a binary fraction, so the two lengths are equal as floats
    dict(name="seg_96k_two_equal", seed=202, sr=96000, ch=2, dur=10.0,
         loud=[(1.5, 3.5), (6.0, 8.0)],
         params={"win_ms": 125.0, "hop_ms": 62.5, "min_seg_sec": 1.0}),
    # 44.1 kHz default (4410 / 2205); the segment starts 0.2 s in: the pad clamps at 0
    dict(name="seg_44k_pad0", seed=203, sr=44100, ch=2, dur=8.0, loud=[(0.2, 5.0)],
         params={"min_seg_sec": 2.0}),
    # 44.1 kHz at 37.5 / 12.5 ms (1653 / 551, odd); loud to the end: the pad clamps at dur
    dict(name="seg_44k_odd_end", seed=204, sr=44100, ch=2, dur=6.0, loud=[(2.0, 6.0)],
         params={"win_ms": 37.5, "hop_ms": 12.5, "min_seg_sec": 1.5, "pad_sec": 0.25}),
    # one level throughout: no window 15 dB above the p10
    dict(name="seg_48k_none", seed=205, sr=48000, ch=2, dur=4.0, loud=[], params={}),
    # the longest segment is under the default min_seg_sec of 60 s
    dict(name="seg_44k_short", seed=206, sr=44100, ch=2, dur=9.0, loud=[(1.0, 2.0), (4.0, 7.5)],
         params={}),
    # shorter than one window: no level at all
    dict(name="seg_48k_tiny", seed=207, sr=48000, ch=2, dur=1000 / 48000, loud=[], params={}),
    # not stereo
    dict(name="seg_48k_mono", seed=208, sr=48000, ch=1, dur=1.0, loud=[(0.2, 0.8)], params={}),
]

CUT_CASES = [
    dict(name="cut_48k_st", seed=211, sr=48000, ch=2, dur=3.0, loud=[(0.5, 2.5)],
         cut_seconds=1.3),
    dict(name="cut_44k_default", seed=212, sr=44100, ch=1, dur=16.75, loud=[(15.0, 16.5)],
         cut_seconds=None),
]

QUIET, AMP = 1e-3, 0.25

BY_NAME = {c["name"]: c for c in SEGMENT_CASES + CUT_CASES}
