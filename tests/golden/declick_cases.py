"""De-click golden cases (tests/golden/declick_<name>.npz): seeds and parameters
only.  ``tests/declick_ref.build_input`` turns a case into its input samples:

* ``kind`` "noise": a 440 Hz sine plus stationary ``synth_stream`` noise, then
  additive clicks (``clicks``: frames given here; ``n_random``: seeded ones) and
  bursts (``bursts``: (start, length) of seeded full-band noise);
* ``kind`` "zero": silence; ``kind`` "square": a full-scale square wave at the
  Nyquist rate (every difference is a hit);
* everything is quantised to ``bits`` so a PCM file round trip is lossless and
  the 16-bit cases have thousands of equal differences.

``params`` are the CLI flags that differ from the defaults.
"""

CASES = [
    # clicks at frames 0 and 5, across the 65535 | 65536 boundary, at the last
    # frame; one ~900-frame burst that is dropped as too long; N - 1 even
    dict(name="declick_stereo24", seed=101, N=200001, ch=2, sr=48000, bits=24, kind="noise",
         clicks=[0, 5, 65536, 120000, 200000], n_random=0, bursts=[(30000, 900)], params={}),
    # N - 1 odd, massive ties
    dict(name="declick_mono16", seed=102, N=100000, ch=1, sr=44100, bits=16, kind="noise",
         clicks=[], n_random=10, bursts=[], params={}),
    dict(name="declick_three96", seed=103, N=120001, ch=3, sr=96000, bits=24, kind="noise",
         clicks=[1], n_random=8, bursts=[(50000, 2000)], params={}),
    dict(name="declick_tiny", seed=104, N=4097, ch=2, sr=48000, bits=24, kind="noise",
         clicks=[2000], n_random=0, bursts=[], params={}),
    dict(name="declick_zero", seed=105, N=50000, ch=2, sr=48000, bits=24, kind="zero",
         clicks=[], n_random=0, bursts=[], params={}),
    dict(name="declick_square", seed=106, N=30001, ch=2, sr=48000, bits=24, kind="square",
         clicks=[], n_random=0, bursts=[], params={}),
    dict(name="declick_k6", seed=107, N=150001, ch=2, sr=48000, bits=16, kind="noise",
         clicks=[], n_random=40, bursts=[(70000, 600)], params={"k": 6.0}),
    dict(name="declick_one", seed=108, N=1, ch=2, sr=48000, bits=24, kind="noise",
         clicks=[], n_random=0, bursts=[], params={}),
    # non-default windows: no padding, no merging, a short length limit
    dict(name="declick_nopad", seed=109, N=60000, ch=2, sr=44100, bits=24, kind="noise",
         clicks=[0, 59999], n_random=12, bursts=[(20000, 300)],
         params={"pad_ms": 0.0, "merge_gap_ms": 0.0, "max_fix_ms": 2.0, "k": 10.0}),
]

BY_NAME = {c["name"]: c for c in CASES}
