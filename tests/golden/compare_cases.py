"""Cases of the compare_audio goldens (tools/make_compare_goldens.py).  Inputs are
the synth pairs of tests/golden/align_cases.py, regenerated from seeds
(``make_pair``: the target is compare_audio's candidate).  Every pair's
full-mode correlation has a float64 margin >= 1e-3 between its top and the
runner-up; ``align_p100007`` is left out on purpose: in full mode the
reference itself lands on a false peak there (margin 2.2e-4)."""
from tests.golden.align_cases import CLI_CASES, DELAY_CASES, SR, make_pair  # noqa: F401

_PAIRS = {c["name"]: c for c in DELAY_CASES + CLI_CASES}


def _pair(name, **kw):
    c = {k: v for k, v in _PAIRS[name].items() if k not in ("chunk_sec", "argv")}
    c.update(pair=name, name=name.replace("align_", "compare_"), **kw)
    return c


# find_delay_by_corr alone
DELAY_CASES_FULL = [
    _pair("align_p1234"),
    _pair("align_m5000"),
    _pair("align_short_base"),       # 3001 against 24000 envelope samples
    _pair("align_short_target"),     # 24000 against 2001
    _pair("align_cli_default"),      # 40 s, shift 777
    _pair("align_cli_2048"),         # 40 s, shift -3210
]

# main(): 12 s pairs; the reference's defaults and smaller values passed to main
MAIN_CASES = [
    dict(_pair("align_p1234"), name="compare_main_p1234", n_fft=4096, hop=2048),
    dict(_pair("align_m5000"), name="compare_main_m5000", n_fft=1024, hop=256),
]

# too little overlap for one frame: np.stack of an empty list
ERROR_CASES = [
    dict(name="compare_err_overlap", pair=None, seed=91, n_base=4000, n_target=4000, shift=0,
         n_fft=4096, hop=2048),
]

MIN_MARGIN = 1e-3


def make_inputs(c):
    """-> (base, cand) float32 [n, 2]."""
    cand, base = make_pair(c)
    return base, cand
