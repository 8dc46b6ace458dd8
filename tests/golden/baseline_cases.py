"""Cases of the compare_to_baseline goldens (tools/make_baseline_goldens.py).
Inputs are the synth pairs of tests/golden/align_cases.py, regenerated from
seeds.  One ``main`` call of the reference takes one baseline and N candidates,
so the two 40 s pairs share ``align_cli_default``'s base (seed 81): the first
candidate is that pair's own target (shift 777), the second is cut from the same
stream with ``align_cli_2048``'s target length and shift (-3210).  Every case's
float64 correlation has a margin >= 1e-3 between its top and the runner-up,
except the 12 s pairs: their base is shorter than the 25 s chunk and as long as
the candidate, so the valid correlation has a single lag and the reference
returns delay 0 whatever the shift (margin: inf)."""
from tests.golden.align_cases import CLI_CASES, DELAY_CASES, SR, make_pair  # noqa: F401

_PAIRS = {c["name"]: c for c in DELAY_CASES + CLI_CASES}
_D, _T = _PAIRS["align_cli_default"], _PAIRS["align_cli_2048"]

# candidates: (file name, seed, n_target, shift); the baseline: (seed, n_base)
_C777 = dict(file="cand_p777.wav", seed=_D["seed"], n_target=_D["n_target"], shift=_D["shift"])
_C3210 = dict(file="cand_m3210.wav", seed=_D["seed"], n_target=_T["n_target"], shift=_T["shift"])
_P1234 = _PAIRS["align_p1234"]

MAIN_CASES = [
    # two candidates in one call; --max_minutes 0.5 caps the 40 s overlaps at 30 s
    dict(name="baseline_two_4096", seed=_D["seed"], n_base=_D["n_base"], cands=[_C777, _C3210],
         n_fft=4096, hop=2048, max_minutes=0.5),
    dict(name="baseline_m3210_1024", seed=_D["seed"], n_base=_D["n_base"], cands=[_C3210],
         n_fft=1024, hop=256, max_minutes=0.5),
    # the single-lag case: 12 s against 12 s, the reference's defaults
    dict(name="baseline_p1234", seed=_P1234["seed"], n_base=_P1234["n_base"],
         cands=[dict(file="cand_p1234.wav", seed=_P1234["seed"], n_target=_P1234["n_target"],
                     shift=_P1234["shift"])],
         n_fft=4096, hop=2048, max_minutes=8.0),
]

ERROR_CASES = [
    # 4000 samples of overlap, fewer than n_fft
    dict(name="baseline_err_short", seed=91, n_base=4000,
         cands=[dict(file="cand_short.wav", seed=91, n_target=4000, shift=0)],
         n_fft=4096, hop=2048, max_minutes=8.0),
    # a cap of zero samples: the reference's only way to an empty overlap
    dict(name="baseline_err_no_overlap", seed=91, n_base=4000,
         cands=[dict(file="cand_short.wav", seed=91, n_target=4000, shift=0)],
         n_fft=4096, hop=2048, max_minutes=0.0),
    # the candidate's file says 44.1 kHz
    dict(name="baseline_err_rate", seed=91, n_base=4000,
         cands=[dict(file="cand_44k.wav", seed=91, n_target=4000, shift=0, sr=44100)],
         n_fft=4096, hop=2048, max_minutes=8.0),
]

MIN_MARGIN = 1e-3
BASELINE_FILE = "baseline.wav"
OUTDIR = "out"


def make_inputs(c):
    """-> (base, [cand, ...]) float32 [n, 2]."""
    base = None
    cands = []
    for k in c["cands"]:
        cand, b = make_pair(dict(seed=k["seed"], n_base=c["n_base"], n_target=k["n_target"],
                                 shift=k["shift"]))
        base = b if base is None else base
        cands.append(cand)
    return base, cands
