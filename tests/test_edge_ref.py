"""CPU: the conditions on the inputs of tests/test_gpu_edge_samples.py.

For every case the device test uses, numpy's float32 run of the float64
statement stays within D / 4 on every output sample with D > 0 (the margin
tests/test_conditioning.py::test_error_model_bounds_reference_float32 uses),
and is an exact zero where D == 0: the bound the device is held to is one the
reference's own arithmetic meets four times over on the very same input.

Two float64 mutations -- the last frame's overlap-add contribution dropped
over its final hop, and the normaliser reading the window sum one sample late
-- each exceed D on a sample with sum w^2 < TAU on every calibrated shape:
samples every other sample-level test masks.
"""
import numpy as np
import pytest

from tests import edge_ref as er
from tomatis_audio_processor_amd import conditioning as cd


def test_every_shape_is_kept():
    """Every calibrated and every extended shape has its cases, in all three
    tail classes (none had to be dropped: numpy meets D / 4 on all)."""
    for shape in er.CORE + er.EXTENDED:
        tails = {c[4] for c in er.ALL_CASES if c[1:3] == shape}
        assert tails == set(er.TAILS), shape


def test_lengths_cover_the_tail_classes():
    """The chooser against the schedules it is derived from."""
    from oracle import tomatis_oracle as orc
    for n_fft, hop in er.CORE:
        L = er.lengths("std", n_fft, hop)
        pes = {t: orc._std_schedule(N, n_fft, hop)[1] for t, N in L.items()}
        assert pes["tail0"] == 0 and pes["plus1"] == hop - 1 and 0 < pes["mid"] < hop - 1
        for N in L.values():
            assert er.F_MIN <= orc._std_schedule(N, n_fft, hop)[2] <= er.F_MAX
    # 2048 / 512: the goldens' tail classes
    L = er.lengths("std", 2048, 512)
    assert (L["tail0"] - 2048) % 512 == 0 and (L["mid"] - 2048) % 512 == 259
    # pe == 0 and hop | n_fft / 2: the last frame ends at N, sum w^2 == 0 at N - 1
    c, y64, s1, s2, D = er.reference(("std", 4096, 1024, 2, "tail0", "4096"))
    assert s2[-1] == 0.0 and 0.0 < s2[-2] < 1e-12
    # pe == 0 where hop does not divide n_fft / 2: the last frame ends
    # (n_fft / 2) % hop short of N, and the reference writes 0 / (0 + 1e-12)
    c, y64, s1, s2, D = er.reference(("std", 2048, 300, 2, "tail0", "generic hop"))
    end = c.geom["first_start"] + (c.geom["n_frames"] - 1) * 300 + 2048
    assert end == c.N - 1024 % 300
    assert not c.oref["y"][end:].any() and c.oref["y"][end - 300:end].any()
    assert not y64[end:].any() and not s2[end:].any() and (D[end:] > 0).all()
    # adaptive / no-pad static: sum w^2 == 0 at sample 0
    for case in (("adaptive", 2048, 512, 2, "mid", "adaptive 2048"),
                 ("static_nopad", 512, 128, 3, "plus1", "static LDS pow2")):
        c, y64, s1, s2, D = er.reference(case)
        assert s2[0] == 0.0 and (s2[:8] < cd.TAU).all()


@pytest.mark.parametrize("case", er.ALL_CASES, ids=er.case_id)
def test_numpy_float32_within_a_quarter_of_the_bound(case):
    c, y64, s1, s2, D = er.reference(case)
    y32, _, _ = er.run_ref(c, dtype=np.float32)
    assert y32.dtype == np.float32
    if c.oref is not None:
        assert len(set(np.unique(c.rows))) >= 2, "both gate states must occur"
    assert (D > 0).any()
    r_all, r_masked, zero = er.ratios(y32, y64, D, s2)
    n_masked = int(((s2 < cd.TAU) & (D > 0)).sum())
    print(f"RATIO [edge {c.path}] {er.case_id(case)}: numpy float32 max err/D all {r_all:.3f} "
          f"masked {r_masked:.3f} ({n_masked} masked samples, peak |y64| "
          f"{np.abs(y64).max() / c.out_scale:.3g})")
    assert r_all <= 0.25, (case, r_all, r_masked)
    assert zero == 0.0, (case, zero)


def _quarter(name, c, y64, s2, D):
    y32, _, _ = er.run_ref(c, dtype=np.float32)
    r_all, r_masked, zero = er.ratios(y32, y64, D, s2)
    print(f"RATIO [edge {c.path}] {name}: numpy float32 max err/D all {r_all:.3f} masked {r_masked:.3f}")
    assert r_all <= 0.25 and zero == 0.0, (name, r_all, r_masked, zero)


@pytest.mark.parametrize("batch", er.BATCHES, ids=er.batch_id)
def test_numpy_float32_on_the_ragged_batches(batch):
    """The three streams of a launch share the first one's gain table."""
    for case, (c, y64, s1, s2, D) in zip(er.batch_cases(batch), er.batch_references(batch)):
        _quarter(er.case_id(case) + " (batch)", c, y64, s2, D)


@pytest.mark.parametrize("silent", er.SILENT, ids=er.batch_id)
def test_numpy_float32_on_the_silent_edges(silent):
    """Silence over 2 n_fft at both ends: the reference is exactly zero over the
    first and last n_fft samples, and no ill-conditioned sample lies elsewhere."""
    c, y64, s1, s2, D = er.silent_reference(silent)
    n = c.n_fft
    assert not c.x[:2 * n].any() and not c.x[-2 * n:].any() and c.x.any()
    assert not y64[:n].any() and not y64[-n:].any()
    assert (s2[n:-n] >= cd.TAU).all()
    if c.mode != "adaptive":
        assert np.abs(y64).max() > 1.2, "the loud middle is over the limit"
    _quarter(er.case_id(c.case) + " (silent edges)", c, y64, s2, D)


@pytest.mark.parametrize("shape", er.CORE, ids=lambda s: f"{s[0]}/{s[1]}")
@pytest.mark.parametrize("mutation", [er.mutation_drop_last_frame_tail, er.mutation_wsum_late],
                         ids=["drop_last_frame_tail", "wsum_one_late"])
def test_mutations_exceed_the_bound_on_masked_samples(mutation, shape):
    n_fft, hop = shape
    mode = "xfade" if shape == (4096, 2048) else "std"
    for case in er.ALL_CASES:
        if case[:3] == (mode, n_fft, hop) and case[4] == "tail0" and case[3] == 2:
            break
    c, y64, s1, s2, D = er.reference(case)
    ym = mutation(c)
    err = np.abs(ym - y64).max(axis=1)
    masked = (s2 < cd.TAU) & (D > 0)
    assert masked.any()
    worst = float((err[masked] / D[masked]).max())
    visible = float((err[~masked & (D > 0)] / D[~masked & (D > 0)]).max())
    print(f"MUTATION {mutation.__name__} {er.case_id(case)}: max err/D masked {worst:.3g}, "
          f"unmasked {visible:.3g}")
    assert worst > 1.0, (case, worst)
