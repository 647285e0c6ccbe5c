"""CPU: the predominant-local-pulse definition of tests/pulse_ref.py on known answers (steady clicks, a tempo switch, silence, priors,
ties), the host-side pieces of audioreactive/beat.py (beat picking, beat phase, detrending) against it, the case lists' own
preconditions, the two entries' refusals, and four deliberately wrong variants that the comparison functions of the GPU tests must
catch."""
import warnings

import numpy as np
import pytest
import torch

import pulse_ref as q

GRID = q.tempo_grid()
HALF = q.WIN / (2 * q.FR)  # seconds from a frame to the end of its window


def frames_of(duration):
    return int(duration * q.FR) + 1


def nearest(beats, clicks):
    return np.abs(np.asarray(beats)[None, :] - np.asarray(clicks)[:, None]).min(axis=1)


# ------------------------------------------------------------------------------------------------ known answers
@pytest.fixture(scope="module")
def steady():
    clicks = q.click_times(120.0, 30.0)
    n = frames_of(30.0)
    return clicks, n, q.plp(q.click_envelope(clicks, n), GRID)


def test_steady_clicks_read_120_bpm_and_one_maximum_per_click(steady):
    clicks, n, (pulse, tempo, power) = steady
    inner = np.arange(q.WIN // 2 + 1, n - q.WIN // 2 - 1)
    assert np.all(np.abs(tempo[inner] - 120.0) <= 1.0), np.unique(tempo[inner])
    beats = q.pick_beats(pulse)
    off = nearest(beats, clicks)
    print(f"steady: {len(beats)} maxima for {len(clicks)} clicks, worst {off.max():.4f} s, pulse in the middle {pulse[inner].max():.3f}")
    assert len(beats) == len(clicks)
    assert off.max() <= 1.0 / q.FR
    assert 0.9 < pulse[inner].max() <= 1.0 + 1e-6 and pulse.min() >= 0


@pytest.fixture(scope="module")
def switch():
    a, b = q.switch_times()
    n = frames_of(60.0)
    return a, b, n, q.plp(q.click_envelope(np.concatenate([a, b]), n), GRID)


def test_tempo_switch_is_followed(switch):
    a, b, n, (pulse, tempo, _) = switch
    t = np.arange(n) / q.FR
    before = (t > HALF + 2 / q.FR) & (t < 30.0 - HALF - 2 / q.FR)
    after = (t > 30.0 + HALF + 2 / q.FR) & (t < 60.0 - HALF - 2 / q.FR)
    assert before.sum() > 100 and after.sum() > 100
    assert np.all(np.abs(tempo[before] - 100.0) <= 1.0), np.unique(tempo[before])
    assert np.all(np.abs(tempo[after] - 150.0) <= 1.0), np.unique(tempo[after])
    beats = q.pick_beats(pulse)
    zone = (30.0 - HALF - 0.5, 30.0 + HALF + 0.5)
    clicks = np.concatenate([a, b])
    outside = clicks[(clicks < zone[0]) | (clicks > zone[1])]
    beats_outside = beats[(beats < zone[0]) | (beats > zone[1])]
    off = nearest(beats, outside)
    print(f"switch: {len(beats_outside)} maxima for {len(outside)} clicks outside {zone[0]:.1f} .. {zone[1]:.1f} s, worst {off.max():.4f} s")
    assert off.max() <= 1.0 / q.FR
    assert len(beats_outside) == len(outside)  # no extra maxima


def test_silence_gives_zeros_no_beats_no_nan():
    pulse, tempo, power = q.plp(np.zeros(500, np.float32), GRID)
    assert np.all(pulse == 0) and np.all(power == 0) and np.all(np.isnan(tempo))
    assert len(q.pick_beats(pulse)) == 0
    a = q.tempogram_peak(np.zeros(500, np.float32), q.make_table(q.hann(q.WIN), q.omega_of(GRID)))
    assert np.all(a["bin"] == -1) and np.all(a["phase"] == 0) and not a["exempt"].any()
    emu = q.pulse_synth(a["bin"], a["phase"], q.hann(q.WIN), q.omega_of(GRID), np.float32)
    assert np.all(emu == 0)


def test_a_prior_selects_the_half_or_the_double_tempo():
    """A click train has a Fourier component of about the same strength at every multiple of its rate: which one a frame reports is the
    prior's to say.  Clicks at 120 BPM read 120 without a prior and 240 with a prior around 240; clicks at 60 BPM (components at 60, 120,
    180, 240, 300) read 60 under a prior around 60 and 240 under one around 240."""
    n = frames_of(30.0)
    inner = np.arange(q.WIN // 2 + 1, n - q.WIN // 2 - 1)
    for rate, start, bpm in ((120.0, None, 120.0), (120.0, 60.0, 120.0), (120.0, 240.0, 240.0), (60.0, 60.0, 60.0), (60.0, 240.0, 240.0)):
        env = q.click_envelope(q.click_times(rate, 30.0), n)
        prior = None if start is None else q.lognormal_prior(GRID, start)
        _, tempo, _ = q.plp(env, GRID, prior=prior)
        assert np.all(np.abs(tempo[inner] - bpm) <= 1.0), (rate, start, np.unique(tempo[inner]))
    assert q.lognormal_prior(GRID, 120.0)[90] == 1 and abs(q.lognormal_prior(GRID, 120.0)[30] - np.exp(-0.5)) < 1e-7  # 120 and 60 BPM


def test_ties_go_to_the_lowest_bin():
    case = dict(n=40, win=8, n_tempi=6, kind="integer", seed=3, grid="integer")  # rows 0, 2, 4 and rows 1, 3, 5 are the same
    env, table = q.make_env(case), q.case_table(case)
    assert np.array_equal(table[0], table[2]) and np.array_equal(table[1], table[3])
    a = q.tempogram_peak(env, table)
    assert np.array_equal(a["S"][:, 0], a["S"][:, 4]) and set(np.unique(a["bin"])) <= {0, 1}
    high = q.tempogram_peak(env, table, variant="ties_high")
    assert set(np.unique(high["bin"])) <= {4, 5}
    re, im, S, _ = q.emulate_peak(env, table)
    assert np.array_equal(S.astype(np.float64), a["S"])  # integers: float32 is exact
    walked = []
    for row in S:  # the walk as the header states it
        best, at = 0.0, -1
        for b, s in enumerate(row):
            if s > best:
                best, at = s, b
        walked.append(at)
    assert np.array_equal(walked, a["bin"])
    nan_row = np.full((1, 4), np.nan)
    assert q.walk_peak(nan_row)[0][0] == -1 and q.walk_peak(np.array([[np.nan, 2.0, np.nan, 2.0]]))[0][0] == 1


# ------------------------------------------------------------------------------------------------ host pieces of the product
def test_beat_phase_from_times_hits_exact_rationals():
    import maua_stylegan2_amd.audioreactive as ar

    times = [1.0, 2.0, 3.0, 4.0]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        one = ar.beat_phase_from_times(times, 8.0, 16, 1)
        two = ar.beat_phase_from_times(times, 8.0, 16, 2)
        quarter = ar.beat_phase_from_times(times, 8.0, 16, 0.25)
        uneven = ar.beat_phase_from_times([1.0, 2.0, 4.0], 8.0, 16, 1)
    assert one.dtype == torch.float32 and one.device.type == "cpu" and one.shape == (16,)
    tau = np.arange(16) / 2.0  # count = tau - 1, extended before the first beat and after the last
    assert np.array_equal(one.numpy(), ((tau - 1) % 1).astype(np.float32))
    assert np.array_equal(one.numpy()[:4], np.float32([0, 0.5, 0, 0.5])) and np.all(two.numpy() == 0)
    assert np.array_equal(quarter.numpy(), ((0.25 * (tau - 1)) % 1).astype(np.float32))
    assert quarter[0] == 0.75 and quarter[2] == 0 and quarter[10] == 0  # one cycle per four beats: b_0 and b_0 + 4 beats
    # intervals of 1 s and 2 s: the second is walked at half the rate, and carries on behind the last beat
    assert np.array_equal(uneven.numpy(), np.float32([0, .5, 0, .5, 0, .25, .5, .75, 0, .25, .5, .75, 0, .25, .5, .75]))
    for div in (1, 2, 0.25):
        assert np.array_equal(ar.beat_phase_from_times(times, 8.0, 16, div).numpy().astype(np.float64), q.beat_phase_from_times(times, 8.0, 16, div))
    for few in ([], [3.0]):
        with pytest.warns(UserWarning, match="need two"):
            z = ar.beat_phase_from_times(few, 8.0, 16)
        assert z.shape == (16,) and not z.any()
    with pytest.raises(ValueError, match="increasing"):
        ar.beat_phase_from_times([1.0, 1.0, 2.0], 8.0, 16)
    rng = np.random.RandomState(0)
    wild = ar.beat_phase_from_times(np.cumsum(rng.uniform(0.2, 0.9, 40)), 25.0, 1000, 3)
    assert float(wild.min()) >= 0 and float(wild.max()) < 1


def test_beat_picking_and_detrending_of_the_product_equal_the_restatement(steady):
    from maua_stylegan2_amd.audioreactive import beat

    _, n, (pulse, _, _) = steady
    got = beat.pick_beats(torch.from_numpy(pulse.astype(np.float32)), q.FR).numpy()
    want = q.pick_beats(pulse.astype(np.float32), q.FR)
    assert got.dtype == np.float64 and np.allclose(got, want, rtol=0, atol=1e-12) and len(got) == len(want)
    assert len(beat.pick_beats(torch.zeros(2), q.FR)) == 0
    flat = torch.tensor([0.0, 0.5, 0.5, 0.2, 0.05, 0.08, 0.05])  # a plateau counts once (its first sample); 0.08 is under the threshold
    assert np.allclose(beat.pick_beats(flat, 1.0).numpy(), q.pick_beats(flat.numpy(), 1.0)) and len(beat.pick_beats(flat, 1.0)) == 1
    env = np.random.RandomState(1).random_sample(1000).astype(np.float32)
    for win in (2, 3, 384):
        d = beat.moving_average_detrend(torch.from_numpy(env), win).numpy()
        assert np.abs(d - q.detrend(env, win)).max() < 1e-6 and d.min() >= 0
    assert np.array_equal(beat.tempo_grid(), q.tempo_grid()) and len(beat.tempo_grid()) == 271
    with pytest.raises(ValueError, match="at most 1024"):
        beat.tempo_grid(30, 300, 0.1)


def test_case_lists_cover_the_shapes_and_keep_the_exempt_cap():
    cases = q.a_cases() + [q.LONG_CASE]
    assert {1, q.TILE, 2 * q.TILE + 5, 20000} <= {c["n"] for c in cases}
    for w in (2, 3, 33, 384, 2048):
        assert {w - 1, w, w + 1} <= {c["n"] for c in cases if c["win"] == w}, w
    assert {1, 2, 63, 64, 65, 271, 1024} <= {c["n_tempi"] for c in cases}
    rounds = [c for c in cases if c["n_tempi"] in (3, 4, 47, 48, 49, 97)]   # three tempi per wave, sixteen waves: 48 a round
    assert {c["n_tempi"] for c in rounds} == {3, 4, 47, 48, 49, 97} and all((c["n"], c["win"]) == (65, 33) for c in rounds)
    assert sum(bool(c.get("prior")) for c in rounds) >= 2 and sum(bool(c.get("tgram")) for c in rounds) >= 2
    assert {"random", "click", "zero"} <= {c["kind"] for c in cases}
    for flag in ("prior", "tgram"):
        assert any(c.get(flag) for c in cases) and any(not c.get(flag) for c in cases)
    for c in cases[:-1]:  # (the long case is checked by the GPU test that uses it)
        env, table, prior, ref, tol = q.a_reference(c)  # asserts the cap
        assert 4 * tol[0] < 1 and 4 * tol[1] < 1, (q.case_id(c), tol)
    assert {q.BLOCK, 2 * q.BLOCK + 5, 20000} <= {c["n"] for c in q.b_cases()}
    assert any((q.pulse_synth(*q.b_operands(c)) == 0).all() for c in q.b_cases() if c.get("window") == "zero_middle")


def test_entries_refuse_bad_arguments_before_any_device_call(built_lib):
    from maua_stylegan2_amd import _lib

    lib, fake = _lib.load(), 0x1000  # never dereferenced
    a = lambda env=fake, n=10, table=fake, win=384, b=271, bin_=fake, ph=fake, pw=fake: lib.maua_tempogram_peak_f32(  # noqa: E731
        env, n, table, win, b, None, bin_, ph, pw, None, None)
    s = lambda bin_=fake, ph=fake, n=10, w=fake, win=384, om=fake, b=271, out=fake: lib.maua_pulse_synth_f32(  # noqa: E731
        bin_, ph, n, w, win, om, b, out, None)
    for call in (a, s):
        for kw in (dict(n=0), dict(n=-1), dict(n=(1 << 22) + 1), dict(win=1), dict(win=2049), dict(b=0), dict(b=1025), dict(bin_=None), dict(ph=None)):
            assert call(**kw) == -22, kw
    assert a(env=None) == -22 and a(table=None) == -22 and a(pw=None) == -22
    assert s(w=None) == -22 and s(om=None) == -22 and s(out=None) == -22


# ------------------------------------------------------------------------------------------------ the comparisons catch wrong kernels
WRONG_CASE = dict(n=2 * q.TILE + 5, win=33, n_tempi=8, kind="random", seed=77)


def as_outputs(a, tgram=True):
    return dict(bin=a["bin"], phase=a["phase"].astype(np.float32), power=a["power"].astype(np.float32),
                tgram=a["S"].astype(np.float32) if tgram else None)


def test_the_comparison_accepts_the_emulation_and_catches_wrong_variants():
    env, table, prior, ref, tol = q.a_reference(WRONG_CASE)
    re, im, S, _ = q.emulate_peak(env, table, prior)
    bins, power = q.walk_peak(S)
    rows, at = np.arange(len(env)), np.maximum(bins, 0)
    emu = dict(bin=bins, power=power, phase=np.where(bins >= 0, np.arctan2(im[rows, at], re[rows, at]), 0).astype(np.float32), tgram=S)
    assert q.compare_peak(emu, ref, tol) == []
    assert q.compare_peak(as_outputs(ref), ref, tol) == []
    flipped = q.compare_peak(as_outputs(q.tempogram_peak(env, table, prior, variant="phase_sign")), ref, tol)
    assert any(p.startswith("phase") for p in flipped) and not any(p.startswith(("bin", "power", "tgram")) for p in flipped)
    shifted = q.compare_peak(as_outputs(q.tempogram_peak(env, table, prior, variant="centre")), ref, tol)
    assert any(p.startswith("tgram") for p in shifted) and any(p.startswith("power") for p in shifted)
    # ties: the integer case, where they are exact
    case = dict(n=40, win=8, n_tempi=6, kind="integer", seed=3, grid="integer")
    ienv, itab = q.make_env(case), q.case_table(case)
    assert np.array_equal(q.emulate_peak(ienv, itab)[2].astype(np.float64), q.tempogram_peak(ienv, itab)["S"])  # float32 is exact here
    iref = q.tempogram_peak(ienv, itab, exact=True)
    itol = q.peak_tolerances(ienv, itab, None, iref)
    assert q.compare_peak(as_outputs(iref), iref, itol) == []
    high = q.compare_peak(as_outputs(q.tempogram_peak(ienv, itab, variant="ties_high", exact=True)), iref, itol)
    assert any(p.startswith("bin") for p in high)


def test_the_pulse_comparison_catches_a_constant_denominator():
    case = dict(n=2 * q.BLOCK + 5, win=33, n_tempi=63, kind="steady", seed=78)
    bins, phase, w, om = q.b_operands(case)
    ref = q.pulse_synth(bins, phase, w, om)
    tol = q.synth_tolerance(bins, phase, w, om, ref)
    assert q.compare_pulse(q.pulse_synth(bins, phase, w, om, np.float32), ref, tol) == []
    wrong = q.pulse_synth(bins, phase, w, om, variant="den_const")
    assert np.abs(wrong[40:100] - ref[40:100]).max() <= tol  # the interior agrees: only the edges tell
    assert q.compare_pulse(wrong, ref, tol) != []
