"""CPU: the pitch tracker's reference (tests/pitch_ref.py) against known answers, the comparison helper against deliberately wrong
variants, the conditions the GPU case list has to meet in float64 alone, the refusals of maua_yin_f32 (no device call is reached), and the
host-side logic of ar.pitch / ar.pitch_weight_latents / ar.raw_pitch on CPU tensors."""
import math
import warnings

import numpy as np
import pytest
import torch

import pitch_ref as pr

EINVAL = -22


# ------------------------------------------------------------------------------------------------ known answers
def test_float64_definition_finds_the_tones():
    """Sines, 3-harmonic complexes and missing-fundamental complexes at 70 .. 1318.5 Hz, sr 22050, frame 2048, hop 512, lags 10 .. 340,
    threshold 0.1, interior frames.  Measured: 1.937 cents worst (the 1318.5 Hz sine, 16.7 samples a period), aperiodicity <= 0.0073."""
    worst_cents, worst_ap = pr.tone_errors(np.float64)
    print(f"float64 definition: worst {worst_cents:.3f} cents, aperiodicity <= {worst_ap:.4f}")
    assert worst_cents <= pr.CENTS_BOUND
    assert worst_ap <= pr.APERIODICITY_BOUND


def test_fp32_emulation_finds_the_tones():
    """The same list through the all-fp32 emulation: the bound plus the emulation's lag figure, taken at the shortest lag."""
    worst_cents, worst_ap = pr.tone_errors(np.float32)
    print(f"fp32 emulation: worst {worst_cents:.3f} cents, aperiodicity <= {worst_ap:.4f}")
    assert worst_cents <= pr.CENTS_BOUND + 1200 * math.log2(1 + pr.LAG_TOL / pr.TONE_TAU_MIN)
    assert worst_ap <= pr.APERIODICITY_BOUND + pr.APERIODICITY_TOL


# ------------------------------------------------------------------------------------------------ the comparison helper
@pytest.fixture(scope="module")
def tone_ref():
    y = pr.tone("harmonics", 220.0, seconds=0.3)
    args = (y, pr.TONE_FRAME, pr.TONE_HOP, pr.TONE_TAU_MIN, pr.TONE_TAU_MAX, pr.TONE_THRESHOLD)
    return args, pr.yin(*args)


def test_helper_passes_the_definition_and_its_fp32_emulation(tone_ref):
    args, ref = tone_ref
    assert pr.compare(pr.yin(*args), ref) == []
    assert pr.compare(pr.yin(*args, dtype=np.float32), ref) == []
    assert pr.unambiguous(ref)[pr.TONE_SKIP:-pr.TONE_SKIP].all()


@pytest.mark.parametrize("variant,flagged", [
    (dict(normalise=False), "cmndf"),     # no division by the running mean
    (dict(lag_offset=1), "tau_int"),      # lag off by one
    (dict(descend=False), "tau_int"),     # the first lag under the threshold instead of the local minimum behind it
    (dict(clamp=False), "aperiodicity"),  # the parabola's minimum, unclamped, is negative on a clean tone
])
def test_helper_flags_each_defect(tone_ref, variant, flagged):
    args, ref = tone_ref
    if "clamp" in variant:  # (a high sine, 16.7 samples a period: the parabola's minimum is -0.0008; at 220 Hz it stays above zero)
        y = pr.tone("sine", 1318.5, seconds=0.3)
        args = (y,) + args[1:]
        ref = pr.yin(*args)
        assert (pr.yin(*args, **variant)["aperiodicity"] < 0).any()
    complaints = pr.compare(pr.yin(*args, **variant), ref)
    assert any(c.startswith(flagged) for c in complaints), complaints


# ------------------------------------------------------------------------------------------------ the GPU case list, float64 alone
def test_case_list_covers_the_sets_and_stays_small():
    cases = pr.gpu_cases()
    assert len({pr.case_id(c) for c in cases}) == len(cases)
    assert {c["frame"] for c in cases} == set(pr.FRAMES)
    assert {(c["tau_min"], c["tau_max"]) for c in cases} == set(pr.TAU_PAIRS)
    assert {c["signal"] for c in cases} == set(pr.EXACT_SIGNALS + pr.NOISY_SIGNALS)
    n_frames = [1 + c["n_samples"] // c["hop"] for c in cases]
    assert max(n_frames) <= pr.MAX_FRAMES and min(n_frames) == 1
    hops = {c["hop"] for c in cases}
    assert {1, 7, 512} <= hops and any(c["hop"] == c["n_samples"] + 3 for c in cases)
    spans = [(c["n_samples"], c["frame"] + c["tau_max"], c["hop"]) for c in cases]
    assert any(n == 1 for n, _, _ in spans) and any(n == 2 for n, _, _ in spans)
    assert any(n in (h - 1, h, h + 1) for n, _, h in spans)
    for delta in (-1, 0, 1):
        assert any(n == span + delta for n, span, _ in spans), delta
    assert any(n == 3 * span + 5 for n, span, _ in spans)


def test_case_list_meets_its_conditions_in_float64():
    """Per case at most 2 % of the frames (one below 50 frames) are ambiguous; the exact signals exempt nothing, and rounding their d' to
    fp32 moves no pick; zeros give d' = 1, tau_int = tau_min, aperiodicity = 1; the emulation passes the helper at the tolerances."""
    worst_exempt = 0
    for case in pr.gpu_cases():
        ref = pr.reference(case)
        emu = pr.reference(case, np.float32)
        n_frames = len(ref["lag"])
        exempt = int((~pr.unambiguous(ref)).sum())
        worst_exempt = max(worst_exempt, exempt)
        assert exempt <= pr.max_exempt(n_frames), (pr.case_id(case), exempt, n_frames)
        if pr.is_exact(case):
            assert exempt == 0
            assert np.array_equal(emu["tau_int"], ref["tau_int"]), pr.case_id(case)
        if case["signal"] == "zeros":
            assert (ref["cmndf"] == 1).all() and (ref["tau_int"] == case["tau_min"]).all() and (ref["aperiodicity"] == 1).all()
            assert (ref["lag"] == case["tau_min"]).all()
        tols = pr.tolerances(case)
        assert pr.compare(emu, ref, *tols, scaled=case["short"]) == [], pr.case_id(case)
        assert ((ref["tau_int"] >= case["tau_min"]) & (ref["tau_int"] <= case["tau_max"])).all()
    print(f"most ambiguous frames in one case: {worst_exempt}")


def test_square_wave_picks_the_smallest_multiple_of_its_period():
    case = dict(frame=65, tau_min=10, tau_max=60, hop=7, n_samples=400, signal="square", threshold=0.1, seed=0, short=False)
    ref = pr.reference(case)
    period = 2 * max(1, (case["tau_min"] + 2) // 2)
    inner = [t for t in range(len(ref["lag"])) if np.all(pr.frame_matrix(pr.make_signal(case), case["frame"], case["hop"], case["tau_max"])[t] != 0)]
    assert inner, pr.case_id(case)
    assert (ref["tau_int"][inner] == period).all() and (ref["aperiodicity"][inner] == 0).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_entry_refuses_each_violated_limit_without_a_device(built_lib):
    """One call per violated limit, the limit value itself on the other side.  A refusal is MAUA_EINVAL before any device call; where no
    device is visible the accepted call comes back with the runtime's error instead (it launches nothing there: the buffers are
    never dereferenced on the host).  With a device the accepted sides are the cases of tests/test_pitch_gpu.py."""
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    fake = 0x1000
    base = dict(y=fake, n=4096, frame=2048, hop=512, tau_min=10, tau_max=340, threshold=0.1, lag=fake, ap=fake, tau=fake, n_frames=None)

    def call(**kw):
        a = dict(base, **kw)
        if a["n_frames"] is None:
            a["n_frames"] = 1 + a["n"] // max(a["hop"], 1)
        return lib.maua_yin_f32(a["y"], a["n"], a["frame"], a["hop"], a["tau_min"], a["tau_max"], a["threshold"], a["lag"], a["ap"], a["tau"],
                                None, a["n_frames"], None)

    refused = [dict(frame=15), dict(frame=4097), dict(tau_min=0), dict(tau_min=340), dict(tau_min=341), dict(tau_max=2049), dict(hop=0),
               dict(hop=-1), dict(n=0), dict(threshold=-1e-6), dict(threshold=float("nan")), dict(threshold=float("inf")),
               dict(n_frames=8), dict(n_frames=10), dict(y=None), dict(lag=None), dict(ap=None), dict(tau=None)]
    for kw in refused:
        assert call(**kw) == EINVAL, kw
    if not torch.cuda.is_available():
        accepted = [dict(), dict(frame=16), dict(frame=4096), dict(tau_min=1), dict(tau_min=339), dict(tau_max=2048), dict(hop=1, n=40),
                    dict(n=1), dict(threshold=0.0), dict(n_frames=9)]
        for kw in accepted:
            assert call(**kw) > 0, kw


# ------------------------------------------------------------------------------------------------ host logic on CPU tensors
def test_hold_fill():
    from maua_stylegan2_amd.audioreactive import signal as sig

    v = torch.tensor([0.1, 0.2, 0.3, 0.4, 0.5, 0.6])
    b = lambda *bits: torch.tensor(bits, dtype=torch.bool)  # noqa: E731
    assert torch.equal(sig.hold_fill(v, b(0, 0, 1, 1, 0, 1)), torch.tensor([0.3, 0.3, 0.3, 0.4, 0.4, 0.6]))  # leading frames
    assert torch.equal(sig.hold_fill(v, b(1, 0, 1, 0, 0, 0)), torch.tensor([0.1, 0.1, 0.3, 0.3, 0.3, 0.3]))  # trailing frames
    assert sig.hold_fill(v, b(0, 0, 0, 0, 0, 0)) is None                                                      # nothing voiced
    assert torch.equal(sig.hold_fill(v, b(0, 0, 0, 1, 0, 0)), torch.full((6,), 0.4))                           # a single voiced frame
    assert torch.equal(sig.hold_fill(v, b(1, 1, 1, 1, 1, 1)), v)
    for bits in [(0, 0, 1, 1, 0, 1), (1, 0, 1, 0, 0, 0), (0, 0, 0, 1, 0, 0)]:  # the numpy restatement the GPU test leans on
        assert np.array_equal(pr.hold_fill(v.numpy(), np.array(bits, bool)), sig.hold_fill(v, b(*bits)).numpy())
    assert pr.hold_fill(v.numpy(), np.zeros(6, bool)) is None


def test_lerp_resize_keeps_end_points_and_steps():
    from maua_stylegan2_amd.audioreactive import signal as sig

    x = torch.tensor([0.0, 0.0, 1.0, 1.0, 0.25])
    for num in (1, 2, 5, 9, 13):
        y = sig.lerp_resize(x, num)
        assert y.shape == (num,) and y[0] == x[0] and (num == 1 or y[-1] == x[-1])
        assert float(y.min()) >= 0.0 and float(y.max()) <= 1.0  # no ringing
        assert np.allclose(y.numpy(), pr.lerp_resize(x.numpy(), num, np.float32), atol=1e-7)
    assert torch.equal(sig.lerp_resize(x, 9)[::2], x)
    assert torch.equal(sig.lerp_resize(x[:1], 4), torch.zeros(4))


def test_pitch_weight_latents():
    import maua_stylegan2_amd.audioreactive as ar

    m = 5
    latents = torch.randn(m, 3, 512, generator=torch.Generator().manual_seed(3))
    pitch = torch.tensor([0.0, 1.0, 0.5, 0.25, 0.75, 0.6, 0.125])
    out = ar.pitch_weight_latents(pitch, latents)
    assert out.shape == (7, 3, 512)
    assert torch.equal(out[0], latents[0]) and torch.equal(out[1], latents[4])                     # exactly 0, exactly 1
    assert torch.equal(out[2], latents[2]) and torch.equal(out[3], latents[1]) and torch.equal(out[4], latents[3])  # exactly on a key
    frac = torch.tensor(0.6) * 4 - 2
    assert torch.equal(out[5], (1 - frac) * latents[2] + frac * latents[3])
    assert torch.equal(out[6], 0.5 * latents[0] + 0.5 * latents[1])
    one = ar.pitch_weight_latents(pitch, latents[:1])                                               # m = 1
    assert one.shape == (7, 3, 512) and all(torch.equal(one[i], latents[0]) for i in range(7))


def test_raw_pitch_says_what_to_change():
    import maua_stylegan2_amd.audioreactive as ar

    y = np.zeros(4096, np.float32)
    with pytest.raises(ValueError, match="raise fmin to at least 10.77 Hz"):
        ar.raw_pitch(y, 22050, fmin=10.0)                 # ceil(22050 / 10) = 2205 > 2048
    with pytest.raises(ValueError, match="raise fmin to at least 21.53 Hz"):
        ar.raw_pitch(y, 44100, fmin=21.0)
    with pytest.raises(ValueError, match="lower fmax to at most 8000 Hz"):
        ar.raw_pitch(y, 8000, fmax=8001.0)                # floor(sr / fmax) = 0
    with pytest.raises(ValueError, match="lower fmin or raise fmax"):
        ar.raw_pitch(y, 22050, fmin=300.0, fmax=300.0)
    with pytest.raises(ValueError, match="lower fmin or raise fmax"):
        ar.raw_pitch(y, 22050, fmin=500.0, fmax=100.0)
    with pytest.raises(ValueError, match="frame_length"):
        ar.raw_pitch(y, 22050, frame_length=8192)


def test_pipeline_reference_holds_notes_through_silences():
    """The numpy pipeline the GPU test compares ar.pitch with: on the arpeggio the height climbs note by note, the silences hold the note
    before them, and the voicing envelope dips in them."""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        height, voicing, f0, conf = pr.arpeggio_reference()
    y, spans = pr.arpeggio()
    n = pr.ARPEGGIO_FRAMES
    centre = lambda lo, hi: int(round((lo + hi) / 2 / len(y) * (n - 1)))  # noqa: E731
    at_notes = [height[centre(lo, hi)] for lo, hi, _ in spans]
    want = [math.log2(f / pr.ARPEGGIO_FMIN) / math.log2(pr.ARPEGGIO_FMAX / pr.ARPEGGIO_FMIN) for _, _, f in spans]
    assert np.allclose(at_notes, want, atol=0.02), (at_notes, want)
    gaps = [centre(spans[i][1], spans[i + 1][0]) for i in range(3)]
    for i, g in enumerate(gaps):
        assert want[i] - 0.03 <= height[g] <= want[i + 1] + 0.03     # held (then smoothed toward the next note), never dropped to 0
        assert voicing[g] < min(voicing[centre(*spans[i][:2])], voicing[centre(*spans[i + 1][:2])]) - 0.1
    assert (conf >= 0).all() and (conf <= 1).all()
