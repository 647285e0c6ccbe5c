"""GPU: the pitch features built on maua_yin_f32 — ar.raw_pitch on known tones, ar.pitch end to end on a synthetic arpeggio against the
same pipeline in float64 numpy (tests/pitch_ref.py), ar.pitch_weight_latents on device tensors, and the shipped examples/melody.py plugin
through generate() on the seeded 32-px generator."""
import argparse
import math
import random
import warnings

import numpy as np
import pytest
import torch

import pitch_ref as pr
from maua_stylegan2_amd import seeding

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture()
def ar(gpu):
    import maua_stylegan2_amd.audioreactive as ar

    before = ar.signal.SMF
    ar.set_SMF(1)
    yield ar
    ar.set_SMF(before)


def test_raw_pitch_finds_the_tones(ar):
    """The host test's tone list through the defaults of ar.raw_pitch (lags 10 .. 340 at 22050 Hz): the reference's bound plus the lag
    tolerance at the shortest lag; a clean tone is voiced."""
    bound = pr.CENTS_BOUND + 1200 * math.log2(1 + pr.LAG_TOL / pr.TONE_TAU_MIN)
    worst_cents, least_conf = 0.0, 1.0
    inner = slice(pr.TONE_SKIP, -pr.TONE_SKIP)
    for kind, freq in pr.tone_cases():
        f0, conf = ar.raw_pitch(pr.tone(kind, freq, seconds=0.5), pr.TONE_SR)
        assert f0.is_cuda and conf.is_cuda and f0.shape == conf.shape == (1 + 11025 // 512,)
        worst_cents = max(worst_cents, float(pr.cents(f0[inner].cpu().numpy(), freq).max()))
        least_conf = min(least_conf, float(conf[inner].min()))
    print(f"ar.raw_pitch: worst {worst_cents:.3f} cents (bound {bound:.3f}), confidence >= {least_conf:.4f}")
    assert worst_cents <= bound
    assert least_conf >= 0.98


def test_pitch_on_an_arpeggio_equals_the_float64_pipeline(ar):
    """ar.pitch(margin=None) — the YIN kernel, hold-fill, the 5-tap median kernel, linear interpolation, the FIR kernel — against the same
    steps in float64 numpy on the float64 YIN.  Tolerance: 4 x the error of the all-fp32 emulation of the whole chain (pitch_ref.py:
    height 4.24e-8, voicing 5.97e-7)."""
    y, spans = pr.arpeggio()
    n = pr.ARPEGGIO_FRAMES
    want_h, want_v, _, _ = pr.arpeggio_reference()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        height, voicing = ar.pitch(y, pr.TONE_SR, n, margin=None, return_voicing=True)
        alone = ar.pitch(y, pr.TONE_SR, n, margin=None)
        on_dev, v_dev = ar.pitch(y, pr.TONE_SR, n, margin=None, return_voicing=True, device="cuda")
    assert height.device.type == "cpu" and voicing.device.type == "cpu" and on_dev.is_cuda and v_dev.is_cuda
    assert height.shape == voicing.shape == (n,) and height.dtype == torch.float32
    assert torch.equal(alone, height) and torch.equal(on_dev.cpu(), height) and torch.equal(v_dev.cpu(), voicing)
    err_h = float(np.abs(height.numpy().astype(np.float64) - want_h).max())
    err_v = float(np.abs(voicing.numpy().astype(np.float64) - want_v).max())
    print(f"ar.pitch against float64: height {err_h:.3g} (tolerance {pr.PIPELINE_HEIGHT_TOL:.3g})  voicing {err_v:.3g} ({pr.PIPELINE_VOICING_TOL:.3g})")
    centre = lambda lo, hi: int(round((lo + hi) / 2 / len(y) * (n - 1)))  # noqa: E731
    level = [math.log2(f / pr.ARPEGGIO_FMIN) / math.log2(pr.ARPEGGIO_FMAX / pr.ARPEGGIO_FMIN) for _, _, f in spans]
    for i in range(3):  # the silences hold the note before them (smoothed toward the next one), the voicing envelope dips
        gap = centre(spans[i][1], spans[i + 1][0])
        assert level[i] - 0.03 <= float(height[gap]) <= level[i + 1] + 0.03
        assert float(voicing[gap]) < min(float(voicing[centre(*spans[i][:2])]), float(voicing[centre(*spans[i + 1][:2])])) - 0.1
    assert err_h <= pr.PIPELINE_HEIGHT_TOL
    assert err_v <= pr.PIPELINE_VOICING_TOL


def test_pitch_of_silence_is_zeros_with_a_warning(ar):
    with pytest.warns(UserWarning, match="no frame reaches the voicing confidence"):
        out = ar.pitch(np.zeros(8000, np.float32), pr.TONE_SR, 12, margin=None)
    assert torch.equal(out, torch.zeros(12))


def test_pitch_weight_latents_on_the_device_equals_the_cpu_bit_for_bit(ar, gpu):
    """One multiply, one floor, one subtraction and the two-term blend, each a separately rounded elementwise op on either device:
    bit for bit."""
    gen = torch.Generator().manual_seed(8)
    latents = torch.randn(7, 6, 512, generator=gen)
    pitch = torch.cat([torch.rand(61, generator=gen), torch.tensor([0.0, 1.0, 0.5, 1 / 6])])
    want = ar.pitch_weight_latents(pitch, latents)
    got = ar.pitch_weight_latents(pitch.to(gpu), latents.to(gpu))
    assert got.is_cuda and torch.equal(got.cpu(), want)
    assert torch.equal(ar.pitch_weight_latents(pitch, latents.to(gpu)).cpu(), want)  # a CPU envelope follows the latents' device


# ------------------------------------------------------------------------------------------------ examples/melody.py through generate()
SIZE, FPS, BATCH, SR = 32, 16, 4, 22050


def two_note_clip():
    """One second: 110 Hz then 440 Hz (harmonics 1-3), with a short noise burst in each half for the onset envelopes."""
    t = np.arange(SR // 2, dtype=np.float64) / SR
    note = lambda f: 0.4 * sum(np.sin(2 * np.pi * h * f * t) / h for h in (1, 2, 3))  # noqa: E731
    y = np.concatenate([note(110.0), note(440.0)])
    rng = np.random.default_rng(21)
    for at in (SR // 4, 3 * SR // 4):
        y[at: at + 400] += 0.3 * rng.standard_normal(400) * np.exp(-np.arange(400) / 80.0)
    return y.astype(np.float32)


def test_melody_plugin_through_generate(ar, gpu, tmp_path, monkeypatch):
    from maua_stylegan2_amd import generate_audiovisual as gav
    from maua_stylegan2_amd import render
    from maua_stylegan2_amd.audioreactive.examples import melody
    from maua_stylegan2_amd.models.stylegan2 import Generator

    g = Generator(SIZE, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(SIZE, seed=60, rgb_gain=0.3), strict=True)
    g = g.to(gpu).eval()
    monkeypatch.setattr(render, "_output_dims", lambda out_size: (SIZE, SIZE))
    monkeypatch.setattr(render.shutil, "which", lambda name: None)
    for name in ("MAUA_SUBFRAMES", "MAUA_SHUTTER", "MAUA_SHUTTER_LIGHT", "MAUA_PIPE_PIX_FMT"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.chdir(tmp_path)
    clip = two_note_clip()
    monkeypatch.setattr(ar, "load_audio", lambda audio_file, offset, duration: (clip, SR, 1.0))
    monkeypatch.setattr(gav, "load_generator", lambda **kw: g)
    np.save("lat.npy", seeding.seeded_latents(8, g.n_latent, seed=11).numpy())

    captured, seen = [], {}
    orig_capture = g.capture_graph

    def capture(batch, lane=0, **kw):
        captured.append([type(b["transform"]).__name__ for b in kw.get("bends") or []])
        assert all(hasattr(b["transform"], "run_static") for b in kw["bends"])
        return orig_capture(batch, lane=lane, **kw)

    def initialize(args):
        args = melody.initialize(args)
        seen["melody"], seen["bass"] = args.melody.clone(), args.bass_line.clone()
        return args

    monkeypatch.setattr(g, "capture_graph", capture)

    def run(name):
        random.seed(5), np.random.seed(5), torch.manual_seed(5), torch.cuda.manual_seed_all(5)
        args = argparse.Namespace(fps=FPS, latent_count=8)
        out = gav.generate(ckpt=None, audio_file="stub.wav", initialize=initialize, get_latents=melody.get_latents, get_noise=melody.get_noise,
                           get_bends=melody.get_bends, latent_file="lat.npy", G_res=SIZE, out_size=SIZE, fps=FPS, batch=BATCH,
                           output_file=str(tmp_path / name), args=args)
        return np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(-1, SIZE, SIZE, 3)

    first = run("first.mp4")
    assert first.shape[0] == FPS and first.std() > 5
    assert captured and all(names == ["Swirl"] for names in captured), captured  # the bend ran inside the captured forward
    tune = seen["melody"]
    assert tune.shape == (FPS,) and float(tune.min()) >= 0 and float(tune.max()) <= 1
    low, high = float(tune[2:6].mean()), float(tune[10:14].mean())
    want = [math.log2(f / 65.0) / math.log2(2100.0 / 65.0) for f in (110.0, 440.0)]
    print(f"melody height: low half {low:.3f} (110 Hz = {want[0]:.3f}), high half {high:.3f} (440 Hz = {want[1]:.3f})")
    assert abs(low - want[0]) < 0.05 and abs(high - want[1]) < 0.05
    assert seen["bass"].shape == (FPS,) and bool(torch.isfinite(seen["bass"]).all())
    halves = np.abs(first[2:6].astype(np.int16) - first[10:14]).mean()
    within = np.abs(first[2:5].astype(np.int16) - first[3:6]).mean()
    print(f"mean |low-note frames - high-note frames| {halves:.2f} grey levels, between neighbours of the low half {within:.2f}")
    assert halves > 0 and halves > within
    n_captured = len(captured)
    second = run("second.mp4")
    assert np.array_equal(first, second)
    assert len(captured) >= n_captured
