"""GPU: the beat and tempo features of audioreactive/beat.py on synthetic audio with known beats — noise bursts every 0.5 s, and a
100 -> 150 BPM switch — the chain link by link against tests/pulse_ref.py on the device's own envelope, the unchanged dynamic-programming
tracker and segmentation, silence, refusals, and the shipped examples/onbeat.py plugin through generate()."""
import argparse
import random
import warnings

import numpy as np
import pytest
import torch

import pulse_ref as q
import segment_ref
from maua_stylegan2_amd import seeding

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SR = q.SR
HALF = q.WIN / (2 * q.FR)     # seconds from a frame to the end of its analysis window
BEAT_TOL = 1.5 / q.FR         # 35 ms: one and a half envelope frames


def burst_clip(times, duration, seed=0):
    """10 ms bursts of white noise at ``times`` (seconds) in ``duration`` seconds of silence."""
    rng = np.random.default_rng(seed)
    y = np.zeros(int(duration * SR), np.float32)
    for t in times:
        at = int(round(t * SR))
        y[at: at + SR // 100] = 0.5 * rng.standard_normal(min(SR // 100, len(y) - at)).astype(np.float32)
    return y


STEADY_CLICKS = np.arange(0.25, 20.0, 0.5)
SWITCH_A, SWITCH_B = np.arange(0.3, 20.0 - 1e-9, 0.6), np.arange(20.0, 40.0 - 0.2, 0.4)


@pytest.fixture(scope="module")
def steady_clip():
    return burst_clip(STEADY_CLICKS, 20.0)


@pytest.fixture(scope="module")
def switch_clip():
    return burst_clip(np.concatenate([SWITCH_A, SWITCH_B]), 40.0, seed=1)


@pytest.fixture()
def ar(gpu):
    import maua_stylegan2_amd.audioreactive as ar

    before = ar.signal.SMF
    ar.set_SMF(1)
    yield ar
    ar.set_SMF(before)


def nearest(beats, clicks):
    return np.abs(np.asarray(beats)[None, :] - np.asarray(clicks)[:, None]).min(axis=1)


# ------------------------------------------------------------------------------------------------ known answers
def test_beats_and_tempo_on_steady_clicks(ar, steady_clip):
    beats = ar.beats(steady_clip, SR)
    assert isinstance(beats, np.ndarray) and beats.dtype == np.float64 and np.all(np.diff(beats) > 0)
    inner = STEADY_CLICKS[(STEADY_CLICKS > HALF) & (STEADY_CLICKS < 20.0 - HALF)]
    off = nearest(beats, inner)
    n = 480
    bpm = ar.tempo(steady_clip, SR, n)
    t = np.arange(n) * 20.0 / (n - 1)
    there = (t > HALF + 0.1) & (t < 20.0 - HALF - 0.1)
    print(f"steady: {len(beats)} beats for {len(STEADY_CLICKS)} clicks, worst {1e3 * off.max():.1f} ms from an inner click (bound {1e3 * BEAT_TOL:.1f}); "
          f"tempo there {float(bpm[there].min()):.2f} .. {float(bpm[there].max()):.2f}")
    assert off.max() <= BEAT_TOL
    assert bpm.shape == (n,) and bpm.device.type == "cpu" and bpm.dtype == torch.float32
    assert float((bpm[there] - 120.0).abs().max()) <= 1.0
    between = beats[(beats > HALF) & (beats < 20.0 - HALF)]
    assert len(between) == len(inner)  # no extra maxima


def test_beats_and_tempo_follow_a_switch(ar, switch_clip):
    beats = ar.beats(switch_clip, SR)
    clicks = np.concatenate([SWITCH_A, SWITCH_B])
    clear = (clicks > HALF) & (clicks < 40.0 - HALF) & (np.abs(clicks - 20.0) > HALF)
    off = nearest(beats, clicks[clear])
    n = 960
    bpm = ar.tempo(switch_clip, SR, n, device="cuda")
    assert bpm.is_cuda
    bpm = bpm.cpu()
    t = np.arange(n) * 40.0 / (n - 1)
    before = (t > HALF + 0.1) & (t < 20.0 - HALF - 0.1)
    after = (t > 20.0 + HALF + 0.1) & (t < 40.0 - HALF - 0.1)
    print(f"switch: worst {1e3 * off.max():.1f} ms on {int(clear.sum())} clear clicks; tempo before {float(bpm[before].min()):.2f} .. {float(bpm[before].max()):.2f}, "
          f"after {float(bpm[after].min()):.2f} .. {float(bpm[after].max()):.2f}")
    assert off.max() <= BEAT_TOL
    assert float((bpm[before] - 100.0).abs().max()) <= 1.0 and float((bpm[after] - 150.0).abs().max()) <= 1.0


def test_beat_phase_is_a_sawtooth_through_the_beats(ar, steady_clip):
    n = 480
    beats = ar.beats(steady_clip, SR)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        phase = ar.beat_phase(steady_clip, SR, n)
        half = ar.beat_phase(steady_clip, SR, n, division=2)
        on_dev = ar.beat_phase(steady_clip, SR, n, device="cuda")
        curve = ar.pulse(steady_clip, SR, n)
        curve_dev = ar.pulse(steady_clip, SR, n, smooth=2, power=2, device="cuda")
    assert phase.shape == curve.shape == (n,) and phase.dtype == curve.dtype == torch.float32
    assert phase.device.type == "cpu" and curve.device.type == "cpu" and on_dev.is_cuda and curve_dev.is_cuda and curve_dev.shape == (n,)
    assert torch.equal(on_dev.cpu(), phase)
    assert float(phase.min()) >= 0 and float(phase.max()) < 1 and float(curve.min()) >= 0 and float(curve.max()) <= 1 + 1e-6
    duration = len(steady_clip) / SR
    assert torch.equal(phase, ar.beat_phase_from_times(beats, duration, n))
    assert torch.equal(half, ar.beat_phase_from_times(beats, duration, n, 2))
    assert np.abs(phase.numpy() - q.beat_phase_from_times(beats, duration, n)).max() < 1e-6
    tau = np.arange(n) * duration / n
    p = phase.numpy()
    for lo, hi in zip(beats[:-1], beats[1:]):  # strictly rising between consecutive beats
        inside = p[(tau >= lo) & (tau < hi)]
        assert len(inside) >= 2 and np.all(np.diff(inside) > 0)
    raw = ar.raw_plp(steady_clip, SR)
    assert all(v.is_cuda and v.shape == (1 + len(steady_clip) // 512,) for v in raw)
    assert float(raw[0].max()) > 0.9  # a steady pulse reaches about 1


# ------------------------------------------------------------------------------------------------ the chain, link by link
@pytest.mark.parametrize("prior", [None, "lognormal"])
def test_raw_plp_link_by_link(ar, switch_clip, prior):
    """The device's onset envelope through the numpy detrending; the device's detrended envelope through the float64 restatement of the
    first entry (the tolerances of the entry test); the device's (bin, phase) through that of the second."""
    from maua_stylegan2_amd.audioreactive import beat

    s = beat._plp_stages(switch_clip, SR, prior=prior, want_tgram=True)
    dev = {k: v.cpu().numpy() for k, v in s.items() if isinstance(v, torch.Tensor)}
    n = 1 + len(switch_clip) // 512
    assert dev["onset"].shape == (n,) and len(s["grid"]) == 271 and s["fr"] == q.FR
    want_env = q.detrend(dev["onset"], q.WIN)
    assert np.abs(dev["env"] - want_env).max() <= 1e-6 * max(1.0, float(want_env.max()))
    om = q.omega_of(s["grid"])
    assert dev["table"].tobytes() == q.make_table(q.hann(q.WIN), om).tobytes()  # both sides read the same float32 table
    assert dev["window"].tobytes() == q.hann(q.WIN).astype(np.float32).tobytes() and dev["omega"].tobytes() == om.astype(np.float32).tobytes()
    p = None if prior is None else q.lognormal_prior(s["grid"])
    assert prior is None or np.abs(dev["prior"] - p).max() <= 1e-7
    p = None if prior is None else dev["prior"]
    ref = q.tempogram_peak(dev["env"], dev["table"], p)
    n_exempt = int(ref["exempt"].sum())
    tol = q.peak_tolerances(dev["env"], dev["table"], p, ref)
    print(f"prior={prior}: {n_exempt} of {n} frames exempt; tolerances 4 x {tol[0]:.3g}, 4 x {tol[1]:.3g}, 4 x {tol[2]:.3g}")
    assert n_exempt <= q.max_exempt(n)
    assert q.compare_peak(dict(bin=dev["bin"], phase=dev["phase"], power=dev["power"], tgram=dev["tgram"]), ref, tol) == []
    want_pulse = q.pulse_synth(dev["bin"], dev["phase"], dev["window"], dev["omega"])
    assert q.compare_pulse(dev["pulse"], want_pulse, q.synth_tolerance(dev["bin"], dev["phase"], dev["window"], dev["omega"], want_pulse)) == []
    want_tempo = np.where(dev["bin"] >= 0, s["grid"][np.maximum(dev["bin"], 0)], np.nan).astype(np.float32)
    assert np.array_equal(dev["tempo"], want_tempo, equal_nan=True)
    tg, grid = ar.tempogram(switch_clip, SR, prior=prior)
    assert tg.is_cuda and tg.shape == (n, 271) and np.array_equal(grid, q.tempo_grid()) and tg.cpu().numpy().tobytes() == dev["tgram"].tobytes()


def test_the_dp_method_and_the_segmentation_are_untouched(ar, steady_clip):
    from maua_stylegan2_amd.audioreactive import segment

    env, _ = segment.onset_envelope(steady_clip, SR)
    _, frames = segment.beat_track(env, SR)
    dp = ar.beats(steady_clip, SR, method="dp")
    assert dp.dtype == np.float64 and np.array_equal(dp, np.asarray(frames, np.float64) * 512 / SR) and len(dp) > 30
    with pytest.raises(ValueError, match="unknown method"):
        ar.beats(steady_clip, SR, method="rnn")
    with pytest.raises(ValueError, match="unknown method"):
        ar.beat_phase(steady_clip, SR, 10, method="rnn")
    track = segment_ref.sectioned_track("AB", 8, 120, seed=1)  # the clip of test_segmentation_gpu.py
    first = ar.laplacian_segmentation(track, SR, k=2)
    ar.beats(track, SR), ar.beat_phase(track, SR, 24)
    assert ar.laplacian_segmentation(track, SR, k=2) == first == segment.laplacian_segmentation(track, SR, k=2)
    want_times, want_labels, _, _ = segment_ref.segment(track, SR, 2)
    assert first[1] == [int(v) for v in want_labels]
    np.testing.assert_allclose(first[0], want_times, rtol=0, atol=0.5 + 1e-9)


def test_silence_and_refusals(ar):
    y = np.zeros(3 * SR, np.float32)
    curve, bpm, strength = ar.raw_plp(y, SR)
    assert not curve.any() and not strength.any() and bool(torch.isnan(bpm).all())
    assert len(ar.beats(y, SR)) == 0 and not ar.pulse(y, SR, 12).any()
    with pytest.warns(UserWarning, match="need two"):
        assert not ar.beat_phase(y, SR, 12).any()
    with pytest.warns(UserWarning, match="no frame"):
        assert not ar.tempo(y, SR, 12).any()
    for kw, advice in ((dict(win=1), "win"), (dict(win=4096), "win"), (dict(tempo_step=0.1), "at most 1024"), (dict(tempo_min=0), "tempo grid"),
                       (dict(prior="flat"), "unknown name"), (dict(prior=np.ones(5)), "one per tempo"), (dict(prior="lognormal", start_bpm=0), "start_bpm")):
        with pytest.raises(ValueError, match=advice):
            ar.raw_plp(y, SR, **kw)


# ------------------------------------------------------------------------------------------------ examples/onbeat.py through generate()
def test_onbeat_plugin_through_generate(ar, gpu, tmp_path, monkeypatch):
    from test_pitch_features_gpu import BATCH, FPS, SIZE

    from maua_stylegan2_amd import generate_audiovisual as gav
    from maua_stylegan2_amd import render
    from maua_stylegan2_amd.audioreactive.examples import onbeat
    from maua_stylegan2_amd.models.stylegan2 import Generator

    g = Generator(SIZE, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(SIZE, seed=60, rgb_gain=0.3), strict=True)
    g = g.to(gpu).eval()
    monkeypatch.setattr(render, "_output_dims", lambda out_size: (SIZE, SIZE))
    monkeypatch.setattr(render.shutil, "which", lambda name: None)
    for name in ("MAUA_SUBFRAMES", "MAUA_SHUTTER", "MAUA_SHUTTER_LIGHT", "MAUA_PIPE_PIX_FMT"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.chdir(tmp_path)
    seconds = 4
    clicks = np.arange(0.25, seconds, 0.5)
    clip = burst_clip(clicks, seconds, seed=2)
    monkeypatch.setattr(ar, "load_audio", lambda audio_file, offset, duration: (clip, SR, float(seconds)))
    monkeypatch.setattr(gav, "load_generator", lambda **kw: g)
    np.save("lat.npy", seeding.seeded_latents(8, g.n_latent, seed=11).numpy())
    seen = {}

    def initialize(args):
        args = onbeat.initialize(args)
        seen.update(kick=args.kick.clone(), bar=args.bar.clone(), pulse=args.pulse.clone())
        return args

    random.seed(5), np.random.seed(5), torch.manual_seed(5), torch.cuda.manual_seed_all(5)
    args = argparse.Namespace(fps=FPS, latent_count=8)
    out = gav.generate(ckpt=None, audio_file="stub.wav", initialize=initialize, get_latents=onbeat.get_latents, get_noise=onbeat.get_noise,
                       get_bends=onbeat.get_bends, latent_file="lat.npy", G_res=SIZE, out_size=SIZE, fps=FPS, batch=BATCH,
                       output_file=str(tmp_path / "onbeat.mp4"), args=args)
    n = seconds * FPS
    frames = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(-1, SIZE, SIZE, 3)
    assert frames.shape[0] == n and frames.std() > 5
    kick = seen["kick"].numpy()
    assert kick.shape == (n,) and kick.min() >= 0 and kick.max() <= 1 and seen["pulse"].shape == (n,) and seen["bar"].shape == (n,)
    # the kick is 1 on a beat and decays: its maxima are the first video frames at or after the beats.  A beat lies within 35 ms of its
    # click and a video frame lasts 62.5 ms: every click has a maximum of the kick no further than two video frames away
    peaks = 1 + np.flatnonzero((kick[1:-1] > kick[:-2]) & (kick[1:-1] >= kick[2:]))
    off = nearest(peaks / FPS, clicks[1:-1])
    print(f"onbeat: kick maxima at video frames {peaks.tolist()}, clicks at {np.round(clicks * FPS, 1).tolist()}, worst {off.max() * FPS:.2f} frames")
    assert off.max() <= 2.0 / FPS
    assert 6 <= len(peaks) <= 9  # one per click, 8 clicks
    bar = seen["bar"].numpy()
    assert np.sum(np.diff(bar) < 0) <= 2  # four seconds at 120 BPM are two loops of four beats
