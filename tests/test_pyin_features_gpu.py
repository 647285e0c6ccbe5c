"""GPU: the pYIN features — ar.raw_pyin on the noisy tones plain YIN gets wrong and on the arpeggio (the known-answer conditions of
tests/test_pyin_host.py), the chain checked link by link on the device's own intermediates, ar.pitch(method="pyin") against the numpy
pipeline on the device's raw outputs, the unchanged default, the shipped examples/melody_pyin.py plugin through generate(), refusals."""
import argparse
import math
import random
import warnings

import numpy as np
import pytest
import torch

import pitch_ref as pr
import pyin_ref as q
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


@pytest.mark.parametrize("freq,snr", q.NOISY_CASES[:2], ids=["220Hz-6dB", "440Hz-6dB"])
def test_raw_pyin_finds_the_tone_that_raw_pitch_loses(ar, freq, snr):
    y = q.noisy_tone(freq, snr)
    f0, voiced, prob = ar.raw_pyin(y, pr.TONE_SR)
    assert f0.is_cuda and voiced.is_cuda and prob.is_cuda and voiced.dtype == torch.bool
    assert f0.shape == voiced.shape == prob.shape == (1 + len(y) // 512,)
    c = pr.cents(f0[q.INTERIOR].cpu().numpy(), freq)
    yin_f0, _ = ar.raw_pitch(y, pr.TONE_SR)
    wrong = float(np.mean(pr.cents(yin_f0[q.INTERIOR].cpu().numpy(), freq) > 50))
    print(f"{freq} Hz at {snr} dB: ar.raw_pyin worst {c.max():.1f} cents, ar.raw_pitch over 50 cents on {100 * wrong:.0f} % of {len(c)} frames")
    assert bool(voiced[q.INTERIOR].all())
    assert c.max() <= q.NOISY_BOUND_CENTS
    assert wrong >= q.NOISY_YIN_WRONG


def test_raw_pyin_on_the_arpeggio(ar):
    y, _ = pr.arpeggio()
    f0, voiced, prob = (t.cpu().numpy() for t in ar.raw_pyin(y, pr.TONE_SR))
    inside, silent = q.arpeggio_frame_sets()
    assert all(voiced[t] for t, _ in inside)
    worst = max(float(pr.cents(f0[t], f)) for t, f in inside)
    print(f"arpeggio: worst {worst:.3f} cents inside the notes (bound {q.ARPEGGIO_BOUND_CENTS}), voiced probability in silence <= {prob[silent].max():.3f}")
    assert worst <= q.ARPEGGIO_BOUND_CENTS
    assert not any(voiced[t] for t in silent)


@pytest.mark.parametrize("signal", ["noisy", "arpeggio"])
def test_the_chain_link_by_link(ar, signal):
    """The device's d' rows through the stage-A restatement against the device's obs / period / voiced_prob (the tolerances of the entry
    test), and the device's own logarithms through the stage-B restatement against the device's delta_last / backptr / states, exactly."""
    y = q.noisy_tone(220.0, 6.0) if signal == "noisy" else pr.arpeggio()[0]
    s = ar.signal._pyin_stages(y, pr.TONE_SR)
    P, W = s["n_bins"], s["width"]
    assert (P, W, s["tau_min"], s["tau_max"]) == (602, 50, 10, 340)
    dev = {k: v.cpu().numpy() for k, v in s.items() if isinstance(v, torch.Tensor)}
    edges = q.bin_edges(pr.TONE_SR, 65.0, 10, P)
    ref_a = q.candidates(dev["cmndf"], 10, 340, q.threshold_prior(), 100, 0.01, edges)
    n_exempt = int(q.near_edge_frames(ref_a, edges).sum())
    print(f"{signal}: {sum(len(c) for c in ref_a['cands'])} candidates on {len(y) // 512 + 1} frames, {n_exempt} frames exempt")
    assert n_exempt <= q.max_exempt(len(ref_a["cands"]))
    assert q.compare_candidates(dev, ref_a, edges) == []
    tri, norm = q.transition_tables(P, W)
    delta, back, states = q.viterbi(dev["logobs_voiced"], dev["logobs_unvoiced"], W, tri, norm, -math.log(2 * P), math.log(0.99), math.log(0.01))
    assert np.array_equal(dev["states"], states)
    assert np.array_equal(dev["backptr"].view(np.uint16), back)
    assert dev["delta_last"].tobytes() == delta.tobytes()
    want = q.decode(states, dev["period"], pr.TONE_SR, 65.0, 10, P)
    assert np.array_equal(dev["voiced_flag"], want["voiced_flag"])
    assert np.allclose(dev["f0"], want["f0"], rtol=1e-6, atol=0)


def test_pitch_with_pyin_equals_the_numpy_pipeline_on_the_raw_outputs(ar):
    y, spans = pr.arpeggio()
    n = pr.ARPEGGIO_FRAMES
    f0, voiced, prob = (t.cpu().numpy() for t in ar.raw_pyin(y, pr.TONE_SR))
    want_h, want_v = q.pyin_pipeline(f0.astype(np.float64), voiced, prob.astype(np.float64), n, pr.ARPEGGIO_FMIN, pr.ARPEGGIO_FMAX)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        height, voicing = ar.pitch(y, pr.TONE_SR, n, margin=None, method="pyin", return_voicing=True)
        alone = ar.pitch(y, pr.TONE_SR, n, margin=None, method="pyin", voicing=0.99)  # (ignored)
        on_dev = ar.pitch(y, pr.TONE_SR, n, margin=None, method="pyin", device="cuda")
    assert height.device.type == "cpu" and on_dev.is_cuda and height.shape == voicing.shape == (n,) and height.dtype == torch.float32
    assert torch.equal(alone, height) and torch.equal(on_dev.cpu(), height)
    err_h = float(np.abs(height.numpy().astype(np.float64) - want_h).max())
    err_v = float(np.abs(voicing.numpy().astype(np.float64) - want_v).max())
    print(f"ar.pitch(method='pyin') against float64: height {err_h:.3g} (tolerance {q.PIPELINE_HEIGHT_TOL:.3g})  voicing {err_v:.3g} ({q.PIPELINE_VOICING_TOL:.3g})")
    centre = lambda lo, hi: int(round((lo + hi) / 2 / len(y) * (n - 1)))  # noqa: E731
    level = [math.log2(f / pr.ARPEGGIO_FMIN) / math.log2(pr.ARPEGGIO_FMAX / pr.ARPEGGIO_FMIN) for _, _, f in spans]
    for i, (lo, hi, _) in enumerate(spans):
        assert abs(float(height[centre(lo, hi)]) - level[i]) < 0.03
    assert err_h <= q.PIPELINE_HEIGHT_TOL
    assert err_v <= q.PIPELINE_VOICING_TOL


def test_the_default_method_is_yin_bit_for_bit(ar):
    y, _ = pr.arpeggio()
    for kw in (dict(margin=None), dict(margin=None, fmax=260.0, bandpass=True), dict()):
        a, av = ar.pitch(y, pr.TONE_SR, 24, return_voicing=True, **kw)
        b, bv = ar.pitch(y, pr.TONE_SR, 24, return_voicing=True, method="yin", **kw)
        assert torch.equal(a, b) and torch.equal(av, bv)


def test_refusals(ar):
    y = np.zeros(4000, np.float32)
    with pytest.raises(ValueError, match="unknown method"):
        ar.pitch(y, pr.TONE_SR, 8, method="crepe")
    for kw, advice in ((dict(fmin=300.0, fmax=200.0), "lower fmin or raise fmax"), (dict(fmin=0.0), "raise fmin"), (dict(fmax=30000.0), "lower fmax"),
                       (dict(fmin=5.0), "raise fmin to at least"), (dict(frame_length=8), "frame_length"), (dict(hop=0), "hop"),
                       (dict(bins_per_semitone=25), "lower bins_per_semitone"), (dict(max_transition_rate=200.0), "lower max_transition_rate"),
                       (dict(n_thresholds=300), "n_thresholds"), (dict(switch_prob=0.0), "switch_prob"), (dict(no_trough_prob=2.0), "no_trough_prob")):
        with pytest.raises(ValueError, match=advice):
            ar.raw_pyin(y, pr.TONE_SR, **kw)
    # digital silence: every d' row is flat, the only mass is the fallback's (no_trough_prob) on the shortest lag
    f0, voiced, prob = ar.raw_pyin(y, pr.TONE_SR)
    assert bool(torch.isfinite(f0).all()) and float(prob.max()) <= 0.0101


# ------------------------------------------------------------------------------------------------ examples/melody_pyin.py through generate()
def test_melody_pyin_plugin_through_generate(ar, gpu, tmp_path, monkeypatch):
    from test_pitch_features_gpu import BATCH, FPS, SIZE, SR, two_note_clip

    from maua_stylegan2_amd import generate_audiovisual as gav
    from maua_stylegan2_amd import render
    from maua_stylegan2_amd.audioreactive.examples import melody_pyin
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
    seen = {}

    def initialize(args):
        args = melody_pyin.initialize(args)
        seen["melody"], seen["bass"] = args.melody.clone(), args.bass_line.clone()
        return args

    random.seed(5), np.random.seed(5), torch.manual_seed(5), torch.cuda.manual_seed_all(5)
    args = argparse.Namespace(fps=FPS, latent_count=8)
    out = gav.generate(ckpt=None, audio_file="stub.wav", initialize=initialize, get_latents=melody_pyin.get_latents, get_noise=melody_pyin.get_noise,
                       get_bends=melody_pyin.get_bends, latent_file="lat.npy", G_res=SIZE, out_size=SIZE, fps=FPS, batch=BATCH,
                       output_file=str(tmp_path / "pyin.mp4"), args=args)
    frames = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(-1, SIZE, SIZE, 3)
    assert frames.shape[0] == FPS and frames.std() > 5
    tune = seen["melody"]
    assert tune.shape == (FPS,) and float(tune.min()) >= 0 and float(tune.max()) <= 1
    low, high = float(tune[2:6].mean()), float(tune[10:14].mean())
    want = [math.log2(f / 65.0) / math.log2(2100.0 / 65.0) for f in (110.0, 440.0)]
    print(f"melody height: low half {low:.3f} (110 Hz = {want[0]:.3f}), high half {high:.3f} (440 Hz = {want[1]:.3f})")
    assert abs(low - want[0]) < 0.05 and abs(high - want[1]) < 0.05
    assert seen["bass"].shape == (FPS,) and bool(torch.isfinite(seen["bass"]).all())
    halves = np.abs(frames[2:6].astype(np.int16) - frames[10:14]).mean()
    within = np.abs(frames[2:5].astype(np.int16) - frames[3:6]).mean()
    assert halves > 0 and halves > within
