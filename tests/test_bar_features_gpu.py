"""GPU: the bar features of audioreactive/bars.py on synthetic audio with known bars — noise bursts at 120 BPM with a 60 Hz thump on
every fourth, at 90 BPM on every third, and a 100 -> 150 BPM switch — the chain link by link against tests/bar_ref.py on the device's
own observations, the per-video-frame features, method="bar" on the beat features with the other methods untouched, silence,
refusals, and the shipped examples/bars.py plugin through generate().  tests/test_bar_host.py checks the same clips on the CPU."""
import argparse
import random
import warnings

import numpy as np
import pytest
import torch

import bar_ref as r
import pulse_ref as q
from maua_stylegan2_amd import seeding

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SR = q.SR
FR = r.FR
AUDIO_TOL = 2.0 / FR    # 46 ms: two envelope frames


@pytest.fixture()
def ar(gpu):
    import maua_stylegan2_amd.audioreactive as ar

    before = ar.signal.SMF
    ar.set_SMF(1)
    yield ar
    ar.set_SMF(before)


@pytest.fixture(scope="module")
def clips():
    return {name: r.audio_clip(name) for name in r.AUDIO_CLIPS}


@pytest.fixture(scope="module")
def stages(gpu, clips):
    """The intermediates of raw_bars per clip, computed once."""
    from maua_stylegan2_amd.audioreactive import bars

    with torch.cuda.device(gpu):
        return {name: bars._bar_stages(clip[0], SR) for name, clip in clips.items()}


# ------------------------------------------------------------------------------------------------ known answers
@pytest.mark.parametrize("name", list(r.AUDIO_CLIPS))
def test_raw_bars_on_audio(ar, clips, stages, name):
    """The tempo grid is coarse (whole frames per beat) and the envelope trails a burst by 0.3 .. 1.7 frames, of which one frame is
    taken off: every judged click has its beat, every judged accent its downbeat, within two frames."""
    _, clicks, every, seconds, clear = clips[name]
    res = stages[name]["result"]
    beats, downs = res.beat_times(), res.downbeat_times()
    beats_ok, worst, downs_ok, worst_down = r.judge_events(beats, downs, clicks, every, clear, AUDIO_TOL)
    scores = res.scores
    print(f"{name}: metre {res.metre}, scores {scores.tolist()}, margin {abs(scores[0] - scores[1]):.1f} nats, {len(beats)} beats, {len(downs)} downbeats, "
          f"worst beat {1e3 * worst:.1f} ms, worst downbeat {1e3 * worst_down:.1f} ms (bound {1e3 * AUDIO_TOL:.1f})")
    assert res.metre == every and isinstance(res.metre, int) and res.fr == FR
    assert beats.dtype == np.float64 and np.all(np.diff(beats) > 0) and set(downs.tolist()) <= set(beats.tolist())
    assert beats_ok and worst <= AUDIO_TOL
    assert downs_ok and worst_down <= AUDIO_TOL
    n = 1 + int(seconds * SR) // 512
    assert res.tempo.is_cuda and res.tempo.shape == (n,) and res.beat.dtype == torch.int32 and res.phase.shape == (n,)
    assert int(res.beat.min()) == 0 and int(res.beat.max()) == every - 1 and float(res.phase.min()) >= 0 and float(res.phase.max()) < 1
    phase = res.phase.cpu().numpy()
    assert np.sum(np.diff(phase) < 0) in (len(downs), len(downs) - 1, len(downs) + 1)   # the phase falls once per bar and nowhere else


@pytest.mark.parametrize("name", list(r.AUDIO_CLIPS))
def test_raw_bars_link_by_link(ar, stages, name):
    """Device activations -> the observations restated (float64 logarithms rounded to fp32: one fp32 ulp) ; device observations ->
    tests/bar_ref.py -> the same scores and paths, bit for bit."""
    s = stages[name]
    lo = s["logobs"].cpu().numpy()
    want_lo = r.observations(s["beat_act"].double().cpu().numpy(), s["down_act"].double().cpu().numpy())
    assert lo.dtype == np.float32 and lo.shape == want_lo.shape
    assert np.abs(lo.astype(np.float64) - want_lo).max() <= 2.0 ** -23 * np.abs(want_lo).max()
    interval, width, lc = ar.bar_model(FR)
    assert np.array_equal(interval, s["interval"]) and np.array_equal(width, s["width"]) and np.array_equal(lc, s["log_change"])
    score, path = r.decode(lo, interval, width, lc, (3, 4))
    assert r.same_bits(s["score"].cpu().numpy(), score) and r.same_bits(s["path"].cpu().numpy(), path)
    res = s["result"]
    best = int(np.argmax(score))
    k, b, j = path[best].T
    assert np.array_equal(res.beat.cpu().numpy(), b) and np.array_equal(res.starts.cpu().numpy(), j == 0)
    np.testing.assert_allclose(res.tempo.cpu().numpy(), 60 * FR / interval[k], rtol=1e-6)
    np.testing.assert_allclose(res.phase.cpu().numpy(), (b + j / interval[k]) / (3, 4)[best], rtol=0, atol=1e-6)
    assert np.array_equal(res.beat_times(), (np.flatnonzero(j == 0) - 1.0) / FR)   # (the envelope's lag: one frame)


# ------------------------------------------------------------------------------------------------ the features
def test_features_per_video_frame(ar, clips, stages):
    from maua_stylegan2_amd.audioreactive import beat

    clip, clicks, every, seconds, clear = clips["120-4"]
    res = stages["120-4"]["result"]
    downs = ar.downbeats(clip, SR)
    assert isinstance(downs, np.ndarray) and downs.dtype == np.float64 and np.array_equal(downs, res.downbeat_times())
    assert ar.metre(clip, SR) == 4 and isinstance(ar.metre(clip, SR), int)
    assert ar.metre(clip, SR, beats_per_bar=(3,)) == 3   # (the only candidate)
    n = 960   # 48 video frames per second: a video frame is 0.9 envelope frames
    phase = ar.bar_phase(clip, SR, n)
    assert phase.shape == (n,) and phase.dtype == torch.float32 and phase.device.type == "cpu" and float(phase.min()) >= 0 and float(phase.max()) < 1
    assert torch.equal(phase, beat.beat_phase_from_times(downs, seconds, n))
    want = q.beat_phase_from_times(downs, seconds, n)
    assert np.abs(phase.numpy() - want).max() < 1e-6
    tau = np.arange(n) * seconds / n
    p = phase.numpy().astype(np.float64)
    for lo, hi in zip(downs[:-1], downs[1:]):
        inside = np.flatnonzero((tau >= lo) & (tau < hi))
        assert np.all(np.diff(p[inside]) > 0), "strictly rising between two downbeats"
        assert p[inside[0]] < 1.5 * (seconds / n) / (hi - lo)   # 0 at the downbeat: the first video frame at or behind it is less than a frame in
    half = ar.bar_phase(clip, SR, n, division=0.5, device="cuda")
    assert half.is_cuda and np.sum(np.diff(half.cpu().numpy()) < 0) in (len(downs) // 2 - 1, len(downs) // 2, len(downs) // 2 + 1)
    rows = ar.bar_beats(clip, SR, n)
    assert rows.shape == (n, 4) and rows.dtype == torch.float32 and rows.device.type == "cpu"
    assert bool(((rows == 0) | (rows == 1)).all()) and bool((rows.sum(1) == 1).all())
    on_downbeat = rows[:, 0].numpy() == 1
    for t in clicks[::4][clear[::4]]:   # half a beat behind an accented click the bar is in beat 0, half a beat behind the next click in beat 1
        assert on_downbeat[int((t + 0.25) * n / seconds)] and rows[int((t + 0.75) * n / seconds), 1] == 1
    soft = ar.bar_beats(clip, SR, n, smooth=3, device="cuda")
    assert soft.is_cuda and soft.shape == (n, 4) and float((soft.sum(1) - 1).abs().max()) < 1e-4 and 0 < float(soft.min()) + 1e-3 and float(soft.max()) <= 1 + 1e-5
    latents = seeding.seeded_latents(6, 4, seed=3)
    assert ar.chroma_weight_latents(rows, latents[:4]).shape == (n, 4, 512)


def test_method_bar_on_the_beat_features_and_the_others_untouched(ar, clips, stages):
    from maua_stylegan2_amd.audioreactive import beat, segment

    clip, clicks, every, seconds, clear = clips["120-4"]
    res = stages["120-4"]["result"]
    found = ar.beats(clip, SR, method="bar")
    assert found.dtype == np.float64 and np.array_equal(found, res.beat_times())
    downs = ar.downbeats(clip, SR)
    at = np.searchsorted(found, downs)
    assert np.array_equal(found[at], downs) and np.all(np.diff(at) == 4)   # every fourth beat is a downbeat
    n = 480
    saw = ar.beat_phase(clip, SR, n, method="bar")
    assert torch.equal(saw, beat.beat_phase_from_times(found, seconds, n))
    # 120 BPM are 21.53 frames per beat: the path alternates between 21 and 22 frames, 123.05 and 117.45 BPM — the grid is 1 / 21 wide
    # there, 3.05 BPM from 120 on its own; tempo(method="bar") measures bar by bar (86 or 87 frames: 120.2 or 118.8 BPM)
    raw = res.tempo.cpu().numpy()
    assert np.minimum(np.abs(raw[50:-50] - 60 * FR / 21), np.abs(raw[50:-50] - 60 * FR / 22)).max() < 1e-3
    bpm = ar.tempo(clip, SR, n, method="bar")
    t = np.arange(n) * seconds / (n - 1)
    there = (t > 1.0) & (t < seconds - 1.0)
    print(f"tempo(method='bar'): {float(bpm[there].min()):.2f} .. {float(bpm[there].max()):.2f} BPM, mean {float(bpm[there].mean()):.2f}")
    assert bpm.shape == (n,) and bpm.device.type == "cpu" and float((bpm[there] - 120.0).abs().max()) <= 3.0
    assert ar.tempo(clip, SR, n, method="bar", device="cuda").is_cuda
    # the other methods, call for call: the default is "plp", and both give what their stages give
    s = beat._plp_stages(clip, SR)
    plp = ar.beats(clip, SR)
    assert plp.tobytes() == ar.beats(clip, SR, method="plp").tobytes() == beat.pick_beats(s["pulse"], s["fr"], 0.1).cpu().numpy().tobytes()
    env, _ = segment.onset_envelope(clip, SR)
    _, frames = segment.beat_track(env, SR)
    assert ar.beats(clip, SR, method="dp").tobytes() == (np.asarray(frames, np.float64) * 512 / SR).tobytes()
    assert torch.equal(ar.tempo(clip, SR, n), ar.tempo(clip, SR, n, 0, None, "plp")) and torch.equal(ar.tempo(clip, SR, n, 2), ar.tempo(clip, SR, n, smooth=2, method="plp"))
    assert torch.equal(ar.beat_phase(clip, SR, n), beat.beat_phase_from_times(plp, seconds, n))
    for call in (lambda: ar.beats(clip, SR, method="rnn"), lambda: ar.beat_phase(clip, SR, 10, method="rnn"), lambda: ar.tempo(clip, SR, 10, method="rnn")):
        with pytest.raises(ValueError, match="unknown method"):
            call()


def test_accent_takes_the_callers_salience(ar, clips, stages):
    """The accent of the 90-3 clip handed to the 120-4 clip's length would be refused; the clip's own cue handed back decodes the same
    bars; a cue that marks every SECOND click of the 120 BPM clip makes a two-beat bar win over three."""
    clip, clicks, every, seconds, clear = clips["120-4"]
    s = stages["120-4"]
    same = ar.raw_bars(clip, SR, accent=s["cue"])
    assert same.metre == 4 and np.array_equal(same.downbeat_times(), s["result"].downbeat_times())
    n = s["onset"].numel()
    cue = np.zeros(n, np.float32)
    for t in clicks[::2]:
        cue[int(round(t * FR)) + 1] = 1.0
    two = ar.raw_bars(clip, SR, beats_per_bar=(3, 2), accent=cue)
    assert two.metre == 2
    with pytest.raises(ValueError, match="accent"):
        ar.raw_bars(clip, SR, accent=cue[:-1])


def test_silence_and_refusals(ar):
    y = np.zeros(3 * SR, np.float32)
    with pytest.warns(UserWarning, match="no onsets"):
        res = ar.raw_bars(y, SR)
    assert res.metre == 0 and not res.scores.any() and not res.tempo.any() and not res.beat.any() and not res.phase.any()
    assert len(res.beat_times()) == 0 and len(res.downbeat_times()) == 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert ar.metre(y, SR) == 0 and len(ar.downbeats(y, SR)) == 0 and not ar.bar_phase(y, SR, 12).any() and not ar.bar_beats(y, SR, 12).any()
        assert not ar.tempo(y, SR, 12, method="bar").any() and len(ar.beats(y, SR, method="bar")) == 0
    for kw, advice in ((dict(tempo_min=10), "raise tempo_min"), (dict(beats_per_bar=(9,)), "beats per bar"), (dict(beats_per_bar=()), "metres"),
                       (dict(tempo_min=0), "tempo_min"), (dict(tempo_min=300), "tempo_min"), (dict(observation_lambda=1), "observation_lambda"),
                       (dict(beats_per_bar=tuple(range(1, 10))), "metres")):
        with pytest.raises(ValueError, match=advice):
            ar.raw_bars(y, SR, **kw)
    with pytest.raises(ValueError, match="sr must be positive"):
        ar.raw_bars(y, 0)


# ------------------------------------------------------------------------------------------------ examples/bars.py through generate()
def test_bars_plugin_through_generate(ar, gpu, tmp_path, monkeypatch):
    from test_pitch_features_gpu import BATCH, FPS, SIZE

    from maua_stylegan2_amd import generate_audiovisual as gav
    from maua_stylegan2_amd import render
    from maua_stylegan2_amd.audioreactive.examples import bars as plugin
    from maua_stylegan2_amd.models.stylegan2 import Generator

    g = Generator(SIZE, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(SIZE, seed=60, rgb_gain=0.3), strict=True)
    g = g.to(gpu).eval()
    monkeypatch.setattr(render, "_output_dims", lambda out_size: (SIZE, SIZE))
    monkeypatch.setattr(render.shutil, "which", lambda name: None)
    for name in ("MAUA_SUBFRAMES", "MAUA_SHUTTER", "MAUA_SHUTTER_LIGHT", "MAUA_PIPE_PIX_FMT"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.chdir(tmp_path)
    seconds = 8
    clicks = q.click_times(90.0, seconds)   # a waltz: 12 clicks, four bars of three
    clip = r.accented_clip(clicks, 3, seconds, seed=2)
    monkeypatch.setattr(ar, "load_audio", lambda audio_file, offset, duration: (clip, SR, float(seconds)))
    monkeypatch.setattr(gav, "load_generator", lambda **kw: g)
    np.save("lat.npy", seeding.seeded_latents(8, g.n_latent, seed=11).numpy())
    seen = {}

    def initialize(args):
        args = plugin.initialize(args)
        seen.update(kick=args.kick.clone(), bar=args.bar.clone(), rows=args.rows.clone(), metre=args.metre)
        return args

    random.seed(5), np.random.seed(5), torch.manual_seed(5), torch.cuda.manual_seed_all(5)
    args = argparse.Namespace(fps=FPS, latent_count=8)
    out = gav.generate(ckpt=None, audio_file="stub.wav", initialize=initialize, get_latents=plugin.get_latents, get_noise=plugin.get_noise,
                       get_bends=plugin.get_bends, latent_file="lat.npy", G_res=SIZE, out_size=SIZE, fps=FPS, batch=BATCH,
                       output_file=str(tmp_path / "bars.mp4"), args=args)
    n = seconds * FPS
    frames = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(-1, SIZE, SIZE, 3)
    assert frames.shape[0] == n and frames.std() > 5
    kick, bar, rows = seen["kick"].numpy(), seen["bar"].numpy(), seen["rows"]
    print(f"bars plugin: metre {seen['metre']}, bar phase falls {int(np.sum(np.diff(bar) < 0))} times, kick {kick.min():.3f} .. {kick.max():.3f}")
    assert seen["metre"] == 3 and rows.shape == (n, 3) and float((rows.sum(1) - 1).abs().max()) < 1e-4
    assert kick.shape == (n,) and kick.min() >= 0 and kick.max() <= 1 and bar.shape == (n,) and bar.min() >= 0 and bar.max() < 1
    assert 2 <= np.sum(np.diff(bar) < 0) <= 4   # eight seconds at 90 BPM are four bars of three beats
    # the kick on the downbeat is the stronger one: what is above the other beats' ceiling of 0.5 sits in beat 0 of the bar, and every
    # downbeat has a video frame (62.5 ms) early enough in its beat (667 ms) for (1 - phase) ** 4 > 0.55
    strong = np.flatnonzero(kick > 0.55)
    assert len(strong) >= 2 and bool((ar.bar_beats(clip, SR, n)[strong, 0] == 1).all())
