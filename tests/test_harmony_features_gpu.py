"""GPU: the chord and key features of audioreactive/harmony.py on synthetic audio whose chords are known — six chords of two seconds
each (C Am F G Em Dm; Cmaj7 Am7 Dm7 G7 Bdim Csus4), built by tests/hmm_ref.py from notes of six decaying partials, with a second of
silence behind and noise clicks every half second — the chain link by link against tests/hmm_ref.py on the device's own observations,
``ar.chords``, ``ar.key``, and the shipped examples/harmony.py plugin through generate().

Every frame further than 0.25 s from a chord change and past the first 0.1 s must carry exactly its chord; the share of frames that
this exempts is asserted (<= 25 %) before anything is decoded."""
import argparse
import random
import warnings

import numpy as np
import pytest
import torch

import hmm_ref as q
from maua_stylegan2_amd import seeding

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SR = q.SR


@pytest.fixture(scope="module")
def triad_clip():
    return q.chord_clip(q.TRIAD_CLIP, clicks=True)


@pytest.fixture(scope="module")
def seventh_clip():
    return q.chord_clip(q.SEVENTH_CLIP, clicks=False, tail=0.0)


@pytest.fixture()
def ar(gpu):
    import maua_stylegan2_amd.audioreactive as ar

    before = ar.signal.SMF
    ar.set_SMF(1)
    yield ar
    ar.set_SMF(before)


def report(name, track, labels, want, judged):
    wrong = np.flatnonzero(judged & (labels != want))
    print(f"{name}: {len(wrong)} of {int(judged.sum())} judged frames wrong" + (f", first at frame {wrong[0]}: {track.names[labels[wrong[0]]]} for "
                                                                                f"{track.names[want[wrong[0]]]}" if len(wrong) else ""))
    return len(wrong)


# ------------------------------------------------------------------------------------------------ labels
def test_the_exempt_share_is_a_quarter_at_most(ar):
    """Decided before any kernel runs: 24.1 % of the frames of the triad clip (135 of 560), 24.0 % of the other (124 of 517)."""
    names = ar.chord_vocabulary("sevenths")[0]
    want, judged, in_tail = q.chord_truth(q.TRIAD_CLIP, names)
    share = 1.0 - judged.mean()
    print(f"triad clip: {len(judged)} frames, {int(judged.sum())} judged, exempt share {share:.3f}, {int(in_tail.sum())} tail frames")
    assert len(judged) == 560 and int(judged.sum()) == 425 and share <= q.MAX_EXEMPT_SHARE
    want, judged, _ = q.chord_truth(q.SEVENTH_CLIP, names, tail=0.0)
    assert int(judged.sum()) == 393 and 1.0 - judged.mean() <= q.MAX_EXEMPT_SHARE


@pytest.mark.parametrize("vocabulary,clicks", [("triads", True), ("triads", False), ("sevenths", True)],
                         ids=["triads-clicks", "triads-clean", "sevenths-clicks"])
def test_triad_clip_labels(ar, triad_clip, vocabulary, clicks):
    clip = triad_clip if clicks else q.chord_clip(q.TRIAD_CLIP, clicks=False)
    want, judged, in_tail = q.chord_truth(q.TRIAD_CLIP, ar.chord_vocabulary(vocabulary)[0])
    assert 1.0 - judged.mean() <= q.MAX_EXEMPT_SHARE  # before the kernel runs
    track = ar.raw_chords(clip, SR, vocabulary=vocabulary)
    labels = track.labels.cpu().numpy()
    n_wrong = report(f"{vocabulary}, clicks={clicks}", track, labels, want, judged)
    assert n_wrong == 0
    assert np.all(labels[in_tail] == len(track.names) - 1), f"tail: {[track.names[i] for i in labels[in_tail]]}"
    assert len(track) == 560 and track.labels.is_cuda and track.labels.dtype == torch.int32
    assert track.posterior.shape == (560, len(track.names)) and track.posterior.dtype == torch.float32 and track.confidence.shape == (560,)
    assert torch.equal(track.confidence, track.posterior.gather(1, track.labels.long()[:, None])[:, 0])
    assert float(track.confidence[torch.from_numpy(judged).to(track.labels.device)].min()) > 0.5
    assert track.times.shape == (560,) and track.times[1] == 512 / SR
    runs = track.segments()
    assert [name for _, _, name in runs if name != "N"][:6] == [f"{r}:{k}" for r, k in q.TRIAD_CLIP]


def test_seventh_clip_labels(ar, seventh_clip):
    want, judged, _ = q.chord_truth(q.SEVENTH_CLIP, ar.chord_vocabulary("sevenths")[0], tail=0.0)
    assert 1.0 - judged.mean() <= q.MAX_EXEMPT_SHARE
    track = ar.raw_chords(seventh_clip, SR, vocabulary="sevenths")
    assert report("sevenths clip", track, track.labels.cpu().numpy(), want, judged) == 0


def test_transposition_rotates_the_labels(ar, triad_clip):
    up = q.chord_clip(q.TRIAD_CLIP, transpose=7, clicks=True)
    for vocabulary in ("triads", "sevenths"):
        base = ar.raw_chords(triad_clip, SR, vocabulary=vocabulary)
        moved = ar.raw_chords(up, SR, vocabulary=vocabulary)
        want, judged, in_tail = q.chord_truth(q.TRIAD_CLIP, moved.names, transpose=7)
        got = moved.labels.cpu().numpy()
        assert report(f"{vocabulary} up 7", moved, got, want, judged) == 0
        assert np.array_equal(got[judged], q.rotate_labels(base.labels.cpu().numpy(), len(base.names), 7)[judged])


# ------------------------------------------------------------------------------------------------ the chain, link by link
@pytest.mark.parametrize("vocabulary", ["triads", "sevenths"])
def test_raw_chords_link_by_link(ar, triad_clip, vocabulary):
    """The device's own observations decoded by the restatement equal labels and posterior exactly; the links before them against
    numpy on the device's chromagram."""
    from maua_stylegan2_amd.audioreactive import harmony

    s = harmony._chord_stages(triad_clip, SR, vocabulary=vocabulary)
    dev = {k: v.cpu().numpy() for k, v in s.items() if isinstance(v, torch.Tensor)}
    T, S = 560, len(s["names"])
    chroma = dev["chroma"].astype(np.float64)
    assert dev["chroma"].shape == (12, T) and dev["logobs"].shape == dev["obs"].shape == (T, S) and dev["logobs"].dtype == np.float32
    energy = chroma.sum(0)
    assert np.abs(dev["energy"] - energy).max() <= 1e-5 * energy.max()
    silent = dev["silent"]
    clear = np.abs(energy - 0.02 * energy.max()) > 1e-5 * energy.max()   # (a frame on the threshold may fall either way in fp32)
    assert np.array_equal(silent[clear], (energy <= 0.02 * energy.max())[clear]) and silent[-20:].all() and not silent[:500].any()
    norm = np.linalg.norm(chroma, axis=0)
    cos = s["templates"].astype(np.float64) @ (chroma / np.where(norm > 0, norm, 1.0))
    assert np.abs(dev["cos"] - cos.T).max() <= 1e-5      # 12 fp32 products of values <= 1
    want_logobs = np.where(silent[:, None], np.where(np.arange(S) == S - 1, 20.0, 0.0)[None, :], 20.0 * dev["cos"]).astype(np.float32)
    assert np.abs(dev["logobs"] - want_logobs).max() <= 4e-6 and np.array_equal(dev["logobs"][silent], want_logobs[silent])
    assert np.all(dev["obs"].max(1) == 1.0) and np.abs(dev["obs"] - np.exp(dev["logobs"] - dev["logobs"].max(1, keepdims=True))).max() <= 1e-6
    stay = np.exp(-1.0 / (SR / 512 * 1.0))
    assert abs(np.exp(s["log_trans"][0, 0]) - stay) < 1e-15 and abs(np.exp(s["log_trans"][0, 1]) - (1 - stay) / (S - 1)) < 1e-15
    delta, _, states = q.viterbi(dev["logobs"], s["log_trans"], s["log_init"])
    assert q.same_bits(dev["labels"], states) and q.same_bits(dev["delta_last"], delta)
    gamma, scale = q.posterior(dev["obs"], np.exp(s["log_trans"]), np.exp(s["log_init"]))
    assert q.same_bits(dev["gamma"], gamma) and q.same_bits(dev["scale"], scale)
    assert q.same_bits(dev["posterior"], gamma.astype(np.float32))
    assert q.same_bits(dev["confidence"], gamma.astype(np.float32)[np.arange(T), states])


# ------------------------------------------------------------------------------------------------ ar.chords, ar.key
def test_chords_per_video_frame(ar, triad_clip):
    n = 13 * 24
    names = ar.chord_vocabulary("triads")[0]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        track = ar.raw_chords(triad_clip, SR)
        root = ar.chords(triad_clip, SR, n, track=track)
        chord = ar.chords(triad_clip, SR, n, by="chord", device="cuda", track=track)
        soft = ar.chords(triad_clip, SR, n, soft=True, track=track)
        home = ar.chords(triad_clip, SR, n, relative_to=7, track=track)
        keyed = ar.chords(triad_clip, SR, n, relative_to="key", track=track)
        fresh = ar.chords(triad_clip, SR, n)
    assert root.shape == soft.shape == home.shape == (n, 12) and chord.shape == (n, 24)
    assert root.device.type == "cpu" and chord.is_cuda and all(v.dtype == torch.float32 for v in (root, chord, soft, home))
    for v in (root, chord, soft, home, keyed):
        assert float((v.sum(1) - 1).abs().max()) <= 1e-5 and float(v.min()) >= 0
    assert torch.equal(fresh, root)
    t = np.arange(n) * 13.0 / n
    want_root = np.array([q.NOTE[r] for r, _ in q.TRIAD_CLIP])[np.minimum((t / 2).astype(int), 5)]
    want_chord = np.array([names.index(f"{r}:{k}") for r, k in q.TRIAD_CLIP])[np.minimum((t / 2).astype(int), 5)]
    changes = np.arange(1, 7) * 2.0
    # judged as the labels are: further than 0.25 s from a change (the end of the sound included: behind it the last chord, D minor,
    # is held over N) and past the first 0.1 s.  Decided before anything is compared: six windows of 0.5 s and 0.1 s are 3.1 of 13 s,
    # 23.8 %; a video frame lies exactly on both edges of every window (0.25 s = 6 frames), one more frame each: 81 of 312, 26.0 %
    judged = (t >= q.EXEMPT_START) & (np.abs(t[:, None] - changes[None, :]).min(1) > q.EXEMPT_CHANGE)
    assert int((~judged).sum()) == 81
    assert np.array_equal(root.argmax(1).numpy()[judged], want_root[judged])
    assert np.array_equal(soft.argmax(1).numpy()[judged], want_root[judged])
    assert np.array_equal(chord.argmax(1).cpu().numpy()[judged], want_chord[judged])
    # how LARGE the maximum is (and how near the mixed latent) is judged four video frames further from every change: the reach of the
    # smoothing (sigma 2 frames).  The resampling and the smoothing are circular: the clip's end against its start is one more change
    reach = q.EXEMPT_CHANGE + 4 / 24
    inner = (np.abs(t[:, None] - changes[None, :]).min(1) > reach) & (t > reach) & (t < 13.0 - reach)
    assert inner.mean() > 0.5
    assert float(root[torch.from_numpy(inner)].max(1).values.min()) > 0.9
    assert np.array_equal(home.argmax(1).numpy()[judged], (want_root[judged] - 7) % 12)     # G is home: column 0
    tonic = ar.key(triad_clip, SR)[0]   # with the clicks and the tail in the mean the relative minor is as good an answer as C major
    assert tonic in (0, 9) and torch.equal(keyed, ar.chords(triad_clip, SR, n, relative_to=tonic, track=track))
    assert np.array_equal(keyed.argmax(1).numpy()[judged], (want_root[judged] - tonic) % 12)
    lat = torch.randn(12, 3, 8, generator=torch.Generator().manual_seed(0))
    mixed = ar.chroma_weight_latents(root, lat)
    assert mixed.shape == (n, 3, 8) and float((mixed[inner] - lat[want_root[inner]]).abs().max()) < 0.2 * float(lat.abs().max())
    with pytest.raises(ValueError, match="relative_to"):
        ar.chords(triad_clip, SR, n, relative_to=12, track=track)
    with pytest.raises(ValueError, match="unknown by"):
        ar.chords(triad_clip, SR, n, by="bass", track=track)


def test_silence_gives_no_chord_and_uniform_rows(ar):
    y = np.zeros(2 * SR, np.float32)
    track = ar.raw_chords(y, SR)
    assert bool((track.labels == 24).all()) and bool(torch.isfinite(track.posterior).all())
    with pytest.warns(UserWarning, match="no frame"):
        rows = ar.chords(y, SR, 12)
    assert rows.shape == (12, 12) and bool((rows == 1 / 12).all())
    for kw in (dict(kappa=0), dict(silence=1.0), dict(vocabulary="jazz"), dict(hold=0)):
        with pytest.raises(ValueError):
            ar.raw_chords(y, SR, **kw)


def test_key_of_the_two_passages(ar):
    """The twelve seconds of C Am F G Em Dm are in C major; up a tritone, in F sharp major.  (The float64 chain on the oracle's
    chromagram scores C major 0.778 against G major's 0.735, and F sharp major 0.828 against C sharp major's 0.678.)"""
    from maua_stylegan2_amd.audioreactive import harmony

    for transpose, want in ((0, (0, "major", "C major")), (6, (6, "major", "F# major"))):
        y = q.chord_clip(q.TRIAD_CLIP, transpose=transpose, clicks=False, tail=0.0)
        got = ar.key(y, SR)
        scores = harmony.key_of_chroma(harmony.chromagram(y, SR).mean(1))[3].numpy()
        order = np.argsort(-scores)
        print(f"transpose {transpose}: {got[2]} {scores[order[0]]:.3f}, runner-up index {order[1]} {scores[order[1]]:.3f}")
        assert got == want and isinstance(got[0], int)


# ------------------------------------------------------------------------------------------------ examples/harmony.py through generate()
def test_harmony_plugin_through_generate(ar, gpu, tmp_path, monkeypatch):
    from test_pitch_features_gpu import BATCH, FPS, SIZE

    from maua_stylegan2_amd import generate_audiovisual as gav
    from maua_stylegan2_amd import render
    from maua_stylegan2_amd.audioreactive.examples import harmony as plugin
    from maua_stylegan2_amd.models.stylegan2 import Generator

    g = Generator(SIZE, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(SIZE, seed=60, rgb_gain=0.3), strict=True)
    g = g.to(gpu).eval()
    monkeypatch.setattr(render, "_output_dims", lambda out_size: (SIZE, SIZE))
    monkeypatch.setattr(render.shutil, "which", lambda name: None)
    for name in ("MAUA_SUBFRAMES", "MAUA_SHUTTER", "MAUA_SHUTTER_LIGHT", "MAUA_PIPE_PIX_FMT"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.chdir(tmp_path)
    chords = q.TRIAD_CLIP[:2]   # C major, A minor: four seconds
    seconds = 4
    clip = q.chord_clip(chords, clicks=True, tail=0.0)
    monkeypatch.setattr(ar, "load_audio", lambda audio_file, offset, duration: (clip, SR, float(seconds)))
    monkeypatch.setattr(gav, "load_generator", lambda **kw: g)
    np.save("lat.npy", seeding.seeded_latents(12, g.n_latent, seed=11).numpy())
    seen = {}

    def initialize(args):
        args = plugin.initialize(args)
        seen.update(chords=args.chords.clone(), doubt=args.doubt.clone())
        return args

    def get_latents(selection, args):
        seen["selection"] = selection.detach().cpu().clone()
        seen["latents"] = plugin.get_latents(selection, args).detach().cpu().clone()
        return seen["latents"].to(selection.device)

    random.seed(5), np.random.seed(5), torch.manual_seed(5), torch.cuda.manual_seed_all(5)
    args = argparse.Namespace(fps=FPS, latent_count=12)
    out = gav.generate(ckpt=None, audio_file="stub.wav", initialize=initialize, get_latents=get_latents, get_noise=plugin.get_noise,
                       latent_file="lat.npy", G_res=SIZE, out_size=SIZE, fps=FPS, batch=BATCH, output_file=str(tmp_path / "harmony.mp4"),
                       args=args)
    n = seconds * FPS
    frames = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(-1, SIZE, SIZE, 3)
    assert frames.shape[0] == n and frames.std() > 5
    weights, doubt = seen["chords"], seen["doubt"]
    assert weights.shape == (n, 12) and float((weights.sum(1) - 1).abs().max()) <= 1e-5 and doubt.shape == (n,)
    assert float(doubt.min()) >= 0 and float(doubt.max()) <= 1
    # the key of two seconds of C major and two of A minor is C major or A minor: the C chord sits in column 0 or 3, A nine above it
    tonic = ar.key(clip, SR)[0]
    assert tonic in (0, 9)
    t = np.arange(n) / FPS
    first, second = (t > 0.5) & (t < 1.5), (t > 2.5) & (t < 3.5)
    assert set(weights.argmax(1)[first].tolist()) == {(0 - tonic) % 12} and set(weights.argmax(1)[second].tolist()) == {(9 - tonic) % 12}
    assert seen["latents"].shape[0] == n
    sel = seen["selection"]
    assert float((seen["latents"][first] - sel[(0 - tonic) % 12]).abs().max()) < 0.2 * float(sel.abs().max())
    assert float(doubt[first].max()) < 0.5
