"""GPU: what is built on maua_nmf_kl_f32 — the planted case through the C ABI (template recovery, monotone divergence, final divergence
against float64), ar.nmf / ar.decompose / ar.components, and the shipped examples/stems.py plugin through generate() on the seeded
32-px generator."""
import argparse
import random
import warnings

import numpy as np
import pytest
import torch

import nmf_ref as nr
from maua_stylegan2_amd import _lib, seeding

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture()
def ar(gpu):
    import maua_stylegan2_amd.audioreactive as ar

    before = ar.signal.SMF
    ar.set_SMF(1)
    yield ar
    ar.set_SMF(before)


def _iterate(v, w, h, n_iter, update_w=1):
    return _lib.load().maua_nmf_kl_f32(v.data_ptr(), w.data_ptr(), h.data_ptr(), v.shape[0], v.shape[1], w.shape[1], n_iter, update_w, 1,
                                       nr.EPS, _lib.stream_ptr(v.device))


def row_cosines(H, H_true):
    a = np.asarray(H, np.float64)
    a = a / np.linalg.norm(a, axis=1, keepdims=True)
    b = H_true / np.linalg.norm(H_true, axis=1, keepdims=True)
    return (a * b).sum(axis=1)


def test_planted_case(gpu):
    """F = 96, T = 400, K = 3, 200 iterations from the seeded start, one call at a time: the divergence of the device's state (evaluated
    in float64 on the host) never rises, every true template is recovered with cosine >= 0.999, and the final divergence is at most
    float64's times (1 + PLANTED_MARGIN).  One call of 200 iterations gives the same bits."""
    V, Wt, _ = nr.planted()
    W0, H0 = nr.seeded_start(V, nr.PLANTED_K, nr.PLANTED_SEED)
    ref = nr.planted_reference()
    with torch.cuda.device(gpu):
        v, w, h = (torch.from_numpy(x).to(gpu) for x in (V, W0, H0))
        trace = [nr.divergence(V, W0, H0)]
        for _ in range(nr.PLANTED_ITERS):
            assert _iterate(v, w, h, 1) == 0
            trace.append(nr.divergence(V, w.cpu().numpy(), h.cpu().numpy()))
        w200, h200 = torch.from_numpy(W0).to(gpu), torch.from_numpy(H0).to(gpu)
        assert _iterate(v, w200, h200, nr.PLANTED_ITERS) == 0
        assert torch.equal(w200, w) and torch.equal(h200, h)
    trace = np.array(trace)
    cosines = nr.template_cosines(w.cpu().numpy(), Wt)
    excess = (trace[-1] - ref["trace"][-1]) / ref["trace"][-1]
    print(f"planted: D {trace[0]:.6g} -> {trace[-1]:.9g} (float64 {ref['trace'][-1]:.9g}, excess {excess:.3g}, allowed {nr.PLANTED_MARGIN:.3g}); "
          f"largest step {np.diff(trace).max():.3g}; cosines {cosines}")
    assert (np.diff(trace) <= 0).all()
    assert (cosines >= nr.PLANTED_COSINE).all()
    assert trace[-1] <= ref["trace"][-1] * (1 + nr.PLANTED_MARGIN)


def test_nmf_recovers_the_planted_factors(ar, gpu):
    V, Wt, Ht = nr.planted()
    W, H = ar.nmf(V, nr.PLANTED_K, n_iter=nr.PLANTED_ITERS, seed=nr.PLANTED_SEED)
    assert W.is_cuda and H.is_cuda and W.dtype == H.dtype == torch.float32
    assert tuple(W.shape) == (nr.PLANTED_F, nr.PLANTED_K) and tuple(H.shape) == (nr.PLANTED_K, nr.PLANTED_T)
    Wn, Hn = W.cpu().numpy(), H.cpu().numpy()
    assert np.allclose(Wn.sum(axis=0), 1, atol=1e-5) and (np.diff(nr.centroids(Wn)) > 0).all()
    # the planted templates sit on ascending thirds of the bins: after the ordering, component k IS template k
    cos_w = [float(nr.template_cosines(Wn[:, k:k + 1], Wt[:, k:k + 1])[0]) for k in range(nr.PLANTED_K)]
    cos_h = row_cosines(Hn, Ht)
    print(f"ar.nmf: template cosines {cos_w}, activation cosines {cos_h}")
    assert min(cos_w) >= nr.PLANTED_COSINE and cos_h.min() >= nr.PLANTED_COSINE
    want_w, want_h = nr.normalise_and_order(nr.planted_reference()["W"], nr.planted_reference()["H"])
    assert float(np.abs(Wn.astype(np.float64) @ Hn - want_w @ want_h).max()) < 1e-3 * float(V.max())
    again = ar.nmf(torch.from_numpy(V), nr.PLANTED_K, n_iter=nr.PLANTED_ITERS, seed=nr.PLANTED_SEED)
    assert torch.equal(again[0], W) and torch.equal(again[1], H)                       # the same answer on every run, tensor or array
    other = ar.nmf(V, nr.PLANTED_K, n_iter=nr.PLANTED_ITERS, seed=nr.PLANTED_SEED + 1)
    assert not torch.equal(other[1], H) and (nr.template_cosines(other[0].cpu().numpy(), Wt) >= nr.PLANTED_COSINE).all()


def test_nmf_with_a_fixed_dictionary_returns_the_planted_activations(ar, gpu):
    V, Wt, Ht = nr.planted()
    W, H = ar.nmf(V, nr.PLANTED_K, n_iter=nr.PLANTED_ITERS, W=Wt.astype(np.float32), update_w=False)
    want_w, _ = nr.normalise_and_order(Wt.astype(np.float32), Ht)
    assert nr.rel_error(W.cpu().numpy(), want_w) < 1e-6  # the dictionary itself, at unit sum
    cos_h = row_cosines(H.cpu().numpy(), Ht)
    d = float(ar.nmf_divergence(torch.from_numpy(V).to(gpu), W, H))
    print(f"fixed dictionary: activation cosines {cos_h}, divergence {d:.6g}")
    assert cos_h.min() >= nr.PLANTED_COSINE and np.isfinite(d)
    with pytest.raises(ValueError, match="needs a dictionary"):
        ar.nmf(V, nr.PLANTED_K, update_w=False)
    with pytest.raises(ValueError, match=r"W must be \[96, 3\]"):
        ar.nmf(V, nr.PLANTED_K, W=Wt[:, :2].astype(np.float32))


def test_nmf_tolerance_stops_early_and_bad_input_is_refused(ar, gpu):
    V, _, _ = nr.planted()
    v = torch.from_numpy(V).to(gpu)
    full = ar.nmf(V, nr.PLANTED_K, n_iter=nr.PLANTED_ITERS)
    early = ar.nmf(V, nr.PLANTED_K, n_iter=nr.PLANTED_ITERS, tol=0.5)      # stops at the first check whose 10 iterations gained < 50 %
    never = ar.nmf(V, nr.PLANTED_K, n_iter=nr.PLANTED_ITERS, tol=0.0)      # the decrease is never below 0: the whole loop, checked
    d_full, d_early = float(ar.nmf_divergence(v, *full)), float(ar.nmf_divergence(v, *early))
    print(f"tol: divergence after the whole loop {d_full:.6g}, stopped early {d_early:.6g}")
    assert d_early > d_full and torch.equal(never[0], full[0]) and torch.equal(never[1], full[1])
    for bad in (-1.0, float("nan"), float("inf")):
        broken = V.copy()
        broken[5, 7] = bad
        with pytest.raises(ValueError, match="finite and non-negative"):
            ar.nmf(broken, nr.PLANTED_K)


# ------------------------------------------------------------------------------------------------ ar.decompose / ar.components
SR = 22050


def tone_and_bursts(seconds=4.0):
    """A 110 Hz tone pulsed at 2 Hz plus white-noise bursts at 3 Hz, and the two gates (amplitude envelopes) per sample."""
    t = np.arange(int(SR * seconds)) / SR
    tone_gate = (0.5 - 0.5 * np.cos(2 * np.pi * 2 * t)) ** 2
    burst_gate = (0.5 - 0.5 * np.cos(2 * np.pi * 3 * t)) ** 6
    rng = np.random.default_rng(31)
    y = 0.5 * tone_gate * np.sin(2 * np.pi * 110 * t) + 0.3 * burst_gate * rng.standard_normal(t.size)
    return y.astype(np.float32), tone_gate, burst_gate


@pytest.mark.parametrize("spectrum,bins", [("mel", 128), ("stft", 1025)])
def test_decompose_separates_a_tone_from_noise_bursts(ar, spectrum, bins):
    """K = 2: the tone is component 0 (the lower centroid) and its activation follows the tone's gate, component 1 the bursts'
    (correlation > 0.9 each; the float64 reference gives 0.999 and 0.992 for either spectrum)."""
    y, tone_gate, burst_gate = tone_and_bursts()
    comps, act = ar.decompose(y, SR, n_components=2, spectrum=spectrum)
    assert comps.is_cuda and tuple(comps.shape) == (2, bins) and tuple(act.shape) == (2, 1 + len(y) // 512)
    comps, act = comps.cpu().numpy(), act.cpu().numpy()
    at = np.minimum(np.arange(act.shape[1]) * 512, len(y) - 1)
    c = nr.centroids(comps.T)
    corr = [float(np.corrcoef(act[0], tone_gate[at])[0, 1]), float(np.corrcoef(act[1], burst_gate[at])[0, 1])]
    print(f"decompose({spectrum}): centroids {c}, correlation with the gates {corr}")
    hz_per_bin = SR / 2048
    assert c[0] < c[1] and (spectrum != "stft" or abs(float(np.argmax(comps[0])) * hz_per_bin - 110) < 2 * hz_per_bin)
    assert corr[0] > 0.9 and corr[1] > 0.9
    with pytest.raises(ValueError, match="unknown spectrum"):
        ar.decompose(y, SR, spectrum="cqt")


def test_components(ar, gpu):
    y, _, _ = tone_and_bursts()
    n = 64
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        env = ar.components(y, SR, n, n_components=2)
        on_dev = ar.components(y, SR, n, n_components=2, device="cuda")
        three = ar.components(y, SR, n, n_components=3, margin=-2, power=2)
    assert env.device.type == "cpu" and on_dev.is_cuda and env.dtype == torch.float32 and tuple(env.shape) == (n, 2) and tuple(three.shape) == (n, 3)
    assert torch.equal(on_dev.cpu(), env)  # the same answer on two runs, wherever it is delivered
    for e in (env, three):
        assert bool(torch.isfinite(e).all()) and float(e.min()) >= 0 and float(e.max()) <= 1
    assert float(env.max(dim=0).values.min()) == 1  # percentile_clip scales every live column to a maximum of 1
    latents = torch.randn(2, 6, 512, generator=torch.Generator().manual_seed(3))
    assert tuple(ar.chroma_weight_latents(env, latents).shape) == (n, 6, 512)
    with pytest.warns(UserWarning, match="the clip is silent"):
        silent = ar.components(np.zeros(8000, np.float32), SR, 12, n_components=3)
    assert torch.equal(silent, torch.zeros(12, 3))


# ------------------------------------------------------------------------------------------------ examples/stems.py through generate()
SIZE, FPS, BATCH = 32, 16, 4


def two_source_clip():
    """One second: a 110 Hz tone in the first half, noise bursts in the second."""
    t = np.arange(SR) / SR
    rng = np.random.default_rng(21)
    tone = 0.5 * np.sin(2 * np.pi * 110 * t) * (t < 0.5) * (0.5 - 0.5 * np.cos(2 * np.pi * 4 * t))
    bursts = 0.3 * rng.standard_normal(SR) * (t >= 0.5) * (0.5 - 0.5 * np.cos(2 * np.pi * 6 * t)) ** 4
    return (tone + bursts).astype(np.float32)


def test_stems_plugin_through_generate(ar, gpu, tmp_path, monkeypatch):
    from maua_stylegan2_amd import generate_audiovisual as gav
    from maua_stylegan2_amd import render
    from maua_stylegan2_amd.audioreactive.examples import default, stems
    from maua_stylegan2_amd.models.stylegan2 import Generator

    g = Generator(SIZE, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(SIZE, seed=60, rgb_gain=0.3), strict=True)
    g = g.to(gpu).eval()
    monkeypatch.setattr(render, "_output_dims", lambda out_size: (SIZE, SIZE))
    monkeypatch.setattr(render.shutil, "which", lambda name: None)
    for name in ("MAUA_SUBFRAMES", "MAUA_SHUTTER", "MAUA_SHUTTER_LIGHT", "MAUA_PIPE_PIX_FMT"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.chdir(tmp_path)
    clip = two_source_clip()
    monkeypatch.setattr(ar, "load_audio", lambda audio_file, offset, duration: (clip, SR, 1.0))
    monkeypatch.setattr(gav, "load_generator", lambda **kw: g)
    np.save("lat.npy", seeding.seeded_latents(12, g.n_latent, seed=11).numpy())  # (the default plugin weights 12 entries by the chromagram)

    captured, seen = [], {}
    orig_capture = g.capture_graph

    def capture(batch, lane=0, **kw):
        bends = kw.get("bends") or []
        captured.append([type(b["transform"]).__name__ for b in bends])
        assert all(hasattr(b["transform"], "run_static") for b in bends)
        return orig_capture(batch, lane=lane, **kw)

    def initialize(args):
        args = stems.initialize(args)
        seen["stems"], seen["hits"] = args.stems.clone(), args.hits.clone()
        return args

    monkeypatch.setattr(g, "capture_graph", capture)

    def run(name, plugin, init):
        random.seed(5), np.random.seed(5), torch.manual_seed(5), torch.cuda.manual_seed_all(5)
        args = argparse.Namespace(fps=FPS, latent_count=12)
        out = gav.generate(ckpt=None, audio_file="stub.wav", initialize=init, get_latents=plugin.get_latents, get_noise=plugin.get_noise,
                           get_bends=getattr(plugin, "get_bends", None), latent_file="lat.npy", G_res=SIZE, out_size=SIZE, fps=FPS, batch=BATCH,
                           output_file=str(tmp_path / name), args=args)
        return np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(-1, SIZE, SIZE, 3)

    first = run("first.mp4", stems, initialize)
    assert first.shape[0] == FPS and first.std() > 5
    assert captured and all(names == ["Swirl"] for names in captured), captured  # the bend ran inside the captured forward: no eager fallback
    env, hits = seen["stems"], seen["hits"]
    assert tuple(env.shape) == (FPS, stems.N_STEMS) and tuple(hits.shape) == (FPS,)
    assert float(env.min()) >= 0 and float(env.max()) <= 1 and float(hits.min()) >= 0 and float(hits.max()) <= 1
    low = env[:, 0]
    print(f"lowest stem: first half {float(low[2:6].mean()):.3f}, second half {float(low[10:14].mean()):.3f}")
    assert float(low[2:6].mean()) > float(low[10:14].mean()) + 0.2  # the tone plays in the first half
    n_captured = len(captured)
    second = run("second.mp4", stems, initialize)
    assert np.array_equal(first, second)
    base = run("default.mp4", default, default.initialize)
    assert len(captured) >= n_captured
    assert base.shape == first.shape and not np.array_equal(base, first)
