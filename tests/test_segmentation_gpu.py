"""GPU: laplacian_segmentation's kernels (csrc/segment.hip) stage by stage against the CPU restatement (tests/segment_ref.py),
red zones around every output, run-to-run identity, the known-answer A B A C track, plot=True and a kelp-style plugin."""
import os

import numpy as np
import pytest
import torch

import segment_ref as ref
from maua_stylegan2_amd import _lib
from maua_stylegan2_amd.audioreactive import segment

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
SR = 22050
RED = 4096
CANARY = 0x7FC0BEEF


def _env(y, gpu):
    env, _ = segment.onset_envelope(torch.from_numpy(y).to(gpu), SR)
    return env


@pytest.mark.parametrize("bpm", [90, 120, 140])
def test_tempogram_and_tempo_on_click_tracks(gpu, bpm):
    y = ref.click_track(bpm, 20.0, seed=bpm)
    env = _env(y, gpu)
    win = int(8.0 * SR) // 512
    tg = segment.tempogram(env, win).cpu().numpy()
    want = ref.tempogram_mean(env.cpu().numpy().astype(np.float64), win)
    np.testing.assert_allclose(tg, want, rtol=1e-5, atol=1e-7)
    assert segment.tempo_from_tempogram(tg, SR) == ref.tempo(want, SR)
    assert abs(ref.tempo(want, SR) - bpm) < 0.05 * bpm


@pytest.mark.parametrize("kind", ["click90", "click140", "noise0", "noise1"])
def test_beat_dp_matches_the_restatement(gpu, kind):
    y = ref.click_track(int(kind[5:]), 15.0) if kind.startswith("click") else ref.noise_burst_track(15.0, seed=int(kind[5:]))
    env = _env(y, gpu)
    e64 = env.double().cpu().numpy()
    bpm, period, ls, cum, back, beats = ref.beat_track(e64, SR)
    tempo, got_beats = segment.beat_track(env, SR)
    x = env.double()
    x = x / x.std()
    gls, gcum, gback = (t.cpu().numpy() for t in segment.beat_dp(x, period))
    np.testing.assert_allclose(gls, ls, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(gcum, cum, rtol=1e-9, atol=1e-9)
    assert np.array_equal(gback, back)
    assert tempo == bpm and np.array_equal(got_beats, beats)


def test_beat_sync_spans_of_any_length(gpu):
    rng = np.random.default_rng(5)
    n = 4000
    x = rng.standard_normal((252, n)).astype(np.float32)
    x[:, 100:110] = 0.5  # ties inside a span
    bounds = np.array([0, 1, 2, 4, 7, 13, 100, 110, 2300, 2301, n])  # spans of 1, 2, 3, 6, 87, 10, 2190, 1, 1699 frames
    spans = list(zip(bounds[:-1], bounds[1:]))
    xd = torch.from_numpy(x).to(gpu)
    med = segment.beat_sync(xd, bounds, median=True).cpu().numpy()
    mean = segment.beat_sync(xd, bounds, median=False).cpu().numpy()
    np.testing.assert_allclose(med, ref.sync(x, spans, np.median), rtol=1e-6, atol=1e-6)
    want_mean = ref.sync(x.astype(np.float64), spans, np.mean).astype(np.float32)
    np.testing.assert_allclose(mean, want_mean, rtol=1e-6, atol=1e-6)
    assert np.array_equal(med[:, 6], np.full(252, 0.5, np.float32))


@pytest.mark.parametrize("s", [7, 64, 301, 1500])
@pytest.mark.parametrize("d", [20, 252])
def test_knn_links_match_the_restatement(gpu, s, d):
    rng = np.random.default_rng(s * 1000 + d)
    x = rng.standard_normal((d, s)).astype(np.float32)
    k = ref.knn_k(s)
    links = segment.knn_links(torch.from_numpy(x).to(gpu), k).cpu().numpy()
    dist = ref.pair_distances(x)
    want = ref.knn_sets(dist, k)
    for i in range(s):
        got = set(np.flatnonzero(links[i] >= 0).tolist())
        if got != want[i]:
            row = sorted(dist[i, j] for j in range(s) if abs(i - j) >= 3)
            assert abs(row[k] - row[k - 1]) <= 1e-5 * row[k], (i, got ^ want[i])
        np.testing.assert_allclose(links[i][sorted(got)], dist[i][sorted(got)], rtol=1e-6)
    both = (links >= 0) & (links.T >= 0)
    assert np.array_equal(links[both], links.T[both])  # d(i, j) and d(j, i) bit for bit


@pytest.mark.parametrize("s", [7, 64, 301])
def test_affinity_and_timelag_median(gpu, s):
    rng = np.random.default_rng(s)
    x = rng.standard_normal((20, s)).astype(np.float32)
    links = segment.knn_links(torch.from_numpy(x).to(gpu), ref.knn_k(s))
    bw = segment.link_bandwidth(links)
    dist = ref.pair_distances(x)
    rec_want, bw_want, _ = ref.affinity(dist, ref.knn_sets(dist, ref.knn_k(s)))
    assert bw == pytest.approx(bw_want, rel=1e-6)
    rec, rf = segment.rec_affinity(links, bw)
    np.testing.assert_allclose(rec.cpu().numpy(), rec_want, atol=1e-6)
    np.testing.assert_allclose(rf.cpu().numpy(), ref.timelag_median_formula(rec.cpu().numpy().astype(np.float64)), atol=1e-6)
    np.testing.assert_allclose(rf.cpu().numpy(), ref.timelag_median_literal(rec_want), atol=1e-6)


class Guard:
    """Exact-size windows between NaN red zones (tests/test_canary_gpu.py style)."""

    def __init__(self, dev):
        self.dev, self.items = dev, []

    def buf(self, n, dtype, fill=None):
        words = n * torch.tensor([], dtype=dtype).element_size() // 4
        raw = torch.full((RED + words + RED,), CANARY, dtype=torch.int32, device=self.dev)
        view = raw[RED: RED + words].view(dtype)
        if fill is not None:
            view.copy_(fill.reshape(-1).to(self.dev, dtype))
        self.items.append((raw, words, fill is None))
        return view

    def check(self):
        for raw, words, is_out in self.items:
            r = raw.cpu().numpy()
            assert (r[:RED] == CANARY).all() and (r[RED + words:] == CANARY).all(), "write outside a buffer"
            if is_out:
                assert not (r[RED: RED + words] == CANARY).any(), "output element left unwritten"


def test_red_zones_around_every_output(gpu):
    lib = _lib.load()
    st = _lib.stream_ptr(gpu)
    g = Guard(gpu)
    rng = np.random.default_rng(9)
    n, win = 1000, 344
    env = g.buf(n, torch.float32, torch.from_numpy(rng.random(n).astype(np.float32)))
    ws = g.buf(lib.maua_tempogram_ws_doubles(n, win), torch.float64)
    tg = g.buf(win, torch.float32)
    assert lib.maua_tempogram_f32(env.data_ptr(), n, win, ws.data_ptr(), tg.data_ptr(), st) == 0
    on = g.buf(n, torch.float64, torch.from_numpy(rng.random(n)))
    ls, cs, bl = g.buf(n, torch.float64), g.buf(n, torch.float64), g.buf(n, torch.int32)
    assert lib.maua_beat_track_f64(on.data_ptr(), n, 21, ls.data_ptr(), cs.data_ptr(), bl.data_ptr(), st) == 0
    rows, spans = 21, 5
    x = g.buf(rows * n, torch.float32, torch.from_numpy(rng.standard_normal(rows * n).astype(np.float32)))
    b = g.buf(spans + 1, torch.int32, torch.tensor([0, 1, 3, 500, 999, 1000], dtype=torch.int32))
    for median in (0, 1):
        out = g.buf(rows * spans, torch.float32)
        assert lib.maua_beat_sync_f32(x.data_ptr(), rows, n, b.data_ptr(), spans, median, out.data_ptr(), st) == 0
    s, d = 77, 20
    feat = g.buf(d * s, torch.float32, torch.from_numpy(rng.standard_normal(d * s).astype(np.float32)))
    lk = g.buf(s * s, torch.float32)
    assert lib.maua_knn_links_f32(feat.data_ptr(), d, s, 16, 3, lk.data_ptr(), st) == 0
    rec, rf = g.buf(s * s, torch.float32), g.buf(s * s, torch.float32)
    assert lib.maua_rec_affinity_f32(lk.data_ptr(), s, 1.5, rec.data_ptr(), rf.data_ptr(), st) == 0
    torch.cuda.synchronize(gpu)
    g.check()
    for t in (tg, ls, cs, rec, rf):
        assert torch.isfinite(t).all()


def test_two_runs_are_bitwise_equal(gpu):
    y = torch.from_numpy(ref.noise_burst_track(12.0, seed=4)).to(gpu)
    env = _env(y.cpu().numpy(), gpu)
    rng = np.random.default_rng(1)
    feat = torch.from_numpy(rng.standard_normal((252, 700)).astype(np.float32)).to(gpu)
    bounds = np.unique(np.concatenate([[0], rng.integers(1, 5000, 300), [5000]]))
    frames = torch.from_numpy(rng.standard_normal((252, 5000)).astype(np.float32)).to(gpu)

    def run():
        tg = segment.tempogram(env, 344)
        x = env.double() / env.double().std()
        dp = segment.beat_dp(x, 22)
        sync = [segment.beat_sync(frames, bounds, m) for m in (True, False)]
        links = segment.knn_links(feat, ref.knn_k(700))
        aff = segment.rec_affinity(links, segment.link_bandwidth(links))
        return [tg, *dp, *sync, links, *aff]

    a, b = run(), run()
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.fixture(scope="module")
def aba_c():
    return ref.sectioned_track("ABAC", 16, 120, seed=0)


def test_known_answer_sections(gpu, aba_c):
    times, labels = segment.laplacian_segmentation(torch.from_numpy(aba_c).to(gpu), SR, k=3)
    assert labels == [0, 1, 0, 2]
    assert len(times) == len(labels) + 1 and times[0] == 0.0
    assert times[-1] == pytest.approx((1 + len(aba_c) // 512 - 1) * 512 / SR)
    beat = 0.5
    for got, want in zip(times[1:4], (8.0, 16.0, 24.0)):
        assert abs(got - want) <= 2 * beat + 1e-9, times
    want_times, want_labels, want_seg, want_beats = ref.segment(aba_c, SR, 3)
    assert labels == [int(v) for v in want_labels]  # the same partition into sections ...
    np.testing.assert_allclose(times, want_times, rtol=0, atol=beat + 1e-9)  # ... with boundaries on the same beats (+- one)
    again = segment.laplacian_segmentation(aba_c, SR, k=3)  # numpy input, second run: identical
    assert again == (times, labels)


def test_public_surface_and_silence(gpu):
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd.audioreactive import signal as sig

    y = ref.sectioned_track("AB", 8, 120, seed=1)
    times, labels = ar.laplacian_segmentation(y, SR, k=2)
    assert (times, labels) == sig.laplacian_segmentation(y, SR, k=2)
    assert labels[0] == 0 and len(times) == len(labels) + 1
    with pytest.raises(ValueError, match="beat-synchronous columns"):
        ar.laplacian_segmentation(np.zeros(5 * SR, np.float32), SR, k=3)


def test_plot_writes_png(gpu, tmp_path, monkeypatch):
    pytest.importorskip("matplotlib")
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("DISPLAY", raising=False)
    segment.laplacian_segmentation(ref.sectioned_track("AB", 8, 120, seed=2), SR, k=2, plot=True)
    assert os.path.getsize(tmp_path / "workspace" / "laplacian_segmentation.png") > 1000


def test_kelp_style_plugin_generates(gpu, tmp_path, monkeypatch):
    """A plugin in the reference's kelp.py style: get_latents segments the track and loops latents per section."""
    import scipy.io.wavfile
    import torch as th

    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import generate_audiovisual as gav
    from maua_stylegan2_amd import render, seeding

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(render.shutil, "which", lambda name: None)
    y = ref.sectioned_track("ABAB", 8, 120, seed=3)
    scipy.io.wavfile.write("track.wav", SR, (y * 32767 / max(1.0, float(np.abs(y).max()))).astype(np.int16))
    np.save("lat.npy", seeding.seeded_latents(8, 16, seed=3).numpy())
    seen = {}

    def get_latents(selection, args):
        timestamps, labels = ar.laplacian_segmentation(args.audio, args.sr, k=2)
        seen["segments"] = (timestamps, labels)
        seen["n_frames"] = args.n_frames
        latents = []
        for (start, stop), lab in zip(zip(timestamps, timestamps[1:]), labels):
            start_frame = int(round(start / args.duration * args.n_frames))
            stop_frame = int(round(stop / args.duration * args.n_frames))
            section = ar.spline_loops(ar.wrapping_slice(selection, lab, 4), n_frames=stop_frame - start_frame, n_loops=1)
            latents.append(section)
        total = sum(len(lat) for lat in latents)
        if total != args.n_frames:
            latents.append(th.cat([latents[-1][[-1]]] * (args.n_frames - total)))
        return ar.gaussian_filter(th.cat(latents).float(), 3)

    def initialize(args):
        args.rms = ar.rms(args.audio, args.sr, args.n_frames, smooth=10, clip=60, power=1)
        return args

    def get_noise(height, width, scale, num_scales, args):
        return None

    out = gav.generate(ckpt=None, audio_file="track.wav", initialize=initialize, get_latents=get_latents, get_noise=get_noise,
                       latent_file="lat.npy", G_res=512, out_size=512, fps=6, batch=4, output_file=str(tmp_path / "o.mp4"))
    times, labels = seen["segments"]
    assert labels[:2] == [0, 1] and len(times) == len(labels) + 1
    n = seen["n_frames"]
    raw = np.fromfile(out + ".rgb24", dtype=np.uint8)
    assert raw.size == n * 512 * 512 * 3
    assert raw.reshape(n, 512, 512, 3).std() > 5
