"""GPU: audioreactive/filters.py on clips of a second or a few — ar.sosfilt and ar.sosfiltfilt against scipy and a long-double loop
under the allowance rule of tests/iir_ref.py, ar.bandpass on tones, ar.bands on alternating bursts (link by link against host
restatements), rms / pitch with the band-pass on the device (ar.set_filter, pitch(filter=)) against the host path, and the shipped
examples/bands.py plugin through generate()."""
import argparse
import math
import random

import numpy as np
import pytest
import scipy.signal
import torch

import iir_ref as q
from maua_stylegan2_amd import seeding

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SR = q.SR


@pytest.fixture()
def ar(gpu):
    import maua_stylegan2_amd.audioreactive as ar

    before, where = ar.signal.SMF, ar.signal.FILTER
    ar.set_SMF(1)
    yield ar
    ar.set_SMF(before)
    ar.set_filter(where)


def tone(freq, seconds, amp=0.5):
    return (amp * np.sin(2 * np.pi * freq * np.arange(int(seconds * SR)) / SR)).astype(np.float32)


@pytest.fixture(scope="module")
def clip():
    """One second: three tones and noise."""
    noise = 0.1 * np.random.default_rng(4).standard_normal(SR).astype(np.float32)
    return (tone(90, 1, 0.3) + tone(440, 1, 0.3) + tone(3000, 1, 0.2) + noise).astype(np.float32)


def allow_for(sos, x, ref):
    """The allowance of iir_ref.allowance for an arbitrary clip: 4 max(err chunked float64, err scipy float64, 16 * 2^-53)."""
    x = x.astype(np.float64)
    return 4.0 * max(q.rel_err(q.chunked(sos, x, q.default_chunk(len(x)))[0][0], ref), q.rel_err(scipy.signal.sosfilt(sos, x), ref), 16 * q.EPS)


@pytest.fixture(scope="module")
def rms_reference(clip):
    """(long-double output of the rms band-pass over the clip, allowance)."""
    sos = q.filters()["rms"]
    ref = q.sequential(sos, clip, dtype=np.longdouble)[0][0]
    return ref, allow_for(sos, clip, ref)


def test_sosfilt_against_scipy(ar, gpu, clip, rms_reference):
    sos = q.filters()["rms"]
    ref, allow = rms_reference
    scale = float(np.max(np.abs(ref)))
    y64 = ar.sosfilt(sos, clip, dtype=torch.float64)
    assert y64.is_cuda and y64.dtype == torch.float64 and y64.shape == (SR,)
    err = float(np.max(np.abs(y64.cpu().numpy().astype(np.longdouble) - ref)))
    theirs = q.rel_err(scipy.signal.sosfilt(sos, clip.astype(np.float64)), ref)
    print(f"ar.sosfilt: |y - long double| = {err / scale:.2e} max|y| (allow {allow:.2e}); scipy {theirs:.2e}")
    assert err <= allow * scale
    y32 = ar.sosfilt(sos, torch.from_numpy(clip).to(gpu))
    assert y32.is_cuda and y32.dtype == torch.float32 and q.same_bits(y32.cpu().numpy(), y64.cpu().numpy().astype(np.float32))
    assert q.same_bits(ar.sosfilt(sos, clip.astype(np.float64), dtype=torch.float64).cpu().numpy(), y64.cpu().numpy())  # (a float widens exactly)
    # a state in, a state out, as scipy returns them; on the host where asked
    zi = 1e-3 * np.random.default_rng(2).standard_normal((12, 2))
    y, zf = ar.sosfilt(sos, clip, zi=zi, dtype=torch.float64, device="cpu")
    want, want_zf = q.sequential(sos, clip, zi=zi[None], dtype=np.longdouble)
    assert not y.is_cuda and zf.shape == (12, 2) and float(np.max(np.abs(y.numpy() - want[0]))) <= allow * scale
    assert float(np.max(np.abs(zf.numpy() - want_zf[0]))) <= allow * max(scale, float(np.max(np.abs(want_zf))))
    # a bank over the one signal, a filter over several signals, an empty signal
    bank = np.stack([q.filters()[k] for k in q.BANKS[12]])
    yb = ar.sosfilt(bank, clip, dtype=torch.float64)
    assert yb.shape == (3, SR) and q.same_bits(yb[0].cpu().numpy(), y64.cpu().numpy())
    rows = ar.sosfilt(sos, np.stack([clip, clip[::-1]]), dtype=torch.float64)
    assert rows.shape == (2, SR) and q.same_bits(rows[0].cpu().numpy(), y64.cpu().numpy())
    assert ar.default_chunk(SR) == 64
    other = ar.sosfilt(sos, clip, dtype=torch.float64, chunk=16)  # another chunk length: other last bits, the same filter
    assert not q.same_bits(other.cpu().numpy(), y64.cpu().numpy()) and float((other - y64).abs().max()) <= 1e-10 * scale
    assert ar.sosfilt(sos, np.zeros(0, np.float32)).shape == (0,)
    with pytest.raises(ValueError):
        ar.sosfilt(np.ones((17, 6)), clip)
    with pytest.raises(ValueError):
        ar.sosfilt(bank, np.stack([clip, clip]))


def filtfilt_steps(sos, x, forward):
    """scipy.signal.sosfiltfilt's steps around any forward filter ``forward(ext, zi) -> y`` (numpy, any float type)."""
    from maua_stylegan2_amd.audioreactive import filters as f

    edge = f.filtfilt_pad(sos)
    ext = np.concatenate([2 * x[0] - x[edge:0:-1], x, 2 * x[-1] - x[-2:-edge - 2:-1]])
    zi = scipy.signal.sosfilt_zi(sos).astype(x.dtype)
    y = forward(ext, zi * ext[0])
    y = forward(y[::-1], zi * y[-1])
    return y[::-1][edge:-edge]


def test_sosfiltfilt_against_scipy(ar, clip):
    sos = q.filters()["lp100"]
    x64 = clip.astype(np.float64)
    ref = filtfilt_steps(sos, clip.astype(np.longdouble), lambda e, z: q.sequential(sos, e, zi=z[None], dtype=np.longdouble)[0][0])
    chunk = q.default_chunk(len(clip) + 2 * 15)
    restated = filtfilt_steps(sos, x64, lambda e, z: q.chunked(sos, e, chunk, zi=z[None])[0][0])
    theirs = scipy.signal.sosfiltfilt(sos, x64)
    allow = 4.0 * max(q.rel_err(restated, ref), q.rel_err(theirs, ref), 16 * q.EPS)
    y = ar.sosfiltfilt(sos, clip, dtype=torch.float64)
    assert y.is_cuda and y.shape == (SR,)
    err = q.rel_err(y.cpu().numpy(), ref)
    print(f"ar.sosfiltfilt: |y - long double| = {err:.2e} max|y| (allow {allow:.2e}); scipy {q.rel_err(theirs, ref):.2e}")
    assert err <= allow
    y32 = ar.sosfiltfilt(sos, clip)
    assert y32.dtype == torch.float32 and q.same_bits(y32.cpu().numpy(), y.cpu().numpy().astype(np.float32))
    both = ar.sosfiltfilt(sos, np.stack([clip, 2 * clip]), dtype=torch.float64)
    assert both.shape == (2, SR) and q.same_bits(both[0].cpu().numpy(), y.cpu().numpy())
    with pytest.raises(ValueError, match="longer than the padding"):
        ar.sosfiltfilt(sos, clip[:15])


def test_bandpass_gains(ar):
    """Tones in and out of a 300-3000 Hz band-pass: the gains are the ones scipy's output has, within the allowance."""
    order, fmin, fmax = 4, 300.0, 3000.0
    sos = scipy.signal.butter(order, [fmin, fmax], "bp", fs=SR, output="sos")
    tones = np.stack([tone(f, 0.5, 1.0) for f in (1000.0, 50.0, 9000.0)])
    ref = q.sequential(np.stack([sos] * 3), tones, dtype=np.longdouble)[0]
    gain = lambda y: float(np.sqrt(np.mean(np.asarray(y, dtype=np.float64)[SR // 4:] ** 2)) / math.sqrt(0.5))  # noqa: E731
    for k, f in enumerate((1000.0, 50.0, 9000.0)):
        allow = allow_for(sos, tones[k], ref[k])
        scale = float(np.max(np.abs(ref[k])))
        y = ar.bandpass(tones[k], SR, fmin, fmax, order=order, dtype=torch.float64).cpu().numpy()
        theirs = scipy.signal.sosfilt(sos, tones[k].astype(np.float64))
        print(f"{f:6.0f} Hz: gain {gain(y):.3e} (scipy {gain(theirs):.3e}), |y - long double| = {q.rel_err(y, ref[k]):.2e} (allow {allow:.2e})")
        assert float(np.max(np.abs(y.astype(np.longdouble) - ref[k]))) <= allow * scale
        assert abs(gain(y) - gain(theirs)) <= 2 * allow * scale / math.sqrt(0.5)
        assert (abs(gain(y) - 1) < 0.01) if k == 0 else (gain(y) < 0.05)
    x = tones[0] + tones[1]
    assert q.same_bits(ar.bandpass(x, SR, fmin, fmax, order=order, zero_phase=True).cpu().numpy(), ar.sosfiltfilt(sos, x).cpu().numpy())
    assert q.same_bits(ar.bandpass(x, SR, 20, 8000).cpu().numpy(), ar.sosfilt(q.filters()["rms"], x).cpu().numpy())


# ------------------------------------------------------------------------------------------------ ar.envelope, ar.bands
def test_envelope_wrapper(ar, gpu):
    x = np.abs(np.random.default_rng(6).standard_normal((300, 5))).astype(np.float32)
    ca, cr = np.float32(ar.envelope_coefficient(0)), np.float32(ar.envelope_coefficient(8))
    y = ar.envelope(x, 0, 8)
    assert not y.is_cuda and q.same_bits(y.numpy(), q.follower(x, ca, cr))
    one = ar.envelope(torch.from_numpy(x[:, 0]).to(gpu), 2, 8)
    assert one.is_cuda and one.shape == (300,)
    assert q.same_bits(one.cpu().numpy(), q.follower(x[:, :1], np.float32(ar.envelope_coefficient(2)), cr)[:, 0])
    ar.set_SMF(2)
    assert q.same_bits(ar.envelope(x, 0, 4).numpy(), y.numpy())  # twice the frame rate, half the frames: the same coefficients
    ar.set_SMF(1)
    y0 = ar.envelope(x, 0, 8, y0=np.full(5, 9.0, np.float32))
    assert q.same_bits(y0.numpy(), q.follower(x, ca, cr, np.full(5, 9.0, np.float32)))


FPS_BANDS, BURST = 24, 1.0


@pytest.fixture(scope="module")
def bursts():
    """Four seconds: 60 Hz, 4 kHz, 60 Hz, 4 kHz, a second each, with 10 ms fades."""
    n = int(BURST * SR)
    fade = np.minimum(1, np.minimum(np.arange(n), n - 1 - np.arange(n)) / (0.01 * SR)).astype(np.float32)
    return np.concatenate([tone(f, BURST) * fade for f in (60.0, 4000.0, 60.0, 4000.0)])


def host_percentile_clip(col, p=100):
    peaks = col[1:-1][(col[1:-1] > col[2:]) & (col[1:-1] > col[:-2])]
    ordered = np.sort(peaks)
    top = ordered[round(0.01 * p * (len(ordered) - 1))]
    clipped = np.clip(col, 0, top)
    return clipped / clipped.max()


def test_bands_on_alternating_bursts(ar, bursts):
    from maua_stylegan2_amd.audioreactive import filters as f

    n_frames = int(4 * BURST * FPS_BANDS)
    release = 3
    env = ar.bands(bursts, SR, n_frames, release=release)
    assert not env.is_cuda and env.shape == (n_frames, 4) and env.dtype == torch.float32
    assert float(env.min()) >= 0 and float(env.max()) <= 1
    centres = [int((k + 0.5) * BURST * FPS_BANDS) for k in range(4)]
    e = env.numpy()
    print("bands at the burst centres:", np.round(e[centres], 3).tolist())
    for k, c in enumerate(centres):
        own, other = (0, 3) if k % 2 == 0 else (3, 0)
        assert e[c, own] > 0.5 and e[c, other] < 0.1, (k, e[c].tolist())
    # link by link
    sos = ar.bank_sos((20, 150, 600, 2500, 8000), SR, 6)
    y = ar.sosfilt(sos, bursts)
    theirs = np.stack([scipy.signal.sosfilt(s, bursts.astype(np.float64)) for s in sos])
    assert y.shape == (4, len(bursts))
    assert float(np.max(np.abs(y.cpu().numpy() - theirs))) <= 1e-6 * float(np.max(np.abs(theirs)))  # float32 output: 2^-24 and change
    level = f.hop_rms(y)
    hops = len(bursts) // 512
    want_level = np.sqrt((y.cpu().numpy().astype(np.float64)[:, : hops * 512].reshape(4, hops, 512) ** 2).mean(-1)).T
    assert level.shape == (hops, 4) and np.allclose(level.cpu().numpy(), want_level, rtol=1e-5, atol=1e-7)
    res = ar.resample(level, n_frames)
    want_res = scipy.signal.resample(level.cpu().numpy().astype(np.float64), n_frames, axis=0)
    assert np.allclose(res.cpu().numpy(), want_res, rtol=0, atol=1e-9)
    lo, hi = level.min(0).values.double(), level.max(0).values.double()
    held = torch.minimum(torch.maximum(res, lo), hi).float()
    followed = ar.envelope(held, 0, release)
    assert q.same_bits(followed.cpu().numpy(), q.follower(held.cpu().numpy(), 1.0, np.float32(ar.envelope_coefficient(release))))
    want = np.stack([host_percentile_clip(col) for col in followed.cpu().numpy().T], 1)
    assert np.allclose(e, want, rtol=1e-6, atol=1e-7)
    # options: a low-pass / high-pass at the ends, smoothing, power, the device
    ends = ar.bands(bursts, SR, n_frames, edges=(None, 150, 2500, None), release=release, smooth=1, power=2, device="cuda")
    assert ends.is_cuda and ends.shape == (n_frames, 3) and float(ends.min()) >= 0 and float(ends.max()) <= 1
    assert float(ends[centres[0], 0]) > 0.5 and float(ends[centres[1], 2]) > 0.5 and float(ends[centres[1], 0]) < 0.1


# ------------------------------------------------------------------------------------------------ rms / pitch with filter="device"
def test_rms_device_filter_against_host(ar, clip, rms_reference):
    ref, allow = rms_reference
    host = ar.signal._butter_bandpass(clip, SR, 20, 8000, "host")
    dev = ar.signal._butter_bandpass(clip, SR, 20, 8000, "device")
    assert isinstance(host, np.ndarray) and host.dtype == np.float32 and dev.is_cuda and dev.dtype == torch.float32
    diff = np.abs(dev.cpu().numpy().astype(np.float64) - host.astype(np.float64))
    bound = np.maximum(np.spacing(np.abs(host)).astype(np.float64), allow * float(np.max(np.abs(ref))))
    print(f"filtered signal: {int((diff > 0).sum())} of {len(diff)} samples differ, max {diff.max():.2e}")
    assert (diff <= bound).all()
    assert ar.signal.FILTER == "host"
    a = ar.rms(clip, SR, 48, smooth=3)
    ar.set_filter("device")
    b = ar.rms(clip, SR, 48, smooth=3)
    ar.set_filter("host")
    print(f"rms envelope: max |device - host| = {float((a - b).abs().max()):.2e}")
    assert a.shape == b.shape == (48,) and not b.is_cuda and float((a - b).abs().max()) <= 1e-4
    with pytest.raises(ValueError, match="unknown filter"):
        ar.set_filter("gpu")
    assert q.same_bits(ar.rms(clip, SR, 48, smooth=3).numpy(), a.numpy())


def test_pitch_device_filter_gives_the_tone(ar):
    y = tone(440.0, 1.0) + tone(40.0, 1.0, 0.4)  # a rumble below the band
    want = math.log2(440.0 / 65.0) / math.log2(2100.0 / 65.0)
    dev = ar.pitch(y, SR, 24, margin=None, bandpass=True, filter="device")
    host = ar.pitch(y, SR, 24, margin=None, bandpass=True)
    ar.set_filter("device")
    assert q.same_bits(ar.pitch(y, SR, 24, margin=None, bandpass=True).numpy(), dev.numpy())
    assert q.same_bits(ar.pitch(y, SR, 24, margin=None, bandpass=True, filter="host").numpy(), host.numpy())
    ar.set_filter("host")
    print(f"pitch height: device {float(dev[4:20].mean()):.4f}, host {float(host[4:20].mean()):.4f}, 440 Hz = {want:.4f}")
    assert dev.shape == (24,) and float((dev[4:20] - want).abs().max()) < 0.05 and float((dev - host).abs().max()) < 1e-3


# ------------------------------------------------------------------------------------------------ examples/bands.py through generate()
def test_bands_plugin_through_generate(ar, gpu, bursts, tmp_path, monkeypatch):
    from test_pitch_features_gpu import BATCH, FPS, SIZE

    from maua_stylegan2_amd import generate_audiovisual as gav
    from maua_stylegan2_amd import render
    from maua_stylegan2_amd.audioreactive.examples import bands as plugin
    from maua_stylegan2_amd.models.stylegan2 import Generator

    g = Generator(SIZE, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(SIZE, seed=60, rgb_gain=0.3), strict=True)
    g = g.to(gpu).eval()
    monkeypatch.setattr(render, "_output_dims", lambda out_size: (SIZE, SIZE))
    monkeypatch.setattr(render.shutil, "which", lambda name: None)
    for name in ("MAUA_SUBFRAMES", "MAUA_SHUTTER", "MAUA_SHUTTER_LIGHT", "MAUA_PIPE_PIX_FMT"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.chdir(tmp_path)
    clip = bursts[: 2 * SR]  # a bass second, a treble second
    monkeypatch.setattr(ar, "load_audio", lambda audio_file, offset, duration: (clip, SR, 2.0))
    monkeypatch.setattr(gav, "load_generator", lambda **kw: g)
    np.save("lat.npy", seeding.seeded_latents(8, g.n_latent, seed=11).numpy())
    captured, seen = [], {}
    orig_capture = g.capture_graph

    def capture(batch, lane=0, **kw):
        captured.append([type(b["transform"]).__name__ for b in kw.get("bends") or []])
        return orig_capture(batch, lane=lane, **kw)

    def initialize(args):
        args = plugin.initialize(args)
        seen["bands"] = args.bands.clone()
        return args

    def get_noise(height, width, scale, num_scales, args):
        seen.setdefault("noise", []).append(width)
        return plugin.get_noise(height, width, scale, num_scales, args)

    monkeypatch.setattr(g, "capture_graph", capture)
    random.seed(5), np.random.seed(5), torch.manual_seed(5), torch.cuda.manual_seed_all(5)
    args = argparse.Namespace(fps=FPS, latent_count=8)
    out = gav.generate(ckpt=None, audio_file="stub.wav", initialize=initialize, get_latents=plugin.get_latents, get_noise=get_noise,
                       get_bends=plugin.get_bends, latent_file="lat.npy", G_res=SIZE, out_size=SIZE, fps=FPS, batch=BATCH,
                       output_file=str(tmp_path / "bands.mp4"), args=args)
    n = 2 * FPS
    frames = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(-1, SIZE, SIZE, 3)
    assert frames.shape[0] == n and frames.std() > 5
    assert captured and all(names == ["Swirl"] for names in captured), captured
    levels = seen["bands"]
    assert levels.shape == (n, 4) and float(levels.min()) >= 0 and float(levels.max()) <= 1 and seen["noise"]
    assert float(levels[FPS // 2, 0]) > 0.5 and float(levels[FPS + FPS // 2, 3]) > 0.5 and float(levels[FPS // 2, 3]) < 0.1
    # the recipe for the layers too wide for per-frame fields
    big = plugin.get_noise(512, 512, 0, 1, argparse.Namespace(n_frames=n, top=levels[:, 3]))
    assert isinstance(big, ar.NoiseSynth)
