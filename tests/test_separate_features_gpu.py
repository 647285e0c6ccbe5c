"""GPU: what is built on maua_nmf_separate_f32 — ``ar.separate`` on the two-tone clip of tests/separate_ref.py (SDR of the stems
against the sources, the stems' sum against the plain STFT round trip, grouping, windows, return types, a fixed dictionary), the stems
as input of the other ``ar.*`` features, and the shipped examples/separated.py plugin.

The float64 restatement of the whole chain (separate_ref.chain, asserted on the CPU in test_separate_host.py) reaches 38.2 - 38.6 dB on
the 220 Hz source and 32.4 - 32.8 dB on the 1760 Hz source at every seed and power, 43 and 37 dB with four components in two groups; the
floor here is 25 dB."""
import argparse

import numpy as np
import pytest
import torch

import separate_ref as sr
from maua_stylegan2_amd import _lib

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SR = sr.SR


@pytest.fixture()
def ar(gpu):
    import maua_stylegan2_amd.audioreactive as ar

    before = ar.signal.SMF
    ar.set_SMF(1)
    yield ar
    ar.set_SMF(before)


@pytest.fixture(scope="module")
def clip():
    x, a, b = sr.two_tone_clip()
    return x.astype(np.float32), a, b


def round_trip(ar, x):
    """istft(stft(x)) through maua_stft_complex_f32 and maua_istft_f32, as ``ar.separate`` calls them."""
    re, im = ar.signal.stft_complex(x)
    dev = re.device
    win = ar.signal._hann(2048, dev)
    ws = torch.empty((re.shape[1], 2048), dtype=torch.float32, device=dev)
    y = torch.empty(len(x), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().maua_istft_f32(re.data_ptr(), im.data_ptr(), win.data_ptr(), 2048, 512, re.shape[1], ws.data_ptr(), y.data_ptr(),
                                              len(x), _lib.stream_ptr(dev)), "maua_istft_f32")
    return y.cpu().numpy()


@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_two_components_recover_the_two_tones(ar, clip, seed, power):
    x, a, b = clip
    stems = ar.separate(x, SR, n_components=2, power=power, n_iter=200, seed=seed)
    assert isinstance(stems, np.ndarray) and stems.dtype == np.float32 and stems.shape == (2, len(x))
    s0, s1 = sr.sdr(stems[0], a), sr.sdr(stems[1], b)
    print(f"seed {seed} power {power}: SDR {s0:.2f} dB (220 Hz), {s1:.2f} dB (1760 Hz); floor {sr.SDR_FLOOR}")
    assert s0 >= sr.SDR_FLOOR and s1 >= sr.SDR_FLOOR
    gap = float(np.abs(stems.astype(np.float64).sum(axis=0) - round_trip(ar, x).astype(np.float64)).max())
    bound = (2 + 2) * 2.0 ** -23 * float(np.abs(x).max())
    print(f"    stems.sum(0) against the round trip: {gap:.3g} (bound {bound:.3g})")
    assert gap <= bound


def test_four_components_in_two_groups(ar, clip):
    x, a, b = clip
    stems, W, H, group = ar.separate(x, SR, n_components=4, groups=2, n_iter=200, return_model=True)
    assert stems.shape == (2, len(x)) and group.dtype == np.int32 and group.tolist() == [0, 0, 1, 1]
    assert W.is_cuda and H.is_cuda and tuple(W.shape) == (1025, 4) and tuple(H.shape) == (4, 1 + len(x) // 512)
    s0, s1 = sr.sdr(stems[0], a), sr.sdr(stems[1], b)
    print(f"K 4 in 2 groups: SDR {s0:.2f} / {s1:.2f} dB")
    assert s0 >= sr.SDR_FLOOR and s1 >= sr.SDR_FLOOR
    given = ar.separate(x, SR, n_components=4, groups=[0, 0, 1, 1], n_iter=200)
    assert np.array_equal(given.view(np.int32), stems.view(np.int32))
    swapped = ar.separate(x, SR, n_components=4, groups=[1, 1, 0, 0], n_iter=200)
    assert np.array_equal(swapped[::-1].view(np.int32), stems.view(np.int32))
    sparse = ar.separate(x, SR, n_components=4, groups=[0, 0, 2, 2], n_iter=200)  # group 1 is empty: a silent stem between the two
    assert sparse.shape == (3, len(x)) and not sparse[1].any()
    assert sr.sdr(sparse[0], a) >= sr.SDR_FLOOR and sr.sdr(sparse[2], b) >= sr.SDR_FLOOR
    gap = float(np.abs(stems.astype(np.float64).sum(axis=0) - round_trip(ar, x).astype(np.float64)).max())
    assert gap <= (2 + 2) * 2.0 ** -23 * float(np.abs(x).max())


def test_one_group_is_the_round_trip_bit_for_bit(ar, clip):
    x = clip[0]
    stems = ar.separate(x, SR, n_components=3, groups=1, n_iter=20)
    assert stems.shape == (1, len(x)) and np.array_equal(stems[0].view(np.int32), round_trip(ar, x).view(np.int32))


def test_windows_of_one_group_give_the_bits_of_one_call(ar, clip):
    x = clip[0]
    whole = ar.separate(x, SR, n_components=5, n_iter=30)
    one_by_one = ar.separate(x, SR, n_components=5, n_iter=30, _window_bytes=1)
    pairs = ar.separate(x, SR, n_components=5, n_iter=30, _window_bytes=2 * (2 * 1025 * (1 + len(x) // 512) * 4))
    assert whole.shape == (5, len(x))
    assert np.array_equal(one_by_one.view(np.int32), whole.view(np.int32)) and np.array_equal(pairs.view(np.int32), whole.view(np.int32))


def test_return_types_and_a_fixed_dictionary(ar, clip, gpu):
    x = clip[0]
    on_host = ar.separate(x, SR, n_components=2, n_iter=50)
    on_dev = ar.separate(torch.from_numpy(x), SR, n_components=2, n_iter=50, device=gpu)
    on_cpu = ar.separate(x, SR, n_components=2, n_iter=50, device="cpu")
    assert isinstance(on_host, np.ndarray) and on_host.dtype == np.float32
    assert isinstance(on_dev, torch.Tensor) and on_dev.is_cuda and on_dev.dtype == torch.float32
    assert isinstance(on_cpu, torch.Tensor) and on_cpu.device.type == "cpu"
    assert np.array_equal(on_dev.cpu().numpy().view(np.int32), on_host.view(np.int32)) and torch.equal(on_cpu, on_dev.cpu())
    _, W, H, _ = ar.separate(x, SR, n_components=2, n_iter=200, return_model=True)
    fixed, W2, H2, _ = ar.separate(x, SR, n_components=2, n_iter=200, W=W, update_w=False, return_model=True)
    assert torch.allclose(W2, W, rtol=1e-5, atol=0)  # the dictionary passes through (unit sum already, ordered already)
    assert tuple(H2.shape) == tuple(H.shape)
    assert sr.sdr(fixed[0], clip[1]) >= sr.SDR_FLOOR and sr.sdr(fixed[1], clip[2]) >= sr.SDR_FLOOR
    with pytest.warns(UserWarning, match="the clip is silent"):
        silent = ar.separate(np.zeros(6000, np.float32), SR, n_components=3)
    assert silent.shape == (3, 6000) and silent.dtype == np.float32 and not silent.any()


def test_a_stem_goes_into_every_feature(ar, clip):
    """``stems[0]`` is accepted by the other features as the clip itself would be, and ``ar.pitch`` of it reads 220 Hz within half a
    semitone on the voiced frames of the 220 Hz source.  Which frames those are is taken from the SOURCE, not from the confidence alone:
    YIN does not see loudness, so the stretches in which only the 1760 Hz source sounds are "voiced" in stem 0 as well — by that
    source's residual, 38 dB down — and the silent stretches hold the last voiced height.  The frames asserted lie in the middle 0.2 s of
    every 0.5 s the 220 Hz source is on (at 60 frames a second: 4.5 sigma of ``ar.pitch``'s smoothing away from its edges), and every
    one of them must be voiced."""
    x = clip[0]
    stems = ar.separate(x, SR, n_components=2, n_iter=200)
    n = 48
    results = {"onsets": ar.onsets(stems[0], SR, n), "rms": ar.rms(stems[0], SR, n), "chroma": ar.chroma(stems[0], SR, n),
               "pitch": ar.pitch(stems[0], SR, n)}
    for name, value in results.items():
        assert isinstance(value, torch.Tensor) and value.shape[0] == n and bool(torch.isfinite(value).all()), name
    assert tuple(results["chroma"].shape) == (n, 12) and results["pitch"].dim() == 1
    fine = int(60 * sr.CLIP_SECONDS)
    height, voicing = ar.pitch(stems[0], SR, fine, return_voicing=True)
    seconds = np.arange(fine) * (sr.CLIP_SECONDS / (fine - 1))
    sounding = (seconds % 1.0 >= 0.15) & (seconds % 1.0 <= 0.35)
    hz = 65.0 * (2100.0 / 65.0) ** height.double().numpy()  # the log height between the fmin and fmax of ar.pitch
    off = 12 * np.abs(np.log2(hz[sounding] / 220.0))
    print(f"ar.pitch of stem 0: {int(sounding.sum())} frames inside the 220 Hz source, lowest voicing {float(voicing.numpy()[sounding].min()):.3f}, "
          f"worst {float(off.max()):.3f} semitones from 220 Hz")
    assert sounding.sum() >= 40 and (voicing.numpy()[sounding] >= 0.5).all() and off.max() <= 0.5


def test_the_separated_plugin(ar, clip, tmp_path):
    from maua_stylegan2_amd import seeding
    from maua_stylegan2_amd.audioreactive.examples import separated

    x = clip[0]
    fps = 12
    n = int(fps * sr.CLIP_SECONDS)
    args = separated.initialize(argparse.Namespace(audio=x, sr=SR, n_frames=n, fps=fps))
    assert isinstance(args.separated, np.ndarray) and args.separated.shape == (separated.N_STEMS, len(x))
    for name in ("bass_line", "bass_level", "hits", "lo_onsets", "hi_onsets"):
        value = getattr(args, name)
        assert tuple(value.shape) == (n,) and bool(torch.isfinite(value).all()), name
    selection = seeding.seeded_latents(12, 10, seed=11)
    latents = separated.get_latents(selection, args)
    assert tuple(latents.shape) == (n, 10, 512) and bool(torch.isfinite(latents).all())
    noise = separated.get_noise(16, 16, 2, 9, args)
    assert tuple(noise.shape) == (n, 1, 16, 16) and noise.is_cuda and bool(torch.isfinite(noise).all())
    assert separated.get_noise(512, 512, 8, 9, args) is None
    bends = separated.get_bends(args)
    assert len(bends) == 1 and tuple(bends[0]["modulation"].shape) == (n,) and bool(torch.isfinite(bends[0]["modulation"]).all())
    assert bends[0]["transform"](bends[0]["modulation"]).capturable  # the render stays on the graph lanes
    ar.save_audio(tmp_path / "low.wav", args.separated[0], SR)
    back, _ = ar.signal._read_audio_file(tmp_path / "low.wav", SR)
    assert np.abs(back - np.clip(args.separated[0], -1, 1)).max() <= 1.0 / 32768
