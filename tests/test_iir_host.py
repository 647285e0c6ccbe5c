"""Host (no GPU): the definitions of tests/iir_ref.py are what they claim to be, the allowance the GPU tests use is honest, and four
deliberately wrong versions of the chunked algorithm are caught by the very comparisons the GPU tests make.  Also the host-side halves
of audioreactive/filters.py: sosfiltfilt's padding rule against scipy, the coefficient mapping of ar.envelope, the band designs."""
import math

import numpy as np
import pytest
import scipy.signal

import iir_ref as q

ALL_CHUNKS = (4, 64, 128)  # (the default is 64 for every length the GPU tests judge against the long-double loop)


def test_longdouble_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "np.longdouble is no reference on this machine"


@pytest.mark.parametrize("name", ["hp30", "lp100", "bp20_200", "rms", "pitch"])
def test_sequential_float64_is_scipy(name):
    sos = q.filters()[name]
    x = q.signals()[0, :3000].astype(np.float64)
    y, zf = q.sequential(sos, x)
    assert q.same_bits(y[0], scipy.signal.sosfilt(sos, x))
    zi = np.random.default_rng(5).standard_normal((len(sos), 2))
    want, want_zf = scipy.signal.sosfilt(sos, x, zi=zi)
    y, zf = q.sequential(sos, x, zi=zi[None])
    assert q.same_bits(y[0], want) and q.same_bits(zf[0], want_zf)


@pytest.mark.parametrize("name", sorted(q.EXACT))
@pytest.mark.parametrize("chunk", [1, 4, 7, 64])
def test_chunked_equals_sequential_on_integers(name, chunk):
    sos = q.EXACT[name]
    x = q.exact_signal(203)
    zi = np.arange(1, 2 * len(sos) + 1, dtype=np.float64).reshape(1, len(sos), 2)
    for z in (None, zi):
        want, want_zf = q.sequential(sos, x, zi=z)
        got, zf = q.chunked(sos, x, chunk, zi=z)
        assert q.same_bits(got, want) and q.same_bits(zf, want_zf)
    if name == "running_sum":
        assert q.same_bits(q.chunked(sos, x, chunk)[0][0], np.cumsum(x))


def test_default_chunk_restated():
    assert [q.default_chunk(n) for n in (0, 1, 32768, 32769, 131072, 131073, 5292000, 1 << 30)] == [64, 64, 64, 128, 128, 256, 1024, 4096]


@pytest.mark.parametrize("name", sorted(q.filters()))
def test_chunked_error_ceiling(name):
    """err_chunked_f64 <= 1e-10 for every filter of the case list and every chunk length the GPU tests use: the allowance derived from
    it cannot hide a broken kernel.  (Worst found: the 8th-order 20-200 Hz band-pass with 4-sample chunks.)"""
    for chunk in ALL_CHUNKS:
        err_c, err_s = q.errors(name, chunk)
        print(f"{name} chunk {chunk}: err_chunked {err_c:.2e} err_sequential {err_s:.2e} allow {q.allowance(name, chunk):.2e}")
        assert err_c <= 1e-10 and err_s <= 1e-10


@pytest.mark.parametrize("chunk", [4, 64, 2048])
def test_chunked_with_state_and_short_last_chunk(chunk):
    """zi, zf and a last chunk shorter than the others (or a single chunk) against the long-double loop."""
    sos = q.filters()["pitch"]
    n = 1531
    x = q.signals()[1, :n].astype(np.float64)
    zi = 1e-3 * np.random.default_rng(9).standard_normal((1, len(sos), 2))
    ref, ref_zf = q.sequential(sos, x, zi=zi, dtype=np.longdouble)
    got, zf = q.chunked(sos, x, chunk, zi=zi)
    scale = float(np.max(np.abs(ref)))
    assert q.rel_err(got, ref) <= 1e-10 and float(np.max(np.abs(zf - ref_zf))) <= 1e-10 * max(scale, float(np.max(np.abs(ref_zf))))


@pytest.mark.parametrize("variant", ["carry_dropped", "carry_late", "sections_reversed", "zi_swapped"])
def test_wrong_variants_are_caught(variant):
    """Each wrong version fails the comparison of the GPU tests (|y - long double| <= allow max|y|) on a filter of the case list, and
    the bit-for-bit comparison on the integer cases.  (Sections commute from a zero state: the state is what tells them apart.)"""
    name, chunk, n = "lp100", 64, 1000
    sos = q.filters()[name]
    x = q.signals()[0, :n].astype(np.float64)
    zi = np.random.default_rng(11).standard_normal((1, len(sos), 2)) * np.array([1.0, -0.7])
    ref, _ = q.sequential(sos, x, zi=zi, dtype=np.longdouble)
    allow = q.allowance(name, chunk)
    assert q.rel_err(q.chunked(sos, x, chunk, zi=zi)[0], ref) <= allow
    assert q.rel_err(q.chunked(sos, x, chunk, zi=zi, variant=variant)[0], ref) > 1e6 * allow
    mix, xi = q.EXACT["mix"], q.exact_signal(203)
    zi = np.array([[[1.0, 2.0], [3.0, 4.0]]])
    assert not q.same_bits(q.chunked(mix, xi, 7, zi=zi, variant=variant)[0], q.sequential(mix, xi, zi=zi)[0])


def test_follower_restatement():
    x = np.array([[0.0], [1.0], [1.0], [0.0], [0.0]], np.float32)
    y = q.follower(x, 0.5, 0.25)
    assert y[:, 0].tolist() == [0.0, 0.5, 0.75, 0.5625, 0.421875]
    assert q.follower(x, 1.0, 1.0).tolist() == x.tolist() and q.follower(x, 0.0, 0.0, y0=[3.0]).tolist() == [[3.0]] * 5
    x = np.array([[1.0, 1.0], [np.nan, 1.0], [2.0, 2.0]], np.float32)
    y = q.follower(x, 0.5, 0.5)
    assert np.isnan(y[1:, 0]).all() and y[:, 1].tolist() == [1.0, 1.0, 1.5]


# ------------------------------------------------------------------------------------------------ audioreactive/filters.py, host side
def test_filtfilt_padding_is_scipys():
    """With the padding length of ar.filtfilt_pad and the odd extension of filters._odd_ext, forward-flip-forward-flip through scipy's
    own sosfilt reproduces scipy.signal.sosfiltfilt bit for bit — for even and odd orders (a first-order section shortens the pad)."""
    import torch

    from maua_stylegan2_amd.audioreactive import filters as f

    x = q.signals()[0, :700].astype(np.float64)
    for sos in (q.filters()["lp100"], q.filters()["rms"], scipy.signal.butter(3, 500, "hp", fs=q.SR, output="sos"),
                scipy.signal.butter(5, [300, 900], "bp", fs=q.SR, output="sos"), f.bank_sos((None, 200), q.SR, 6)[0]):
        edge = f.filtfilt_pad(sos)
        ext = f._odd_ext(torch.from_numpy(x), edge).numpy()
        assert len(ext) == len(x) + 2 * edge
        zi = scipy.signal.sosfilt_zi(sos)
        y, _ = scipy.signal.sosfilt(sos, ext, zi=zi * ext[0])
        y, _ = scipy.signal.sosfilt(sos, y[::-1], zi=zi * y[-1])
        assert q.same_bits(np.ascontiguousarray(y[::-1][edge:-edge]), scipy.signal.sosfiltfilt(sos, x))


def test_envelope_coefficient_mapping():
    import maua_stylegan2_amd.audioreactive as ar

    smf = ar.signal.SMF
    try:
        ar.set_SMF(1)
        assert ar.envelope_coefficient(0) == 1.0 and ar.envelope_coefficient(-3) == 1.0 and ar.envelope_coefficient(math.inf) == 0.0
        assert ar.envelope_coefficient(float("nan")) == 1.0
        for tau in (0.5, 1, 8, 100):
            assert ar.envelope_coefficient(tau) == -math.expm1(-1.0 / tau)
        assert abs(ar.envelope_coefficient(1 / math.log(2)) - 0.5) < 1e-15
        ar.set_SMF(2)  # twice the frame rate: the same time constant is twice the frames
        assert ar.envelope_coefficient(4) == -math.expm1(-1.0 / 8) and ar.envelope_coefficient(0) == 1.0
    finally:
        ar.set_SMF(smf)


def test_band_designs():
    import maua_stylegan2_amd.audioreactive as ar

    edges = ar.band_edges(4, 20, 8000)
    assert len(edges) == 5 and edges[0] == 20.0 and edges[-1] == 8000.0
    assert np.allclose(np.diff(np.log(edges)), math.log(400) / 4)
    mel = ar.band_edges(3, 100, 4000, scale="mel")
    steps = np.diff(ar.signal._hz_to_mel(np.array(mel)))
    assert len(mel) == 4 and np.allclose(steps, steps[0])
    with pytest.raises(ValueError):
        ar.band_edges(3, scale="bark")
    sos = ar.bank_sos((None, 150, 600, None), q.SR, order=6)
    assert sos.shape == (3, 6, 6)
    assert q.same_bits(sos[1], scipy.signal.butter(6, [150, 600], "bp", fs=q.SR, output="sos"))
    assert q.same_bits(sos[0, :3], scipy.signal.butter(6, 150, "lp", fs=q.SR, output="sos")) and (sos[0, 3:] == q.IDENTITY).all()
    assert q.same_bits(sos[2, :3], scipy.signal.butter(6, 600, "hp", fs=q.SR, output="sos")) and (sos[2, 3:] == q.IDENTITY).all()
    assert q.same_bits(ar.butter_sos(12, [20, 8000], "bp", q.SR), q.filters()["rms"])
