"""Beat and tempo features on the MI355X: the predominant local pulse (Grosche & Mueller, "Extracting predominant local pulse
information from music recordings", IEEE TASLP 2011).  No counterpart in the reference; parity with librosa.beat.plp is not claimed,
the definition is include/maua_hip.h ("Predominant local pulse") and tests/pulse_ref.py.

Pipeline: the onset envelope the dynamic-programming tracker of segment.py sees -> optionally minus its moving average -> a Fourier
tempogram on an arbitrary tempo grid, of which only every frame's strongest tempo and its phase are kept (maua_tempogram_peak_f32: the
[frames, window] Hankel matrix and the [frames, tempi] map of the torch formulation are never stored) -> the overlap-add of every
frame's windowed sinusoid (maua_pulse_synth_f32, gather form) -> a pulse curve in [0, 1] whose maxima are the beats.  Unlike
``segment.beat_track`` it assumes no global tempo, so it follows a tempo change, and it yields continuous signals: ``pulse`` (the curve),
``tempo`` (BPM) and ``beat_phase`` (a sawtooth through the beats) per video frame.  Peak picking, the beat-phase mapping and the
resampling are a handful of torch / numpy operations on O(frames) values.
"""
import math
import warnings

import numpy as np
import torch as th

from .. import _lib
from . import segment as _seg
from . import signal as _sig

__all__ = ["raw_plp", "tempogram", "pulse", "tempo", "beats", "beat_phase", "beat_phase_from_times", "PULSE_MAX_WIN", "PULSE_MAX_TEMPI"]

PULSE_MAX_FRAMES = 1 << 22  # MAUA_PULSE_MAX_FRAMES, MAUA_PULSE_MAX_WIN, MAUA_PULSE_MAX_TEMPI (include/maua_hip.h)
PULSE_MAX_WIN = 2048
PULSE_MAX_TEMPI = 1024

_TABLES = {}  # (device, win, tempo_min, tempo_max, tempo_step, frames per second) -> the grid and its device tables, oldest dropped beyond 8


def tempo_grid(tempo_min=30, tempo_max=300, tempo_step=1):
    """The tempi tempo_min, tempo_min + tempo_step, ... up to tempo_max in BPM (float64)."""
    if not (tempo_min > 0 and tempo_max >= tempo_min and tempo_step > 0):
        raise ValueError(f"tempo grid: need 0 < tempo_min <= tempo_max and tempo_step > 0 (got {tempo_min}, {tempo_max}, {tempo_step})")
    count = int(math.floor((tempo_max - tempo_min) / tempo_step + 1e-9)) + 1
    if count > PULSE_MAX_TEMPI:
        raise ValueError(f"tempo grid: {count} tempi, at most {PULSE_MAX_TEMPI} — raise tempo_step or narrow the range")
    return tempo_min + tempo_step * np.arange(count, dtype=np.float64)


def _tables(win, tempo_min, tempo_max, tempo_step, fr):
    """(grid in BPM, table [B, win, 2], window [win], omega [B]): the float32 tables both kernels read, built in float64 and rounded once,
    cached on the device per (win, grid, frame rate)."""
    if not (isinstance(win, (int, np.integer)) and 2 <= win <= PULSE_MAX_WIN):
        raise ValueError(f"win must be an integer in 2 .. {PULSE_MAX_WIN} frames (got {win!r})")
    dev = th.device("cuda", th.cuda.current_device())
    key = (dev.index, int(win), float(tempo_min), float(tempo_max), float(tempo_step), float(fr))
    hit = _TABLES.get(key)
    if hit is None:
        grid = tempo_grid(tempo_min, tempo_max, tempo_step)
        omega = 2.0 * np.pi * grid / (60.0 * fr)
        k = np.arange(win, dtype=np.float64)
        window = 0.5 - 0.5 * np.cos(2.0 * np.pi * k / win)  # periodic Hann
        arg = omega[:, None] * k[None, :]
        table = np.stack([window * np.cos(arg), -window * np.sin(arg)], axis=-1).astype(np.float32)
        hit = (grid, th.from_numpy(table).to(dev), th.from_numpy(window.astype(np.float32)).to(dev), th.from_numpy(omega.astype(np.float32)).to(dev))
        _TABLES[key] = hit
        while len(_TABLES) > 8:
            _TABLES.pop(next(iter(_TABLES)))
    return hit


# ------------------------------------------------------------------------------------------------ device stages
def tempogram_peak(env, table, prior=None, want_tgram=False):
    """(bin int32 [N], phase [N], power [N], tgram [N, B] or None) on the device of an envelope [N] against a table [B, W, 2] and an
    optional prior [B], numpy arrays or tensors on any device (maua_tempogram_peak_f32)."""
    shape = tuple(table.shape)
    if len(shape) != 3 or shape[2] != 2:
        raise ValueError(f"tempogram_peak: the table must be [tempi, window, 2] (got {shape})")
    n_tempi, win, _ = shape
    if prior is not None and int(np.prod(prior.shape)) != n_tempi:
        raise ValueError(f"tempogram_peak: prior has {int(np.prod(prior.shape))} values for {n_tempi} tempi")
    env, table = _sig._to_dev(env).reshape(-1), _sig._to_dev(table)
    n = env.numel()
    bins = th.empty(n, dtype=th.int32, device=env.device)
    phase, power = th.empty(n, dtype=th.float32, device=env.device), th.empty(n, dtype=th.float32, device=env.device)
    tgram = th.empty((n, n_tempi), dtype=th.float32, device=env.device) if want_tgram else None
    if prior is not None:
        prior = _sig._to_dev(prior).reshape(-1)
    _lib.call("maua_tempogram_peak_f32", env, n, table, win, n_tempi, prior, bins, phase, power, tgram)
    return bins, phase, power, tgram


def pulse_synth(bins, phase, window, omega):
    """pulse [N] on the device of (bin, phase) [N], window [W] and omega [B], numpy arrays or tensors on any device
    (maua_pulse_synth_f32)."""
    if int(np.prod(bins.shape)) != int(np.prod(phase.shape)):
        raise ValueError(f"pulse_synth: {int(np.prod(bins.shape))} bins for {int(np.prod(phase.shape))} phases, need one of each per frame")
    bins, phase = _sig._to_dev(bins, th.int32).reshape(-1), _sig._to_dev(phase).reshape(-1)
    window, omega = _sig._to_dev(window).reshape(-1), _sig._to_dev(omega).reshape(-1)
    n = bins.numel()
    out = th.empty(n, dtype=th.float32, device=bins.device)
    _lib.call("maua_pulse_synth_f32", bins, phase, n, window, window.numel(), omega, omega.numel(), out)
    return out


def moving_average_detrend(env, win):
    """env minus its mean over the ``win`` frames [t - win // 2, t - win // 2 + win) (zeros outside the clip, always divided by win),
    clamped at 0: a slowly varying loudness is not a pulse.  Sums in float64 on the device."""
    n = env.numel()
    c = th.cat([th.zeros(1, dtype=th.float64, device=env.device), th.cumsum(env.double(), 0)])
    at = th.arange(n, device=env.device) - win // 2
    mean = (c[(at + win).clamp(0, n)] - c[at.clamp(0, n)]) / win
    return (env.double() - mean).clamp(min=0).float()


def _prior(prior, grid, start_bpm):
    if prior is None:
        return None
    if isinstance(prior, str):
        if prior != "lognormal":
            raise ValueError(f"prior: unknown name {prior!r}: use 'lognormal', an array of one weight per tempo, or None")
        if not start_bpm > 0:
            raise ValueError(f"start_bpm must be positive (got {start_bpm!r})")
        prior = np.exp(-0.5 * np.log2(grid / float(start_bpm)) ** 2)
    p = _sig._to_dev(prior if isinstance(prior, th.Tensor) else np.asarray(prior, dtype=np.float32)).reshape(-1)
    if p.numel() != len(grid) or bool((p < 0).any()) or not bool(th.isfinite(p).all()):
        raise ValueError(f"prior: need {len(grid)} finite non-negative weights, one per tempo")
    return p


def _plp_stages(audio, sr, tempo_min=30, tempo_max=300, tempo_step=1, win=384, prior=None, start_bpm=120, detrend=True, want_tgram=False):
    """Every intermediate of :func:`raw_plp` as device tensors (the link-by-link test reads them)."""
    if not sr > 0:
        raise ValueError(f"sr must be positive (got {sr!r})")
    audio = audio.detach().float().reshape(-1) if isinstance(audio, th.Tensor) else np.ascontiguousarray(audio, dtype=np.float32).reshape(-1)
    fr = float(sr) / _seg.HOP
    grid, table, window, omega = _tables(win, tempo_min, tempo_max, tempo_step, fr)
    onset, _ = _seg.onset_envelope(audio, sr)
    if onset.numel() > PULSE_MAX_FRAMES:
        raise ValueError(f"{onset.numel()} envelope frames, at most {PULSE_MAX_FRAMES}: analyse the clip in parts")
    env = moving_average_detrend(onset, win) if detrend else onset
    p = _prior(prior, grid, start_bpm)
    bins, phase, power, tgram = tempogram_peak(env, table, p, want_tgram)
    curve = pulse_synth(bins, phase, window, omega)
    grid_dev = _sig._const_dev(grid.astype(np.float32))
    bpm = th.where(bins >= 0, grid_dev[bins.clamp(min=0).long()], th.full_like(power, float("nan")))
    return dict(onset=onset, env=env, bin=bins, phase=phase, power=power, tgram=tgram, pulse=curve, tempo=bpm, grid=grid, fr=fr, prior=p,
                window=window, omega=omega, table=table)


def raw_plp(audio, sr, tempo_min=30, tempo_max=300, tempo_step=1, win=384, prior=None, start_bpm=120, detrend=True):
    """Predominant local pulse: ``(pulse [N], tempo [N] in BPM, strength [N])`` as device tensors at sr / 512 frames per second,
    N = 1 + len / 512.  ``pulse`` is in [0, 1], about 1 where the beat is steady, with one maximum per beat; ``tempo`` is the strongest
    tempo of the ``win`` frames (periodic Hann; 384 = 8.9 s at 22050 Hz) around each frame on the grid tempo_min, tempo_min + tempo_step
    ... tempo_max, NaN where the window holds no energy; ``strength`` is that tempo's windowed Fourier power.  The envelope is
    ``segment.onset_envelope`` (what the dynamic-programming tracker sees); ``detrend`` subtracts its moving average over ``win`` frames
    and clamps at 0.  ``prior`` weights the tempi: None, "lognormal" (exp(-log2(tempo / start_bpm)^2 / 2), one octave wide, against
    half- and double-tempo readings) or one non-negative weight per tempo."""
    s = _plp_stages(audio, sr, tempo_min, tempo_max, tempo_step, win, prior, start_bpm, detrend)
    return s["pulse"], s["tempo"], s["power"]


def tempogram(audio, sr, tempo_min=30, tempo_max=300, tempo_step=1, win=384, prior=None, start_bpm=120, detrend=True):
    """``(power [N, B] on the device, grid [B] in BPM as a numpy array)``: the whole Fourier tempogram of which :func:`raw_plp` keeps the
    row maxima — for plots, and for picking tempi by other rules."""
    s = _plp_stages(audio, sr, tempo_min, tempo_max, tempo_step, win, prior, start_bpm, detrend, want_tgram=True)
    return s["tgram"], s["grid"]


# ------------------------------------------------------------------------------------------------ features per video frame
def pulse(audio, sr, n_frames, smooth=0, power=1, device=None):
    """The pulse curve per video frame in [0, 1], a CPU tensor unless ``device=`` is given: :func:`raw_plp` -> linear interpolation to
    ``n_frames`` -> ``** power`` (sharper flashes) -> Gaussian smoothing when ``smooth`` > 0."""
    curve = _sig.lerp_resize(raw_plp(audio, sr)[0], n_frames) ** power
    if smooth > 0:
        curve = _sig.gaussian_filter(curve, smooth)
    return curve.to(device if device is not None else "cpu")


def tempo(audio, sr, n_frames, smooth=0, device=None, method="plp"):
    """The local tempo in BPM per video frame, a CPU tensor unless ``device=`` is given: frames without a tempo hold the last one
    (leading ones take the first) -> 5-tap median -> linear interpolation -> Gaussian smoothing when ``smooth`` > 0.  Zeros, with a
    warning, when no frame has a tempo (silence).  ``method="bar"``: the tempo path of the bar-pointer model instead of the tempogram's
    per-frame maximum, measured bar by bar (``bars.Bars.bar_tempo``: the model's beats are whole frames long, a grid 1 / 21 wide at
    120 BPM, which a bar of them averages out); a clip without one whole bar falls back on the per-beat steps."""
    if method == "bar":
        from . import bars

        res = bars.raw_bars(audio, sr)
        bpm = res.bar_tempo()
        if res.metre > 0 and bool(th.isnan(bpm).all()):
            bpm = res.tempo
    elif method == "plp":
        _, bpm, _ = raw_plp(audio, sr)
    else:
        raise ValueError(f"tempo: unknown method {method!r}: use 'plp' or 'bar'")
    held = _sig.hold_fill(bpm, ~th.isnan(bpm))
    if held is None:
        warnings.warn("tempo: no frame of the clip has a pulse; returning zeros", stacklevel=2)
        out = th.zeros(int(n_frames), dtype=th.float32, device=bpm.device)
    else:
        out = _sig.lerp_resize(_sig._median5(held), n_frames)
        if smooth > 0:
            out = _sig.gaussian_filter(out, smooth)
    return out.to(device if device is not None else "cpu")


def pick_beats(curve, fr, threshold=0.1):
    """Beat times in seconds (float64, on the curve's device): the interior maxima P[m] > P[m-1], P[m] >= P[m+1], P[m] > threshold of a
    pulse curve at ``fr`` frames per second, each moved by the vertex of the parabola through its three samples."""
    p = curve.double()
    if p.numel() < 3:
        return p.new_zeros(0)
    a, b, c = p[:-2], p[1:-1], p[2:]
    at = th.nonzero((b > a) & (b >= c) & (b > threshold)).reshape(-1)
    a, b, c = a[at], b[at], c[at]
    curv = a - 2 * b + c
    delta = th.where(curv < 0, 0.5 * (a - c) / th.where(curv < 0, curv, th.ones_like(curv)), th.zeros_like(curv)).clamp(-0.5, 0.5)
    return (at.double() + 1 + delta) / fr


def beats(audio, sr, method="plp", threshold=0.1):
    """Beat times in seconds, a float64 numpy array.  ``method="plp"``: the maxima above ``threshold`` of the pulse curve of
    :func:`raw_plp`, refined between frames — follows tempo changes.  ``method="dp"``: the frames of ``segment.beat_track`` (one global
    tempo, dynamic programming; what ``laplacian_segmentation`` uses) times 512 / sr.  ``method="bar"``: the beats of the bar-pointer
    model (``bars.raw_bars``), the ones its downbeats are counted on."""
    if method == "plp":
        s = _plp_stages(audio, sr)
        return pick_beats(s["pulse"], s["fr"], threshold).cpu().numpy()
    if method == "dp":
        audio = audio.detach().float().reshape(-1) if isinstance(audio, th.Tensor) else np.ascontiguousarray(audio, dtype=np.float32).reshape(-1)
        env, _ = _seg.onset_envelope(audio, sr)
        _, frames = _seg.beat_track(env, sr)
        return np.asarray(frames, dtype=np.float64) * _seg.HOP / float(sr)
    if method == "bar":
        from . import bars

        return bars.raw_bars(audio, sr).beat_times()
    raise ValueError(f"beats: unknown method {method!r}: use 'plp', 'dp' or 'bar'")


def beat_phase_from_times(times, duration, n_frames, division=1):
    """The position inside the beat per video frame, a float32 CPU tensor in [0, 1): with beat times b_0 < ... < b_{K-1} (seconds), the
    beat count c(tau) is piecewise linear through (b_i, i), extended before b_0 and after b_{K-1} with the first and last interval;
    video frame j sits at tau_j = j duration / n_frames and gets frac(division c(tau_j)).  ``division=2`` gives two cycles per beat,
    ``division=0.25`` one cycle per four beats.  Fewer than two beats: a warning and zeros.  Pure host arithmetic in float64."""
    times = np.asarray(times, dtype=np.float64).reshape(-1)
    n_frames = int(n_frames)
    if len(times) < 2:
        warnings.warn(f"beat_phase: {len(times)} beat(s) found, need two to measure a beat; returning zeros", stacklevel=2)
        return th.zeros(n_frames, dtype=th.float32)
    if not bool(np.all(np.diff(times) > 0)):
        raise ValueError("beat_phase_from_times: the beat times must be strictly increasing")
    tau = np.arange(n_frames, dtype=np.float64) * (float(duration) / n_frames)
    i = np.clip(np.searchsorted(times, tau, side="right") - 1, 0, len(times) - 2)
    x = division * (i + (tau - times[i]) / (times[i + 1] - times[i]))
    return th.from_numpy((x - np.floor(x)).astype(np.float32)).clamp_(max=float(np.nextafter(np.float32(1), np.float32(0))))


def beat_phase(audio, sr, n_frames, division=1, method="plp", device=None):
    """A sawtooth through the beats per video frame: 0 on a beat, rising to 1 at the next (:func:`beat_phase_from_times` of
    :func:`beats`), a float32 CPU tensor unless ``device=`` is given.  ``(1 - beat_phase) ** 4`` is a flash on every beat that decays
    before the next; ``division=0.25`` is a loop position that comes round once per four beats."""
    n = audio.numel() if isinstance(audio, th.Tensor) else np.asarray(audio).size
    out = beat_phase_from_times(beats(audio, sr, method=method), n / float(sr), n_frames, division)
    return out.to(device if device is not None else "cpu")
