"""Bars and metre on the MI355X: the bar-pointer model (Whiteley, Cemgil & Godsill, "Bayesian modelling of temporal structure in
musical audio", ISMIR 2006) on the state space of Krebs, Boeck & Widmer ("An efficient state-space model for joint tempo and meter
tracking", ISMIR 2015).  No counterpart in the reference; parity with madmom's DBN trackers is not claimed, the definition is
include/maua_hip.h ("Bar-pointer model") and tests/bar_ref.py.

A hidden Markov model over (tempo, beat in the bar, position in the beat) is decoded jointly, once per candidate bar length: the path
gives the tempo, the beats and the downbeats, the best-scoring model the metre.  Pipeline: the onset envelope of segment.py, scaled to
a beat activation -> a downbeat activation from the low-frequency flux of the same spectrogram (or the caller's own ``accent``) ->
three log-likelihoods per frame (no beat, beat, downbeat) -> maua_bar_viterbi_f64, one workgroup per bar length -> per-frame tempo,
beat number and bar phase.  Activations and the mapping to video frames are a handful of torch / numpy operations on O(frames)
values.
"""
import math
import warnings

import numpy as np
import torch as th

from .. import _lib
from . import segment as _seg
from . import signal as _sig

__all__ = ["bar_model", "bar_observations", "bar_viterbi", "raw_bars", "downbeats", "metre", "bar_phase", "bar_beats", "Bars",
           "BAR_MAX_TEMPI", "BAR_MAX_BEATS", "BAR_MAX_INTERVAL", "BAR_MAX_MODELS"]

BAR_MAX_FRAMES = 1 << 22  # MAUA_BAR_MAX_* (include/maua_hip.h)
BAR_MAX_TEMPI = 128
BAR_MAX_BEATS = 8
BAR_MAX_INTERVAL = 1024
BAR_MAX_MODELS = 8
BAR_MAX_LANES = 1024

# Frames by which the onset envelope trails the sound.  segment.onset_envelope puts the rise from STFT frame m to m + 1 at index
# m + 3 (librosa's centring: the first difference plus half a window of 2048 at a hop of 512), and a sharp attack raises the dB
# spectrum as soon as the window of a frame reaches it, before the frame centred on it.  Measured on noise bursts at known times the
# decoded beat frame trails the burst by 0.3 .. 1.7 frames, 0.95 on average: one frame is taken off every time.
ENVELOPE_LAG = 1.0
ACTIVATION_PERCENTILE = 90.0
KICK_HZ = 200.0
KICK_RANGE_DB = 40.0    # the low bands are floored this far below their maximum: from an 80 dB floor ANY onset is a large rise in dB


# ------------------------------------------------------------------------------------------------ the model (host)
def bar_model(fr, tempo_min=55, tempo_max=215, transition_lambda=40, observation_lambda=16):
    """``(interval int32 [K], width int32 [K], log_change float64 [K, K])`` of the bar-pointer model at ``fr`` envelope frames per
    second: one tempo per whole beat interval from ceil(60 fr / tempo_max) to floor(60 fr / tempo_min) frames; a beat is observed
    during the first ``width = max(1, interval // observation_lambda)`` frames of its interval; the tempo may change at a beat, from
    interval i' to i with probability proportional to exp(-transition_lambda |i / i' - 1|), normalised over i.  40 is madmom's 100
    at 100 frames per second scaled to 43 frames per second, where whole-frame intervals are coarse: a tempo between two of them has
    to alternate, which a stiffer model refuses in favour of half the tempo."""
    if not (fr > 0 and tempo_min > 0 and tempo_max >= tempo_min):
        raise ValueError(f"bar_model: need fr > 0 and 0 < tempo_min <= tempo_max (got {fr}, {tempo_min}, {tempo_max})")
    if not (transition_lambda >= 0 and observation_lambda > 1):
        raise ValueError(f"bar_model: need transition_lambda >= 0 and observation_lambda > 1 (got {transition_lambda}, {observation_lambda})")
    lo, hi = max(1, math.ceil(60.0 * fr / tempo_max)), math.floor(60.0 * fr / tempo_min)
    if hi < lo:
        raise ValueError(f"bar_model: no whole beat interval between {tempo_min} and {tempo_max} BPM at {fr:.3f} frames per second")
    interval = np.arange(lo, hi + 1, dtype=np.int32)
    width = np.maximum(1, interval // int(observation_lambda)).astype(np.int32)
    ratio = interval[None, :].astype(np.float64) / interval[:, None].astype(np.float64)
    p = np.exp(-float(transition_lambda) * np.abs(ratio - 1.0))
    with np.errstate(divide="ignore"):
        log_change = np.log(p / p.sum(1, keepdims=True))
    return interval, width, log_change


def bar_observations(beat_act, down_act, observation_lambda=16):
    """The log-likelihoods [N, 3] float32 (no beat, beat, downbeat) on the device of a beat activation ``a`` and a downbeat
    activation ``d`` per frame (tensors or arrays): with a clipped to [1e-3, 1 - 1e-3] and d to [0.05, 0.95],
    log((1 - a) / (observation_lambda - 1)), log(a (1 - d)), log(a d).  Computed in float64, rounded once."""
    a = _sig._to_dev(beat_act, th.float64).reshape(-1).clamp(1e-3, 1 - 1e-3)
    d = _sig._to_dev(down_act, th.float64).reshape(-1).clamp(0.05, 0.95)
    if a.numel() != d.numel():
        raise ValueError(f"bar_observations: {a.numel()} beat activations for {d.numel()} downbeat activations")
    return th.stack([((1 - a) / (observation_lambda - 1)).log(), (a * (1 - d)).log(), (a * d).log()], 1).float().contiguous()


def _check_model(interval, width, log_change, beats_per_bar, n_frames):
    interval = np.ascontiguousarray(np.asarray(interval).reshape(-1), dtype=np.int32)
    width = np.ascontiguousarray(np.asarray(width).reshape(-1), dtype=np.int32)
    beats = np.ascontiguousarray(np.asarray(beats_per_bar).reshape(-1), dtype=np.int32)
    K = len(interval)
    if not 1 <= n_frames <= BAR_MAX_FRAMES:
        raise ValueError(f"bar_viterbi: {n_frames} frames, need 1 .. {BAR_MAX_FRAMES}: analyse the clip in parts")
    if not 1 <= K <= BAR_MAX_TEMPI:
        raise ValueError(f"bar_viterbi: {K} tempi, need 1 .. {BAR_MAX_TEMPI}: raise tempo_min or lower tempo_max")
    if len(width) != K or tuple(np.shape(log_change)) != (K, K):
        raise ValueError(f"bar_viterbi: {K} intervals need {K} widths and a [{K}, {K}] matrix (got {len(width)} and {tuple(np.shape(log_change))})")
    if interval[0] < 1 or interval[-1] > BAR_MAX_INTERVAL or bool(np.any(np.diff(interval) <= 0)):
        raise ValueError(f"bar_viterbi: the intervals must be strictly ascending in 1 .. {BAR_MAX_INTERVAL} frames: raise tempo_min")
    if bool(np.any(width < 1)) or bool(np.any(width > interval)):
        raise ValueError("bar_viterbi: every width must lie in 1 .. its interval")
    if not 1 <= len(beats) <= BAR_MAX_MODELS or beats.min() < 1 or beats.max() > BAR_MAX_BEATS:
        raise ValueError(f"bar_viterbi: need 1 .. {BAR_MAX_MODELS} metres of 1 .. {BAR_MAX_BEATS} beats per bar (got {beats.tolist()})")
    if K * int(beats.max()) > BAR_MAX_LANES or _lib.load().maua_bar_lds_bytes(K, int(beats.max()), int(interval[-1])) == 0:
        raise ValueError(f"bar_viterbi: {K} tempi x {int(beats.max())} beats x {int(interval[-1])} frames do not fit one compute unit: "
                         "raise tempo_min (shorter intervals, fewer tempi), lower tempo_max, or decode fewer beats per bar")
    return interval, width, beats


def bar_viterbi(logobs, interval, width, log_change, beats_per_bar=(3, 4)):
    """The most probable path of the bar-pointer model, once per bar length: ``(score float64 [n_models], path int32 [n_models, N, 3])``
    on the device, ``path[m, t] = (tempo index, beat in the bar, frame in the beat)``, beat 0 the downbeat.  ``logobs`` [N, 3] as
    :func:`bar_observations` makes them, the model as :func:`bar_model` does.  Scores of different bar lengths are comparable: every
    model explains every frame.  maua_bar_viterbi_f64: a ValueError where the entry would refuse."""
    shape = tuple(getattr(logobs, "shape", ()))
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"bar_viterbi: logobs must be [N, 3] (got {shape})")
    n_frames = int(shape[0])
    interval, width, beats = _check_model(interval, width, log_change, beats_per_bar, n_frames)
    logobs = _sig._to_dev(logobs)
    dev = logobs.device
    K, n_models = len(interval), len(beats)
    lc = _sig._const_dev(np.asarray(log_change.cpu() if isinstance(log_change, th.Tensor) else log_change, dtype=np.float64))
    ws = th.empty(_lib.load().maua_bar_ws_bytes(n_frames, K, int(beats.max()), n_models), dtype=th.uint8, device=dev)
    score = th.empty(n_models, dtype=th.float64, device=dev)
    path = th.empty((n_models, n_frames, 3), dtype=th.int32, device=dev)
    _lib.call("maua_bar_viterbi_f64", logobs, n_frames, interval, width, lc, K, beats, n_models, ws, score, path)
    return score, path


# ------------------------------------------------------------------------------------------------ activations
def _spread(x):
    """max over the frames t - 1, t, t + 1."""
    pad = th.cat([x[:1], x, x[-1:]])
    return th.maximum(th.maximum(pad[:-2], pad[1:-1]), pad[2:])


def _percentile(x, p):
    return _sig.percentile(x, p) if x.numel() else 0.0


def kick_flux(power, sr):
    """The positive dB flux of the mel bands centred below 200 Hz (the kick drum's range, 40 dB of it), summed, on the onset envelope's time axis:
    the cue for the accent when the caller gives none.  ``power`` is the |STFT|^2 that segment.onset_envelope returns."""
    fb = _sig.mel_filterbank(sr, _seg.N_FFT, 128)
    edges = _sig._mel_to_hz(np.linspace(_sig._hz_to_mel(0.0), _sig._hz_to_mel(sr / 2.0), 130))
    low = fb[edges[1:-1] < KICK_HZ]
    if len(low) == 0:
        low = fb[:1]
    db = _sig.project(np.ascontiguousarray(low), power, to_db=True)
    db = th.maximum(db, db.max() - KICK_RANGE_DB)
    flux = th.clamp(db[:, 1:] - db[:, :-1], min=0).sum(0)
    pad = 1 + _seg.N_FFT // (2 * _seg.HOP)
    return th.cat([th.zeros(pad, device=flux.device), flux])[: db.shape[1]].contiguous()


def _activations(onset, cue):
    """(beat_act, down_act) in [0, 1] of the onset envelope and an accent cue per frame, None for a clip without onsets.  beat_act: the
    envelope over the 90th percentile of its non-zero frames.  down_act: the cue's maximum over +-1 frame (its peak and the
    envelope's can land a frame apart), over its own 90th percentile among the frames with beat_act > 0.1, mapped affinely into
    [0.05, 0.95]."""
    nonzero = onset[onset > 0]
    if nonzero.numel() == 0:
        return None
    top = _percentile(nonzero, ACTIVATION_PERCENTILE)
    beat_act = (onset / top).clamp(0, 1)
    cue = _spread(cue.to(onset.device).float().reshape(-1))
    on_beats = cue[beat_act > 0.1]
    scale = _percentile(on_beats, ACTIVATION_PERCENTILE) if on_beats.numel() else 0.0
    down_act = 0.05 + 0.9 * (cue / scale).clamp(0, 1) if scale > 0 else th.full_like(cue, 0.5)
    return beat_act, down_act


class Bars:
    """What :func:`raw_bars` found: ``metre`` (beats per bar of the best model), ``scores`` (log-probability per candidate, a numpy
    array in the order of ``beats_per_bar``), and per envelope frame on the device ``tempo`` (BPM, float32), ``beat`` (int32, 0 = the
    downbeat) and ``phase`` (position in the bar in [0, 1), float32), at ``fr`` frames per second.  ``beat_times()`` and
    ``downbeat_times()`` are float64 numpy arrays in seconds."""

    def __init__(self, metre, scores, beats_per_bar, tempo, beat, phase, starts, fr):
        self.metre, self.scores, self.beats_per_bar, self.tempo, self.beat, self.phase, self.starts, self.fr = (
            metre, scores, beats_per_bar, tempo, beat, phase, starts, fr)

    def frame_to_time(self, frames):
        return (np.asarray(frames, dtype=np.float64) - ENVELOPE_LAG) / self.fr

    def beat_times(self):
        t = self.frame_to_time(th.nonzero(self.starts).reshape(-1).cpu().numpy())
        return t[t >= 0]

    def bar_tempo(self):
        """BPM per envelope frame measured over the bar the frame is in — ``metre`` beats in the frames from its downbeat to the next —
        on the device, NaN in the bars that the ends of the clip cut.  ``tempo`` itself moves in steps of whole frames per beat (123.0
        or 117.4 BPM for 120 at 43 frames per second, and a path through 120 alternates between them); over a bar the steps average out."""
        nan = th.full_like(self.tempo, float("nan"))
        if self.metre == 0:
            return nan
        bar = th.cumsum((self.starts & (self.beat == 0)).long(), 0)   # 0 before the first downbeat
        n_bars = int(bar[-1])
        length = th.bincount(bar, minlength=n_bars + 1).float()
        return th.where((bar >= 1) & (bar < n_bars), 60.0 * self.fr * self.metre / length[bar], nan)

    def downbeat_times(self):
        t = self.frame_to_time(th.nonzero(self.starts & (self.beat == 0)).reshape(-1).cpu().numpy())
        return t[t >= 0]


def _bar_stages(audio, sr, beats_per_bar=(3, 4), tempo_min=55, tempo_max=215, transition_lambda=40, observation_lambda=16, accent=None):
    """Every intermediate of :func:`raw_bars` as device tensors (the link-by-link test reads them); ``result`` is the Bars object."""
    if not sr > 0:
        raise ValueError(f"sr must be positive (got {sr!r})")
    audio = audio.detach().float().reshape(-1) if isinstance(audio, th.Tensor) else np.ascontiguousarray(audio, dtype=np.float32).reshape(-1)
    fr = float(sr) / _seg.HOP
    interval, width, log_change = bar_model(fr, tempo_min, tempo_max, transition_lambda, observation_lambda)
    beats = np.asarray(beats_per_bar, dtype=np.int32).reshape(-1)
    onset, power = _seg.onset_envelope(audio, sr)
    n = onset.numel()
    _check_model(interval, width, log_change, beats, n)
    if accent is None:
        cue = kick_flux(power, sr)
    else:
        cue = _sig._to_dev(accent if isinstance(accent, th.Tensor) else np.asarray(accent, dtype=np.float32)).reshape(-1)
        if cue.numel() != n:
            raise ValueError(f"accent: {cue.numel()} values for {n} envelope frames (sr / 512 per second)")
    acts = _activations(onset, cue)
    out = dict(onset=onset, cue=cue, interval=interval, width=width, log_change=log_change, fr=fr, beats_per_bar=beats)
    if acts is None:
        warnings.warn("raw_bars: the clip has no onsets; returning zeros", stacklevel=3)
        zero = th.zeros(n, dtype=th.float32, device=onset.device)
        out["result"] = Bars(0, np.zeros(len(beats)), beats, zero, zero.int(), zero.clone(), zero.bool(), fr)
        return out
    beat_act, down_act = acts
    logobs = bar_observations(beat_act, down_act, observation_lambda)
    score, path = bar_viterbi(logobs, interval, width, log_change, beats)
    scores = score.cpu().numpy()
    best = int(np.argmax(scores))  # (the first maximum: the earlier candidate on a tie)
    B = int(beats[best])
    k, b, j = path[best, :, 0].long(), path[best, :, 1], path[best, :, 2]
    iv = _sig._const_dev(interval.astype(np.float32))[k]
    tempo = 60.0 * fr / iv
    phase = ((b.float() + j.float() / iv) / B).clamp(max=float(np.nextafter(np.float32(1), np.float32(0))))
    out.update(beat_act=beat_act, down_act=down_act, logobs=logobs, score=score, path=path,
               result=Bars(B, scores, beats, tempo, b.contiguous(), phase, j == 0, fr))
    return out


def raw_bars(audio, sr, beats_per_bar=(3, 4), tempo_min=55, tempo_max=215, transition_lambda=40, observation_lambda=16, accent=None):
    """Tempo, beats, downbeats and metre in one pass: a :class:`Bars`.  The bar-pointer model of :func:`bar_model` is decoded once per
    entry of ``beats_per_bar`` and the best-scoring one kept.  The beat activation is ``segment.onset_envelope`` over a high percentile
    of its non-zero frames; the downbeat activation comes from ``accent`` — the caller's own salience per envelope frame (sr / 512 per
    second), say ``ar.onsets(fmax=150)`` resampled — or, when None, from the positive dB flux of the mel bands below 200 Hz.  One metre
    per clip; a clip without onsets warns and returns zeros (metre 0)."""
    return _bar_stages(audio, sr, beats_per_bar, tempo_min, tempo_max, transition_lambda, observation_lambda, accent)["result"]


# ------------------------------------------------------------------------------------------------ features per video frame
def _duration(audio, sr):
    return (audio.numel() if isinstance(audio, th.Tensor) else np.asarray(audio).size) / float(sr)


def downbeats(audio, sr, **raw):
    """Downbeat times in seconds, a float64 numpy array (``**raw`` goes to :func:`raw_bars`)."""
    return raw_bars(audio, sr, **raw).downbeat_times()


def metre(audio, sr, **raw):
    """Beats per bar, an int: the best-scoring candidate of ``beats_per_bar`` (0 for a clip without onsets)."""
    return int(raw_bars(audio, sr, **raw).metre)


def bar_phase(audio, sr, n_frames, division=1, device=None, **raw):
    """A sawtooth through the downbeats per video frame: 0 on a downbeat, rising to 1 at the next
    (:func:`beat_phase_from_times` of :func:`downbeats`), a float32 CPU tensor unless ``device=`` is given.  As a loop position it
    closes on the downbeat in any metre; ``division=0.5`` comes round once per two bars."""
    from .beat import beat_phase_from_times

    out = beat_phase_from_times(downbeats(audio, sr, **raw), _duration(audio, sr), n_frames, division)
    return out.to(device if device is not None else "cpu")


def bar_beats(audio, sr, n_frames, smooth=0, device=None, **raw):
    """Which beat of the bar every video frame is in: ``[n_frames, metre]`` float32 rows, one-hot, Gaussian-smoothed along time when
    ``smooth`` > 0; a CPU tensor unless ``device=`` is given.  ``ar.chroma_weight_latents(rows, selection[:metre])`` gives every beat
    of the bar its own latent.  A clip without onsets: ``[n_frames, 1]`` zeros."""
    res = raw_bars(audio, sr, **raw)
    n_frames = int(n_frames)
    if res.metre == 0:
        return th.zeros((n_frames, 1), dtype=th.float32, device=device if device is not None else "cpu")
    tau = th.arange(n_frames, dtype=th.float64, device=res.beat.device) * (_duration(audio, sr) / n_frames)
    at = (tau * res.fr + ENVELOPE_LAG).round().long().clamp(0, res.beat.numel() - 1)
    rows = th.nn.functional.one_hot(res.beat[at].long(), res.metre).float()
    if smooth > 0:
        rows = _sig.gaussian_filter(rows, smooth)
    return rows.to(device if device is not None else "cpu")
