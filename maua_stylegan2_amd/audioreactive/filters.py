"""Recursive (IIR) filters and band envelopes on the MI355X — no counterpart in the reference, which filters on the host.

  * :func:`sosfilt` / :func:`sosfiltfilt`: ``scipy.signal.sosfilt`` / ``sosfiltfilt`` for one filter or a bank of them in one call, on
    the device (``maua_sosfilt_f64``, csrc/iir.hip: float64 transposed direct form II, time cut into chunks and stitched by an exact
    carry; the arithmetic is defined in include/maua_hip.h and restated in tests/iir_ref.py).
  * :func:`butter_sos`, :func:`bandpass`, :func:`band_edges`: the designs in front of it (scipy on the host: a few numbers).
  * :func:`envelope`: attack / release follower over per-frame features (``maua_env_follow_f32``).
  * :func:`bands`: "bass / mids / highs" levels per video frame: one filter-bank call, RMS per hop, resampling, the follower.

Audio stays on the device: inputs may be numpy arrays or tensors anywhere; the filters return tensors on the current HIP device unless
``device=`` says otherwise, :func:`bands` a CPU tensor like the other envelopes.
"""
import math

import numpy as np
import scipy.signal
import torch as th

from .. import _lib
from . import signal as _sig

__all__ = ["sosfilt", "sosfiltfilt", "butter_sos", "bandpass", "band_edges", "envelope", "envelope_coefficient", "bands", "bank_sos",
           "filtfilt_pad", "default_chunk", "hop_rms"]

MAX_SECTIONS, MAX_FILTERS, MAX_CHUNK = 16, 64, 65536  # MAUA_SOS_MAX_* (include/maua_hip.h)
BANDS_HOP = 512


def default_chunk(n):
    """The chunk length ``maua_sosfilt_f64`` uses for ``n`` samples when none is given (``maua_sosfilt_default_chunk``)."""
    return int(_lib.load().maua_sosfilt_default_chunk(int(n)))


def _as_sos(sos):
    """[n_sections, 6] or [F, n_sections, 6] -> (float64 [F, n_sections, 6] normalised to a0 = 1, was a single filter)."""
    if isinstance(sos, th.Tensor):
        sos = sos.detach().cpu().numpy()
    sos = np.array(sos, dtype=np.float64)
    single = sos.ndim == 2
    if single:
        sos = sos[None]
    if sos.ndim != 3 or sos.shape[2] != 6:
        raise ValueError(f"sosfilt: sos must be [n_sections, 6] or [F, n_sections, 6] (got {list(sos.shape)})")
    if not 1 <= sos.shape[1] <= MAX_SECTIONS or not 1 <= sos.shape[0] <= MAX_FILTERS:
        raise ValueError(f"sosfilt: 1 .. {MAX_SECTIONS} sections and 1 .. {MAX_FILTERS} filters per call (got {sos.shape[1]} and {sos.shape[0]})")
    if not np.all(np.isfinite(sos)) or np.any(sos[:, :, 3] == 0):
        raise ValueError("sosfilt: sos must be finite with a0 != 0")
    return np.ascontiguousarray(sos / sos[:, :, 3:4]), single


def _signal_on_device(x):
    """numpy / tensor -> contiguous device tensor, float64 kept, everything else float32."""
    if isinstance(x, np.ndarray):
        wide = x.dtype == np.float64
    else:
        x = th.as_tensor(x)
        wide = x.dtype == th.float64
    return _sig._to_dev(x, th.float64 if wide else th.float32)


def _run(sos, x, zi, chunk, want64, want32, want_zf):
    """One ``maua_sosfilt_f64`` call.  sos float64 [F, ns, 6] (host, normalised); x a device tensor [n] (shared) or [F, n]; zi None or a
    device float64 [F, ns, 2].  -> (y64 or None, y32 or None, zf or None), each [F, n]."""
    lib = _lib.load()
    F, ns = sos.shape[:2]
    shared = x.dim() == 1
    n = x.shape[-1]
    if not shared and x.shape[0] != F:
        raise ValueError(f"sosfilt: {F} filters need one signal or {F} of them (got {x.shape[0]})")
    chunk = 0 if chunk is None else int(chunk)
    if not 0 <= chunk <= MAX_CHUNK:
        raise ValueError(f"sosfilt: chunk must be 1 .. {MAX_CHUNK} samples (got {chunk})")
    dev = x.device
    if n == 0:  # (an empty tensor has no address to pass: nothing to filter, the state stays)
        zf = (th.zeros((F, ns, 2), dtype=th.float64, device=dev) if zi is None else zi.clone()) if want_zf else None
        return (x.new_empty((F, 0), dtype=th.float64) if want64 else None, x.new_empty((F, 0), dtype=th.float32) if want32 else None, zf)
    sos_d = _sig._const_dev(sos, np.float64)
    ws = th.empty(max(int(lib.maua_sosfilt_ws_doubles(F, ns, n, chunk)), 1), dtype=th.float64, device=dev)
    y64 = th.empty((F, n), dtype=th.float64, device=dev) if want64 else None
    y32 = th.empty((F, n), dtype=th.float32, device=dev) if want32 else None
    zf = th.empty((F, ns, 2), dtype=th.float64, device=dev) if want_zf else None
    is64 = x.dtype == th.float64
    _lib.call("maua_sosfilt_f64", sos_d, F, ns, None if is64 else x, x if is64 else None, 1 if shared else F, n, chunk, zi, y64, y32, zf, ws)
    return y64, y32, zf


def _shape_in(sos, x):
    sos, single = _as_sos(sos)
    x = _signal_on_device(x)
    if x.dim() not in (1, 2):
        raise ValueError(f"sosfilt: x must be [n] or [F, n] (got {list(x.shape)})")
    squeeze = single and x.dim() == 1
    if single and x.dim() == 2:  # one filter over several signals: the same sections for every row
        if x.shape[0] > MAX_FILTERS:
            raise ValueError(f"sosfilt: at most {MAX_FILTERS} signals per call (got {x.shape[0]})")
        sos = np.ascontiguousarray(np.broadcast_to(sos, (x.shape[0],) + sos.shape[1:]))
    return sos, x, squeeze


def _out_dtype(dtype):
    if dtype not in (th.float32, th.float64):
        raise ValueError(f"sosfilt: dtype must be torch.float32 or torch.float64 (got {dtype})")
    return dtype == th.float64


def sosfilt(sos, x, zi=None, chunk=None, dtype=th.float32, device=None):
    """``scipy.signal.sosfilt(sos, x)`` along the last axis on the device.  ``sos`` [n_sections, 6] (one filter) or [F, n_sections, 6]
    (a bank); ``x`` [n] or [F, n]: a bank over one signal returns [F, n], one filter over [F, n] filters every row.  Computed in
    float64 whatever the input; ``dtype`` is the type of the result (float32: each sample rounded once from the double).  With ``zi``
    ([n_sections, 2] or [F, n_sections, 2], scipy's layout) the result is ``(y, zf)`` as in scipy, zf float64.  ``chunk`` overrides the
    chunk length of the parallel scan (last bits only).  The result stays on the HIP device unless ``device=`` is given."""
    sos, x, squeeze = _shape_in(sos, x)
    F, ns = sos.shape[:2]
    want64 = _out_dtype(dtype)
    zi_d = None
    if zi is not None:
        if tuple(zi.shape) not in ((ns, 2), (F, ns, 2)):
            raise ValueError(f"sosfilt: zi must be [{ns}, 2] or [{F}, {ns}, 2] (got {list(zi.shape)})")
        zi_d = _sig._to_dev(zi, th.float64)
        if zi_d.dim() == 2:
            zi_d = zi_d[None].expand(F, ns, 2).contiguous()
    y64, y32, zf = _run(sos, x, zi_d, chunk, want64, not want64, zi is not None)
    y = y64 if want64 else y32
    if squeeze:
        y, zf = y[0], (zf[0] if zf is not None else None)
    if device is not None:
        y, zf = y.to(device), (zf.to(device) if zf is not None else None)
    return (y, zf) if zi is not None else y


def filtfilt_pad(sos):
    """Samples of odd extension ``scipy.signal.sosfiltfilt`` puts at either end by default: 3 (2 n_sections + 1 - min(number of
    sections with b2 == 0, number with a2 == 0))."""
    sos = np.asarray(sos, dtype=np.float64).reshape(-1, 6)
    ntaps = 2 * sos.shape[0] + 1
    ntaps -= min(int((sos[:, 2] == 0).sum()), int((sos[:, 5] == 0).sum()))
    return 3 * ntaps


def _odd_ext(x, edge):
    """scipy's odd extension along the last axis with torch ops: 2 x[0] - x[edge .. 1], x, 2 x[-1] - x[-2 .. -edge-1]."""
    left = 2 * x[..., :1] - x[..., 1:edge + 1].flip(-1)
    right = 2 * x[..., -1:] - x[..., -edge - 1:-1].flip(-1)
    return th.cat([left, x, right], dim=-1)


def sosfiltfilt(sos, x, chunk=None, dtype=th.float32, device=None):
    """``scipy.signal.sosfiltfilt(sos, x)`` (zero phase, default odd padding) on the device: odd extension by :func:`filtfilt_pad`
    samples, forward from the steady state of the first sample (``scipy.signal.sosfilt_zi``, computed on the host, times the edge
    sample), flip, forward again, flip, unpad.  Everything between the two passes is float64.  Shapes as in :func:`sosfilt`."""
    sos, x, squeeze = _shape_in(sos, x)
    F = sos.shape[0]
    want64 = _out_dtype(dtype)
    edge = max(filtfilt_pad(s) for s in sos)
    if any(filtfilt_pad(s) != edge for s in sos):
        raise ValueError("sosfiltfilt: the filters of one bank must share scipy's padding length (same count of first-order sections)")
    n = x.shape[-1]
    if n <= edge:
        raise ValueError(f"sosfiltfilt: the signal must be longer than the padding, {edge} samples (got {n})")
    zi_unit = _sig._const_dev(np.stack([scipy.signal.sosfilt_zi(s) for s in sos]), np.float64)  # [F, ns, 2]
    ext = _odd_ext(x.to(th.float64), edge)
    if ext.dim() == 1:
        first = ext[:1].reshape(1, 1, 1)
    else:
        first = ext[:, :1, None]
    y, _, _ = _run(sos, ext.contiguous(), (zi_unit * first).contiguous(), chunk, True, False, False)
    y = y.flip(-1).contiguous()
    y, _, _ = _run(sos, y, (zi_unit * y[:, :1, None]).contiguous(), chunk, True, False, False)
    y = y.flip(-1)[:, edge:-edge]
    y = (y if want64 else y.to(th.float32)).contiguous()
    if squeeze:
        y = y[0]
    return y if device is None else y.to(device)


def butter_sos(order, band, btype, sr):
    """``scipy.signal.butter(order, band, btype, fs=sr, output="sos")``: float64 [n_sections, 6]."""
    return scipy.signal.butter(order, band, btype, fs=sr, output="sos")


def bandpass(audio, sr, fmin, fmax, order=12, zero_phase=False, dtype=th.float32, device=None):
    """``audio`` through the Butterworth band-pass [fmin, fmax] Hz of :func:`rms` (``order`` sections), on the device;
    ``zero_phase`` runs it forwards and backwards (:func:`sosfiltfilt`)."""
    sos = butter_sos(order, [fmin, fmax], "bp", sr)
    return (sosfiltfilt if zero_phase else sosfilt)(sos, audio, dtype=dtype, device=device)


def band_edges(n_bands, fmin=20, fmax=8000, scale="log"):
    """``n_bands + 1`` edges from fmin to fmax in Hz, equal steps in log frequency (``"log"``) or on the mel scale (``"mel"``)."""
    n_bands = int(n_bands)
    if n_bands < 1 or not 0 < fmin < fmax:
        raise ValueError(f"band_edges: n_bands >= 1 and 0 < fmin < fmax (got {n_bands}, {fmin}, {fmax})")
    if scale == "log":
        edges = np.geomspace(float(fmin), float(fmax), n_bands + 1)
    elif scale == "mel":
        edges = _sig._mel_to_hz(np.linspace(_sig._hz_to_mel(fmin), _sig._hz_to_mel(fmax), n_bands + 1))
    else:
        raise ValueError(f"band_edges: unknown scale {scale!r} (expected 'log' or 'mel')")
    edges[0], edges[-1] = float(fmin), float(fmax)
    return tuple(float(e) for e in edges)


def bank_sos(edges, sr, order=6):
    """The Butterworth bank between consecutive ``edges``: float64 [len(edges) - 1, n_sections, 6].  An edge of None at either end
    makes that band a low-pass / high-pass.  A low- or high-pass of ``order`` has half the sections of a band-pass; it is filled up
    with identity sections [1 0 0 1 0 0] (y = x), so that the bank is one call."""
    edges = list(edges)
    if len(edges) < 2:
        raise ValueError("bank_sos: at least two edges")
    if any(e is None for e in edges[1:-1]):
        raise ValueError("bank_sos: only the first and the last edge may be None")
    filters = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        if lo is None and hi is None:
            raise ValueError("bank_sos: a band needs at least one edge")
        if lo is None:
            filters.append(butter_sos(order, hi, "lp", sr))
        elif hi is None:
            filters.append(butter_sos(order, lo, "hp", sr))
        else:
            filters.append(butter_sos(order, [lo, hi], "bp", sr))
    ns = max(f.shape[0] for f in filters)
    identity = np.array([1.0, 0, 0, 1, 0, 0])
    return np.stack([np.concatenate([f, np.tile(identity, (ns - f.shape[0], 1))]) for f in filters])


def envelope_coefficient(tau):
    """Smoothing coefficient of a time constant of ``tau`` video frames (scaled by SMF like a Gaussian's radius): 1 - exp(-1 / (tau
    SMF)); tau <= 0 is instantaneous (1)."""
    tau = float(tau) * _sig.SMF
    if not tau > 0:
        return 1.0
    return float(-math.expm1(-1.0 / tau))


def envelope(x, attack, release, y0=None):
    """Attack / release follower along time (dim 0) of ``x`` [n_frames] or [n_frames, C] on the device (``maua_env_follow_f32``):
    y[t] = y[t-1] + k (x[t] - y[t-1]) with k = :func:`envelope_coefficient` of ``attack`` where x[t] > y[t-1], of ``release`` elsewhere.
    It starts from x[0] (``y0`` [C]: from there).  float32, returned on the device ``x`` came from."""
    src_device = x.device if isinstance(x, th.Tensor) else th.device("cpu")
    xd = _sig._to_dev(x)
    if xd.dim() not in (1, 2):
        raise ValueError(f"envelope: x must be [n_frames] or [n_frames, C] (got {list(xd.shape)})")
    t = xd.shape[0]
    c = xd.shape[1] if xd.dim() == 2 else 1
    y0d = None
    if y0 is not None:
        y0d = _sig._to_dev(th.as_tensor(y0).reshape(-1))
        if y0d.numel() != c:
            raise ValueError(f"envelope: y0 must have {c} entries (got {y0d.numel()})")
    y = th.empty_like(xd)
    if t and c:
        _lib.call("maua_env_follow_f32", xd, y0d, y, t, c, envelope_coefficient(attack), envelope_coefficient(release))
    return y.to(src_device)


def hop_rms(y, hop=BANDS_HOP):
    """Root mean square of every full ``hop`` samples of y [F, n] -> [n // hop, F] (torch ops; a signal shorter than a hop is one frame)."""
    n = y.shape[-1]
    if n < hop:
        return y.pow(2).mean(-1).sqrt()[None]
    frames = n // hop
    return y[:, : frames * hop].reshape(y.shape[0], frames, hop).pow(2).mean(-1).sqrt().t().contiguous()


def _clip_columns(x, clip):
    """:func:`percentile_clip` per column; a column without a strict local maximum (silence, a ramp) is scaled by its maximum alone."""
    cols = []
    for col in x.unbind(1):
        middle = col[1:-1]
        if bool(((middle > col[2:]) & (middle > col[:-2])).any()):
            cols.append(_sig.percentile_clip(col, clip))
        else:
            top = col.clamp(min=0).max()
            cols.append(col.clamp(min=0) / top if float(top) > 0 else th.zeros_like(col))
    return th.stack(cols, 1)


def bands(audio, sr, n_frames, edges=(20, 150, 600, 2500, 8000), order=6, attack=0, release=8, smooth=0, clip=100, power=1, device=None):
    """Level of every frequency band per video frame, [n_frames, n_bands] in [0, 1] — "bass / mids / highs" with a fast attack and a slow
    release.  :func:`bank_sos` between consecutive ``edges`` over the shared signal in one call -> RMS per 512-sample hop -> Fourier
    resampling to ``n_frames`` (held inside the range of each band) -> :func:`envelope` (``attack``, ``release`` in video frames) ->
    optional Gaussian ``smooth`` -> ``percentile_clip`` per column -> ``** power``.  A CPU tensor unless ``device=`` is given."""
    y = sosfilt(bank_sos(edges, sr, order), _sig._to_dev(audio).reshape(-1))
    level = hop_rms(y)
    env = _sig.resample(level, n_frames)
    env = th.minimum(th.maximum(env, level.min(0).values.double()), level.max(0).values.double()).float()
    env = envelope(env, attack, release)
    if smooth:
        env = _sig.gaussian_filter(env, smooth)
        env = env.reshape(int(n_frames), -1)
    env = _clip_columns(env, clip) ** power
    return env.to(device if device is not None else "cpu")
