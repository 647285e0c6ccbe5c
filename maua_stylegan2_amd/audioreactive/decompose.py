"""Spectrogram factorisation: which SOURCE plays when.  No counterpart in the reference.

Non-negative matrix factorisation of a magnitude spectrogram, V [F, T] ~ W [F, K] . H [K, T], under the generalised Kullback-Leibler
divergence by multiplicative updates (Lee & Seung 2000): W holds K spectral templates, H their activations over time.  The updates run
on the device as two fused HIP kernels (csrc/nmf.hip behind maua_nmf_kl_f32) that never store W.H or V / (W.H); there is no torch
formulation to fall back to.

  * :func:`nmf`         the factorisation of any non-negative matrix
  * :func:`decompose`   templates and activations of a clip's mel or STFT magnitude spectrogram
  * :func:`components`  one envelope in [0, 1] per component and video frame, post-processed like :func:`signal.onsets`; feeds
                        ``ar.chroma_weight_latents`` unchanged
  * :func:`separate`    the SOUND of every source: soft masks from the factorisation on the complex STFT (csrc/separate.hip behind
                        maua_nmf_separate_f32), one inverse STFT per stem; a stem goes into every ``ar.*`` feature like the clip itself
"""
import math
import warnings

import numpy as np
import torch as th

from .. import _lib
from . import signal as _signal

__all__ = ["nmf", "decompose", "components", "separate", "nmf_divergence", "NMF_MAX_COMPONENTS", "SEPARATE_MAX_GROUPS"]

NMF_MAX_COMPONENTS = 32  # MAUA_NMF_MAX_K (include/maua_hip.h)
SEPARATE_MAX_GROUPS = 32  # MAUA_SEPARATE_MAX_GROUPS
_SEPARATE_WINDOW_BYTES = 256 << 20  # bound on the two masked-spectrum buffers of one maua_nmf_separate_f32 call
_CHECK_EVERY = 10        # iterations between two evaluations of the divergence when ``tol`` is given


def _iterate(V, W, H, n_iter, update_w, update_h, eps):
    F, T = V.shape
    _lib.call("maua_nmf_kl_f32", V, W, H, F, T, W.shape[1], int(n_iter), int(update_w), int(update_h), float(eps))


def nmf_divergence(V, W, H, eps=1e-12):
    """Generalised Kullback-Leibler divergence sum (V log(V / P) - V + P), P = max(W . H, eps), of device tensors as a 0-d float64
    device tensor (maua_nmf_kl_div_f32: P in fp32 as the updates compute it, the terms and the sums in double).  ``V`` [F, T], ``W`` [F, K]
    and ``H`` [K, T] are numpy arrays or tensors on any device; float32 contiguous tensors on the current device are used as they are,
    and then nothing synchronises.  ValueError: shapes that do not agree, K outside 1 .. 32."""
    shapes = tuple(tuple(x.shape) for x in (V, W, H))
    if any(len(s) != 2 for s in shapes) or 0 in shapes[0]:
        raise ValueError(f"nmf_divergence: V, W and H must be matrices [F, T], [F, K] and [K, T], V not empty (got {shapes})")
    (F, T), K = shapes[0], shapes[1][1]
    if shapes[1] != (F, K) or shapes[2] != (K, T):
        raise ValueError(f"nmf_divergence: V {shapes[0]} needs W [{F}, K] and H [K, {T}] with one K (got {shapes[1]} and {shapes[2]})")
    if not 1 <= K <= NMF_MAX_COMPONENTS:
        raise ValueError(f"nmf_divergence: {K} components, need 1 .. {NMF_MAX_COMPONENTS}")
    if F * T >= 2 ** 31:
        raise ValueError(f"nmf_divergence: V has {F * T} elements, the device kernels index fewer than 2^31")
    V, W, H = _signal._to_dev(V), _signal._to_dev(W), _signal._to_dev(H)
    cols = th.empty(T, dtype=th.float64, device=V.device)
    _lib.call("maua_nmf_kl_div_f32", V, W, H, F, T, W.shape[1], float(eps), cols)
    return cols.sum()


def _normalise_and_order(W, H):
    """Templates to unit sum (their activations scaled the other way: W . H is unchanged), then ascending spectral centroid."""
    total = W.sum(dim=0)
    total = th.where(total > 0, total, th.ones_like(total))
    W, H = W / total[None, :], H * total[:, None]
    bins = th.arange(W.shape[0], dtype=th.float64, device=W.device)
    mass = W.double().sum(dim=0)
    centroid = (bins[:, None] * W.double()).sum(dim=0) / th.where(mass > 0, mass, th.ones_like(mass))
    order = th.argsort(centroid, stable=True)  # ties keep their index order
    return W[:, order].contiguous(), H[order].contiguous()


def nmf(V, n_components, n_iter=200, seed=0, W=None, update_w=True, eps=1e-12, tol=None):
    """(W [F, K], H [K, T]) float32 device tensors with V ~ W . H for a non-negative ``V`` [F, T] (numpy array or tensor, any device).

    Start: deterministic from ``seed`` on the host — ``rng = numpy.random.default_rng(seed)``; ``rng.random((F, K))`` then
    ``rng.random((K, T))``, both times ``sqrt(mean(V) / K)`` (so that W . H starts at the scale of V), rounded to float32.  A given
    ``W`` [F, K] replaces the drawn one as the start (the draw still happens: H does not depend on whether W was given); with
    ``update_w=False`` it is the fixed dictionary and only the activations are computed.
    Loop: ``n_iter`` iterations of H step, W step on the device.  With ``tol`` the divergence is evaluated every 10 iterations and the
    loop stops once its relative decrease over those 10 falls below ``tol``; the default ``tol=None`` enqueues everything at once and
    never synchronises.
    After the loop every template is scaled to unit sum and its activation row the other way (W . H is unchanged), and the components
    are ordered by ascending spectral centroid of their template, ties by index: component 0 is the lowest on every run.
    ValueError: a negative or non-finite value in ``V`` (or ``W``), ``n_components`` outside 1 .. 32, a ``W`` of the wrong shape."""
    K = int(n_components)
    if not 1 <= K <= NMF_MAX_COMPONENTS:
        raise ValueError(f"nmf: n_components ({n_components}) must lie in 1 .. {NMF_MAX_COMPONENTS}")
    if n_iter < 0:
        raise ValueError(f"nmf: n_iter ({n_iter}) must not be negative")
    if not (math.isfinite(eps) and eps > 0):
        raise ValueError(f"nmf: eps ({eps}) must be finite and positive")
    V = _signal._to_dev(V)
    if V.dim() != 2 or V.numel() == 0:
        raise ValueError(f"nmf: V must be a non-empty [F, T] matrix (got shape {tuple(V.shape)})")
    F, T = V.shape
    if F * T >= 2 ** 31:
        raise ValueError(f"nmf: V has {F * T} elements, the device kernels index fewer than 2^31")
    if not bool((th.isfinite(V) & (V >= 0)).all()):
        raise ValueError("nmf: V must be finite and non-negative (a magnitude or power spectrogram)")
    rng = np.random.default_rng(seed)
    scale = math.sqrt(float(V.mean(dtype=th.float64)) / K)
    w0 = (rng.random((F, K)) * scale).astype(np.float32)
    h0 = (rng.random((K, T)) * scale).astype(np.float32)
    if W is not None:
        Wd = _signal._to_dev(W).clone()
        if tuple(Wd.shape) != (F, K):
            raise ValueError(f"nmf: W must be [{F}, {K}] (got {tuple(Wd.shape)})")
        if not bool((th.isfinite(Wd) & (Wd >= 0)).all()):
            raise ValueError("nmf: W must be finite and non-negative")
    else:
        if not update_w:
            raise ValueError("nmf: update_w=False needs a dictionary W")
        Wd = th.from_numpy(w0).to(V.device)
    Hd = th.from_numpy(h0).to(V.device)
    if tol is None:
        if n_iter:
            _iterate(V, Wd, Hd, n_iter, update_w, True, eps)
    else:
        done, before = 0, None
        while done < n_iter:
            chunk = min(_CHECK_EVERY, n_iter - done)
            _iterate(V, Wd, Hd, chunk, update_w, True, eps)
            done += chunk
            now = float(nmf_divergence(V, Wd, Hd, eps))
            if before is not None and before - now < tol * abs(before):
                break
            before = now
    return _normalise_and_order(Wd, Hd)


def _spectrogram(audio, sr, spectrum, n_mels):
    power = _signal.stft_power(audio)
    if spectrum == "mel":
        power = _signal.project(_signal.mel_filterbank(sr, 2048, n_mels), power)
    elif spectrum != "stft":
        raise ValueError(f"decompose: unknown spectrum {spectrum!r} (expected 'mel' or 'stft')")
    return th.sqrt(power.clamp_(min=0))


def decompose(audio, sr, n_components=8, spectrum="mel", n_mels=128, n_iter=200, seed=0):
    """(components [K, bins], activations [K, 1 + len // 512]) of a clip, float32 on the device: :func:`nmf` of the magnitude spectrogram
    V = sqrt(mel_filterbank . |STFT|^2) (``spectrum="mel"``, ``n_mels`` bins) or sqrt(|STFT|^2) (``"stft"``, 1025 bins), frame 2048,
    hop 512.  Component 0 has the lowest spectral centroid."""
    W, H = nmf(_spectrogram(audio, sr, spectrum, n_mels), n_components, n_iter=n_iter, seed=seed)
    return W.t().contiguous(), H


def _clip_column(x, clip):
    """``signal.percentile_clip`` of one envelope; an envelope without a strict local maximum (a dead or constant component) is only
    clamped at 0 and scaled to a maximum of 1."""
    x = x.clamp(min=0)
    top = float(x.max())
    if top <= 0:
        return th.zeros_like(x)
    middle = x[1:-1]
    if x.shape[0] >= 3 and bool(((middle > x[2:]) & (middle > x[:-2])).any()):
        return _signal.percentile_clip(x, clip)
    return x / top


def components(audio, sr, n_frames, n_components=8, smooth=2, clip=100, power=1, margin=None, device=None, spectrum="mel", n_mels=128,
               n_iter=200, seed=0):
    """[n_frames, K] in [0, 1], a CPU tensor unless ``device=`` is given: one envelope per component of :func:`decompose` and video frame,
    column 0 the lowest source.  ``margin``: first take the percussive part (``margin > 0``) or the harmonic part (``margin < 0``, at
    ``-margin``) of the clip with :func:`signal.hpss`.  Every activation row then goes through the chain of :func:`signal.onsets`: Fourier
    resampling to ``n_frames`` clamped to the row's own range, causal Gaussian smoothing, percentile clip, ``power``.  The result weights a
    selection of K latents through ``ar.chroma_weight_latents`` as a chromagram does.  Silence gives zeros with a warning."""
    y = audio
    if margin:
        y = _signal.percussive(audio, margin=margin) if margin > 0 else _signal.harmonic(audio, margin=-margin)
    _, act = decompose(y, sr, n_components=n_components, spectrum=spectrum, n_mels=n_mels, n_iter=n_iter, seed=seed)
    out_device = device if device is not None else "cpu"
    K = act.shape[0]
    if not float(act.max()) > 0:
        warnings.warn("components: the clip is silent, no component is active; returning zeros", stacklevel=2)
        return th.zeros((int(n_frames), K), dtype=th.float32, device=out_device)
    low, high = act.amin(dim=1).double(), act.amax(dim=1).double()
    env = th.clamp(_signal.resample(act.t(), n_frames), min=low[None, :], max=high[None, :]).float()
    env = _signal.gaussian_filter(env, smooth, causal=0).reshape(int(n_frames), K)
    env = th.stack([_clip_column(env[:, k], clip) for k in range(K)], dim=1) ** power
    return env.to(out_device)


def _resolve_groups(groups, n_components):
    """(group int32 [K], G) of the ``groups`` argument of :func:`separate`."""
    K = int(n_components)
    if groups is None:
        return np.arange(K, dtype=np.int32), K
    if isinstance(groups, (int, np.integer)) and not isinstance(groups, (bool, np.bool_)):
        G = int(groups)
        if not 1 <= G <= SEPARATE_MAX_GROUPS:
            raise ValueError(f"separate: groups ({groups}) as a count must lie in 1 .. {SEPARATE_MAX_GROUPS}")
        group = np.empty(K, np.int32)
        for g, run in enumerate(np.array_split(np.arange(K), G)):
            group[run] = g
        return group, G
    if isinstance(groups, (str, bytes, bool, np.bool_)) or not hasattr(groups, "__len__"):
        raise ValueError(f"separate: groups must be None, a count or a sequence of {K} group ids (got {groups!r})")
    ids = np.asarray(groups.cpu() if isinstance(groups, th.Tensor) else groups)
    if ids.shape != (K,) or ids.dtype.kind not in "iu":
        raise ValueError(f"separate: groups must hold one integer id per component, {K} in all (got {groups!r})")
    if int(ids.min()) < 0 or int(ids.max()) >= SEPARATE_MAX_GROUPS:
        raise ValueError(f"separate: group ids must lie in 0 .. {SEPARATE_MAX_GROUPS - 1} (got {groups!r})")
    return ids.astype(np.int32), int(ids.max()) + 1


def _masked_spectra(re, im, W, H, group, G, power, g0, n_out, out_re, out_im):
    F, T = re.shape
    ids = np.ascontiguousarray(group, np.int32)
    _lib.call("maua_nmf_separate_f32", re, im, W, H, ids, F, T, W.shape[1], G, power, g0, n_out, out_re, out_im)


def separate(audio, sr, n_components=8, groups=None, power=2, n_iter=200, seed=0, W=None, update_w=True, device=None, return_model=False,
             _window_bytes=_SEPARATE_WINDOW_BYTES):
    """Stems [G, len(audio)] float32: the clip split into G sources that add up to it.  A numpy array (what ``load_audio`` returns, so
    that ``stems[g]`` goes into every ``ar.*`` feature unchanged) unless ``device=`` is given, then a tensor on that device.

    Chain, all on the device: complex STFT (frame 2048, hop 512, periodic Hann, as :func:`signal.hpss`) -> V = sqrt(re^2 + im^2) ->
    :func:`nmf` (``n_components``, ``n_iter``, ``seed``, ``W``, ``update_w``; components ordered by ascending spectral centroid) -> soft
    masks (maua_nmf_separate_f32: stem g's share of the model, sum_{k in g} W H, over the whole model; ``power=2`` the Wiener mask on the
    squares, ``power=1`` the ratio mask; they sum to 1, an equal split where the model is silent) -> one inverse STFT per stem.
    ``groups``: None, one stem per component; an int G, the ordered components in G contiguous runs sized as
    ``numpy.array_split(range(K), G)``, stem 0 the lowest (beyond K the last runs are empty and their stems silent); a sequence of K ints in 0 .. G - 1 (G = max + 1), used as given.
    ``sr`` is accepted for symmetry with the other features; nothing here depends on it.
    ``return_model=True``: (stems, W [F, K], H [K, T], group int32 [K]), W and H device tensors.
    A silent clip gives zeros with a warning.  ValueError: ``power`` not 1 or 2, empty audio, a ``groups`` that is none of the above."""
    if power not in (1, 2) or isinstance(power, bool):
        raise ValueError(f"separate: power ({power!r}) must be 1 (ratio mask) or 2 (Wiener mask)")
    group, G = _resolve_groups(groups, n_components)
    n = int(np.prod(np.shape(audio))) if not isinstance(audio, th.Tensor) else audio.numel()
    if n == 0:
        raise ValueError("separate: the audio is empty")
    y = _signal._to_dev(audio).reshape(-1)
    dev = y.device
    re, im = _signal.stft_complex(y)
    V = th.sqrt(re * re + im * im)
    Wd, Hd = nmf(V, n_components, n_iter=n_iter, seed=seed, W=W, update_w=update_w)
    stems = th.zeros((G, n), dtype=th.float32, device=dev)
    if not float(V.max()) > 0:
        warnings.warn("separate: the clip is silent, every stem is silent; returning zeros", stacklevel=2)
    else:
        F, T = re.shape
        per_call = max(1, min(G, int(_window_bytes) // (2 * F * T * 4)))
        out_re = th.empty((per_call, F, T), dtype=th.float32, device=dev)
        out_im = th.empty_like(out_re)
        win = _signal._hann(2048, dev)
        frames_ws = th.empty((T, 2048), dtype=th.float32, device=dev)
        for g0 in range(0, G, per_call):
            n_out = min(per_call, G - g0)
            _masked_spectra(re, im, Wd, Hd, group, G, int(power), g0, n_out, out_re, out_im)
            for j in range(n_out):
                _lib.call("maua_istft_f32", out_re[j], out_im[j], win, 2048, 512, T, frames_ws, stems[g0 + j], n)
    out = stems.to(device) if device is not None else stems.cpu().numpy()
    return (out, Wd, Hd, group) if return_model else out
