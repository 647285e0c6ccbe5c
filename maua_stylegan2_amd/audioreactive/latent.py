"""Latent / noise helpers with the reference's ``audioreactive.latent`` surface.

Mirrors /root/reference/audioreactive/latent.py: chroma_weight_latents :15-26 · slerp :29-45 · slerp_loops :48-83 ·
spline_loops :86-107 · wrapping_slice :110-133 · generate_latents :136-159 · save/load_latents :162-181 ·
perlin_noise :188-246.  Beyond the reference: spline_loops / slerp_loops take a CUDA selection and then run on the device, and loop_sections
builds a whole sectioned sequence of such loops in one launch (csrc/latent_loops.hip).  perlin_noise runs as one HIP kernel (csrc/signal.hip perlin3d_kernel) from the same numpy-RNG
gradient angles the reference draws; generate_latents maps z through the mapping network of the MI355X generator
(the evident intent — the reference's map_latents branch normalises over a singleton axis).
"""
import numpy as np
import torch as th
from scipy import interpolate

from .. import _lib
from .signal import _const_dev, _dev, _to_dev, gaussian_filter


def chroma_weight_latents(chroma, latents):
    """[n_frames, notes] x [notes, n_latent, 512] -> [n_frames, n_latent, 512]."""
    return th.einsum("tn,nld->tld", chroma.to(latents.device, latents.dtype), latents)


def pitch_weight_latents(pitch, latents):
    """[n_frames] pitch height in [0, 1] x [m, n_latent, 512] -> [n_frames, n_latent, 512]: a piecewise-linear walk along the selection
    (the counterpart of :func:`chroma_weight_latents` for ``ar.pitch``).  With p = pitch (m - 1) a frame is
    (1 - frac) latents[floor p] + frac latents[min(floor p + 1, m - 1)]: height 0 is the first entry, 1 the last, k / (m - 1) entry k.
    Plain torch on the device of ``latents``."""
    m = latents.shape[0]
    p = pitch.to(latents.device, latents.dtype).clamp(0, 1) * (m - 1)
    low = p.floor()
    frac = (p - low)[:, None, None]
    low = low.long().clamp(max=m - 1)
    return (1 - frac) * latents[low] + frac * latents[(low + 1).clamp(max=m - 1)]


def slerp(val, low, high):
    """Great-circle interpolation between two vectors (reference :29-45).  ``val`` may be a scalar or an array of
    fractions: all of them are evaluated at once, one row per fraction."""
    low, high = np.asarray(low), np.asarray(high)
    frac = np.asarray(val, dtype=np.float64)
    if frac.ndim:
        frac = frac.reshape(frac.shape + (1,) * low.ndim)
    cosine = np.dot(low.ravel() / np.linalg.norm(low), high.ravel() / np.linalg.norm(high))
    angle = np.arccos(np.clip(cosine, -1.0, 1.0))
    sine = np.sin(angle)
    if sine == 0:  # parallel vectors: the geodesic degenerates to the straight line
        return low + frac * (high - low)
    return (np.sin((1.0 - frac) * angle) * low + np.sin(frac * angle) * high) / sine


def _on_device(x):
    return isinstance(x, th.Tensor) and x.is_cuda


def slerp_loops(latent_selection, n_frames, n_loops, smoothing=1, loop=True):
    """Looping latent sequence along great circles between consecutive selection entries (reference :48-83): every key
    gets n_frames // n_loops // n_keys frames, the loop is Gaussian-smoothed along time and tiled to ``n_frames``.
    Differences from the reference, both needed for it to run at all or off 1024 px: the float64 interpolant is cast to
    float32 before the filter (the reference's conv1d rejects it) and the layer axis is
    the selection's own instead of a hard-coded 18.  A CUDA selection is looped on its device (float32 CUDA result, loop_sections)."""
    if _on_device(latent_selection):
        return _device_loop(latent_selection, n_frames, n_loops, "slerp", loop, smoothing)
    keys = np.asarray(latent_selection)
    n_layers = keys.shape[1]
    if loop:
        keys = np.concatenate([keys, keys[:1]])
    fractions = np.linspace(0.0, 1.0, int(n_frames // max(1, n_loops) // len(keys)))
    legs = [slerp(fractions, keys[k][0], keys[(k + 1) % len(keys)][0]) for k in range(len(keys))]
    cycle = gaussian_filter(th.from_numpy(np.concatenate(legs)).float(), smoothing)
    frames = cycle.repeat(int(n_frames / len(cycle)), 1)
    if len(frames) != n_frames:
        frames = th.cat([frames, frames[: n_frames - len(frames)]])
    return frames[:, None, :].repeat(1, n_layers, 1)


def spline_loops(latent_selection, n_frames, n_loops, loop=True):
    """Looping latent sequence on the cubic spline through the selection entries (reference :86-107): float64 on the host for a numpy or
    CPU-tensor selection; a CUDA selection is looped on its device (float32 CUDA result, loop_sections)."""
    if _on_device(latent_selection):
        return _device_loop(latent_selection, n_frames, n_loops, "spline", loop, 1)
    latent_selection = np.asarray(latent_selection)
    if loop:
        latent_selection = np.concatenate([latent_selection, latent_selection[[0]]])
    x = np.linspace(0, 1, int(n_frames // max(1, n_loops)))
    knots = np.linspace(0, 1, latent_selection.shape[0])
    flat = latent_selection.reshape(latent_selection.shape[0], -1)
    base = np.zeros((len(x), flat.shape[1]))
    for j in range(flat.shape[1]):
        base[:, j] = interpolate.splev(x, interpolate.splrep(knots, flat[:, j]))
    base = th.from_numpy(base.reshape((len(x),) + latent_selection.shape[1:]))
    out = th.cat([base] * int(n_frames / len(base)), axis=0)
    if n_frames - len(out) > 0:
        out = th.cat([out, out[0: n_frames - len(out)]])
    return out[:n_frames]


# ------------------------------------------------------------------------------------------------ loops on the device
# For a fixed knot count m and period P the interpolating spline is a linear map of its keys, base = W @ keys with W [P, m] a function of
# (m, P) alone; the per-leg sine weights of slerp_loops and its circular smoothing are linear in the keys as well once the leg angles are
# known.  A looping sequence, and a whole sequence of sections each looping through its own slice of the selection, is therefore one
# gather-and-blend: out[f] = sum_i W[row(f), i] * selection[key(section(f), i)] (maua_keyframe_blend_f32, csrc/latent_loops.hip).
LOOP_MAX_KEYS = 32  # MAUA_LOOP_MAX_KEYS (include/maua_hip.h): keys of one loop, the closing key included
LOOP_KINDS = ("spline", "slerp")
_SPLINE_WEIGHTS = {}  # (m, P) -> float64 [P, m], insertion-ordered (oldest dropped beyond 64 entries)


def spline_weights(m, P):
    """W [P, m] (float64, host, read-only) with spline_loops' base == W @ keys for m keys (the closing key included) and a period of P
    frames: column i is the spline through the i-th unit vector, from the same splrep / splev calls on the same knots and abscissae."""
    m, P = int(m), int(P)
    if m < 4:
        raise ValueError(f"a cubic spline loop needs at least 4 keys, the closing key included (got {m})")
    if P < 1:
        raise ValueError(f"a loop period of {P} frames: n_frames // n_loops must be at least 1")
    hit = _SPLINE_WEIGHTS.get((m, P))
    if hit is None:
        x, knots = np.linspace(0, 1, P), np.linspace(0, 1, m)
        hit = np.stack([interpolate.splev(x, interpolate.splrep(knots, unit)) for unit in np.eye(m)], axis=1)
        hit.setflags(write=False)
        _SPLINE_WEIGHTS[(m, P)] = hit
        while len(_SPLINE_WEIGHTS) > 64:
            _SPLINE_WEIGHTS.pop(next(iter(_SPLINE_WEIGHTS)))
    return hit


def slerp_weights(keys0, P_leg, smoothing=1):
    """W [m * P_leg, m] (float32, device) with slerp_loops' smoothed cycle == W @ keys0 for the m keys ``keys0`` [m, D] (layer 0 of the
    selection entries, the closing key included): leg k runs from key k to key (k + 1) % m over P_leg frames with the sine weights of
    ``slerp`` — angles from float64 dot products, the straight line where sin(angle) is 0 or not finite, chosen on the device — and the
    cycle's circular Gaussian smoothing is applied to the weights instead (the filter is linear: same taps, SMF and radius clamp)."""
    keys0 = _to_dev(keys0, th.float64)
    m, P_leg = keys0.shape[0], int(P_leg)
    if P_leg < 1:
        raise ValueError(f"{P_leg} frames per key: n_frames // n_loops // n_keys must be at least 1")
    unit = keys0.reshape(m, -1) / keys0.reshape(m, -1).norm(dim=1, keepdim=True)
    angle = th.acos((unit * unit.roll(-1, 0)).sum(1).clamp(-1.0, 1.0))[:, None]
    sine = th.sin(angle)
    frac = _const_dev(np.linspace(0.0, 1.0, P_leg))[None, :]
    straight = (sine == 0) | ~th.isfinite(sine)
    low = th.where(straight, 1.0 - frac, th.sin((1.0 - frac) * angle) / sine)  # [m, P_leg]: weight of key k on leg k
    high = th.where(straight, frac.expand(m, -1), th.sin(frac * angle) / sine)  # ... and of key (k + 1) % m
    eye = th.eye(m, dtype=th.float64, device=keys0.device)
    w = low[:, :, None] * eye[:, None, :] + high[:, :, None] * eye.roll(-1, 0)[:, None, :]
    return gaussian_filter(w.reshape(m * P_leg, m).float(), smoothing).reshape(m * P_leg, m)


def _loop_period(kind, n_frames, n_loops, m):
    """Frames of one period, as the host paths compute them: n_frames // n_loops for a spline, m whole legs of that for a slerp."""
    period = int(n_frames // max(1, n_loops))
    return period if kind == "spline" else m * int(period // m)


def _check_sections(frames, periods, n_frames):
    total = sum(frames)
    if any(f < 0 for f in frames):
        raise ValueError(f"section lengths must not be negative (got {list(frames)})")
    if len(periods) != len(frames):
        raise ValueError(f"{len(frames)} sections but {len(periods)} periods")
    if total > n_frames:
        raise ValueError(f"the sections hold {total} frames, more than n_frames = {n_frames}")
    if n_frames > total == 0:
        raise ValueError(f"{n_frames} frames to fill but every section is empty: there is no last frame to repeat")
    for s, (f, p) in enumerate(zip(frames, periods)):
        if f > 0 and p < 1:
            raise ValueError(f"section {s}: {f} frames give a loop period of {p} frames; lower its n_loops (or its key count, for a slerp)")


def loop_frame_tables(frames, periods, n_frames=None, row_bases=None, device="cpu"):
    """(row_of_frame, sec_of_frame), int32 [n_frames] on ``device``, for sections of ``frames[s]`` frames that each tile their own
    ``periods[s]`` weight rows — the period int(n / P) times, then its head as the tail, i.e. row (f - start) % P — stored from row
    ``row_bases[s]`` on (default: one block per section, in order).  Empty sections own no frame; frames from sum(frames) up to
    ``n_frames`` repeat the last one.  A few torch ops on ``device``; the section lists themselves are checked on the host."""
    frames, periods = [int(f) for f in frames], [int(p) for p in periods]
    total = sum(frames)
    n_frames = total if n_frames is None else int(n_frames)
    _check_sections(frames, periods, n_frames)
    if row_bases is None:
        row_bases = np.cumsum([0] + [p if f > 0 else 0 for f, p in zip(frames, periods)])[:-1]
    ends = np.cumsum(frames)
    meta = th.tensor(np.stack([ends, ends - frames, [max(p, 1) for p in periods], [int(b) for b in row_bases]]).astype(np.int64)).to(device)
    f = th.arange(n_frames, device=device).clamp_(max=max(total - 1, 0))
    sec = th.bucketize(f, meta[0], right=True)  # first section that ends beyond f: empty sections are stepped over
    row = meta[3][sec] + (f - meta[1][sec]) % meta[2][sec]
    return row.int(), sec.int()


def _loop_sequence(selection, key_rows, frames, n_loops, n_frames, kind, loop, smoothing):
    """One launch for sections looping through ``key_rows[s]`` (rows of ``selection``): float32 [n_frames, *selection.shape[1:]]."""
    if kind not in LOOP_KINDS:
        raise ValueError(f"kind must be one of {LOOP_KINDS} (got {kind!r})")
    shape = tuple(selection.shape)
    n_sel, tail = shape[0], shape[1:]
    frames = [int(f) for f in frames]
    m = len(key_rows[0]) + (1 if loop else 0)
    if m > LOOP_MAX_KEYS:
        raise ValueError(f"{m} keys per loop (the closing key included) exceed the device path's {LOOP_MAX_KEYS}")
    if kind == "spline" and m < 4:
        raise ValueError(f"a cubic spline loop needs at least 4 keys, the closing key included (got {m})")
    if kind == "slerp" and len(shape) != 3:
        raise ValueError(f"a slerp loop needs a [n, layers, dim] selection (got {list(shape)})")
    periods = [_loop_period(kind, f, n, m) if f > 0 else 0 for f, n in zip(frames, n_loops)]
    n_frames = sum(frames) if n_frames is None else int(n_frames)
    _check_sections(frames, periods, n_frames)
    sel = _to_dev(selection)  # (everything above is refused on the host, before the device is touched)
    dev = sel.device
    out = th.empty((n_frames,) + tail, dtype=th.float32, device=dev)
    if n_frames == 0:
        return out
    key_idx = np.asarray([list(rows) + list(rows[:1] if loop else []) for rows in key_rows], dtype=np.int32).reshape(len(frames), m)
    blocks, bases, n_rows, shared = [], [], 0, {}
    with th.cuda.device(dev):  # (kept: _const_dev below allocates on the current device)
        for s, (f, period) in enumerate(zip(frames, periods)):
            if f == 0:
                bases.append(0)
            elif kind == "spline" and period in shared:  # W depends on (m, P) alone
                bases.append(shared[period])
            else:
                if kind == "spline":
                    shared[period] = n_rows
                    blocks.append(_const_dev(spline_weights(m, period), np.float32))
                else:  # the angles are those of the section's own keys, layer 0
                    blocks.append(slerp_weights(sel[th.from_numpy(key_idx[s].astype(np.int64)).to(dev), 0], period // m, smoothing))
                bases.append(n_rows)
                n_rows += period
        weights = (blocks[0] if len(blocks) == 1 else th.cat(blocks)).contiguous()
        # a slerp loop moves layer 0 of its keys and repeats it over the layers: the bank holds that repetition
        bank = (sel.reshape(n_sel, -1) if kind == "spline" else sel[:, :1].expand(-1, tail[0], -1).reshape(n_sel, -1)).contiguous()
        row_of_frame, sec_of_frame = loop_frame_tables(frames, periods, n_frames, bases, dev)
        idx = th.from_numpy(key_idx).to(dev)
        _lib.call("maua_keyframe_blend_f32", bank, n_sel, bank.shape[1], idx, weights, row_of_frame, sec_of_frame, out, n_frames, len(frames), n_rows, m)
    return out


def _device_loop(selection, n_frames, n_loops, kind, loop, smoothing):
    """spline_loops / slerp_loops of a CUDA selection: one section through every entry, on the selection's device."""
    n_frames = int(n_frames)
    if n_frames < 1:
        raise ValueError(f"a loop of {n_frames} frames: n_frames must be at least 1")
    with th.cuda.device(selection.device):
        return _loop_sequence(selection, [range(selection.shape[0])], [n_frames], [n_loops], n_frames, kind, loop, smoothing)


def loop_sections(selection, frames, key_starts, n_keys, n_loops, n_frames=None, kind="spline", loop=True, smoothing=1):
    """A sequence of sections that each loop through their own slice of ``selection``, built on the current device in one launch: section s
    is spline_loops (``kind="slerp"``: slerp_loops, with ``smoothing``) of wrapping_slice(selection, key_starts[s], n_keys) with
    ``frames[s]`` frames and ``n_loops[s]`` loops (``n_loops``: one value for all sections or one per section; fractions allowed).
    Frames from sum(frames) up to ``n_frames`` repeat the last frame; a section of 0 frames contributes nothing.  float32 CUDA
    [n_frames, *selection.shape[1:]], bit-identical to concatenating the per-section calls on a CUDA selection."""
    frames, key_starts, n_keys = [int(f) for f in frames], [int(k) for k in key_starts], int(n_keys)
    n_sel = len(selection)
    if len(key_starts) != len(frames):
        raise ValueError(f"{len(frames)} sections but {len(key_starts)} key_starts")
    n_loops = list(n_loops) if np.ndim(n_loops) else [n_loops] * len(frames)
    if len(n_loops) != len(frames):
        raise ValueError(f"{len(frames)} sections but {len(n_loops)} n_loops")
    if not 1 <= n_keys <= n_sel:
        raise ValueError(f"n_keys must lie in 1 .. {n_sel}, the size of the selection (got {n_keys})")
    for s, start in enumerate(key_starts):
        if not 0 <= start < n_sel:
            raise ValueError(f"section {s}: key_start {start} lies outside 0 .. {n_sel - 1}")
    key_rows = [wrapping_slice(selection, start, n_keys, return_indices=True).tolist() for start in key_starts]
    if not key_rows:
        key_rows = [list(range(n_keys))]  # (no sections at all: only the key count is looked at)
    return _loop_sequence(selection, key_rows, frames, n_loops, n_frames, kind, loop, smoothing)


def wrapping_slice(tensor, start, length, return_indices=False):
    """``length`` entries of ``tensor`` from ``start``, continuing at the beginning when the end is reached (reference
    :110-133).  Like the reference the slice wraps at most once — a request that would lap the tensor again ends at
    (start + length) mod n — and a slice that starts AT the end has no head: it is the first (start + length) mod n entries.
    A start beyond the end raises, as the reference's ``arange(start, n)`` does."""
    n = tensor.shape[0]
    end = start + length
    if start > n and end > n:
        raise RuntimeError(f"wrapping_slice: start {start} lies beyond the tensor ({n} entries)")
    head = length if end <= n else max(n - start, 0)   # entries taken before the wrap
    tail = 0 if end <= n else end % n                  # entries taken from the beginning
    k = th.arange(head + tail)
    indices = th.where(k < head, k + start, k - head)
    if n == 1:
        indices = indices.new_zeros(1)
    return indices if return_indices else tensor[indices]


_MAPPING_CACHE = {}  # (checkpoint path, mtime, size, latent_dim, n_mlp, device) -> mapping network on the device (8 MB; one entry)


def _mapping_network(ckpt, latent_dim, n_mlp):
    """The checkpoint's mapping network (``style.*``) on the current device.  Built ON the device without initial values when a checkpoint
    will overwrite every tensor (eight 512 x 512 normal draws + scalings on the CPU were 0.05 s of a 0.9 s job), and kept for the next job on
    the same checkpoint FILE (path, mtime, size) — the generator itself is kept the same way (generate_audiovisual._cached_generator)."""
    import os

    from ..models import stylegan2 as sg2

    dev = th.device("cuda", th.cuda.current_device())
    key = None
    if ckpt is not None:
        try:
            st = os.stat(ckpt)
            key = (os.path.realpath(ckpt), st.st_mtime_ns, st.st_size, latent_dim, n_mlp, dev.index)
        except OSError:
            key = None
        if key is not None and _MAPPING_CACHE.get("key") == key:
            return _MAPPING_CACHE["net"]
    sg2._SKIP_INIT.on = ckpt is not None
    try:
        with th.device(dev):
            mapping = th.nn.Sequential(sg2.PixelNorm(), *[sg2.EqualLinear(latent_dim, latent_dim, lr_mul=0.01, activation="fused_lrelu")
                                                          for _ in range(n_mlp)])
    finally:
        sg2._SKIP_INIT.on = False
    if ckpt is not None:
        try:  # zip-format checkpoints are mapped: only the pages of the eight style.* matrices are ever read
            weights = th.load(ckpt, map_location="cpu", mmap=True)["g_ema"]
        except (RuntimeError, ValueError, TypeError):
            weights = th.load(ckpt, map_location="cpu")["g_ema"]
        mapping.load_state_dict({k[len("style."):]: v for k, v in weights.items() if k.startswith("style.")}, strict=True)
        del weights
    mapping = mapping.to(dev)
    if key is not None:
        _MAPPING_CACHE.clear()
        _MAPPING_CACHE.update(key=key, net=mapping)
    return mapping


def generate_latents(n_latents, ckpt, G_res, noconst=False, latent_dim=512, n_mlp=8, channel_multiplier=2):
    """``n_latents`` random w vectors, each repeated over the generator's layers: [n_latents, n_latent, latent_dim] on the
    CPU (reference :136-159).  Only the mapping network is needed for that, so only its ``style.*`` tensors are read from
    the checkpoint and put on the device (the reference builds and uploads a second full generator).  z is mapped on
    [N, latent_dim] — the evident intent; the reference's map_latents branch normalises over a singleton axis."""
    mapping = _mapping_network(ckpt, latent_dim, n_mlp)
    w = mapping(th.randn((n_latents, latent_dim), device="cuda"))
    n_layers = 2 * int(np.log2(G_res)) - 2
    return w[:, None, :].repeat(1, n_layers, 1).cpu()


def save_latents(latents, filename):
    np.save(filename, latents.numpy() if isinstance(latents, th.Tensor) else np.asarray(latents))


def load_latents(filename):
    return th.from_numpy(np.load(filename))


def perlin_gradients(res, tileable=(True, False, False), rng=None):
    """Unit gradient lattice [r0+1, r1+1, r2+1, 3] from two uniform angle draws (reference :209-218)."""
    rand = np.random.rand if rng is None else rng.random
    theta = 2 * np.pi * rand(res[0] + 1, res[1] + 1, res[2] + 1)
    phi = 2 * np.pi * rand(res[0] + 1, res[1] + 1, res[2] + 1)
    g = np.stack((np.sin(phi) * np.cos(theta), np.sin(phi) * np.sin(theta), np.cos(phi)), axis=3)
    if tileable[0]:
        g[-1, :, :] = g[0, :, :]
    if tileable[1]:
        g[:, -1, :] = g[:, 0, :]
    if tileable[2]:
        g[:, :, -1] = g[:, :, 0]
    return g.astype(np.float32)


def perlin_noise(shape, res, tileable=(True, False, False), interpolant=None, gradients=None):
    """3-D Perlin noise tensor of ``shape`` on the current HIP device (reference :188-246; quintic fade only)."""
    if interpolant is not None:
        raise NotImplementedError("the HIP Perlin kernel implements the default quintic interpolant")
    if any(s % r for s, r in zip(shape, res)):
        raise ValueError("shape must be a multiple of res")
    g = perlin_gradients(res, tileable) if gradients is None else gradients if isinstance(gradients, th.Tensor) else np.asarray(gradients)
    lattice = (res[0] + 1, res[1] + 1, res[2] + 1, 3)
    if tuple(g.shape) != lattice:
        raise ValueError(f"perlin_noise: res {tuple(res)} needs gradients of shape {lattice} (got {tuple(g.shape)})")
    gd = _to_dev(g)
    out = th.empty(tuple(shape), dtype=th.float32, device=gd.device)
    _lib.call("maua_perlin3d_f32", gd, out, shape[0], shape[1], shape[2], res[0], res[1], res[2])
    return out
