"""The temporal fold (csrc/temporal_fold.hip, render.fold_frames) restated in numpy, in uint64: the two formulas of include/maua_hip.h,
the shutters and the sRGB table builder.  Written from the specification, not from the product's code: the tests compare the two."""
import numpy as np


def shutter_ref(shutter, n):
    if shutter == "box":
        return [1] * n
    if shutter == "tent":
        return [min(i + 1, n - i) for i in range(n)]
    return [int(p) for p in shutter.split(",")]


def accumulate_ref(frames, weights, decode=None):
    """frames uint8 [groups * N, frame_bytes], weights N integers -> (L uint64 [groups, frame_bytes], W): the rounded weighted mean
    floor((sum_i w_i * x_i + floor(W / 2)) / W) of the N sub-frames of every group, x the bytes themselves or decode[byte]."""
    frames = np.asarray(frames)
    n = len(weights)
    assert frames.ndim == 2 and frames.dtype == np.uint8 and frames.shape[0] % n == 0
    total = int(sum(weights))
    assert 1 <= n <= 16 and total > 0 and all(0 <= w <= 255 for w in weights)
    values = frames.astype(np.uint64) if decode is None else np.asarray(decode).astype(np.uint64)[frames]
    values = values.reshape(frames.shape[0] // n, n, frames.shape[1])
    acc = (values * np.asarray(weights, dtype=np.uint64)[None, :, None]).sum(axis=1, dtype=np.uint64)
    assert acc.max(initial=0) + total // 2 < 2 ** 32  # what the kernel's 32-bit sums rely on
    return (acc + np.uint64(total // 2)) // np.uint64(total), total


def fold_ref(frames, weights, decode=None, encode_threshold=None):
    """uint8 [groups * N, frame_bytes] -> uint8 [groups, frame_bytes].  Encoded light without tables; linear light with both:
    out = max{ v : encode_threshold[v] <= L }."""
    assert (decode is None) == (encode_threshold is None)
    mean, _ = accumulate_ref(frames, weights, decode)
    if decode is None:
        assert mean.max(initial=0) <= 255
        return mean.astype(np.uint8)
    thr = np.asarray(encode_threshold).astype(np.uint64)
    assert thr.shape == (256,) and thr[0] == 0 and np.all(np.diff(thr.astype(np.int64)) >= 0)
    # max{v : thr[v] <= L} = (number of v with thr[v] <= L) - 1 for a non-decreasing table that starts at 0
    return (np.searchsorted(thr, mean, side="right") - 1).astype(np.uint8)


def srgb_to_linear(c):
    c = np.asarray(c, dtype=np.float64)
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def linear_to_srgb(lin):
    lin = np.asarray(lin, dtype=np.float64)
    return np.where(lin <= 0.0031308, 12.92 * lin, 1.055 * lin ** (1.0 / 2.4) - 0.055)


def srgb_encode_all():
    """rint(255 * linear_to_srgb(L / 65535)) for every 16-bit L, int64 [65536]."""
    return np.rint(255.0 * linear_to_srgb(np.arange(65536, dtype=np.float64) / 65535.0)).astype(np.int64)


def srgb_tables_ref():
    """(decode, encode_threshold) uint16 [256]: decode[v] = rint(65535 * srgb_to_linear(v / 255)); encode_threshold[v] = the smallest L whose
    encoding is >= v, found by a plain scan."""
    decode = np.rint(65535.0 * srgb_to_linear(np.arange(256, dtype=np.float64) / 255.0)).astype(np.uint16)
    encoded = srgb_encode_all()
    threshold = np.array([int(np.nonzero(encoded >= v)[0][0]) for v in range(256)], dtype=np.uint16)
    return decode, threshold


def fold_video_ref(frames, weights, light="encoded"):
    """uint8 [n, ...] rendered frames -> [n // N, ...] delivered frames, sRGB tables for linear light."""
    frames = np.asarray(frames)
    flat = frames.reshape(frames.shape[0], -1)
    tables = srgb_tables_ref() if light == "linear" else (None, None)
    return fold_ref(flat, weights, *tables).reshape((frames.shape[0] // len(weights),) + frames.shape[1:])
