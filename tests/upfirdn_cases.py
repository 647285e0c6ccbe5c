"""The case list of the entry-level tests of maua_upfirdn2d_f32 (tests/test_upfirdn2d_entries_host.py proves what it reaches,
tests/test_upfirdn2d_entries_gpu.py runs it).  A case is the entry's 14 geometry integers in the order of UPFIRDN_CASES of
tests/test_native_ops_entries_gpu.py: (major, in_h, in_w, minor, kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1).

The entry has 16 kernels behind one dispatch (csrc/upfirdn2d.hip): fir_tile_kernel<K, K, WX, false, 24> for K = 2, 3, 4, fir_up2_kernel<WX, 16>
and fir_down2_kernel<WX, 8>, each with WX = 1, 2, 4 chosen by the output width, and fir_generic_kernel.  A workgroup of a tiled kernel is WX
wave strips side by side and 4 / WX on top of each other: tiles of 96 x 64, 48 x 128, 24 x 256 outputs (tile), 64 x 128, 32 x 256, 16 x 512
(up2), 32 x 64, 16 x 128, 8 x 256 (down2).  The shapes are the smallest that cross those edges; which instance a case takes is never
restated here — the host test asks maua_upfirdn2d_plan_instance."""
import numpy as np

BLUR, UP, DOWN = (1, 1, 1, 1), (2, 2, 1, 1), (1, 1, 2, 2)


def _tile(major, out_h, out_w, k, px0, px1, py0, py1):
    """up = down = 1 with k x k taps, by its output shape."""
    return (major, out_h + k - 1 - py0 - py1, out_w + k - 1 - px0 - px1, 1, k, k) + BLUR + (px0, px1, py0, py1)


def _up2(major, out_h, out_w, px0, px1, py0, py1):
    """up = 2 with 4 x 4 taps, by its output shape: out = 2 in + pad0 + pad1 - 3."""
    assert (out_h + 3 - py0 - py1) % 2 == 0 and (out_w + 3 - px0 - px1) % 2 == 0
    return (major, (out_h + 3 - py0 - py1) // 2, (out_w + 3 - px0 - px1) // 2, 1, 4, 4) + UP + (px0, px1, py0, py1)


def _down2(major, out_h, out_w, px0, px1, py0, py1, odd=0):
    """down = 2 with 4 x 4 taps, by its output shape: out = (in + pad0 + pad1 - 4) // 2 + 1; ``odd``: one more input row and column,
    which the floor drops."""
    return (major, 2 * out_h + 2 - py0 - py1 + odd, 2 * out_w + 2 - px0 - px1 + odd, 1, 4, 4) + DOWN + (px0, px1, py0, py1)


CASES = {
    # ---- up = down = 1 (fir_tile_kernel)
    "tile4_tiny": (2, 5, 7, 1, 4, 4) + BLUR + (1, 1, 1, 1),
    "tile4_two_tile_rows_w64": (3, 97, 64, 1, 4, 4) + BLUR + (2, 1, 1, 2),
    "tile3_h96_w63": (2, 96, 63, 1, 3, 3) + BLUR + (1, 1, 1, 1),
    "tile2_per_axis_pads": (3, 30, 41, 1, 2, 2) + BLUR + (1, 0, 0, 1),
    "tile4_w65": (2, 50, 65, 1, 4, 4) + BLUR + (2, 1, 1, 1),
    "tile3_h48_w128": (3, 48, 128, 1, 3, 3) + BLUR + (1, 1, 1, 1),
    "tile2_no_pad_w99": (2, 47, 100, 1, 2, 2) + BLUR + (0, 0, 0, 0),
    "tile4_w257": (2, 25, 257, 1, 4, 4) + BLUR + (2, 1, 2, 1),
    "tile3_h24_w129": (3, 24, 129, 1, 3, 3) + BLUR + (1, 1, 1, 1),
    "tile2_w300": (1, 26, 300, 1, 2, 2) + BLUR + (1, 0, 1, 0),
    "tile4_crop": (2, 40, 40, 1, 4, 4) + BLUR + (-1, 0, -3, 2),
    "tile4_pads_wider_than_a_tile": (1, 10, 40, 1, 4, 4) + BLUR + (70, 3, 100, 0),  # whole tiles of zeros
    "tile4_one_pixel": (3, 1, 1, 1, 4, 4) + BLUR + (3, 3, 3, 3),
    "tile3_crop_both_axes": (2, 12, 13, 1, 3, 3) + BLUR + (-2, 1, -2, 1),
    # ---- up = 2 (fir_up2_kernel)
    "up2_8x8": (2, 4, 4, 1, 4, 4) + UP + (2, 1, 2, 1),
    "up2_66x128": (2, 33, 64, 1, 4, 4) + UP + (2, 1, 2, 1),
    "up2_34x130": (3, 17, 65, 1, 4, 4) + UP + (2, 1, 2, 1),
    "up2_18x514": (2, 9, 257, 1, 4, 4) + UP + (2, 1, 2, 1),
    "up2_odd_width": (2, 20, 67, 1, 4, 4) + UP + (1, 1, 1, 1),  # the lone last column
    "up2_phases_a": (2, 19, 23, 1, 4, 4) + UP + (1, 2, 2, 1),  # both column and row phases
    "up2_phases_b": (2, 19, 23, 1, 4, 4) + UP + (2, 1, 1, 2),
    "up2_crop": (1, 40, 70, 1, 4, 4) + UP + (5, -2, -1, 1),
    "up2_taps_3x4": (3, 21, 45, 1, 3, 4) + UP + (2, 1, 0, 3),
    "up2_taps_1x4": (2, 9, 140, 1, 1, 4) + UP + (2, 1, 0, 0),
    "up2_taps_4x1": (2, 9, 11, 1, 4, 1) + UP + (0, 0, 2, 1),
    "up2_taps_1x1": (2, 16, 129, 1, 1, 1) + UP + (0, 0, 0, 0),
    "up2_taps_2x2": (2, 16, 16, 1, 2, 2) + UP + (1, 0, 1, 0),
    "up2_one_pixel": (3, 1, 1, 1, 4, 4) + UP + (2, 1, 2, 1),
    "up2_taps_3x4_square_pads": (2, 7, 9, 1, 3, 4) + UP + (2, 1, 2, 1),
    # ---- down = 2 (fir_down2_kernel)
    "down2_4x4": (2, 8, 8, 1, 4, 4) + DOWN + (1, 1, 1, 1),
    "down2_33x64": (2, 66, 128, 1, 4, 4) + DOWN + (1, 1, 1, 1),
    "down2_17x65": (3, 34, 131, 1, 4, 4) + DOWN + (1, 1, 1, 1),
    "down2_9x257": (2, 18, 515, 1, 4, 4) + DOWN + (1, 1, 1, 1),
    "down2_per_axis_pads": (2, 37, 41, 1, 4, 4) + DOWN + (2, 1, 0, 3),
    "down2_crop": (1, 40, 70, 1, 4, 4) + DOWN + (5, -2, -1, 1),
    "down2_taps_3x2": (2, 29, 130, 1, 3, 2) + DOWN + (1, 0, 1, 1),
    "down2_taps_1x1": (2, 16, 129, 1, 1, 1) + DOWN + (0, 0, 0, 0),
    "down2_taps_1x4": (2, 9, 140, 1, 1, 4) + DOWN + (2, 1, 0, 0),
    "down2_one_pixel": (3, 1, 1, 1, 4, 4) + DOWN + (3, 3, 3, 3),
    "down2_one_output": (1, 2, 2, 1, 4, 4) + DOWN + (1, 1, 1, 1),
    # ---- everything else (fir_generic_kernel)
    "generic_minor_2_blur": (2, 9, 10, 2, 4, 4) + BLUR + (2, 1, 2, 1),
    "generic_minor_3_up2": (2, 5, 4, 3, 4, 4) + UP + (2, 1, 2, 1),
    "generic_taps_3x4": (2, 12, 70, 1, 3, 4) + BLUR + (1, 2, 1, 1),
    "generic_taps_5x5": (2, 12, 70, 1, 5, 5) + BLUR + (2, 2, 2, 2),
    "generic_taps_1x1": (2, 5, 6, 1, 1, 1) + BLUR + (0, 0, 0, 0),
    "generic_taps_5x5_up2": (2, 7, 9, 1, 5, 5) + UP + (3, 2, 2, 3),
    "generic_up_2_1": (2, 6, 7, 1, 4, 4, 2, 1, 1, 1, 2, 1, 1, 2),
    "generic_down_1_2": (2, 9, 8, 1, 4, 4, 1, 1, 1, 2, 1, 1, 1, 1),
    "generic_up2_down2": (2, 8, 9, 1, 4, 4, 2, 2, 2, 2, 2, 1, 2, 1),
    "generic_up3": (2, 5, 6, 1, 3, 3, 3, 3, 1, 1, 1, 1, 1, 1),
    "generic_per_axis_everything": (3, 6, 11, 1, 3, 5, 2, 3, 3, 1, 2, -1, 1, 3),
}

# Per tiled instance, by output shape: "rows" — two tile rows, the last partial, two planes of odd size, pad_x0 != pad_y0 (for WX = 4 also
# two tile columns, the last partial); "exact" — a height that is a whole tile, on the instance's exact width (WX = 1, 2) or just past
# the dispatch edge (WX = 4); "edge" — WX = 2 just past its dispatch edge.
for _k in (2, 3, 4):
    _p = _k - 1  # pads that sum to k - 1 per axis keep the size; the "rows" cases do not
    CASES.update({
        f"tile{_k}_wx1_rows": _tile(2, 101, 63, _k, 1, _k - 2, 0, _k - 1),
        f"tile{_k}_wx1_exact": _tile(1, 96, 64, _k, _p // 2, _p - _p // 2, _p - _p // 2, _p // 2),
        f"tile{_k}_wx2_rows": _tile(2, 53, 127, _k, 0, _k - 1, 2, _k - 1),
        f"tile{_k}_wx2_exact": _tile(1, 48, 128, _k, _p - _p // 2, _p // 2, _p // 2, _p - _p // 2),
        f"tile{_k}_wx2_edge": _tile(1, 48, 65, _k, 1, 0, 0, 1),
        f"tile{_k}_wx4_rows": _tile(2, 29, 293, _k, 2, _k - 1, 1, 0),
        f"tile{_k}_wx4_exact": _tile(1, 24, 129, _k, 0, 1, 1, 1),
    })
CASES.update({
    "up2_wx1_rows": _up2(2, 69, 127, 2, 2, 1, 1),
    "up2_wx1_exact": _up2(1, 64, 128, 2, 1, 2, 1),
    "up2_wx2_rows": _up2(2, 37, 255, 2, 2, 3, 1),
    "up2_wx2_exact": _up2(1, 32, 256, 1, 2, 2, 1),
    "up2_wx2_edge": _up2(1, 32, 129, 2, 2, 1, 2),
    "up2_wx4_rows": _up2(2, 21, 551, 3, 1, 0, 2),
    "up2_wx4_exact": _up2(1, 16, 257, 1, 1, 2, 1),
    "down2_wx1_rows": _down2(2, 37, 63, 2, 1, 1, 1, odd=1),
    "down2_wx1_exact": _down2(1, 32, 64, 1, 1, 1, 1),
    "down2_wx2_rows": _down2(2, 21, 127, 0, 3, 1, 2, odd=1),
    "down2_wx2_exact": _down2(1, 16, 128, 1, 1, 2, 1),
    "down2_wx2_edge": _down2(1, 16, 65, 1, 2, 2, 1, odd=1),
    "down2_wx4_rows": _down2(2, 11, 293, 1, 2, 3, 0, odd=1),
    "down2_wx4_exact": _down2(1, 8, 129, 2, 1, 1, 1),
})

# Geometries maua_upfirdn2d_f32 and its plan refuse with MAUA_EINVAL, each one change away from a good call.
_GOOD = (2, 8, 8, 1, 4, 4, 1, 1, 1, 1, 2, 1, 2, 1)
_FIELDS = ("major", "in_h", "in_w", "minor", "kh", "kw", "up_x", "up_y", "down_x", "down_y")
REFUSED = {"major -1": (-1,) + _GOOD[1:]}
for _i in range(1, 10):
    for _v in (0, -1):
        REFUSED[f"{_FIELDS[_i]} {_v}"] = _GOOD[:_i] + (_v,) + _GOOD[_i + 1:]
REFUSED.update({
    "taps larger than the padded input, both axes": (1, 2, 2, 1, 4, 4, 1, 1, 1, 1, 0, 1, 0, 1),
    "taps larger than the padded input, x only": (1, 8, 2, 1, 4, 4, 1, 1, 1, 1, 0, 1, 2, 1),
    "taps larger than the padded input, y only": (1, 2, 8, 1, 4, 4, 1, 1, 1, 1, 2, 1, 0, 1),
    "crop that leaves no column": (2, 4, 4, 1, 2, 2, 1, 1, 1, 1, -3, -3, 0, 0),
    "negative span under down 2": (1, 2, 2, 1, 4, 4, 1, 1, 2, 2, 0, 1, 0, 1),  # (C division would round it toward one output)
    "negative span under up 2": (1, 1, 1, 1, 4, 4, 2, 2, 1, 1, 0, 1, 0, 0),
})


def _seed(case):
    """The seeding rule of the typed tests (tests/test_native_ops_entries_gpu.py upfirdn_operands)."""
    major, in_h, in_w, minor, kh, kw = case[:6]
    return in_h * 131 + in_w * 7 + kh + minor


def integer_operands(case):
    """x in -8 .. 8, k in -4 .. 4, as fp32: every product and partial sum of the op is an integer far below 2^24, exact in fp32."""
    major, in_h, in_w, minor, kh, kw = case[:6]
    r = np.random.default_rng(_seed(case))
    return r.integers(-8, 9, (major, in_h, in_w, minor)).astype(np.float32), r.integers(-4, 5, (kh, kw)).astype(np.float32)


def real_operands(case):
    """x ~ N(0, 1), k ~ 0.5 N(0, 1), as fp32."""
    major, in_h, in_w, minor, kh, kw = case[:6]
    r = np.random.default_rng(_seed(case))
    return r.standard_normal((major, in_h, in_w, minor)).astype(np.float32), (0.5 * r.standard_normal((kh, kw))).astype(np.float32)


# The 16 instances, as maua_upfirdn2d_plan_instance names them.
TILED = [f"tile{k}.wx{wx}" for k in (2, 3, 4) for wx in (1, 2, 4)] + [f"{fam}.wx{wx}" for fam in ("up2", "down2") for wx in (1, 2, 4)]
INSTANCES = TILED + ["generic"]
# Output widths on which the one-tile-column instances must be seen (their last lane in use) and the two sides of every dispatch edge.
EXACT_WIDTHS = {"tile": (64, 128), "down2": (64, 128), "up2": (128, 256)}
EDGE_WIDTHS = {"tile": (64, 65, 128, 129), "down2": (64, 65, 128, 129), "up2": (128, 129, 256, 257)}
