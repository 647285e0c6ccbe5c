"""CPU: the table of the dedicated convolution kernels (tests/golden/conv_dedicated_instances.json) is consistent, its rounding ratios
are sane, and the bounds of tests/test_conv_dedicated_gpu.py CAN fail: each of six subtle errors, applied to the float32 emulation or
to the fp64 reference chain on the GPU test's own operands, exceeds the test's bound at one element or more on every row of its mode."""
import numpy as np
import pytest
import torch

import conv_ref
import test_conv_dedicated_gpu as t
from conv_ref import U32, conv_and_magnitude
from maua_stylegan2_amd import _lib

ROWS = t.ROWS
NAMES = (["modconv_w2d_kernel<4, 2, 2, false>", "modconv_w2d_kernel<4, 2, 2, true>", "modconv_w2d_kernel<2, 2, 3, false>",
          "modconv_w2d_kernel<2, 2, 3, true>", "modconv_w2dw_kernel<false>", "modconv_w2dw_kernel<true>"]
         + [f"modconv_up2d_kernel<{cc}, 0, {pre}, 32>" for cc in (4, 8) for pre in ("false", "true")]
         + ["modconv_up2d_kernel<8, 2, false, 32>", "modconv_up2d_kernel<8, 2, true, 32>", "modconv_up2d_kernel<8, 0, false, 16>",
            "modconv_sbf16_kernel<-1>", "modconv_sbf16_up_kernel"])
ROWS5 = [r for r in ROWS if r["mode"] == 5]
ROWS6 = [r for r in ROWS if r["mode"] == 6 and r["entry"] == "modconv3x3"]
BLUR = [r for r in ROWS if r["entry"] != "modconv3x3"]


def test_the_table_is_consistent():
    lib = _lib.load()
    keys = [(r["entry"], r["mode"], r["cin"], r["cout"], r["h"], r["w"], r["batch"], r["pre"]) for r in ROWS]
    assert len(set(keys)) == len(keys)
    assert {r["name"] for r in ROWS} == set(NAMES) and len(NAMES) == 6 + 7 + 2
    for r in ROWS:
        shape = (r["cin"], r["cout"], r["h"], r["w"])
        ok = {5: lib.maua_modconv_w2d_ok, 6: lib.maua_modconv_up2d_ok, 7: lib.maua_modconv_sbf16_ok, 8: lib.maua_modconv_sbf16_up_ok}[r["mode"]]
        if r["entry"] == "upconv_blur":
            assert lib.maua_upconv_blur_ok(*shape) == 1, r
        elif r["entry"] == "upconv_blur_lowres":
            assert lib.maua_lowres_ok(*shape, 6) == 1, r
        else:
            assert ok(*shape) == 1, r
    for mode, cin, cout, h, w, fuse_act in t.REFUSED:
        if not fuse_act:
            assert (lib.maua_modconv_w2d_ok if mode == 5 else lib.maua_modconv_up2d_ok)(cin, cout, h, w) == 0
    for shape in [(12, 32, 8, 32), (264, 32, 8, 32), (8, 48, 8, 32), (8, 32, 8, 48), (8, 32, 12, 32)]:
        assert lib.maua_upconv_blur_ok(*shape) == 0


def test_rounding_ratios_are_sane():
    """1 <= R <= 500, the sanity cap of tests/test_weight_pack_gpu.py; measured on these rows: 4.5 .. 29.5."""
    for r in ROWS:
        if r["mode"] in (5, 6):
            assert 1.0 <= r["R"] <= 500.0, r
        else:
            assert r["R"] is None


def _exceeds(row, got, d_null=False):
    _, x, _, s, _, d, wt = t.operands(row, d_null)
    want, mag = conv_and_magnitude(x, s, d, wt, row["mode"] == 6)
    err = (torch.from_numpy(got.astype(np.float64)) - want).abs()
    return bool((err > t.raw_bound(row, mag)).any())


def _emulate(row, styles_shift=False, **kw):
    _, x, _, s, _, d, wt = t.operands(row, False)
    if styles_shift:
        s = torch.roll(s, 1, 0)
    xs = (x * s[:, :, None, None]).numpy().astype(np.float32)
    gain = (np.float32(1.0 / np.sqrt(row["cin"] * 9)) * d.numpy()).astype(np.float32)[:, :, None, None]
    fn = conv_ref.emulate_w2d_f32 if row["mode"] == 5 else conv_ref.emulate_up2d_f32
    return fn(xs, wt[0].numpy(), gain, **kw)


@pytest.mark.parametrize("row", ROWS5 + ROWS6, ids=t._id)
def test_the_unperturbed_emulation_is_inside_the_bound(row):
    assert not _exceeds(row, _emulate(row))


@pytest.mark.parametrize("row", ROWS5, ids=t._id)
def test_a_weight_transform_constant_off_by_2_to_the_minus_10_fails(row):
    """(a) the 1/24 of F(4,3) (row 3 of G: g0 / 24, g1 / 12, g2 / 6 all come from that multiply) off by a relative 2^-10."""
    mats = [m.copy() for m in conv_ref.w2d_matrices()]
    mats[4][3] *= 1.0 + 2.0 ** -10
    assert _exceeds(row, _emulate(row, mats=mats))


@pytest.mark.parametrize("row", ROWS5, ids=t._id)
def test_a_sign_in_the_inverse_transform_along_y_fails(row):
    """(b) the sign of one row of the F(2,3) inverse transform along y."""
    mats = [m.copy() for m in conv_ref.w2d_matrices()]
    mats[2][1] *= -1.0
    assert _exceeds(row, _emulate(row, mats=mats))


@pytest.mark.parametrize("pos", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("row", ROWS6, ids=t._id)
def test_a_dropped_product_fails(row, pos):
    """(c) one of mode 6's 25 products dropped at one of the four odd-odd positions."""
    assert _exceeds(row, _emulate(row, drop=pos))


@pytest.mark.parametrize("row", [r for r in ROWS5 + ROWS6 if r["batch"] > 1], ids=t._id)
def test_the_styles_of_the_previous_image_fail(row):
    """(d) image b convolved with the styles of image b - 1."""
    assert _exceeds(row, _emulate(row, styles_shift=True))


@pytest.mark.parametrize("row", BLUR, ids=t._id)
def test_swapped_or_unflipped_blur_taps_fail(row):
    """(e) the blur's row and column factors swapped, (f) the taps not flipped: the fp64 chain with either error against the right one."""
    taps = conv_ref.asymmetric_taps()
    _, x, _, s, _, d, wt = t.operands(row, False)
    conv = conv_and_magnitude(x, s, d, wt, True)
    want, p = conv_ref.upconv_styled64(x, s, d, wt, taps, conv=conv)
    bound = t.blur_bound(row, taps, p, splits=4 if row["entry"] == "upconv_blur_lowres" else 0)
    for wrong in (taps.t().contiguous(), torch.flip(taps, [0, 1])):
        got, _ = conv_ref.upconv_styled64(x, s, d, wt, wrong, conv=conv)
        assert bool(((got - want).abs() > bound).any())
    same, _ = conv_ref.upconv_styled64(x, s, d, wt, taps.clone(), conv=conv)
    assert bool(((same - want).abs() <= bound).all())
