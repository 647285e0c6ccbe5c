"""GPU: maua_torgb_f32 (general form, csrc/torgb.hip) and maua_blur_noise_act_f32 (csrc/upfirdn2d.hip, fir_tile_kernel<.., TAIL = true>)
through the C ABI against float64 numpy restatements of the formulas in include/maua_hip.h.

ToRGB.  want[b,c,Y,X] = sum_i (wscale w[c,i] s[b,i]) x[b,i,Y,X] + bias[c] + up2(skip)[b,c,Y,X]; up2 = the zero-stuffed canvas, pad (2, 1),
true convolution with k4.  Elementwise bound  |got - want| <= (cin + 80) * 2^-24 * A,  A = the same expression with every product replaced
by its absolute value: a term passes through at most cin / ks fused multiply-adds, ks - 1 combine adds (ks <= 64), two roundings of the
modulated weight, one bias add and five skip operations (four multiply-adds and the add of their sum).  One term is A / cin on average,
so a dropped channel shows for any cin below about 4000.

Blur tail.  y = lrelu_0.2(upfirdn2d(x, k, pad = (pad0, pad1)) * gain[b,c] + noise_w * noise[b or 0] + bias[c]) * sqrt(2) * post_s[b,c].
Bound  (kh * kw + 8) * 2^-24 * sqrt(2) * |post| * (|gain| sum |k||x| + |noise_w noise| + |bias|):  kh * kw tap operations, and eight
roundings in the tail (sqrt(2) folded into gain, noise weight and bias: three; two multiply-adds; the 0.2 constant and its product; the
post multiply).  The leaky ReLU is 1-Lipschitz, so the bound holds across the kink.

Every buffer is a tests/redzone.py window; the reference and bound functions are checked on the CPU in tests/test_image_tail_refs_host.py.
Worst error / bound ratios are printed per case ([torgb], [blur_tail])."""
import ctypes

import numpy as np
import pytest
import torch

from maua_stylegan2_amd import _lib
from redzone import Guard

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

U = 2.0 ** -24
EINVAL, ENOSYS = -22, -38
SQRT2 = np.sqrt(2.0)

# ---------------------------------------------------------------------------------------------------------------- ToRGB
# (batch, cin, h, w, bias given, styles as a window of a wider table, taps)
TORGB_CASES = [
    (1, 8, 32, 32, True, False, "gen"),
    (1, 9, 32, 32, False, True, "rand"),
    (1, 17, 16, 16, True, True, "gen"),
    (1, 40, 16, 16, True, False, "rand"),
    (3, 72, 8, 12, False, False, "gen"),
    (1, 100, 2, 12, True, True, "rand"),
    (8, 512, 4, 4, True, False, "gen"),
    (1, 600, 8, 8, True, True, "rand"),
    (1, 9, 9, 9, True, False, "gen"),
    (2, 37, 5, 7, False, True, "gen"),
    (2, 130, 6, 6, True, True, "rand"),
    (1, 12, 2, 6, False, False, "rand"),
    (2, 3, 2, 2, True, True, "gen"),
    (1, 1, 1, 1, True, False, "gen"),
]
TORGB_SPLITS = [(4, 256, 1), (4, 128, 2), (4, 64, 4), (4, 32, 8), (4, 16, 16), (4, 8, 32), (4, 4, 64), (4, 4, 64), (1, 128, 2), (1, 32, 8),
                (1, 16, 16), (1, 16, 16), (1, 4, 64), (1, 4, 64)]
TORGB_LDS_MAX_CIN_SPLIT = 4437  # pad4(3 cin) + 3072 floats <= 16384 floats


def torgb_split(batch, cin, h, w):
    """Mirror of the launcher's split loop (csrc/torgb.hip): (vec, pixel groups per workgroup, channel slices).  Coverage only."""
    vec = 4 if w % 4 == 0 else 1
    quads = h * w // vec
    qpb, ks_log2 = 256, 0
    while qpb > 4 and (qpb // 2 >= quads or (-(-quads // qpb) * batch < 512 and (cin >> ks_log2) > 8)):
        qpb >>= 1
        ks_log2 += 1
    return vec, qpb, 1 << ks_log2


def torgb_lds_bytes(batch, cin, h, w):
    _, qpb, ks = torgb_split(batch, cin, h, w)
    return 4 * (((3 * cin + 3) & ~3) + (ks * qpb * 12 if ks > 1 else 0))


def generator_k4():
    """The generator's Upsample taps: outer([1, 3, 3, 1]) normalised, times factor^2 (models/stylegan2.py make_kernel)."""
    k = np.outer([1.0, 3.0, 3.0, 1.0], [1.0, 3.0, 3.0, 1.0])
    return (k / k.sum() * 4).astype(np.float32)


def torgb_operands(case):
    """Seeded fp32 operands of one case; the skip is present wherever h and w are even."""
    batch, cin, h, w, with_bias, wide_s, taps = case
    r = np.random.default_rng(1000 * cin + 10 * h + w + batch)
    f = lambda *s: r.standard_normal(s).astype(np.float32)  # noqa: E731
    s_stride, s_col = (cin + 5, 3) if wide_s else (cin, 0)
    table = f(batch * s_stride) + np.float32(1)  # (a [batch, s_stride] table; this layer's styles are columns s_col .. s_col + cin of it)
    ops = dict(x=f(batch, cin, h, w), w=f(3, cin), table=table, s_col=s_col, s_stride=s_stride,
               bias=0.3 * f(3) if with_bias else None, skip=None, k4=None, wscale=np.float32(1.0 / np.sqrt(cin)))
    ops["s"] = np.stack([table[s_col + b * s_stride: s_col + b * s_stride + cin] for b in range(batch)])
    if h % 2 == 0 and w % 2 == 0:
        ops["skip"] = f(batch, 3, h // 2, w // 2)
        ops["k4"] = generator_k4() if taps == "gen" else 0.5 * f(4, 4)
    return ops


def up2_ref(skip, k4):
    """Upsample of [B, 3, sh, sw] in float64: zero-stuff by 2, pad (2, 1), true convolution with the 4 x 4 taps."""
    b, c, sh, sw = skip.shape
    canvas = np.zeros((b, c, 2 * sh + 3, 2 * sw + 3))
    canvas[:, :, 2:2 + 2 * sh:2, 2:2 + 2 * sw:2] = skip
    kf = np.asarray(k4, np.float64)[::-1, ::-1]
    out = np.zeros((b, c, 2 * sh, 2 * sw))
    for i in range(4):
        for j in range(4):
            out += kf[i, j] * canvas[:, :, i:i + 2 * sh, j:j + 2 * sw]
    return out


def torgb_ref(ops):
    """(want, bound) in float64, elementwise."""
    f8 = lambda a: np.asarray(a, np.float64)  # noqa: E731
    x, w, s = f8(ops["x"]), f8(ops["w"]), f8(ops["s"])
    cin = x.shape[1]
    wm = float(ops["wscale"]) * w[None] * s[:, None, :]  # [B, 3, cin]
    want = np.einsum("bci,bihw->bchw", wm, x)
    mag = np.einsum("bci,bihw->bchw", np.abs(wm), np.abs(x))
    if ops["bias"] is not None:
        want = want + f8(ops["bias"])[None, :, None, None]
        mag = mag + np.abs(f8(ops["bias"]))[None, :, None, None]
    if ops["skip"] is not None:
        want = want + up2_ref(f8(ops["skip"]), ops["k4"])
        mag = mag + up2_ref(np.abs(f8(ops["skip"])), np.abs(ops["k4"]))
    return want, (cin + 80) * U * mag


def _torgb_launch(gpu, ops, shape, **override):
    """One guarded call; returns (rc, guard, y).  ``override``: w / s / k4 / skip = None (a NULL pointer), sizes."""
    lib = _lib.load()
    batch, cin, h, w = shape
    g = Guard(gpu)
    x = g.inp(ops["x"], "x")
    wt = g.inp(ops["w"], "w")
    table = g.inp(ops["table"], "s")
    bias = g.inp(ops["bias"], "bias") if ops["bias"] is not None else None
    skip = g.inp(ops["skip"], "skip") if ops["skip"] is not None else None
    k4 = g.inp(ops["k4"], "k4") if ops["k4"] is not None else None
    y = g.out((batch, 3, h, w), "y")
    p = dict(x=x.data_ptr(), w=wt.data_ptr(), s=table.data_ptr() + 4 * ops["s_col"], bias=_lib.ptr(bias), skip=_lib.ptr(skip), k4=_lib.ptr(k4),
             y=y.data_ptr(), batch=batch, cin=cin, h=h, wdt=w)
    p.update(override)
    rc = lib.maua_torgb_f32(p["x"], p["w"], p["s"], ops["s_stride"], p["bias"], p["skip"], p["k4"], p["y"], p["batch"], p["cin"], p["h"], p["wdt"],
                            float(ops["wscale"]), _lib.stream_ptr(gpu))
    return rc, g, y


def _ratio(got, want, bound, label, tag):
    err = np.abs(got.astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"[{tag}] {label}: worst error / bound {worst:.4f} (max error {float(err.max()) if err.size else 0.0:.3e})")
    assert worst <= 1.0, (label, worst)
    return worst


def test_torgb_case_list_reaches_every_split():
    """The split the launcher takes for every listed shape is the one the table names, and the list reaches ks = 1 .. 64 at both widths
    of the pixel group where the shape allows it."""
    got = [torgb_split(*c[:4]) for c in TORGB_CASES]
    assert got == TORGB_SPLITS, got
    assert {ks for _, _, ks in got} == {1, 2, 4, 8, 16, 32, 64}
    assert {v for v, _, _ in got} == {1, 4}
    assert any(c[4] for c in TORGB_CASES) and any(not c[4] for c in TORGB_CASES)
    assert any(c[5] for c in TORGB_CASES) and any(not c[5] for c in TORGB_CASES)
    for vec in (1, 4):  # both tap sets, with a skip, at both widths
        assert {c[6] for c in TORGB_CASES if c[2] % 2 == 0 and c[3] % 2 == 0 and (4 if c[3] % 4 == 0 else 1) == vec} == {"gen", "rand"}


@pytest.mark.parametrize("case", TORGB_CASES, ids=lambda c: "x".join(map(str, c[:4])))
def test_torgb_general_form_against_float64(gpu, case):
    ops = torgb_operands(case)
    rc, g, y = _torgb_launch(gpu, ops, case[:4])
    assert rc == 0, rc
    g.check(written=("y",))
    want, bound = torgb_ref(ops)
    _ratio(y.cpu().numpy(), want, bound, f"{case[:4]} split {torgb_split(*case[:4])} skip {ops['skip'] is not None}", "torgb")


def test_torgb_refusals_leave_the_output_untouched(gpu):
    shape = (2, 12, 4, 4)
    ops = torgb_operands(shape + (True, False, "gen"))
    odd_h = torgb_operands((1, 5, 3, 4, True, False, "gen"))
    odd_h["skip"], odd_h["k4"] = np.zeros((1, 3, 1, 2), np.float32), generator_k4()
    odd_w = torgb_operands((1, 5, 4, 3, True, False, "gen"))
    odd_w["skip"], odd_w["k4"] = np.zeros((1, 3, 2, 1), np.float32), generator_k4()
    refused = [(ops, shape, dict(s=None)), (ops, shape, dict(w=None)), (odd_h, (1, 5, 3, 4), {}), (odd_w, (1, 5, 4, 3), {}),
               (ops, shape, dict(k4=None)), (ops, shape, dict(x=None)), (ops, shape, dict(y=None))]
    refused += [(ops, shape, {name: v}) for name in ("batch", "cin", "h", "wdt") for v in (0, -1)]
    for o, shp, override in refused:
        rc, g, _ = _torgb_launch(gpu, o, shp, **override)
        assert rc == EINVAL, (shp, override, rc)
        assert g.untouched("y"), (shp, override)
        g.check()


def test_torgb_lds_limit(gpu):
    """Dynamic LDS of the general form is pad4(3 cin) + 3072 floats once the channel loop is split: the largest cin inside 64 KB is served
    and compared, the next one is refused with MAUA_ENOSYS before any launch."""
    ok, over = TORGB_LDS_MAX_CIN_SPLIT, TORGB_LDS_MAX_CIN_SPLIT + 1
    assert torgb_split(1, ok, 2, 2)[2] > 1 and torgb_lds_bytes(1, ok, 2, 2) == 65536 and torgb_lds_bytes(1, over, 2, 2) > 65536
    case = (1, ok, 2, 2, True, False, "gen")
    ops = torgb_operands(case)
    rc, g, y = _torgb_launch(gpu, ops, case[:4])
    assert rc == 0, rc
    g.check(written=("y",))
    want, bound = torgb_ref(ops)
    _ratio(y.cpu().numpy(), want, bound, f"cin {ok} (64 KB of LDS)", "torgb")
    case = (1, over, 2, 2, True, False, "gen")
    rc, g, y = _torgb_launch(gpu, torgb_operands(case), case[:4])
    assert rc == ENOSYS, rc
    assert g.untouched("y")
    g.check()


# ---------------------------------------------------------------------------------------------------------------- blur tail
# operand combinations: (gain, noise: None / "shared" (stride 0) / "per_sample", bias, post_s with a stride wider than channels)
BLUR_COMBOS = {
    "all": (True, "per_sample", True, True),
    "no_gain_shared_noise": (False, "shared", True, False),
    "no_noise_no_bias": (True, None, False, True),
    "plain": (True, "per_sample", True, False),
}
# (batch, channels, in_h, in_w, k, pad0, pad1, combos)
BLUR_CASES = [
    (2, 3, 9, 9, 4, 1, 1, ("no_gain_shared_noise",)),
    (1, 2, 70, 100, 3, 1, 1, ("all", "no_gain_shared_noise", "no_noise_no_bias")),
    (2, 2, 20, 200, 2, 1, 0, ("all", "no_gain_shared_noise")),
    (1, 1, 17, 300, 4, 2, 2, ("no_noise_no_bias",)),
    (2, 3, 515, 66, 4, 1, 1, ("all",)),
    (1, 2, 40, 40, 4, -1, 0, ("plain",)),
    (1, 1, 5, 5, 4, 5, 2, ("no_noise_no_bias",)),
    (1, 1, 1, 1, 2, 1, 0, ("no_noise_no_bias",)),
]
BLUR_RUNS = [c[:7] + (combo,) for c in BLUR_CASES for combo in c[7]]


def blur_operands(run):
    batch, channels, in_h, in_w, k, pad0, pad1, combo = run
    with_gain, noise_kind, with_bias, with_post = BLUR_COMBOS[combo]
    out_h, out_w = in_h + pad0 + pad1 - k + 1, in_w + pad0 + pad1 - k + 1
    r = np.random.default_rng(100 * in_h + in_w + 7 * k + len(combo))
    f = lambda *s: r.standard_normal(s).astype(np.float32)  # noqa: E731
    ops = dict(x=f(batch, channels, in_h, in_w), k=0.4 * f(k, k), pad0=pad0, pad1=pad1, gain=None, noise=None, noise_w=0.8 * f(1), bias=None,
               post_table=None, post=None, post_stride=0, out=(out_h, out_w))
    if with_gain:
        ops["gain"] = f(batch, channels) + np.float32(1.5)
    if noise_kind:
        ops["noise"] = f(batch if noise_kind == "per_sample" else 1, out_h, out_w)
    if with_bias:
        ops["bias"] = 0.5 * f(channels)
    if with_post:
        ops["post_stride"] = channels + 3
        ops["post_table"] = f(batch, channels + 3) + np.float32(1)
        ops["post"] = ops["post_table"][:, :channels]
    return ops


def pad_crop(a, p0, p1, axis):
    """Zero padding of ``a`` along ``axis`` by p0 in front and p1 behind; a negative pad crops."""
    a = np.moveaxis(a, axis, 0)
    if p0 < 0:
        a, p0 = a[-p0:], 0
    if p1 < 0:
        a, p1 = a[:max(a.shape[0] + p1, 0)], 0
    z = lambda n: np.zeros((n,) + a.shape[1:], a.dtype)  # noqa: E731
    return np.moveaxis(np.concatenate([z(p0), a, z(p1)]), 0, axis)


def fir_ref(x, k, pad0, pad1):
    """upfirdn2d with up = down = 1 on the last two axes in float64: pad or crop, correlate with the flipped taps."""
    kh, kw = k.shape
    c = pad_crop(pad_crop(x, pad0, pad1, -2), pad0, pad1, -1)
    oh, ow = c.shape[-2] - kh + 1, c.shape[-1] - kw + 1
    kf = k[::-1, ::-1]
    out = np.zeros(c.shape[:-2] + (oh, ow))
    for i in range(kh):
        for j in range(kw):
            out += kf[i, j] * c[..., i:i + oh, j:j + ow]
    return out


def blur_tail_ref(ops):
    """(want, bound) in float64, elementwise."""
    f8 = lambda a: np.asarray(a, np.float64)  # noqa: E731
    x, k = f8(ops["x"]), f8(ops["k"])
    kh, kw = k.shape
    pre = fir_ref(x, k, ops["pad0"], ops["pad1"])
    mag = fir_ref(np.abs(x), np.abs(k), ops["pad0"], ops["pad1"])
    if ops["gain"] is not None:
        pre = pre * f8(ops["gain"])[:, :, None, None]
        mag = mag * np.abs(f8(ops["gain"]))[:, :, None, None]
    if ops["noise"] is not None:
        term = float(ops["noise_w"][0]) * f8(ops["noise"])[:, None]  # [B or 1, 1, oh, ow]
        pre = pre + term
        mag = mag + np.abs(term)
    if ops["bias"] is not None:
        pre = pre + f8(ops["bias"])[None, :, None, None]
        mag = mag + np.abs(f8(ops["bias"]))[None, :, None, None]
    post = f8(ops["post"])[:, :, None, None] if ops["post"] is not None else 1.0
    want = np.where(pre > 0, pre, 0.2 * pre) * SQRT2 * post
    return want, (kh * kw + 8) * U * SQRT2 * np.abs(post) * mag


def _blur_launch(gpu, ops, shape, kh=None, kw=None, **override):
    lib = _lib.load()
    batch, channels, in_h, in_w = shape
    k = ops["k"]
    g = Guard(gpu)
    x = g.inp(ops["x"], "x")
    kt = g.inp(k, "k")
    gain = g.inp(ops["gain"], "gain") if ops["gain"] is not None else None
    noise = g.inp(ops["noise"], "noise") if ops["noise"] is not None else None
    nw = g.inp(ops["noise_w"], "noise_w")
    bias = g.inp(ops["bias"], "bias") if ops["bias"] is not None else None
    post = g.inp(ops["post_table"], "post_s") if ops["post_table"] is not None else None
    out_h, out_w = ops["out"]
    y = g.out((batch, channels, max(out_h, 1), max(out_w, 1)), "y")
    nstride = out_h * out_w if noise is not None and ops["noise"].shape[0] > 1 else 0
    p = dict(x=x.data_ptr(), k=kt.data_ptr(), y=y.data_ptr(), batch=batch, channels=channels, in_h=in_h, in_w=in_w, noise=_lib.ptr(noise),
             noise_w=nw.data_ptr(), src=None, noise_slot=0)
    p.update(override)
    rc = lib.maua_blur_noise_act_f32(p["x"], p["k"], p["y"], p["batch"], p["channels"], p["in_h"], p["in_w"], kh or k.shape[0], kw or k.shape[1],
                                     ops["pad0"], ops["pad1"], _lib.ptr(gain), p["noise"], nstride, p["noise_w"], _lib.ptr(bias), p["src"],
                                     p["noise_slot"], _lib.ptr(post), ops["post_stride"], _lib.stream_ptr(gpu))
    return rc, g, y


def test_blur_tail_run_list_rotates_every_operand_over_every_tap_size():
    for k in (2, 3, 4):
        combos = [BLUR_COMBOS[r[7]] for r in BLUR_RUNS if r[4] == k]
        assert any(not c[0] for c in combos), k                 # gain NULL
        assert any(c[1] is None for c in combos), k             # noise NULL
        assert any(c[1] == "shared" for c in combos), k         # noise_batch_stride == 0
        assert any(not c[2] for c in combos), k                 # bias NULL
        assert any(c[3] for c in combos), k                     # post_s, post_stride > channels
    big = [r for r in BLUR_RUNS if r[2] + r[5] + r[6] - r[4] + 1 > 512]
    assert big and all(BLUR_COMBOS[r[7]][1] == "per_sample" and r[0] > 1 and r[1] > 1 for r in big)


@pytest.mark.parametrize("run", BLUR_RUNS, ids=lambda r: "-".join(map(str, r)))
def test_blur_tail_against_float64(gpu, run):
    ops = blur_operands(run)
    rc, g, y = _blur_launch(gpu, ops, run[:4])
    assert rc == 0, rc
    g.check(written=("y",))
    want, bound = blur_tail_ref(ops)
    assert y.shape == want.shape
    _ratio(y.cpu().numpy(), want, bound, f"{run}", "blur_tail")


def test_blur_tail_refusals_leave_the_output_untouched(gpu):
    shape = (1, 2, 12, 12)
    ops = blur_operands(shape + (4, 1, 1, "all"))
    src = torch.zeros(ctypes.sizeof(_lib.FrameSource), dtype=torch.uint8, device=gpu)  # (refused before it is read)
    cases = [(dict(kh=4, kw=3), ENOSYS), (dict(kh=3, kw=4), ENOSYS), (dict(kh=1, kw=1), ENOSYS), (dict(kh=5, kw=5), ENOSYS),
             (dict(noise_w=None), EINVAL), (dict(src=src.data_ptr(), noise_slot=-1), EINVAL),
             (dict(src=src.data_ptr(), noise_slot=_lib.MAX_NOISE_SLOTS), EINVAL), (dict(src=src.data_ptr(), noise_w=None), EINVAL),
             (dict(x=None), EINVAL), (dict(k=None), EINVAL), (dict(y=None), EINVAL)]
    cases += [({name: v}, EINVAL) for name in ("batch", "channels", "in_h", "in_w") for v in (0, -1)]
    for override, code in cases:
        rc, g, _ = _blur_launch(gpu, ops, shape, **override)
        assert rc == code, (override, rc)
        assert g.untouched("y"), override
        g.check()
    empty = blur_operands((1, 1, 2, 2, 4, 0, 0, "no_noise_no_bias"))  # 2 + 0 + 0 - 4 + 1 < 1 rows
    rc, g, _ = _blur_launch(gpu, empty, (1, 1, 2, 2))
    assert rc == EINVAL and g.untouched("y")
    g.check()
