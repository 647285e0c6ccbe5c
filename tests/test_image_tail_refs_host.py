"""Host: the references and bounds of tests/test_image_tail_gpu.py, test_delivery_gpu.py and test_native_ops_entries_gpu.py, checked on the
CPU against numpy fp32 stand-ins of each kernel's arithmetic — serial fp32 accumulation in the slice order of the launcher's split for
ToRGB, tap-ordered fp32 accumulation for the blur tail and the typed upfirdn2d, the integer twin for the resize, a scalar loop for
fused_bias_act.  Every stand-in passes its bound on every listed case, and a stand-in with one deliberate defect (a channel dropped,
taps not flipped, a clamp at the frame edge, a bias index without the modulo) misses it: the bounds are neither unsatisfiable nor slack."""
import numpy as np
import pytest

import test_delivery_gpu as dl
import test_image_tail_gpu as it
import test_native_ops_entries_gpu as no

F32, F64 = np.float32, np.float64
SQRT2_F32 = F32(np.sqrt(2.0))


def fma32(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in fp64; the sum is rounded there and once more to fp32."""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def worst_ratio(got, want, bound):
    err = np.abs(np.asarray(got, F64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max())


# ---------------------------------------------------------------------------------------------------------------- ToRGB
def torgb_standin(ops, shape, drop=None):
    batch, cin, h, w = shape
    _, _, ks = it.torgb_split(*shape)
    x = ops["x"]
    wm = ((ops["wscale"] * ops["w"]).astype(F32)[None] * ops["s"][:, None, :]).astype(F32)  # [B, 3, cin]
    per = -(-cin // ks)
    total = None
    for sl in range(ks):
        acc = np.zeros((batch, 3, h, w), F32)
        for i in range(sl * per, min(cin, sl * per + per)):
            if i != drop:
                acc = fma32(wm[:, :, i, None, None], x[:, None, i], acc)
        total = acc if total is None else (total + acc).astype(F32)
    if ops["bias"] is not None:
        total = (total + ops["bias"].astype(F32)[None, :, None, None]).astype(F32)
    if ops["skip"] is not None:
        sh, sw = h // 2, w // 2
        canvas = np.zeros((batch, 3, h + 3, w + 3), F32)
        canvas[:, :, 2:2 + 2 * sh:2, 2:2 + 2 * sw:2] = ops["skip"]
        a = np.zeros((batch, 3, h, w), F32)
        for i in range(4):
            for j in range(4):  # (a tap on a stuffed zero adds nothing: the kernel skips it)
                a = fma32(ops["k4"][3 - i, 3 - j], canvas[:, :, i:i + h, j:j + w], a)
        total = (total + a).astype(F32)
    return total


def test_torgb_case_list_and_split_mirror():
    got = [it.torgb_split(*c[:4]) for c in it.TORGB_CASES]
    assert got == it.TORGB_SPLITS
    assert {ks for _, _, ks in got} == {1, 2, 4, 8, 16, 32, 64} and {v for v, _, _ in got} == {1, 4}
    ok = it.TORGB_LDS_MAX_CIN_SPLIT
    assert it.torgb_lds_bytes(1, ok, 2, 2) <= 65536 < it.torgb_lds_bytes(1, ok + 1, 2, 2)
    # (1, 600, 8, 8): 16 pixel groups in four workgroups; slices of ceil(600 / 64) = 10 channels (one 8-wide trip and a remainder of two),
    # the last four of the 64 slices empty.  (2, 3, 2, 2): one channel per slice, 61 slices empty
    vec, qpb, ks = it.torgb_split(1, 600, 8, 8)
    assert -(-(8 * 8 // vec) // qpb) == 4 and -(-600 // ks) == 10 and 60 * 10 == 600
    assert it.torgb_split(2, 3, 2, 2)[2] == 64


@pytest.mark.parametrize("case", it.TORGB_CASES, ids=lambda c: "x".join(map(str, c[:4])))
def test_torgb_bound_holds_for_fp32_and_catches_a_dropped_channel(case):
    ops = it.torgb_operands(case)
    want, bound = it.torgb_ref(ops)
    good = worst_ratio(torgb_standin(ops, case[:4]), want, bound)
    dropped = worst_ratio(torgb_standin(ops, case[:4], drop=case[1] // 2), want, bound)
    print(f"[torgb host] {case[:4]}: fp32 stand-in {good:.4f} of the bound, one channel dropped {dropped:.1f}x")
    assert good <= 1.0, (case, good)
    assert dropped > 1.0, (case, dropped)


# ---------------------------------------------------------------------------------------------------------------- blur tail
def blur_standin(ops, flip=True):
    x, k = ops["x"], ops["k"]
    kh, kw = k.shape
    c = it.pad_crop(it.pad_crop(x, ops["pad0"], ops["pad1"], -2), ops["pad0"], ops["pad1"], -1)
    oh, ow = ops["out"]
    kf = k[::-1, ::-1] if flip else k
    acc = None
    for i in range(kh):
        for j in range(kw):
            win = c[..., i:i + oh, j:j + ow]
            acc = (kf[i, j] * win).astype(F32) if acc is None else fma32(kf[i, j], win, acc)
    g = (SQRT2_F32 * ops["gain"]).astype(F32)[:, :, None, None] if ops["gain"] is not None else SQRT2_F32
    bs = (ops["bias"] * SQRT2_F32).astype(F32)[None, :, None, None] if ops["bias"] is not None else F32(0)
    inner = bs
    if ops["noise"] is not None:
        inner = fma32(F32(ops["noise_w"][0] * SQRT2_F32), ops["noise"][:, None], bs)
    t = fma32(acc, g, inner)
    val = np.maximum(t, (F32(0.2) * t).astype(F32))
    if ops["post"] is not None:
        val = (val * ops["post"][:, :, None, None]).astype(F32)
    return val


def test_blur_tail_run_list_rotation():
    it.test_blur_tail_run_list_rotates_every_operand_over_every_tap_size()


@pytest.mark.parametrize("run", it.BLUR_RUNS, ids=lambda r: "-".join(map(str, r)))
def test_blur_tail_bound_holds_for_fp32_and_catches_unflipped_taps(run):
    ops = it.blur_operands(run)
    want, bound = it.blur_tail_ref(ops)
    assert want.shape == run[:2] + ops["out"]
    good = worst_ratio(blur_standin(ops), want, bound)
    unflipped = worst_ratio(blur_standin(ops, flip=False), want, bound)
    print(f"[blur_tail host] {run}: fp32 stand-in {good:.4f} of the bound, taps not flipped {unflipped:.1f}x")
    assert good <= 1.0, (run, good)
    assert unflipped > 1.0, (run, unflipped)


# ---------------------------------------------------------------------------------------------------------------- delivery
def test_frames_statement_on_the_boundaries():
    """The fp32 statement itself: monotone in x, 0 and 255 at the clamp's edges and beyond, and every byte value reached."""
    vals = np.sort(dl.adversarial_values())
    q = dl.frames_ref(vals.reshape(1, 1, 1, -1).repeat(3, axis=1))[0, 0, :, 0]
    assert (np.diff(q.astype(np.int64)) >= 0).all() and set(q.tolist()) == set(range(256))
    assert q[0] == 0 and q[-1] == 255 and q[vals == F32(-1)].max() == 0 and q[vals == F32(1)].min() == 255
    x, idx = dl.frames_input(1, 80, 80)  # 6400 >= 4 * 1291 pixels: every value in every lane of a 4-pixel group
    seen = np.zeros((vals.size, 4), bool)
    seen[idx[0, 0].reshape(-1), np.arange(6400) % 4] = True
    assert seen.all()
    nan = dl.frames_ref(np.full((1, 3, 1, 1), np.nan, F32))
    assert (nan == 0).all()


def resize_clamped_to_the_frame(frame, x0, y0, cw, ch, ow, oh):
    """The twin with its one defect: taps clamped to the frame instead of the crop."""
    bits = 22

    def taps(n_in, n_out, off, n_frame):
        o = np.arange(n_out, dtype=np.int64)
        num, den = (2 * o + 1) * n_in - n_out, 2 * n_out
        i0 = np.floor_divide(num, den)
        f = (num - i0 * den).astype(F64) / den
        k1 = np.floor(0.5 + f * (1 << bits)).astype(np.int64)
        k0 = np.floor(0.5 + (1 - f) * (1 << bits)).astype(np.int64)
        return np.clip(off + i0, 0, n_frame - 1), np.clip(off + i0 + 1, 0, n_frame - 1), k0, k1

    f = frame.astype(np.int64)
    xa, xb, kx0, kx1 = taps(cw, ow, x0, frame.shape[1])
    ya, yb, ky0, ky1 = taps(ch, oh, y0, frame.shape[0])
    h = np.clip((kx0[None, :, None] * f[:, xa] + kx1[None, :, None] * f[:, xb] + (1 << (bits - 1))) >> bits, 0, 255)
    v = np.clip((ky0[:, None, None] * h[ya] + ky1[:, None, None] * h[yb] + (1 << (bits - 1))) >> bits, 0, 255)
    return v.astype(np.uint8)


def test_resize_twin_is_pil_on_the_whole_list_and_the_decoy_catches_a_frame_clamp():
    """The twin equals PIL on every combination (resize_ref asserts it where PIL imports).  A tap clamped to the frame reads a decoy pixel
    at least 128 away from its neighbour in the crop, with a weight of at least 0.5 / (n + 1) >= 1 / 196 on the last output column or row
    of an up-scaled axis: more than half a grey level, so every case that up-scales an axis shows it."""
    assert len(dl.RESIZE_CASES) == 1236
    for n, (cw, ch, ow, oh) in enumerate(dl.RESIZE_CASES):
        frame = dl.decoy_frame(1, cw, ch, n)
        want = dl.resize_ref(frame, cw, ch, ow, oh)[0]
        assert want.shape == (oh, ow, 3)
        bad = resize_clamped_to_the_frame(frame[0], dl.X0, dl.Y0, cw, ch, ow, oh)
        if ow > cw or oh > ch:
            assert not np.array_equal(bad, want), (cw, ch, ow, oh)
        else:
            assert np.array_equal(bad, want)  # (the identity reads no neighbour)


# ---------------------------------------------------------------------------------------------------------------- native ops
def bias_act_loop(x, b, ref, size_b, step_b, act, grad, alpha, scale, out_type, arith, modulo=True):
    """The kernel's scalar path, one element at a time."""
    out = np.zeros(x.size, out_type)
    a, s = arith(F32(alpha)), arith(F32(scale))
    table = None if b is None or size_b <= 0 else np.concatenate([b.astype(arith), np.full(64, 9.0, arith)])  # (what lies behind the table)
    for i in range(x.size):
        v = arith(x[i])
        if table is not None:
            v = arith(v + table[(i // step_b) % size_b if modulo else i // step_b])
        r = arith(ref[i]) if ref is not None else arith(0)
        code = act * 10 + grad
        if code in (12, 32):
            o = arith(0)
        elif code == 30:
            o = v if v > 0 else arith(v * a)
        elif code == 31:
            o = v if r > 0 else arith(v * a)
        else:
            o = v
        out[i] = np.float16(np.float64(o) * np.float64(s)) if out_type == np.float16 else out_type(arith(o * s))
    return out


@pytest.mark.parametrize("suffix", ["f32", "f16", "f64"])
def test_bias_act_model_is_the_scalar_loop_and_catches_a_missing_modulo(suffix):
    out_type, arith, _ = no.TYPES[suffix]
    for name in ("vector_bias_wraps", "size_x_not_4", "step_b_not_4", "no_ref", "no_bias", "size_b_zero"):
        case = no.BIAS_ACT_CASES[name]
        x, b, ref = no.bias_act_operands(case, out_type)
        for act, grad in no.CODES:
            args = (x, b, ref, case["size_b"], case["step_b"], act, grad, 0.2, 1.4142135381698608, out_type, arith)
            model = no.bias_act_model(*args)
            assert np.array_equal(no._bits(model), no._bits(bias_act_loop(*args))), (suffix, name, act, grad)
            if name == "vector_bias_wraps" and act * 10 + grad not in (12, 32):
                assert not np.array_equal(no._bits(model), no._bits(bias_act_loop(*args, modulo=False)))
    for name in ("vector_bias_wraps", "second_trip_vector", "second_trip_scalar"):  # the index wraps mid-tensor
        case = no.BIAS_ACT_CASES[name]
        assert case["n"] // case["step_b"] > case["size_b"] and (case["n"] // case["step_b"]) % case["size_b"]


def upfirdn_standin(x, k, params, suffix, flip=True):
    """Tap-ordered accumulation in the accumulator type (fp32 for half), one rounding to the tensor type."""
    up_x, up_y, down_x, down_y, px0, px1, py0, py1 = params
    arith = F32 if suffix == "f16" else F64
    major, in_h, in_w, minor = x.shape
    kh, kw = k.shape
    canvas = np.zeros((major, in_h * up_y, in_w * up_x, minor), arith)
    canvas[:, ::up_y, ::up_x] = x.astype(arith)
    canvas = no.pad_crop(no.pad_crop(canvas, py0, py1, 1), px0, px1, 2)
    oh, ow = canvas.shape[1] - kh + 1, canvas.shape[2] - kw + 1
    kf = (k[::-1, ::-1] if flip else k).astype(arith)
    acc = np.zeros((major, oh, ow, minor), arith)
    for i in range(kh):
        for j in range(kw):
            acc = (acc + (kf[i, j] * canvas[:, i:i + oh, j:j + ow]).astype(arith)).astype(arith)
    return acc[:, ::down_y, ::down_x].astype(x.dtype)


@pytest.mark.parametrize("name", list(no.UPFIRDN_CASES))
@pytest.mark.parametrize("suffix", ["f16", "f64"])
def test_upfirdn_typed_bound_holds_and_catches_unflipped_taps(suffix, name):
    case = no.UPFIRDN_CASES[name]
    x, k = no.upfirdn_operands(case, no.TYPES[suffix][0])
    want, bound = no.upfirdn_ref_and_bound(x, k, case[6:], suffix)
    assert want.shape == no.upfirdn_out_shape(case)
    good = worst_ratio(upfirdn_standin(x, k, case[6:], suffix), want, bound)
    print(f"[upfirdn2d_{suffix} host] {name}: stand-in {good:.4f} of the bound")
    assert good <= 1.0, (suffix, name, good)
    if k.size > 1:
        assert worst_ratio(upfirdn_standin(x, k, case[6:], suffix, flip=False), want, bound) > 1.0
