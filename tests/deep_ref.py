"""The numpy twins of csrc/deep_frames.hip (no device): the fp32 quantiser to 16 bits, the integer BT.709 limited-range matrix to 10 bits
in int64, the three planar layouts, and the 16-bit crop + resize.  The GPU tests compare the kernels with these bit for bit; the host tests
pin the twins themselves (known answers, the float64 definition, the 8-bit twin)."""
import numpy as np

F32 = np.float32
SUBSAMPLINGS = (420, 422, 444)
BLOCK = {420: (2, 2), 422: (1, 2), 444: (1, 1)}  # rows x columns of luma per chroma sample
FMT_OF = {420: "yuv420p10le", 422: "yuv422p10le", 444: "yuv444p10le"}
D = 10000 * 65535

KNOWN = {  # 16-bit RGB -> (Y, Cb, Cr), BT.709 limited range, 10 bits
    "white": ((65535, 65535, 65535), (940, 512, 512)),
    "black": ((0, 0, 0), (64, 512, 512)),
    "red": ((65535, 0, 0), (250, 409, 960)),
    "green": ((0, 65535, 0), (691, 167, 105)),
    "blue": ((0, 0, 65535), (127, 960, 471)),
    "yellow": ((65535, 65535, 0), (877, 64, 553)),
    "cyan": ((0, 65535, 65535), (754, 615, 64)),
    "magenta": ((65535, 0, 65535), (313, 857, 919)),
    "grey": ((32768, 32768, 32768), (502, 512, 512)),
}


def quant16(x):
    """fp32 [...] -> uint16: ((clip(x, -1, 1) + 1) * 32767.5).astype(uint16) with every operand np.float32 (two correctly rounded
    operations, a truncating cast).  A NaN is taken to -1 first: the device clamp is fminf(fmaxf(x, -1), 1)."""
    x = np.asarray(x, dtype=F32)
    x = np.where(np.isnan(x), F32(-1), x).astype(F32)
    q = (np.clip(x, F32(-1), F32(1)) + F32(1)) * F32(32767.5)
    assert q.dtype == F32
    return q.astype(np.uint16)


def quant8(x):
    """The 8-bit quantiser (maua_frames_to_u8), for the comparison through codes // 257."""
    x = np.asarray(x, dtype=F32)
    x = np.where(np.isnan(x), F32(-1), x).astype(F32)
    return ((np.clip(x, F32(-1), F32(1)) + F32(1)) * F32(127.5)).astype(np.uint8)


def frames_to_u16(img):
    """fp32 [b, 3, h, w] -> uint16 [b, h, w, 3]."""
    return np.ascontiguousarray(quant16(img).transpose(0, 2, 3, 1))


def luma(rgb):
    """[..., 3] 16-bit codes -> Y, int64."""
    c = np.asarray(rgb).astype(np.int64)
    lum = 2126 * c[..., 0] + 7152 * c[..., 1] + 722 * c[..., 2]
    return 64 + (2 * 876 * lum + D) // (2 * D)


def chroma(sums, n):
    """[..., 3] int64 sums of the R, G, B codes of a block of ``n`` pixels -> (Cb, Cr), int64."""
    s = np.asarray(sums).astype(np.int64)
    sr, sg, sb = s[..., 0], s[..., 1], s[..., 2]
    lum = 2126 * sr + 7152 * sg + 722 * sb
    eb, er = 2 * 9278 * 65535 * n, 2 * 7874 * 65535 * n
    num_b = 2 * (512 * eb + 896 * (10000 * sb - lum)) + eb
    num_r = 2 * (512 * er + 896 * (10000 * sr - lum)) + er
    assert num_b.min(initial=1) > 0 and num_r.min(initial=1) > 0 and max(num_b.max(initial=1), num_r.max(initial=1)) < 2 ** 44
    return num_b // (2 * eb), num_r // (2 * er)


def block_sums(rgb, sub):
    """uint16 [b, h, w, 3] -> int64 [b, h / bh, w / bw, 3]: the box sums of the chroma blocks."""
    bh, bw = BLOCK[sub]
    b, h, w, _ = rgb.shape
    assert h % bh == 0 and w % bw == 0
    return rgb.astype(np.int64).reshape(b, h // bh, bh, w // bw, bw, 3).sum(axis=(2, 4))


def yuv_p10(rgb, sub):
    """uint16 [b, h, w, 3] -> uint16 [b, frame]: per frame the Y plane [h, w], then U, then V ([h/2, w/2], [h, w/2] or [h, w])."""
    rgb = np.asarray(rgb)
    b = rgb.shape[0]
    bh, bw = BLOCK[sub]
    y = luma(rgb)
    cb, cr = chroma(block_sums(rgb, sub), bh * bw)
    assert y.min(initial=64) >= 64 and y.max(initial=64) <= 940
    for plane in (cb, cr):
        assert plane.min(initial=64) >= 64 and plane.max(initial=64) <= 960
    return np.concatenate([y.reshape(b, -1), cb.reshape(b, -1), cr.reshape(b, -1)], axis=1).astype(np.uint16)


def frame_samples(sub, h, w):
    bh, bw = BLOCK[sub]
    return h * w + 2 * (h // bh) * (w // bw)


def resize_taps(n_in, n_out, bits=22):
    """The tap function of the 8-bit twin (tests/test_host_logic.py pil_bilinear_upscale_restated, csrc resize_tap): per output index the two
    clamped source indices and the coefficients rounded to ``bits`` fractional bits."""
    o = np.arange(n_out, dtype=np.int64)
    num, den = (2 * o + 1) * n_in - n_out, 2 * n_out
    i0 = np.floor_divide(num, den)
    f = (num - i0 * den).astype(np.float64) / den
    k1 = np.floor(0.5 + f * (1 << bits)).astype(np.int64)
    k0 = np.floor(0.5 + (1 - f) * (1 << bits)).astype(np.int64)
    return np.clip(i0, 0, n_in - 1), np.clip(i0 + 1, 0, n_in - 1), k0, k1


def crop_resize(frame, x0, y0, cw, ch, ow, oh, top=65535, bits=22):
    """[H, W, 3] integer frame -> [oh, ow, 3] int64: the crop up-scaled with the 2-tap filter in int64, the horizontal pass rounded half up
    and clamped to 0 .. ``top``, then the vertical pass on that.  ``top`` = 255 is the 8-bit twin."""
    f = np.asarray(frame)[y0:y0 + ch, x0:x0 + cw].astype(np.int64)
    xa, xb, kx0, kx1 = resize_taps(cw, ow, bits)
    ya, yb, ky0, ky1 = resize_taps(ch, oh, bits)
    half = 1 << (bits - 1)
    h = np.clip((kx0[None, :, None] * f[:, xa] + kx1[None, :, None] * f[:, xb] + half) >> bits, 0, top)
    return np.clip((ky0[:, None, None] * h[ya] + ky1[:, None, None] * h[yb] + half) >> bits, 0, top)


def crop_resize_u16(frames, x0, y0, cw, ch, ow, oh):
    """uint16 [b, H, W, 3] -> uint16 [b, oh, ow, 3]."""
    return np.stack([crop_resize(f, x0, y0, cw, ch, ow, oh) for f in frames]).astype(np.uint16)


def crop_resize_float64(frame, x0, y0, cw, ch, ow, oh):
    """The same 2-tap filter in float64, without any rounding (the definition the integer form approximates)."""
    f = np.asarray(frame)[y0:y0 + ch, x0:x0 + cw].astype(np.float64)

    def taps(n_in, n_out):
        pos = (np.arange(n_out, dtype=np.float64) + 0.5) * n_in / n_out - 0.5
        i0 = np.floor(pos)
        return np.clip(i0, 0, n_in - 1).astype(np.int64), np.clip(i0 + 1, 0, n_in - 1).astype(np.int64), pos - i0

    xa, xb, fx = taps(cw, ow)
    ya, yb, fy = taps(ch, oh)
    h = (1 - fx)[None, :, None] * f[:, xa] + fx[None, :, None] * f[:, xb]
    return (1 - fy)[:, None, None] * h[ya] + fy[:, None, None] * h[yb]


def deliver(img, pix_fmt, box=None):
    """fp32 [b, 3, h, w] -> the bytes of the deep frames, uint8 [b, bytes]: what render.frames_to_deep computes (``box`` = (x0, y0, cw, ch,
    ow, oh): the wide-output crop + resize on the 16-bit master)."""
    master = frames_to_u16(img)
    if box is not None:
        master = crop_resize_u16(master, *box)
    b = master.shape[0]
    if pix_fmt == "rgb48le":
        return master.reshape(b, -1).astype("<u2").view(np.uint8)
    sub = {v: k for k, v in FMT_OF.items()}[pix_fmt]
    return yuv_p10(master, sub).astype("<u2").view(np.uint8)
