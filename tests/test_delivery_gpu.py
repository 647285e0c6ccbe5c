"""GPU: maua_frames_to_u8 and maua_crop_resize_u8 (csrc/runtime.hip) through the C ABI, bit for bit.

Frame epilogue: equal to the numpy fp32 statement ((clip(x, -1, 1) + 1) * 127.5).astype(uint8) with every operand np.float32, on inputs
that sit on and next to every quantisation boundary (for each k in 0..255 the fp32 value nearest k / 127.5 - 1 and its neighbours up to
two ulps away), the clamp's edges, signed zeros, infinities, the smallest subnormal and +-3 — tiled so that on the two large shapes every
value meets every colour and every position of a 4-pixel group.  A NaN becomes 0 (include/maua_hip.h).  The fused epilogues of the last
layer share the quantiser (csrc/epilogue.h rgb8_quant is the same expression), so the statement covers them.

Crop + resize: equal to tests/test_host_logic.py::pil_bilinear_upscale_restated (the integer twin, pinned to PIL on the host) and, where
PIL imports, to PIL.Image.resize(BILINEAR) of the crop itself.  The crop sits at (x0, y0) = (2, 1) inside a frame whose surrounding
pixels differ from their neighbours inside the crop by at least 128, so that a tap clamped to the frame instead of the crop shows.

Every buffer is a tests/redzone.py window."""
import numpy as np
import pytest
import torch

from maua_stylegan2_amd import _lib
from redzone import CANARY_BITS, Guard
from test_host_logic import pil_bilinear_upscale_restated

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

EINVAL, ENOSYS = -22, -38
F32 = np.float32

# ---------------------------------------------------------------------------------------------------------------- frame epilogue
# (batch, h, w, input skew in floats, output skew in bytes)
FRAME_CASES = [(1, 4, 8, 0, 0), (3, 5, 7, 0, 0), (2, 1, 1, 0, 0), (1, 2, 2, 0, 0), (2, 16, 16, 1, 0), (2, 16, 16, 0, 1),
               (1, 2052, 2048, 0, 0), (1, 591, 593, 0, 0)]
FRAME_GRID_ELEMENTS = 4096 * 256  # pack_grid's cap: work items of one grid-stride trip


def adversarial_values():
    """fp32 values on and around every quantisation boundary and the clamp's edges (an odd count: see frames_input)."""
    vals = []
    for k in range(256):
        v = F32(np.float64(k) / 127.5 - 1.0)
        lo1, hi1 = np.nextafter(v, F32(-np.inf)), np.nextafter(v, F32(np.inf))
        vals += [np.nextafter(lo1, F32(-np.inf)), lo1, v, hi1, np.nextafter(hi1, F32(np.inf))]
    one_up = np.nextafter(F32(1), F32(np.inf))
    vals += [F32(1), F32(-1), one_up, -one_up, F32(0.0), F32(-0.0), F32(np.inf), F32(-np.inf), np.nextafter(F32(0), F32(1)), F32(3), F32(-3)]
    vals = np.array(vals, dtype=F32)
    assert vals.size % 2 == 1 and not np.isnan(vals).any()
    return vals


def frames_input(batch, h, w):
    """x[b, c, p] = values[(p + 431 c + 977 b) % L]: L is odd, so wherever a plane holds 4 L pixels or more every value meets every
    position of a 4-pixel group in every colour."""
    vals = adversarial_values()
    p = np.arange(h * w, dtype=np.int64)
    idx = (p[None, None, :] + 431 * np.arange(3)[None, :, None] + 977 * np.arange(batch)[:, None, None]) % vals.size
    return vals[idx].reshape(batch, 3, h, w), idx.reshape(batch, 3, h, w)


def frames_ref(x):
    """The fp32 statement, NCHW -> NHWC.  A NaN is taken to -1 first (the documented behaviour of the device clamp)."""
    x = np.where(np.isnan(x), F32(-1), x).astype(F32)
    q = (np.clip(x, F32(-1), F32(1)) + F32(1)) * F32(127.5)
    assert q.dtype == F32
    return np.ascontiguousarray(q.astype(np.uint8).transpose(0, 2, 3, 1))


def _canary_bytes(n, first_byte):
    pattern = np.frombuffer(np.uint32(CANARY_BITS).tobytes(), np.uint8)
    return pattern[(first_byte + np.arange(n)) % 4]


def _check_u8(g, n):
    """Red zones, and "every element written" where the window is whole dwords: a last dword of which only one byte belongs to the window
    still equals the canary whenever that byte is 0xEF, written or not (the comparison with the reference covers those windows)."""
    g.check(written=("out",) if n % 4 == 0 else (), nonfinite_ok=("out",))


def _frames_launch(gpu, x, in_skew=0, out_skew=0):
    """One guarded call; the windows start ``in_skew`` floats / ``out_skew`` bytes into 16-byte aligned buffers, the bytes before and
    behind them keep the canary.  Returns (rc, out as numpy [B, H, W, 3])."""
    lib = _lib.load()
    batch, _, h, w = x.shape
    n = batch * h * w * 3
    g = Guard(gpu)
    xin = g.out((n + in_skew,), "x")
    xin[in_skew:].copy_(torch.from_numpy(x.reshape(-1)))
    out = g.out((n + out_skew,), "out", torch.uint8)
    assert xin.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    rc = lib.maua_frames_to_u8(xin.data_ptr() + 4 * in_skew, out.data_ptr() + out_skew, batch, h, w, _lib.stream_ptr(gpu))
    if rc != 0:
        return rc, g, None
    if out_skew:
        g.check()
        assert np.array_equal(out[:out_skew].cpu().numpy(), _canary_bytes(out_skew, 0)), "write in front of the skewed output window"
    else:
        _check_u8(g, n)
    if in_skew:
        assert bool((xin[:in_skew].view(torch.int32) == CANARY_BITS).all())
    return rc, g, out[out_skew:].cpu().numpy().reshape(batch, h, w, 3)


@pytest.mark.parametrize("case", FRAME_CASES, ids=lambda c: "-".join(map(str, c)))
def test_frames_to_u8_on_every_quantisation_boundary(gpu, case):
    batch, h, w, in_skew, out_skew = case
    x, idx = frames_input(batch, h, w)
    rc, _, got = _frames_launch(gpu, x, in_skew, out_skew)
    assert rc == 0, rc
    want = frames_ref(x)
    bad = int((got != want).sum())
    print(f"[frames_to_u8] {case}: {bad} of {want.size} bytes differ from the fp32 statement")
    assert bad == 0, (case, bad)
    vector = (h * w) % 4 == 0 and in_skew == 0 and out_skew % 4 == 0
    items = batch * h * w // 4 if vector else batch * h * w * 3
    if h * w > 100000:
        assert items > FRAME_GRID_ELEMENTS, "this case is here for the second grid-stride trip"
        n_vals = adversarial_values().size
        for c in range(3):  # every value in every colour at every position of a 4-pixel group
            seen = np.zeros((n_vals, 4), bool)
            seen[idx[0, c].reshape(-1), np.arange(h * w) % 4] = True
            assert seen.all()
    else:
        assert items <= FRAME_GRID_ELEMENTS


def test_frames_to_u8_paths_agree_and_a_nan_becomes_zero(gpu):
    """The statement's value on the boundaries themselves (k / 127.5 - 1 quantises to k wherever fp32 says so — computed, not assumed),
    and the documented NaN: fmaxf(NaN, -1) = -1, hence 0, on the 16-byte path and on the scalar one."""
    x, _ = frames_input(1, 4, 8)
    x[0, 0, 0, 1], x[0, 1, 2, 3], x[0, 2, 3, 7] = np.nan, -np.nan, F32(np.nan)
    want = frames_ref(x)
    assert want[0, 0, 1, 0] == 0 and want[0, 2, 3, 1] == 0 and want[0, 3, 7, 2] == 0
    for in_skew in (0, 1):
        rc, _, got = _frames_launch(gpu, x, in_skew, 0)
        assert rc == 0 and np.array_equal(got, want), in_skew


def test_frames_to_u8_refusals(gpu):
    lib = _lib.load()
    g = Guard(gpu)
    x, out = g.inp(np.zeros((1, 3, 2, 2), F32), "x"), g.out((12,), "out", torch.uint8)
    st = _lib.stream_ptr(gpu)
    for args in ((None, out.data_ptr(), 1, 2, 2), (x.data_ptr(), None, 1, 2, 2), (x.data_ptr(), out.data_ptr(), 0, 2, 2),
                 (x.data_ptr(), out.data_ptr(), 1, 0, 2), (x.data_ptr(), out.data_ptr(), 1, 2, -1)):
        assert lib.maua_frames_to_u8(*args, st) == EINVAL, args
    assert g.untouched("out")
    g.check()


# ---------------------------------------------------------------------------------------------------------------- crop + resize
X0, Y0 = 2, 1
CROP_WIDTHS = list(range(1, 20)) + [31, 32, 33, 64, 97]
HEIGHTS = [(1, 1), (1, 3), (2, 5), (5, 5), (7, 9), None]  # None: square (ch = cw, oh = ow)


def resize_cases():
    """(cw, ch, ow, oh): per crop width the distinct output widths, times the six height pairs — 206 x 6 = 1236 combinations."""
    out = []
    for cw in CROP_WIDTHS:
        for ow in sorted({cw, cw + 1, cw + 2, cw + 3, 2 * cw, 2 * cw + 1, 3 * cw - 1, 7 * cw + 3, cw + 17}):
            for hh in HEIGHTS:
                out.append((cw,) + (hh[0], ow, hh[1]) if hh else (cw, cw, ow, ow))
    return out


RESIZE_CASES = resize_cases()
RESIZE_CHUNKS = 6


def decoy_frame(batch, cw, ch, seed, fill=None):
    """[batch, ch + 3, cw + 4, 3] uint8: a random (or constant) crop at (X0, Y0); every pixel outside the crop is 255 where the nearest
    pixel inside it is below 128 and 0 otherwise."""
    r = np.random.default_rng(seed)
    crop = r.integers(0, 256, (batch, ch, cw, 3), dtype=np.uint8) if fill is None else np.full((batch, ch, cw, 3), fill, np.uint8)
    in_h, in_w = ch + 3, cw + 4
    yy = np.clip(np.arange(in_h) - Y0, 0, ch - 1)
    xx = np.clip(np.arange(in_w) - X0, 0, cw - 1)
    nearest = crop[:, yy][:, :, xx]
    frame = np.where(nearest < 128, 255, 0).astype(np.uint8)
    frame[:, Y0:Y0 + ch, X0:X0 + cw] = crop
    return frame


def resize_ref(frame, cw, ch, ow, oh):
    """The integer twin per frame, and PIL itself on the crop where it imports (asserted equal to the twin)."""
    want = np.stack([pil_bilinear_upscale_restated(f, X0, Y0, cw, ch, ow, oh) for f in frame])
    try:
        import PIL.Image
    except ImportError:
        return want
    for f, wnt in zip(frame, want):
        pil = np.array(PIL.Image.fromarray(np.ascontiguousarray(f[Y0:Y0 + ch, X0:X0 + cw])).resize((ow, oh), PIL.Image.BILINEAR))
        assert np.array_equal(pil, wnt), ("the twin left PIL", cw, ch, ow, oh)
    return want


def _resize_launch(gpu, frame, box, out_shape=None):
    lib = _lib.load()
    batch, in_h, in_w, _ = frame.shape
    x0, y0, cw, ch, ow, oh = box
    g = Guard(gpu)
    fin = g.inp(frame, "in", torch.uint8)
    out = g.out(out_shape or (batch, oh, ow, 3), "out", torch.uint8)
    rc = lib.maua_crop_resize_u8(fin.data_ptr(), out.data_ptr(), batch, in_h, in_w, x0, y0, cw, ch, ow, oh, _lib.stream_ptr(gpu))
    return rc, g, out


def _resize_case(gpu, batch, cw, ch, ow, oh, seed, fill=None):
    frame = decoy_frame(batch, cw, ch, seed, fill)
    rc, g, out = _resize_launch(gpu, frame, (X0, Y0, cw, ch, ow, oh))
    assert rc == 0, rc
    _check_u8(g, out.numel())
    want = resize_ref(frame, cw, ch, ow, oh)
    bad = int((out.cpu().numpy() != want).sum())
    assert bad == 0, ((batch, cw, ch, ow, oh), bad)


def test_resize_case_list_is_the_one_counted():
    assert len(RESIZE_CASES) == 1236 and all(ow >= cw and oh >= ch for cw, ch, ow, oh in RESIZE_CASES)


@pytest.mark.parametrize("chunk", range(RESIZE_CHUNKS))
def test_crop_resize_small_ratios_against_the_twin_and_pil(gpu, chunk):
    """Every combination of the list, batch 1 and batch 3 alternating."""
    cases = RESIZE_CASES[chunk::RESIZE_CHUNKS]
    for n, (cw, ch, ow, oh) in enumerate(cases):
        _resize_case(gpu, 1 if n % 2 else 3, cw, ch, ow, oh, seed=1000 * chunk + n)
    print(f"[crop_resize_u8] chunk {chunk}: {len(cases)} shapes, 0 bytes differ from the twin and from PIL")


@pytest.mark.parametrize("fill", [0, 255])
def test_crop_resize_constant_frames(gpu, fill):
    """All-0 and all-255 crops stay constant (the coefficients of a tap pair sum to 2^22 exactly)."""
    for batch, cw, ch, ow, oh in ((1, 5, 7, 9, 11), (3, 13, 2, 30, 5), (1, 1, 1, 4, 3)):
        _resize_case(gpu, batch, cw, ch, ow, oh, seed=fill, fill=fill)


def test_crop_resize_second_grid_stride_trip(gpu):
    """1400 x 1500 output pixels: 2,100,000 > 8192 * 256."""
    ow, oh = 1400, 1500
    assert ow * oh > 8192 * 256
    _resize_case(gpu, 1, 700, 750, ow, oh, seed=77)


def test_crop_resize_refusals_leave_the_output_untouched(gpu):
    frame = decoy_frame(2, 8, 6, 5)  # [2, 9, 12, 3]
    ok = (X0, Y0, 8, 6, 16, 12)
    refused = [((X0, Y0, 8, 6, 7, 12), ENOSYS), ((X0, Y0, 8, 6, 16, 5), ENOSYS),             # a down-scale on either axis
               ((5, Y0, 8, 6, 16, 12), EINVAL), ((X0, 4, 8, 6, 16, 12), EINVAL),              # the crop leaves the frame
               ((-1, Y0, 8, 6, 16, 12), EINVAL), ((X0, -1, 8, 6, 16, 12), EINVAL),
               ((X0, Y0, 0, 6, 16, 12), EINVAL), ((X0, Y0, 8, -1, 16, 12), EINVAL), ((X0, Y0, 8, 6, 0, 12), EINVAL),
               ((X0, Y0, 8, 6, 16, 0), EINVAL)]
    for box, code in refused:
        rc, g, _ = _resize_launch(gpu, frame, box, out_shape=(2, 12, 16, 3))
        assert rc == code, (box, rc)
        assert g.untouched("out"), box
        g.check()
    lib = _lib.load()
    g = Guard(gpu)
    fin, out = g.inp(frame, "in", torch.uint8), g.out((2, 12, 16, 3), "out", torch.uint8)
    st = _lib.stream_ptr(gpu)
    assert lib.maua_crop_resize_u8(None, out.data_ptr(), 2, 9, 12, *ok, st) == EINVAL
    assert lib.maua_crop_resize_u8(fin.data_ptr(), None, 2, 9, 12, *ok, st) == EINVAL
    for batch, in_h, in_w in ((0, 9, 12), (2, 0, 12), (2, 9, -3)):
        assert lib.maua_crop_resize_u8(fin.data_ptr(), out.data_ptr(), batch, in_h, in_w, *ok, st) == EINVAL
    assert g.untouched("out")
    g.check()
