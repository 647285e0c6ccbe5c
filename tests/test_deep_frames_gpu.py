"""GPU: the deep frame delivery — the four entries of csrc/deep_frames.hip through the C ABI, bit for bit against the numpy twins of
tests/deep_ref.py (pinned on the host by tests/test_deep_frames_host.py), and the deep pipe formats through synthesize / render_shard.

Every buffer of a launch is a tests/redzone.py window; the uint16 buffers are uint8 windows of twice the length (the guard knows no
16-bit type), optionally skewed off the vector alignment: the bytes in front of a skewed window keep the canary."""
import os

import numpy as np
import pytest
import torch

import deep_ref as dr
from maua_stylegan2_amd import _lib, seeding
from redzone import CANARY_BITS, Guard
from test_delivery_gpu import RESIZE_CASES, X0, Y0

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

EINVAL, ENOSYS = -22, -38
F32 = np.float32
GRID_STRIPS = 1024 * 256  # strips one trip of the planar kernels' grid covers per frame (GRID_CAP workgroups of 256 threads)


def _canary_bytes(n):
    return np.frombuffer(np.uint32(CANARY_BITS).tobytes(), np.uint8)[np.arange(n) % 4]


def _window(g, name, n_bytes, skew, data=None):
    """A guarded uint8 window of ``skew`` + ``n_bytes`` bytes on a 16-byte aligned start; the payload begins ``skew`` bytes in."""
    win = g.out((n_bytes + skew,), name, torch.uint8)
    assert win.data_ptr() % 16 == 0
    if data is not None:
        win[skew:].copy_(torch.from_numpy(np.ascontiguousarray(data).view(np.uint8).reshape(-1)))
    return win


def _read_u16(g, win, skew, shape):
    """Red zones intact, the skew bytes untouched; the payload as uint16."""
    g.check()
    host = win.cpu().numpy()
    assert np.array_equal(host[:skew], _canary_bytes(skew)), "write in front of the skewed window"
    return host[skew:].view("<u2").reshape(shape)


# ------------------------------------------------------------------------------------------------------------------------ (a) the quantiser
def boundary_values():
    """Every one of the 65 536 code boundaries k / 32767.5 - 1 (rounded to fp32) with its two fp32 neighbours, the clamp's edges, signed
    zeros, the infinities, NaNs of both signs, a subnormal and values far outside."""
    v = (np.arange(65536, dtype=np.float64) / 32767.5 - 1.0).astype(F32)
    one_up = np.nextafter(F32(1), F32(np.inf))
    extra = np.array([1, -1, one_up, -one_up, 0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, np.nextafter(F32(0), F32(1)), 3, -3, 1e30, -1e30], F32)
    return np.concatenate([np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf)), extra])


def _frames_to_u16(gpu, x, in_skew=0, out_skew=0):
    batch, _, h, w = x.shape
    n = x.size
    g = Guard(gpu)
    xin = _window(g, "x", 4 * n, in_skew, x)
    out = _window(g, "out", 2 * n, out_skew)
    rc = _lib.load().maua_frames_to_u16(xin.data_ptr() + in_skew, out.data_ptr() + out_skew, batch, h, w, _lib.stream_ptr(gpu))
    assert rc == 0, rc
    return _read_u16(g, out, out_skew, (batch, h, w, 3))


# (h, w, input skew in bytes, output skew in bytes): the vector path; a plane that is no multiple of 4; the input 4 bytes off the 16-byte
# grid; the output 2 bytes off the 8-byte grid
@pytest.mark.parametrize("case", [(8, 8193, 0, 0), (7, 9365, 0, 0), (8, 8193, 4, 0), (8, 8193, 0, 2)], ids=lambda c: "-".join(map(str, c)))
def test_frames_to_u16_on_every_code_boundary(gpu, case):
    h, w, in_skew, out_skew = case
    vals = boundary_values()
    assert 3 * h * w >= vals.size
    x = vals[np.arange(3 * h * w) % vals.size].reshape(1, 3, h, w)  # every value once, in one launch
    want = dr.frames_to_u16(x)
    got = _frames_to_u16(gpu, x, in_skew, out_skew)
    bad = int((got != want).sum())
    print(f"[frames_to_u16] {case}: {bad} of {want.size} samples differ from the fp32 statement")
    assert bad == 0
    flat = dr.quant16(vals)
    assert flat[65536] == 0 and flat[2 * 65536 - 1] == 65535 and len(np.unique(flat)) == 65536  # (the twin itself reaches every code)


def test_frames_to_u16_batches_small_shapes_and_refusals(gpu):
    rng = np.random.default_rng(3)
    for batch, h, w in [(3, 5, 7), (2, 1, 1), (2, 16, 16), (1, 2, 2)]:
        x = rng.uniform(-1.2, 1.2, (batch, 3, h, w)).astype(F32)
        x.reshape(-1)[::5] = boundary_values()[rng.integers(0, 3 * 65536, x.reshape(-1)[::5].size)]
        assert np.array_equal(_frames_to_u16(gpu, x), dr.frames_to_u16(x)), (batch, h, w)
    lib, st = _lib.load(), _lib.stream_ptr(gpu)
    g = Guard(gpu)
    xin, out = g.inp(np.zeros((1, 3, 2, 2), F32), "x"), g.out((24,), "out", torch.uint8)
    for args in ((None, out.data_ptr(), 1, 2, 2), (xin.data_ptr(), None, 1, 2, 2), (xin.data_ptr(), out.data_ptr(), 0, 2, 2),
                 (xin.data_ptr(), out.data_ptr(), 1, 0, 2), (xin.data_ptr(), out.data_ptr(), 1, 2, -1)):
        assert lib.maua_frames_to_u16(*args, st) == EINVAL, args
    assert g.untouched("out")
    g.check()


# ------------------------------------------------------------------------------------------------------------------------ (c) and (d)
# (h, w): one block; one whole strip of the packed kernel; a strip and a partial one; whole strips on several rows; four strips and a partial one
PLANAR_SHAPES = [(2, 2), (2, 8), (4, 10), (6, 16), (2, 36)]
ODD_SHAPES = {420: [], 422: [(3, 6)], 444: [(3, 5), (1, 1)]}  # what the subsampling allows beyond even sizes
KNOWN_RGB = np.array([v[0] for v in dr.KNOWN.values()], np.uint16)


def _operands(kind, batch, h, w, seed):
    if kind == "known":  # one 2 x 2 block per colour, walking through the list
        yy, xx, bb = np.arange(h)[None, :, None] // 2, np.arange(w)[None, None, :] // 2, np.arange(batch)[:, None, None]
        return KNOWN_RGB[(yy * ((w + 1) // 2) + xx + bb) % len(KNOWN_RGB)]
    if kind == "zeros":
        return np.zeros((batch, h, w, 3), np.uint16)
    if kind == "ones":
        return np.full((batch, h, w, 3), 65535, np.uint16)
    return np.random.default_rng(seed).integers(0, 65536, (batch, h, w, 3), dtype=np.uint16)


def _rgb48_to_yuv(gpu, rgb, sub, in_skew=0, out_skew=0):
    batch, h, w, _ = rgb.shape
    n_out = dr.frame_samples(sub, h, w)
    g = Guard(gpu)
    src = _window(g, "rgb", 2 * rgb.size, in_skew, rgb.astype("<u2"))
    out = _window(g, "out", 2 * batch * n_out, out_skew)
    rc = _lib.load().maua_rgb48_to_yuv_p10(src.data_ptr() + in_skew, out.data_ptr() + out_skew, batch, h, w, sub, _lib.stream_ptr(gpu))
    assert rc == 0, rc
    return _read_u16(g, out, out_skew, (batch, n_out))


def _f32_to_yuv(gpu, x, sub, in_skew=0, out_skew=0):
    batch, _, h, w = x.shape
    n_out = dr.frame_samples(sub, h, w)
    g = Guard(gpu)
    src = _window(g, "x", 4 * x.size, in_skew, x)
    out = _window(g, "out", 2 * batch * n_out, out_skew)
    rc = _lib.load().maua_frames_to_yuv_p10_f32(src.data_ptr() + in_skew, out.data_ptr() + out_skew, batch, h, w, sub, _lib.stream_ptr(gpu))
    assert rc == 0, rc
    return _read_u16(g, out, out_skew, (batch, n_out))


@pytest.mark.parametrize("sub", dr.SUBSAMPLINGS)
def test_rgb48_to_yuv_p10_equals_the_twin_bit_for_bit(gpu, sub):
    n = 0
    for h, w in PLANAR_SHAPES + ODD_SHAPES[sub]:
        for batch in (1, 3):
            for kind in ("known", "zeros", "ones", "random"):
                rgb = _operands(kind, batch, h, w, seed=100 * h + w + batch)
                got = _rgb48_to_yuv(gpu, rgb, sub)
                assert np.array_equal(got, dr.yuv_p10(rgb, sub)), (sub, h, w, batch, kind)
                n += 1
    # buffers off the vector alignment: shapes the vector path would take go through the scalar one
    for h, w, in_skew, out_skew in [(6, 16, 0, 2), (6, 16, 2, 0), (2, 8, 8, 8), (4, 32, 0, 6)]:
        rgb = _operands("random", 3, h, w, seed=h + w + in_skew)
        rgb[0, :2, :2] = 65535
        assert np.array_equal(_rgb48_to_yuv(gpu, rgb, sub, in_skew, out_skew), dr.yuv_p10(rgb, sub)), (sub, h, w, in_skew, out_skew)
        n += 1
    print(f"[rgb48_to_yuv_p10] {sub}: {n} launches, 0 samples differ from the integer twin")


def test_known_colours_come_out_as_the_table_says(gpu):
    w = 2 * len(dr.KNOWN)
    frame = np.repeat(np.repeat(KNOWN_RGB[None, None], 2, axis=1), 2, axis=2).reshape(1, 2, w, 3)
    want = np.array([v[1] for v in dr.KNOWN.values()])
    got = _rgb48_to_yuv(gpu, frame, 420)[0]
    assert list(got[:w:2]) == list(want[:, 0]) and list(got[2 * w: 2 * w + w // 2]) == list(want[:, 1])
    assert list(got[2 * w + w // 2:]) == list(want[:, 2])


@pytest.mark.parametrize("entry", ["rgb48", "f32"])
def test_planar_kernels_second_grid_stride_trip(gpu, entry):
    """4:4:4 (one row per strip: the fewest pixels per strip) on the smallest 2048-wide frame whose strips exceed one trip of the grid."""
    h, w = (1026, 2048) if entry == "rgb48" else (514, 2048)
    strips = h * w // (8 if entry == "rgb48" else 4)
    assert GRID_STRIPS < strips <= GRID_STRIPS + w  # (a few rows more than one trip: the second trip is a partial one)
    rng = np.random.default_rng(h)
    if entry == "rgb48":
        rgb = rng.integers(0, 65536, (1, h, w, 3), dtype=np.uint16)
        got = _rgb48_to_yuv(gpu, rgb, 444)
    else:
        x = rng.uniform(-1.1, 1.1, (1, 3, h, w)).astype(F32)
        rgb = dr.frames_to_u16(x)
        got = _f32_to_yuv(gpu, x, 444)
    assert np.array_equal(got, dr.yuv_p10(rgb, 444))


def _float_operands(batch, h, w, seed):
    """fp32 images between -1.1 and 1.1 with every third value on or next to a code boundary and a few specials."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.1, 1.1, (batch, 3, h, w)).astype(F32)
    flat = x.reshape(-1)
    vals = boundary_values()
    flat[::3] = vals[rng.integers(0, vals.size, flat[::3].size)]
    flat[:4] = [1.0, -1.0, np.inf, np.nan][: flat[:4].size]
    return x


@pytest.mark.parametrize("sub", dr.SUBSAMPLINGS)
def test_frames_to_yuv_p10_f32_is_the_conversion_of_the_master(gpu, sub):
    """(d) == (c) applied to (a), both computed on the device, and == the twin."""
    n = 0
    cases = [(h, w, b, 0, 0) for h, w in PLANAR_SHAPES + ODD_SHAPES[sub] for b in (1, 3)]
    cases += [(6, 16, 3, 4, 0), (6, 16, 3, 0, 2), (2, 8, 1, 8, 4), (4, 32, 2, 0, 6)]  # off the vector alignment
    for h, w, batch, in_skew, out_skew in cases:
        x = _float_operands(batch, h, w, seed=1000 * sub + 10 * h + w + batch)
        got = _f32_to_yuv(gpu, x, sub, in_skew, out_skew)
        master = _frames_to_u16(gpu, x)
        assert np.array_equal(master, dr.frames_to_u16(x))
        assert np.array_equal(got, _rgb48_to_yuv(gpu, master, sub)), (sub, h, w, batch, in_skew, out_skew)
        assert np.array_equal(got, dr.yuv_p10(dr.frames_to_u16(x), sub)), (sub, h, w, batch, in_skew, out_skew)
        n += 1
    print(f"[frames_to_yuv_p10_f32] {sub}: {n} cases, 0 samples differ from (c) of (a) and from the twin")


def test_planar_entries_refusals_leave_the_output_untouched(gpu):
    lib, st = _lib.load(), _lib.stream_ptr(gpu)
    g = Guard(gpu)
    rgb = g.inp(np.zeros(2 * 3 * 8 * 8 * 3, np.uint8), "rgb", torch.uint8)
    x = g.inp(np.zeros((3, 3, 8, 8), F32), "x")
    out = g.out((2 * 3 * 8 * 8 * 3,), "out", torch.uint8)
    for entry, src in ((lib.maua_rgb48_to_yuv_p10, rgb), (lib.maua_frames_to_yuv_p10_f32, x)):
        for b, h, w, sub in [(1, 3, 4, 420), (1, 4, 3, 420), (1, 4, 3, 422), (1, 0, 4, 444), (1, 4, -1, 444), (-1, 4, 4, 420), (1, 4, 4, 421),
                             (1, 4, 4, 0), (1, 4, 4, 10)]:
            assert entry(src.data_ptr(), out.data_ptr(), b, h, w, sub, st) == EINVAL, (b, h, w, sub)
        assert entry(None, out.data_ptr(), 1, 4, 4, 420, st) == EINVAL and entry(src.data_ptr(), None, 1, 4, 4, 420, st) == EINVAL
        assert entry(src.data_ptr(), out.data_ptr(), 0, 4, 4, 420, st) == 0  # an empty batch: success, nothing launched
    assert g.untouched("out")
    g.check()


# ------------------------------------------------------------------------------------------------------------------------ (b) crop + resize
def decoy_frame16(batch, cw, ch, seed, fill=None):
    """[batch, ch + 3, cw + 4, 3] uint16: a random (or constant) crop at (X0, Y0); every pixel outside the crop is 65535 where the nearest
    pixel inside it is below 32768 and 0 otherwise, so that a tap clamped to the frame instead of the crop shows."""
    r = np.random.default_rng(seed)
    crop = r.integers(0, 65536, (batch, ch, cw, 3), dtype=np.uint16) if fill is None else np.full((batch, ch, cw, 3), fill, np.uint16)
    yy = np.clip(np.arange(ch + 3) - Y0, 0, ch - 1)
    xx = np.clip(np.arange(cw + 4) - X0, 0, cw - 1)
    frame = np.where(crop[:, yy][:, :, xx] < 32768, 65535, 0).astype(np.uint16)
    frame[:, Y0:Y0 + ch, X0:X0 + cw] = crop
    return frame


def _resize_launch(gpu, frame, box, out_shape=None):
    batch, in_h, in_w, _ = frame.shape
    x0, y0, cw, ch, ow, oh = box
    shape = out_shape or (batch, oh, ow, 3)
    g = Guard(gpu)
    fin = _window(g, "in", 2 * frame.size, 0, frame.astype("<u2"))
    out = _window(g, "out", 2 * int(np.prod(shape)), 0)
    rc = _lib.load().maua_crop_resize_u16(fin.data_ptr(), out.data_ptr(), batch, in_h, in_w, x0, y0, cw, ch, ow, oh, _lib.stream_ptr(gpu))
    return rc, g, out, shape


def _resize_case(gpu, batch, cw, ch, ow, oh, seed, fill=None):
    frame = decoy_frame16(batch, cw, ch, seed, fill)
    rc, g, out, shape = _resize_launch(gpu, frame, (X0, Y0, cw, ch, ow, oh))
    assert rc == 0, rc
    got = _read_u16(g, out, 0, shape)
    want = dr.crop_resize_u16(frame, X0, Y0, cw, ch, ow, oh)
    bad = int((got != want).sum())
    assert bad == 0, ((batch, cw, ch, ow, oh), bad)


RESIZE_CHUNKS = 6


@pytest.mark.parametrize("chunk", range(RESIZE_CHUNKS))
def test_crop_resize_u16_small_ratios_against_the_twin(gpu, chunk):
    """Every combination of the 8-bit case list, batch 1 and batch 3 alternating."""
    cases = RESIZE_CASES[chunk::RESIZE_CHUNKS]
    for n, (cw, ch, ow, oh) in enumerate(cases):
        _resize_case(gpu, 1 if n % 2 else 3, cw, ch, ow, oh, seed=1000 * chunk + n)
    print(f"[crop_resize_u16] chunk {chunk}: {len(cases)} shapes, 0 samples differ from the twin")


@pytest.mark.parametrize("fill", [0, 32768, 65535])
def test_crop_resize_u16_constant_frames(gpu, fill):
    for batch, cw, ch, ow, oh in ((1, 5, 7, 9, 11), (3, 13, 2, 30, 5), (1, 1, 1, 4, 3)):
        _resize_case(gpu, batch, cw, ch, ow, oh, seed=fill, fill=fill)


def test_crop_resize_u16_refusals_leave_the_output_untouched(gpu):
    frame = decoy_frame16(2, 8, 6, 5)  # [2, 9, 12, 3]
    ok = (X0, Y0, 8, 6, 16, 12)
    refused = [((X0, Y0, 8, 6, 7, 12), ENOSYS), ((X0, Y0, 8, 6, 16, 5), ENOSYS),             # a down-scale on either axis
               ((5, Y0, 8, 6, 16, 12), EINVAL), ((X0, 4, 8, 6, 16, 12), EINVAL),              # the crop leaves the frame
               ((-1, Y0, 8, 6, 16, 12), EINVAL), ((X0, -1, 8, 6, 16, 12), EINVAL),
               ((X0, Y0, 0, 6, 16, 12), EINVAL), ((X0, Y0, 8, -1, 16, 12), EINVAL), ((X0, Y0, 8, 6, 0, 12), EINVAL),
               ((X0, Y0, 8, 6, 16, 0), EINVAL)]
    for box, code in refused:
        rc, g, _, _ = _resize_launch(gpu, frame, box, out_shape=(2, 12, 16, 3))
        assert rc == code, (box, rc)
        assert g.untouched("out"), box
        g.check()
    lib, st = _lib.load(), _lib.stream_ptr(gpu)
    rc, g, out, _ = _resize_launch(gpu, frame, (X0, Y0, 8, 6, 7, 12), out_shape=(2, 12, 16, 3))
    fin = g.inp(frame.astype("<u2").view(np.uint8), "in2", torch.uint8)
    assert lib.maua_crop_resize_u16(None, out.data_ptr(), 2, 9, 12, *ok, st) == EINVAL
    assert lib.maua_crop_resize_u16(fin.data_ptr(), None, 2, 9, 12, *ok, st) == EINVAL
    for batch, in_h, in_w in ((0, 9, 12), (2, 0, 12), (2, 9, -3)):
        assert lib.maua_crop_resize_u16(fin.data_ptr(), out.data_ptr(), batch, in_h, in_w, *ok, st) == EINVAL
    assert g.untouched("out")
    g.check()


# ------------------------------------------------------------------------------------------------------------------------ the render level
N_FRAMES, BATCH, SIZE = 7, 2, 64  # 3 captured batches + an eager tail batch of 1
IMAGE_TOL = 1e-3  # the bound tests/test_render_gpu.py puts on fp32 images


def _render(*args, size=SIZE, **kwargs):
    """render_shard at the generator's own frame size, into the fallback file (the technique of tests/test_yuv420_gpu.py)."""
    from maua_stylegan2_amd import render

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(render, "_output_dims", lambda out_size: (size, size))
        mp.setattr(render.shutil, "which", lambda name: None)
        mp.delenv("MAUA_PIPE_PIX_FMT", raising=False)
        mp.delenv("MAUA_SUBFRAMES", raising=False)
        return render.render_shard(*args, **kwargs)


@pytest.fixture(scope="module")
def job(gpu, tmp_path_factory):
    """The seeded generator, its fp32 images on the graph lanes (3 captured batches + the eager tail: the lanes a render of the same job
    uses) and on the eager path, and the default rgb24 render of the same job — computed once, read-only."""
    from maua_stylegan2_amd import render
    from maua_stylegan2_amd.models.stylegan2 import Generator

    g = Generator(SIZE, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(SIZE, seed=4), strict=True)
    g = g.to(gpu).eval()
    lat = seeding.seeded_latents(N_FRAMES, g.n_latent, seed=6)
    noise = seeding.seeded_noise(N_FRAMES, SIZE, seed=7)
    noise[-1] = None
    tmp = tmp_path_factory.mktemp("deep")

    def images(**kw):
        out = []
        for first, img in render.synthesize(g, lat, noise, BATCH, frames="f32", **kw):
            assert img.dtype == torch.float32 and tuple(img.shape[1:]) == (3, SIZE, SIZE) and first == sum(t.shape[0] for t in out)
            out.append(img.clone())
        torch.cuda.synchronize()
        return torch.cat(out).cpu().numpy()

    lanes, eager = images(), images(use_graph=False)
    frame_kinds = sorted({key[-1] for key in g._graph_lanes if isinstance(key[-1], tuple) and key[-1][:1] == ("frames",)})
    out = str(tmp / "rgb.mp4")
    assert _render(g, lat, noise, 0, N_FRAMES / 30, BATCH, SIZE, out, None, 1.0, [], {}, False, "slow", None) == N_FRAMES
    rgb = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(N_FRAMES, SIZE, SIZE, 3)
    for a in (lanes, eager, rgb):
        a.setflags(write=False)
    return dict(g=g, lat=lat, noise=noise, lanes=lanes, eager=eager, rgb=rgb, tmp=tmp, frame_kinds=frame_kinds)


def test_synthesize_f32_on_graph_lanes_equals_the_eager_path(gpu, job):
    from maua_stylegan2_amd import render

    assert job["lanes"].shape == (N_FRAMES, 3, SIZE, SIZE) and job["lanes"].std() > 0.05
    err = float(np.abs(job["lanes"] - job["eager"]).max())
    print(f"[deep render] fp32 images, graph lanes vs eager: max |difference| = {err:.3e}")
    assert err <= IMAGE_TOL
    # the frame kind is part of the cache key: the fp32 lanes sit next to the uint8 ones, and both are reused
    assert job["frame_kinds"] == [("frames", "f32")]
    g = job["g"]
    keys = set(g._graph_lanes)
    assert any(("frames", "f32") in key for key in keys) and any(("frames", "f32") not in key for key in keys)
    lanes_before = dict(g._graph_lanes)
    for kw in ({}, {"frames": "f32"}):
        for _ in render.synthesize(g, job["lat"], job["noise"], BATCH, **kw):
            pass
    torch.cuda.synchronize()
    assert g._graph_lanes == lanes_before  # nothing re-captured, nothing evicted


def test_default_rgb24_render_is_the_eager_paths_bytes(gpu, job):
    """The default path after the deep lanes exist: the rgb24 file equals the uint8 frames of the eager path, as it always did."""
    from maua_stylegan2_amd import render

    frames = [u8.clone() for _, u8 in render.synthesize(job["g"], job["lat"], job["noise"], BATCH, use_graph=False)]
    torch.cuda.synchronize()
    eager_u8 = torch.cat(frames).cpu().numpy()
    assert eager_u8.dtype == np.uint8 and eager_u8.shape == job["rgb"].shape
    assert np.array_equal(job["rgb"], eager_u8)
    assert job["rgb"].std() > 5


@pytest.mark.parametrize("fmt", ["rgb48le", "yuv420p10le", "yuv422p10le", "yuv444p10le"])
def test_render_shard_deep_format_equals_the_twin_on_the_lanes_images(gpu, job, fmt):
    """A render into the fallback file: frame count, order and every byte are the twin applied to the fp32 images of the same lanes —
    captured batches and the eager tail batch alike.  rgb48le // 257 is within one code of the rgb24 render of the same inputs."""
    from maua_stylegan2_amd import render

    out = str(job["tmp"] / f"{fmt}.mp4")
    written = _render(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out, None, 1.0, [], {}, False, "slow", None,
                      pipe_pix_fmt=fmt)
    assert written == N_FRAMES
    n_bytes = render.deep_frame_bytes(fmt, SIZE, SIZE)
    assert not os.path.exists(out + ".rgb24") and os.path.getsize(out + "." + fmt) == N_FRAMES * n_bytes
    assert (n_bytes,) == render._stream_frame_shape(job["g"], SIZE, fmt)
    got = np.fromfile(out + "." + fmt, dtype=np.uint8).reshape(N_FRAMES, n_bytes)
    want = dr.deliver(job["lanes"], fmt)
    assert np.array_equal(got, want)
    assert len({got[i].tobytes() for i in range(N_FRAMES)}) == N_FRAMES  # (distinct frames: the order is really checked)
    if fmt == "rgb48le":
        codes = got.view("<u2").reshape(N_FRAMES, SIZE, SIZE, 3).astype(np.int64)
        diff = np.abs(codes // 257 - job["rgb"].astype(np.int64))
        print(f"[deep render] rgb48le // 257 vs rgb24: {int((diff != 0).sum())} of {diff.size} samples differ, max {int(diff.max())}")
        assert diff.max() <= 1
        assert len(np.unique(codes)) > 4096  # more levels than 8 bits hold


def test_frames_to_deep_refusals_and_scratch_reuse(gpu, job):
    from maua_stylegan2_amd import render

    img = torch.from_numpy(job["lanes"][:2].copy()).to(gpu)
    scratch = {}
    first = render.frames_to_deep(img, SIZE, "yuv420p10le", scratch)
    again = render.frames_to_deep(img, SIZE, "yuv420p10le", scratch)
    assert first.data_ptr() == again.data_ptr() and len(scratch) == 1 and first.dtype == torch.uint8
    assert tuple(first.shape) == (2, SIZE * SIZE * 3)
    assert tuple(render.frames_to_deep(img[:0], SIZE, "rgb48le", scratch).shape) == (0, SIZE * SIZE * 6)
    with pytest.raises(ValueError, match="even"):
        render.frames_to_deep(img[:, :, :63], SIZE, "yuv444p10le", scratch)
    with pytest.raises(ValueError, match="deep pipe format"):
        render.frames_to_deep(img, SIZE, "yuv420p", scratch)
    with pytest.raises(RuntimeError, match="fp32"):
        render.frames_to_deep(img.to(torch.uint8), SIZE, "rgb48le", scratch)
    with pytest.raises(ValueError, match="8-bit only"):
        render.render_folded(job["g"], job["lat"][:4], [None] * job["g"].num_layers, 0, 1.0, BATCH, 512, None, None, 1.0, [], {}, False, "slow",
                             None, pipe_pix_fmt="rgb48le", fold=render.TemporalFold(2))


def test_wide_render_reaches_the_16_bit_resize(gpu, tmp_path):
    """``out_size`` 1920 on the smallest generator whose frames are 2048 px wide (1024^2 built for 1920 output, plus the layer-0 bend that
    widens the constant to 4 x 8: the route of tests/test_render_gpu.py): the fp32 images go through the 16-bit master, the crop + resize
    and the planar conversion on the device — equal to the twin on the same images — and a render writes 1920x1080 frames of 3 bytes per
    pixel."""
    from maua_stylegan2_amd import render
    from maua_stylegan2_amd.models.stylegan2 import Generator

    torch.manual_seed(11)
    with torch.device(gpu):
        g = Generator(1024, 512, 8, channel_multiplier=2, constant_input=True, output_size=1920)
    g = g.to(gpu).eval()
    n, batch = 2, 2
    lat = seeding.seeded_latents(n, g.n_latent, seed=8)
    noise = [None] * g.num_layers
    pad = torch.nn.ReplicationPad2d((2, 2, 0, 0))
    bends = [{"layer": 0, "transform": pad}]
    (first, img), = list(render.synthesize(g, lat, noise, batch, bends=bends, frames="f32"))
    assert first == 0 and tuple(img.shape) == (n, 3, 1024, 2048)
    box = (112, 0, 1824, 1024, 1920, 1080)
    got = render.frames_to_deep(img, 1920, "yuv420p10le", {})
    torch.cuda.synchronize()
    assert tuple(got.shape) == (n, 1920 * 1080 * 3) == (n,) + render._stream_frame_shape(g, 1920, "yuv420p10le")
    assert np.array_equal(got.cpu().numpy(), dr.deliver(img.cpu().numpy(), "yuv420p10le", box))
    out = str(tmp_path / "wide.mp4")
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(render.shutil, "which", lambda name: None)
        mp.delenv("MAUA_PIPE_PIX_FMT", raising=False)
        mp.delenv("MAUA_SUBFRAMES", raising=False)
        written = render.render_shard(g, lat, noise, 0, n / 30, batch, 1920, out, None, 1.0, bends, {}, False, "slow", None,
                                      pipe_pix_fmt="yuv420p10le")
    assert written == n and os.path.getsize(out + ".yuv420p10le") == n * 1920 * 1080 * 3
    planes = np.fromfile(out + ".yuv420p10le", dtype="<u2").reshape(n, -1)
    assert planes.max() <= 960 and planes.min() >= 64 and planes[:, :1920 * 1080].std() > 1
