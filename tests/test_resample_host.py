"""CPU: the definition of the device resampler and everything of it that runs on the host.

  * the numpy twin (tests/resample_ref.py) against Pillow itself, bit for bit, on a committed case list;
  * maua_resample_coeffs against the twin's tables, integer for integer, and its refusals;
  * render.FrameResize geometry on hand-computed values; the frame shapes the sink and the transports see; environment and namespace
    parsing; the pinned parameter lists; the dispatch without a delivery size, call for call;
  * four deliberately wrong twins, each told apart from the definition by the case list the GPU tests run.
"""
import argparse
import inspect

import numpy as np
import pytest

import resample_ref as rr

EINVAL, ENOSYS = -22, -38

# ((W, H), (w, h), box): up-scale, down-scale and mixed; integer crops; one identity axis
PIL_GEOMETRIES = [
    ((37, 23), (64, 40), None), ((37, 23), (11, 7), None), ((64, 48), (20, 90), None), ((50, 40), (50, 17), None),
    ((50, 40), (31, 40), (3, 2, 47, 39)), ((130, 70), (33, 21), (10, 0, 120, 70)), ((5, 3), (65, 17), None), ((90, 60), (9, 6), None),
    ((60, 45), (40, 30), None), ((40, 30), (40, 30), (1, 1, 39, 29)),
]
AXES = [(37, 0, 37, 64), (37, 0, 37, 11), (50, 3, 47, 31), (130, 10, 120, 33), (5, 0, 5, 65), (90, 0, 90, 9), (60, 0, 60, 40), (7, 6, 7, 3),
        (1024, 0, 1024, 1920), (1024, 0, 1024, 3840), (2048, 0, 2048, 3840), (1024, 0, 1024, 512), (1024, 224, 800, 1080)]


def _images(W, H, seed):
    r = np.random.default_rng(seed)
    return r.integers(0, 256, (H, W, 3), dtype=np.uint8), (r.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)


@pytest.mark.parametrize("filt", list(rr.FILTERS))
def test_twin_equals_pillow_bit_for_bit(filt):
    Image = pytest.importorskip("PIL.Image")
    flt = {"box": Image.BOX, "bilinear": Image.BILINEAR, "hamming": Image.HAMMING, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[filt]
    for n, ((W, H), size, box) in enumerate(PIL_GEOMETRIES):
        for img in _images(W, H, n):
            want = np.array(Image.fromarray(img).resize(size, flt, box=box))
            assert np.array_equal(rr.resize(img, size, filt, box), want), (filt, W, H, size, box)


def test_sixteen_bit_twin_extends_the_eight_bit_rule():
    """On codes that are 257 x an 8-bit value the 16-bit pass is the 8-bit sum scaled by 257 before the shift: both stay within one code of
    each other after scaling, and a constant frame stays constant at both depths."""
    img8 = _images(23, 17, 3)[0]
    img16 = img8.astype(np.uint16) * 257
    for filt in rr.FILTERS:
        a, b = rr.resize(img8, (40, 9), filt).astype(np.int64) * 257, rr.resize(img16, (40, 9), filt).astype(np.int64)
        assert np.abs(a - b).max() <= 2 * 257, filt
        for fill, dtype in ((255, np.uint8), (65535, np.uint16), (21845, np.uint16)):
            assert (rr.resize(np.full((9, 11, 3), fill, dtype), (30, 4), filt) == fill).all(), (filt, fill)


@pytest.mark.parametrize("filt", list(rr.FILTERS))
def test_native_coefficients_equal_the_twins_integer_for_integer(built_lib, filt):
    from maua_stylegan2_amd import _lib

    for n, in0, in1, m in AXES:
        rc, k, bounds = _lib.resample_coeffs(n, in0, in1, m, filt)
        want_k, want_b = rr.coeffs(n, in0, in1, m, filt)
        assert rc == want_k.shape[1] == rr.ksize_of(in0, in1, m, filt), (filt, n, in0, in1, m, rc)
        assert np.array_equal(k, want_k) and np.array_equal(bounds, want_b), (filt, n, in0, in1, m)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= n).all() and (bounds[:, 1] <= rc).all()


def test_native_coefficients_refusals(built_lib):
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    k, b = np.zeros(64 * 64, np.int32), np.zeros((64, 2), np.int32)
    call = lambda n, in0, in1, m, f, cap=k.size, kp=k.ctypes.data, bp=b.ctypes.data: lib.maua_resample_coeffs(n, in0, in1, m, f, kp, bp, cap)  # noqa: E731
    assert call(10, 0, 10, 20, 4) == 7 and call(10, 0, 10, 20, 0) == 3
    for bad in ((0, 0, 10, 20, 4), (10, 0, 10, 0, 4), (10, -1, 10, 20, 4), (10, 5, 5, 20, 4), (10, 6, 5, 20, 4), (10, 0, 11, 20, 4),
                (10, 0, 10, 20, 5), (10, 0, 10, 20, -1)):
        assert call(*bad) == EINVAL, bad
    assert call(10, 0, 10, 20, 4, cap=20 * 7 - 1) == EINVAL and call(10, 0, 10, 20, 4, cap=20 * 7) == 7
    assert call(10, 0, 10, 20, 4, kp=None) == EINVAL and call(10, 0, 10, 20, 4, bp=None) == EINVAL
    # taps: lanczos 10 : 1 is 2 * 30 + 1 = 61, 10.5 : 1 is 2 * 32 + 1 = 65 > MAUA_RESAMPLE_MAX_TAPS
    assert call(640, 0, 640, 64, 4) == 61 and call(672, 0, 672, 64, 4) == ENOSYS and call(6400, 0, 6400, 64, 1) == ENOSYS
    assert _lib.resample_coeffs(672, 0, 672, 64, "lanczos") == (ENOSYS, None, None) and _lib.resample_coeffs(8, 0, 8, 4, "sinc")[0] == EINVAL
    assert _lib.RESAMPLE_FILTERS == rr.FILTER_IDS and _lib.RESAMPLE_MAX_TAPS == rr.MAX_TAPS


def test_frame_resize_geometry_on_hand_computed_values(built_lib):
    from maua_stylegan2_amd import render

    geo = lambda size, fit, W, H: render.FrameResize(size, fit=fit).geometry(W, H)  # noqa: E731
    # crop: 1024^2 -> 16:9 keeps (1024 * 1080 + 960) // 1920 = 576 rows, centred at (1024 - 576) // 2 = 224
    assert geo("1920x1080", "crop", 1024, 1024) == ((0, 224, 1024, 800), (0, 0, 1920, 1080))
    # crop: 2048 x 1024 -> UHD keeps (1024 * 3840 + 1080) // 2160 = 1820 columns from (2048 - 1820) // 2 = 114
    assert geo((3840, 2160), "crop", 2048, 1024) == ((114, 0, 1934, 1024), (0, 0, 3840, 2160))
    assert geo("512x512", "crop", 1024, 1024) == ((0, 0, 1024, 1024), (0, 0, 512, 512))
    assert geo("1000x10", "crop", 10, 1000) == ((0, 499, 10, 500), (0, 0, 1000, 10))           # (10 * 10 + 500) // 1000 = 0 -> 1 row
    assert geo("1920x1080", "stretch", 1024, 1024) == ((0, 0, 1024, 1024), (0, 0, 1920, 1080))
    # pad: 1024^2 into 1920 x 1080 is a 1080^2 window at x = 420; 2048 x 1024 into 1280 x 720 is 1280 x 640 at y = 40
    assert geo("1920x1080", "pad", 1024, 1024) == ((0, 0, 1024, 1024), (420, 0, 1080, 1080))
    assert geo("1280x720", "pad", 2048, 1024) == ((0, 0, 2048, 1024), (0, 40, 1280, 640))
    # evenness: 1000 x 700 into 501 x 301: (1000 * 301 + 350) // 700 = 430 wide, 301 -> 300 high, offsets (35 & ~1, 0 & ~1)
    assert geo("501x301", "pad", 1000, 700) == ((0, 0, 1000, 700), (34, 0, 430, 300))
    assert geo("100x50", "pad", 1000, 10) == ((0, 0, 1000, 10), (0, 24, 100, 2))                # (10 * 100 + 500) // 1000 = 1 -> 2 rows
    assert geo("641x361", "pad", 1024, 1024)[1] == (140, 0, 360, 360)                           # ((641 - 360) // 2) & ~1 = 140
    for fit in render.RESIZE_FITS:
        for W, H, w, h in ((1024, 1024, 1920, 1080), (2048, 1024, 3840, 2160), (1000, 700, 501, 301), (33, 77, 64, 64), (5, 3, 2, 2)):
            assert geo((w, h), fit, W, H) == rr.fit_geometry(W, H, w, h, fit)
            (x0, y0, x1, y1), (x, y, dw, dh) = geo((w, h), fit, W, H)
            assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H and 0 <= x and x + dw <= w and 0 <= y and y + dh <= h
    assert render.FrameResize("1280X720").size == (1280, 720) and render.FrameResize((8, 6), "box", "pad").key() == (8, 6, "box", "pad")
    for bad in ("1920", "1920x", "axb", "0x10", "10x-2", "1x2x3", (1, 2, 3)):
        with pytest.raises(ValueError, match="deliver_size|delivery size"):
            render.FrameResize(bad)
    with pytest.raises(ValueError, match="--deliver_filter"):
        render.FrameResize("8x8", filter="sinc")
    with pytest.raises(ValueError, match="--deliver_fit"):
        render.FrameResize("8x8", fit="fill")
    with pytest.raises(ValueError, match="--deliver_fit pad"):
        render.FrameResize("1x8", fit="pad").geometry(10, 10)


def test_stream_frame_shape_and_sink_dimensions_per_pipe_format(built_lib):
    from maua_stylegan2_amd import render

    g = type("G", (), {"size": 1024})
    resize = render.FrameResize("1280x720")
    shape = render._stream_frame_shape
    assert shape(g, 1024, "rgb24", resize) == (720, 1280, 3) and shape(g, 1920, "rgb24", resize) == (720, 1280, 3)
    assert shape(g, 1024, "yuv420p", resize) == (1280 * 720 * 3 // 2,)
    assert shape(g, 1024, "mjpeg", resize) == (render.mjpeg_slot_bytes(1280, 720),)
    for fmt in render.DEEP_PIX_FMTS:
        assert shape(g, 1024, fmt, resize) == (render.deep_frame_bytes(fmt, 1280, 720),)
    assert shape(g, 1024, "rgb24") == (1024, 1024, 3) == shape(g, 1024, "rgb24", None) and shape(g, 1920) == (1080, 1920, 3)  # as before
    # the sink a render opens is built from the delivery size; odd sides are refused by name for the formats that need even ones
    odd = render.FrameResize("1281x720")
    for fmt in ("yuv420p",) + render.DEEP_PIX_FMTS:
        with pytest.raises(ValueError, match="--deliver_size 1281x720"):
            render.check_deliver_size(odd, fmt)
        with pytest.raises(ValueError, match="--deliver_size 1281x720"):
            render.render_delivered(None, np.zeros((4, 1, 1)), [], 0, 1.0, 4, 1024, None, None, 1.0, [], {}, False, "slow", None, pipe_pix_fmt=fmt,
                                    resize=odd)
    for fmt in ("rgb24", "mjpeg"):
        render.check_deliver_size(odd, fmt)
    render.check_deliver_size(None, "yuv420p")
    seen = []

    class Sink(render.FrameSink):
        def __init__(self, output_file, width, height, *a, **kw):
            seen.append((width, height, kw.get("pix_fmt")))
            raise RuntimeError("far enough")

    import unittest.mock as mock

    with mock.patch.object(render, "FrameSink", Sink), mock.patch.object(render, "device_of", lambda g: None):
        for fmt in ("rgb24", "yuv420p", "mjpeg", "rgb48le", "yuv420p10le"):
            with pytest.raises(RuntimeError, match="far enough"):
                render.render_delivered(None, np.zeros((4, 1, 1)), [], 0, 1.0, 4, 1024, None, None, 1.0, [], {}, False, "slow", None,
                                        pipe_pix_fmt=fmt, resize=resize)
        with pytest.raises(RuntimeError, match="far enough"):
            render.render_delivered(None, np.zeros((4, 1, 1)), [], 0, 1.0, 4, 1920, None, None, 1.0, [], {}, False, "slow", None)
    assert seen == [(1280, 720, f) for f in ("rgb24", "yuv420p", "mjpeg", "rgb48le", "yuv420p10le")] + [(1920, 1080, "rgb24")]
    # a delivered frame that happens to be 2048 px wide is not the reference's wide output: the sink takes it as it is, PIL is not reached
    import sys

    with mock.patch.dict(sys.modules, {"PIL": None, "PIL.Image": None}):
        sink = render.FrameSink(None, 2048, 1152, 30)
        sink.write(np.zeros((1152, 2048, 3), np.uint8))
        assert sink.count == 1


def test_environment_and_namespace_parsing(monkeypatch, built_lib):
    from maua_stylegan2_amd import generate_audiovisual as gav
    from maua_stylegan2_amd import render

    for name in ("MAUA_DELIVER_SIZE", "MAUA_DELIVER_FILTER", "MAUA_DELIVER_FIT"):
        monkeypatch.delenv(name, raising=False)
    assert render._resize_from_env() is None
    monkeypatch.setenv("MAUA_DELIVER_FILTER", "nonsense")  # not read without a size
    assert render._resize_from_env() is None
    monkeypatch.setenv("MAUA_DELIVER_SIZE", "1920x1080")
    with pytest.raises(ValueError, match="--deliver_filter"):
        render._resize_from_env()
    monkeypatch.setenv("MAUA_DELIVER_FILTER", "bicubic")
    monkeypatch.setenv("MAUA_DELIVER_FIT", "pad")
    assert render._resize_from_env().key() == (1920, 1080, "bicubic", "pad")
    monkeypatch.delenv("MAUA_DELIVER_FILTER")
    monkeypatch.delenv("MAUA_DELIVER_FIT")
    assert render._resize_from_env().key() == (1920, 1080, "lanczos", "crop")

    ns = argparse.Namespace
    assert gav._resize_of(ns()) is None and gav._resize_of(ns(deliver_size=None, deliver_filter="box")) is None
    assert gav._resize_of(ns(deliver_size="640x360")).key() == (640, 360, "lanczos", "crop")
    assert gav._resize_of(ns(deliver_size=(640, 360), deliver_filter="hamming", deliver_fit="stretch")).key() == (640, 360, "hamming", "stretch")
    args = gav.build_parser().parse_args(["--ckpt", "c.pt", "--audio_file", "a.wav"])
    assert (args.deliver_size, args.deliver_filter, args.deliver_fit) == (None, "lanczos", "crop") and gav._resize_of(args) is None
    args = gav.build_parser().parse_args(["--ckpt", "c.pt", "--audio_file", "a.wav", "--deliver_size", "3840x2160", "--deliver_filter", "bicubic",
                                          "--deliver_fit", "pad"])
    assert gav._resize_of(args).key() == (3840, 2160, "bicubic", "pad")
    with pytest.raises(SystemExit):
        gav.build_parser().parse_args(["--ckpt", "c.pt", "--audio_file", "a.wav", "--deliver_filter", "sinc"])


def test_pinned_signatures_are_unchanged_and_render_delivered_extends_them(built_lib):
    from maua_stylegan2_amd import generate_audiovisual as gav
    from maua_stylegan2_amd import render

    shard = list(inspect.signature(render.render_shard).parameters)
    assert len(shard) == 17 and shard[-2:] == ["transport", "pipe_pix_fmt"]
    assert list(inspect.signature(render.render_folded).parameters) == shard + ["fold"]
    delivered = inspect.signature(render.render_delivered).parameters
    assert list(delivered) == shard + ["fold", "resize"] and delivered["fold"].default is None and delivered["resize"].default is None
    assert list(inspect.signature(render.render).parameters)[-1] == "ffmpeg_preset" and len(inspect.signature(render.render).parameters) == 14
    for fn in (render.render, render.render_shard, render.render_folded, gav.generate):
        assert not {"resize", "deliver_size", "deliver_filter", "deliver_fit"} & set(inspect.signature(fn).parameters)
    assert list(inspect.signature(render.resize_frames).parameters) == ["frames", "resize", "scratch"]


def test_four_wrong_twins_are_told_apart_by_the_gpu_case_list():
    """Vertical pass first, no rounded intermediate, round-to-nearest in place of the +0.5 truncation, unnormalised weights: each differs
    from the definition on at least one geometry (and input) of the list the GPU tests compare bit for bit."""
    import test_resample_gpu as gpu_cases

    for variant in ("vertical_first", "no_intermediate", "nearest", "unnormalised"):
        told = []
        for n, (name, batch, (W, H), size, filt, box, _, _) in enumerate(gpu_cases.SOURCES):
            frames = gpu_cases.make_frames("u8", batch, H, W, seed=100 + n, binary=bool(n % 2))
            if not np.array_equal(rr.resize(frames, size, filt, box, variant=variant), rr.resize(frames, size, filt, box)):
                told.append(name)
        assert told, variant
        print(f"{variant}: told apart by {len(told)} of {len(gpu_cases.SOURCES)} geometries ({', '.join(told[:4])} ...)")
