"""CPU: the deep pipe formats (rgb48le, yuv420p10le, yuv422p10le, yuv444p10le) without a device — the numpy twins of csrc/deep_frames.hip
(tests/deep_ref.py: the oracles the GPU tests in tests/test_deep_frames_gpu.py compare the kernels against, bit for bit) pinned to known
answers, to the float64 definition of BT.709 and to the 8-bit twins; the frame sink's deep branch, the fallback file, the CLI choices, the
transport frame shape, the refusal of a temporal fold, and the launchers' argument checks."""
import json
import os

import numpy as np
import pytest

import deep_ref as dr
from test_host_logic import pil_bilinear_upscale_restated
from test_yuv420_host import _stand_in_ffmpeg

EINVAL, ENOSYS = -22, -38
DEEP = ("rgb48le", "yuv420p10le", "yuv422p10le", "yuv444p10le")
BYTES_PER_PIXEL = {"rgb48le": 6, "yuv444p10le": 6, "yuv422p10le": 4, "yuv420p10le": 3}


# ------------------------------------------------------------------------------------------------------------------------ the matrix
def test_known_answers_per_pixel_and_as_uniform_blocks():
    for name, (rgb, (y, cb, cr)) in dr.KNOWN.items():
        px = np.array(rgb, np.int64)
        assert int(dr.luma(px)) == y, name
        for n in (1, 2, 4):  # a uniform block of n pixels gives the pixel's own chroma
            got_cb, got_cr = dr.chroma(n * px, n)
            assert (int(got_cb), int(got_cr)) == (cb, cr), (name, n)
    # ... and through the planar layouts: one 2 x 2 block per colour
    frame = np.zeros((1, 2, 2 * len(dr.KNOWN), 3), np.uint16)
    for i, (rgb, _) in enumerate(dr.KNOWN.values()):
        frame[0, :, 2 * i: 2 * i + 2] = rgb
    want = np.array([v[1] for v in dr.KNOWN.values()])
    w = frame.shape[2]
    for sub in dr.SUBSAMPLINGS:
        planar = dr.yuv_p10(frame, sub)[0]
        assert planar.shape == (dr.frame_samples(sub, 2, w),)
        bh, bw = dr.BLOCK[sub]
        assert np.array_equal(planar[:w], np.repeat(want[:, 0], 2)) and np.array_equal(planar[w:2 * w], np.repeat(want[:, 0], 2))
        u = planar[2 * w:].reshape(2, 2 // bh, w // bw)
        assert np.array_equal(u[0], np.tile(np.repeat(want[:, 1], 2 // bw), (2 // bh, 1))), sub
        assert np.array_equal(u[1], np.tile(np.repeat(want[:, 2], 2 // bw), (2 // bh, 1))), sub


def _real_definition(mean):
    """BT.709 limited range at 10 bits in float64 on R'G'B' in [0, 1]: Kr = 0.2126, Kg = 0.7152, Kb = 0.0722."""
    r, g, b = mean[..., 0], mean[..., 1], mean[..., 2]
    ey = 0.2126 * r + 0.7152 * g + 0.0722 * b
    return 64.0 + 876.0 * ey, 512.0 + 896.0 * (b - ey) / (2 * (1 - 0.0722)), 512.0 + 896.0 * (r - ey) / (2 * (1 - 0.2126))


def test_integer_matrix_against_the_float64_definition():
    """4096 random pixels and, per subsampling, 4096 random blocks: the integer formula is the exact rational value of the definition
    rounded half up, so every sample is within 0.5 (+ 1e-9 for the float64 evaluation) of it.  No exemptions."""
    rng = np.random.default_rng(709)
    px = rng.integers(0, 65536, (4096, 3), dtype=np.int64)
    px[:len(dr.KNOWN)] = [v[0] for v in dr.KNOWN.values()]
    y_real, _, _ = _real_definition(px / 65535.0)
    err = np.abs(dr.luma(px) - y_real)
    print(f"[deep] luma: max |integer - float64| = {err.max():.6f}")
    assert err.max() <= 0.5 + 1e-9
    for sub in dr.SUBSAMPLINGS:
        n = dr.BLOCK[sub][0] * dr.BLOCK[sub][1]
        blocks = rng.integers(0, 65536, (4096, n, 3), dtype=np.int64)
        blocks[:len(dr.KNOWN)] = np.array([v[0] for v in dr.KNOWN.values()])[:, None, :]
        sums = blocks.sum(axis=1)
        cb, cr = dr.chroma(sums, n)
        _, cb_real, cr_real = _real_definition(sums / n / 65535.0)
        e_b, e_r = np.abs(cb - cb_real).max(), np.abs(cr - cr_real).max()
        print(f"[deep] chroma {sub}: max |integer - float64| = {e_b:.6f} (Cb), {e_r:.6f} (Cr)")
        assert e_b <= 0.5 + 1e-9 and e_r <= 0.5 + 1e-9, sub


def test_grey_axis_and_ranges():
    """R = G = B gives Cb = Cr = 512 at every level and block size; Y stays in 64 .. 940 and chroma in 64 .. 960 on random operands and on
    the corners of the cube."""
    grey = np.arange(65536, dtype=np.int64)
    rgb = np.stack([grey] * 3, axis=-1)
    for n in (1, 2, 4):
        cb, cr = dr.chroma(n * rgb, n)
        assert (cb == 512).all() and (cr == 512).all(), n
    y = dr.luma(rgb)
    assert y[0] == 64 and y[-1] == 940 and (np.diff(y) >= 0).all()
    rng = np.random.default_rng(5)
    px = np.concatenate([rng.integers(0, 65536, (100000, 3), dtype=np.int64),
                         np.array([[r, g, b] for r in (0, 65535) for g in (0, 65535) for b in (0, 65535)], np.int64)])
    y = dr.luma(px)
    assert y.min() >= 64 and y.max() <= 940
    for n in (1, 2, 4):
        sums = px * n if n == 1 else px[rng.integers(0, len(px), (len(px), n))].sum(axis=1)
        cb, cr = dr.chroma(sums, n)
        assert min(cb.min(), cr.min()) >= 64 and max(cb.max(), cr.max()) <= 960, n
    corners = px[-8:]
    cb, cr = dr.chroma(corners, 1)
    assert {int(cb.min()), int(cb.max()), int(cr.min()), int(cr.max())} == {64, 960}


# ------------------------------------------------------------------------------------------------------------------------ the quantiser
def test_quantiser_edges_and_agreement_with_the_8_bit_one():
    """NaN and -inf give 0, +inf and 1 give 65535; q16 // 257 differs from the 8-bit code by at most 1 everywhere: on 2 * 10^6 random fp32
    values, and on every 8-bit and 16-bit code boundary with its two fp32 neighbours."""
    f = dr.F32
    assert list(dr.quant16([np.nan, -np.inf, np.inf, 1.0, -1.0, 0.0, -0.0, 3.0, -3.0])) == [0, 0, 65535, 65535, 0, 32767, 32767, 65535, 0]
    rng = np.random.default_rng(16)
    x = rng.uniform(-1.05, 1.05, 2_000_000).astype(f)
    edges = []
    for levels in (255, 65535):
        v = (np.arange(levels + 1, dtype=np.float64) / (levels / 2.0) - 1.0).astype(f)
        edges += [v, np.nextafter(v, f(-np.inf)), np.nextafter(v, f(np.inf))]
    for name, vals in (("random", x), ("boundaries", np.concatenate(edges))):
        q16, q8 = dr.quant16(vals).astype(np.int64), dr.quant8(vals).astype(np.int64)
        diff = np.abs(q16 // 257 - q8)
        print(f"[deep] quantiser, {name}: q16 // 257 != q8 on {int((diff != 0).sum())} of {vals.size} values, max difference {int(diff.max())}")
        assert diff.max() <= 1, name
    assert dr.quant16(x).min() == 0 and dr.quant16(x).max() == 65535


# ------------------------------------------------------------------------------------------------------------------------ the resize
RESIZE_BOXES = [(1, 1, 4, 3), (5, 7, 9, 11), (13, 2, 30, 5), (8, 6, 8, 6), (3, 3, 4, 4), (17, 9, 19, 64), (33, 5, 66, 6), (97, 4, 114, 7)]


def test_resize_twin_constant_frames_the_float64_filter_and_the_8_bit_twin():
    """A constant frame stays constant (a tap pair's coefficients sum to 2^22 exactly).  Against the same 2-tap filter in float64 the bound
    is 1.1 codes: 0.5 for each of the two roundings — the horizontal one passes through the vertical pass with weight at most 1 — plus the
    coefficient quantisation, at most 2^-23 per coefficient on a sample of at most 65535, i.e. 65535 * 2^-22 < 0.016 per tap pair and pass.
    With 8-bit operands and the clamp at 255 the twin IS the 8-bit twin that is pinned to PIL."""
    rng = np.random.default_rng(22)
    worst = 0.0
    for cw, ch, ow, oh in RESIZE_BOXES:
        for fill in (0, 1, 32768, 65535):
            frame = np.full((ch + 3, cw + 4, 3), fill, np.uint16)
            assert (dr.crop_resize(frame, 2, 1, cw, ch, ow, oh) == fill).all(), (cw, ch, ow, oh, fill)
        frame = rng.integers(0, 65536, (ch + 3, cw + 4, 3), dtype=np.uint16)
        frame[1, 2], frame[ch, cw + 1] = 65535, 0
        got = dr.crop_resize(frame, 2, 1, cw, ch, ow, oh)
        assert got.shape == (oh, ow, 3) and got.min() >= 0 and got.max() <= 65535
        err = np.abs(got - dr.crop_resize_float64(frame, 2, 1, cw, ch, ow, oh)).max()
        worst = max(worst, err)
        assert err <= 1.1, ((cw, ch, ow, oh), err)
        small = rng.integers(0, 256, (ch + 3, cw + 4, 3), dtype=np.uint8)
        assert np.array_equal(dr.crop_resize(small, 2, 1, cw, ch, ow, oh, top=255), pil_bilinear_upscale_restated(small, 2, 1, cw, ch, ow, oh))
    print(f"[deep] resize twin: max |integer - float64 filter| = {worst:.4f} codes")
    assert np.array_equal(dr.crop_resize_u16(frame[None], 2, 1, cw, ch, ow, oh)[0], got)


# ------------------------------------------------------------------------------------------------------------------------ the sink
@pytest.mark.parametrize("fmt", DEEP)
def test_frame_sink_pipes_deep_frames_to_the_encoder(tmp_path, monkeypatch, built_lib, fmt):
    from maua_stylegan2_amd import render

    _stand_in_ffmpeg(tmp_path, monkeypatch)
    w, h, n = 6, 4, 3
    n_bytes = w * h * BYTES_PER_PIXEL[fmt]
    assert render.deep_frame_bytes(fmt, w, h) == n_bytes
    frames = np.random.default_rng(3).integers(0, 256, (n, n_bytes), dtype=np.uint8)
    out = str(tmp_path / "clip.mp4")
    sink = render.FrameSink(out, w, h, 24, audio_file="song.wav", offset=1.5, duration=2.0, ffmpeg_preset="veryfast", pix_fmt=fmt)
    for frame in frames:
        sink.write(frame)
    for bad in (frames[0][:-1], np.zeros((h, w, 3), np.uint8), np.zeros(n_bytes + 2, np.uint8), np.zeros(n_bytes // 2, np.uint16)):
        with pytest.raises(ValueError, match=f"{fmt} frame"):
            sink.write(bad)
    sink.close()
    assert sink.count == n
    args = json.load(open(out + ".args.json"))
    out_fmt = "yuv420p10le" if fmt == "rgb48le" else fmt
    tags = [] if fmt == "rgb48le" else ["-colorspace", "bt709", "-color_primaries", "bt709", "-color_trc", "bt709", "-color_range", "tv"]
    assert args == (["-hide_banner", "-y", "-v", "warning", "-f", "rawvideo", "-pix_fmt", fmt, "-framerate", "24", "-s", f"{w}x{h}", "-i", "pipe:",
                     "-ss", "1.5", "-t", "2.0", "-guess_layout_max", "0", "-i", "song.wav",
                     "-r", "24", "-vcodec", "libx265", "-pix_fmt", out_fmt, "-tag:v", "hvc1", "-preset", "veryfast"] + tags
                    + ["-b:a", "320K", "-ac", "2", out])
    assert np.array_equal(np.fromfile(out, dtype=np.uint8), frames.reshape(-1))


@pytest.mark.parametrize("fmt", DEEP)
def test_frame_sink_deep_fallback_file_without_a_binary(tmp_path, monkeypatch, built_lib, capsys, fmt):
    from maua_stylegan2_amd import render

    monkeypatch.setattr(render.shutil, "which", lambda name: None)
    w, h, n = 10, 6, 4
    n_bytes = w * h * BYTES_PER_PIXEL[fmt]
    frames = np.arange(n * n_bytes, dtype=np.int64).astype(np.uint8).reshape(n, -1)
    out = str(tmp_path / "clip.mp4")
    sink = render.FrameSink(out, w, h, 30, pix_fmt=fmt)
    for frame in frames:
        sink.write(frame)
    sink.close()
    assert not os.path.exists(out + ".rgb24") and os.path.getsize(out + "." + fmt) == n * n_bytes
    assert np.array_equal(np.fromfile(out + "." + fmt, dtype=np.uint8), frames.reshape(-1))
    printed = capsys.readouterr().out
    out_fmt = "yuv420p10le" if fmt == "rgb48le" else fmt
    assert f"-f rawvideo -pix_fmt {fmt} -framerate 30 -s {w}x{h} -i {out}.{fmt}" in printed
    assert f"-vcodec libx265 -pix_fmt {out_fmt} -tag:v hvc1 -preset slow" in printed
    assert ("-colorspace bt709" in printed) == (fmt != "rgb48le") and "smpte170m" not in printed
    for bad_w, bad_h in ((5, 4), (4, 5)):
        with pytest.raises(ValueError, match="even"):
            render.FrameSink(None, bad_w, bad_h, 30, pix_fmt=fmt)


def test_frame_sink_rgb24_vector_is_unchanged(tmp_path, monkeypatch, built_lib):
    from maua_stylegan2_amd import render

    _stand_in_ffmpeg(tmp_path, monkeypatch)
    w, h = 4, 2
    frame = np.arange(h * w * 3, dtype=np.uint8).reshape(h, w, 3)
    out = str(tmp_path / "clip.mp4")
    sink = render.FrameSink(out, w, h, 30, ffmpeg_preset="slow")
    sink.write(frame)
    sink.close()
    assert json.load(open(out + ".args.json")) == ["-hide_banner", "-y", "-v", "warning", "-f", "rawvideo", "-pix_fmt", "rgb24", "-framerate", "30",
                                                   "-s", f"{w}x{h}", "-i", "pipe:", "-r", "30", "-vcodec", "libx264", "-pix_fmt", "yuv420p",
                                                   "-preset", "slow", out]
    assert np.array_equal(np.fromfile(out, dtype=np.uint8), frame.reshape(-1))


# ------------------------------------------------------------------------------------------------------------------------ the plumbing
def test_cli_choices_and_format_names(monkeypatch, built_lib):
    import inspect

    from maua_stylegan2_amd import generate_audiovisual as gav
    from maua_stylegan2_amd import render

    assert render.PIPE_PIX_FMTS == ("rgb24", "yuv420p", "mjpeg") and render.DEEP_PIX_FMTS == DEEP
    parser = gav.build_parser()
    assert parser.parse_args([]).pipe_pix_fmt == "rgb24"
    for fmt in DEEP + render.PIPE_PIX_FMTS:
        assert parser.parse_args(["--pipe_pix_fmt", fmt]).pipe_pix_fmt == fmt
    for bad in ("nv12", "yuv444p", "mjpeg:85", "", "yuv420p10", "rgb48be", "yuv420p12le"):
        with pytest.raises(SystemExit):
            parser.parse_args(["--pipe_pix_fmt", bad])
    monkeypatch.delenv("MAUA_PIPE_PIX_FMT", raising=False)
    for fmt in DEEP:
        assert render._pipe_pix_fmt(fmt) == fmt
        monkeypatch.setenv("MAUA_PIPE_PIX_FMT", fmt)
        assert render._pipe_pix_fmt(None) == fmt and render._pipe_pix_fmt("rgb24") == "rgb24"
        monkeypatch.delenv("MAUA_PIPE_PIX_FMT")
    for bad in ("nv12", "yuv444p", "rgb48be"):
        with pytest.raises(ValueError, match="pixel format"):
            render._pipe_pix_fmt(bad)
        with pytest.raises(ValueError, match="pixel format"):
            render.FrameSink(None, 4, 4, 30, pix_fmt=bad)
    # no new parameter on the pinned entries; the frame kind is synthesize's trailing keyword
    assert list(inspect.signature(render.render_shard).parameters)[-2:] == ["transport", "pipe_pix_fmt"]
    assert list(inspect.signature(render.render_folded).parameters)[-3:] == ["transport", "pipe_pix_fmt", "fold"]
    assert list(inspect.signature(render.synthesize).parameters)[-1] == "frames"
    assert inspect.signature(render.synthesize).parameters["frames"].default == "u8"
    with pytest.raises(ValueError, match="frame kind"):
        next(render.synthesize(None, [], [], 1, frames="u16"))


def test_transport_frame_shape_for_every_format_and_out_size(built_lib):
    from maua_stylegan2_amd import render

    class G:
        size = 1024

    shape = render._stream_frame_shape
    for size, dims in ((1024, {1024: (1024, 1024), 1920: (1920, 1080), 1080: (1080, 1920)}),
                       (512, {512: (512, 512), 1920: (1024, 512), 1080: (512, 1024)}),
                       (64, {512: (64, 64), 1920: (128, 64), 1080: (64, 128)})):
        G.size = size
        for out_size, (w, h) in dims.items():
            assert shape(G, out_size) == (h, w, 3)  # the 8-bit shapes, as they were
            assert shape(G, out_size, "yuv420p") == (h * w * 3 // 2,)
            for fmt in DEEP:
                assert shape(G, out_size, fmt) == (h * w * BYTES_PER_PIXEL[fmt],), (size, out_size, fmt)
                assert shape(G, out_size, fmt) == (render.deep_frame_bytes(fmt, w, h),)


@pytest.mark.parametrize("fmt", DEEP)
def test_a_temporal_fold_is_refused_before_a_frame_is_rendered(monkeypatch, built_lib, fmt):
    from maua_stylegan2_amd import render

    def no_frames(*a, **k):
        raise AssertionError("a frame was rendered")

    monkeypatch.setattr(render, "synthesize", no_frames)
    monkeypatch.setattr(render, "FrameSink", no_frames)
    monkeypatch.setattr(render, "device_of", no_frames)
    args = (None, np.zeros((8, 1)), [], 0, 1.0, 4, 512, None, None, 1.0, [], {}, False, "slow", None)
    with pytest.raises(ValueError, match="8-bit only"):
        render.render_folded(*args, pipe_pix_fmt=fmt, fold=render.TemporalFold(2))
    monkeypatch.setenv("MAUA_SUBFRAMES", "4")
    with pytest.raises(ValueError, match="8-bit only"):
        render.render_shard(*args, pipe_pix_fmt=fmt)
    monkeypatch.setenv("MAUA_PIPE_PIX_FMT", fmt)
    with pytest.raises(ValueError, match="8-bit only"):
        render.render(*args[:8])
    monkeypatch.setenv("MAUA_SUBFRAMES", "1")  # the plain render is not refused: it gets as far as the generator
    with pytest.raises(AssertionError, match="a frame was rendered"):
        render.render_shard(*args, pipe_pix_fmt=fmt)
    monkeypatch.setattr(render, "_output_dims", lambda out_size: (63, 64))
    with pytest.raises(ValueError, match="even"):
        render.render_shard(*args, pipe_pix_fmt=fmt)


# ------------------------------------------------------------------------------------------------------------------------ the launchers
def test_launchers_reject_bad_arguments_without_a_device(built_lib):
    """Validation runs before any HIP call: NULL buffers, non-positive sizes, odd sizes per subsampling and a bad subsampling are refused;
    batch 0 is a successful no-op of the two planar entries and MAUA_EINVAL for the two that mirror their 8-bit siblings."""
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    fake = 0x1000  # never dereferenced
    for name, n_args in (("maua_frames_to_u16", 6), ("maua_crop_resize_u16", 12), ("maua_rgb48_to_yuv_p10", 7), ("maua_frames_to_yuv_p10_f32", 7)):
        assert name in _lib.exported_symbols() and len(_lib._SIGNATURES[name][1]) == n_args
    u16 = lambda b, h, w, src=fake, dst=fake: lib.maua_frames_to_u16(src, dst, b, h, w, None)  # noqa: E731
    for b, h, w in [(0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, -2, 4), (1, 4, -1)]:
        assert u16(b, h, w) == EINVAL, (b, h, w)
    assert u16(1, 4, 4, src=None) == EINVAL and u16(1, 4, 4, dst=None) == EINVAL
    resize = lambda box, b=2, in_h=9, in_w=12, src=fake, dst=fake: lib.maua_crop_resize_u16(src, dst, b, in_h, in_w, *box, None)  # noqa: E731
    ok = (2, 1, 8, 6, 16, 12)
    assert resize(ok, src=None) == EINVAL and resize(ok, dst=None) == EINVAL
    for kw in (dict(b=0), dict(b=-1), dict(in_h=0), dict(in_w=-3)):
        assert resize(ok, **kw) == EINVAL, kw
    for box, code in [((2, 1, 8, 6, 7, 12), ENOSYS), ((2, 1, 8, 6, 16, 5), ENOSYS), ((5, 1, 8, 6, 16, 12), EINVAL), ((2, 4, 8, 6, 16, 12), EINVAL),
                      ((-1, 1, 8, 6, 16, 12), EINVAL), ((2, -1, 8, 6, 16, 12), EINVAL), ((2, 1, 0, 6, 16, 12), EINVAL),
                      ((2, 1, 8, -1, 16, 12), EINVAL), ((2, 1, 8, 6, 0, 12), EINVAL), ((2, 1, 8, 6, 16, 0), EINVAL)]:
        assert resize(box) == code, box
    for entry in (lib.maua_rgb48_to_yuv_p10, lib.maua_frames_to_yuv_p10_f32):
        call = lambda b, h, w, sub, src=fake, dst=fake: entry(src, dst, b, h, w, sub, None)  # noqa: E731
        for sub in dr.SUBSAMPLINGS:
            for b, h, w in [(1, 0, 4), (1, 4, 0), (1, -2, 4), (1, 4, -2), (-1, 4, 4), (0, 0, 4)]:
                assert call(b, h, w, sub) == EINVAL, (sub, b, h, w)
            assert call(1, 4, 4, sub, src=None) == EINVAL and call(1, 4, 4, sub, dst=None) == EINVAL
            assert call(0, 4, 4, sub) == 0 and call(0, 2, 2, sub, src=None, dst=None) == 0
        # odd sizes: 4:2:0 needs even h and w, 4:2:2 an even w, 4:4:4 takes both (refused here for the NULL buffer only after the size check)
        assert call(1, 3, 4, 420) == EINVAL and call(1, 4, 3, 420) == EINVAL and call(0, 3, 4, 420) == EINVAL and call(0, 4, 5, 420) == EINVAL
        assert call(1, 4, 3, 422) == EINVAL and call(0, 4, 3, 422) == EINVAL and call(0, 3, 4, 422) == 0
        assert call(0, 3, 5, 444) == 0 and call(0, 1, 1, 444) == 0
        for sub in (0, 1, 411, 440, 4200, -420, 10):
            assert call(1, 4, 4, sub) == EINVAL and call(0, 4, 4, sub) == EINVAL, sub
        assert call(70000, 4, 4, 420) == ENOSYS  # more frames than the grid's y
