"""CPU: the planar YUV 4:2:0 pipe format without a device — the integer definition of the conversion (the oracle the GPU tests in
tests/test_yuv420_gpu.py compare csrc/yuv420.hip against, bit for bit), the frame sink's yuv420p branch, the fallback file, the CLI flag
and the way the format travels from generate() into the render loop."""
import argparse
import json
import os
import stat

import numpy as np
import pytest

KNOWN = {  # RGB -> (Y, Cb, Cr), BT.601 limited range
    "white": ((255, 255, 255), (235, 128, 128)),
    "black": ((0, 0, 0), (16, 128, 128)),
    "red": ((255, 0, 0), (81, 90, 240)),
    "green": ((0, 255, 0), (145, 54, 34)),
    "blue": ((0, 0, 255), (41, 240, 110)),
}


def luma_oracle(rgb):
    """[..., 3] uint8 -> Y, int64: 16 + (65481 R + 128553 G + 24966 B + 127500) // 255000."""
    c = rgb.astype(np.int64)
    return 16 + (65481 * c[..., 0] + 128553 * c[..., 1] + 24966 * c[..., 2] + 127500) // 255000


def chroma_oracle(sums):
    """[..., 3] int64 sums of a 2 x 2 block's R, G, B (0 .. 1020) -> (Cb, Cr), int64."""
    sr, sg, sb = (sums[..., i].astype(np.int64) for i in range(3))
    cb = (130560000 + 510000 - 37797 * sr - 74203 * sg + 112000 * sb) // 1020000
    cr = (130560000 + 510000 + 112000 * sr - 93786 * sg - 18214 * sb) // 1020000
    return cb, cr


def yuv420p_oracle(rgb):
    """uint8 [b, h, w, 3] (h, w even) -> uint8 [b, h * w * 3 // 2]: per frame the Y plane, then U, then V (I420)."""
    rgb = np.asarray(rgb)
    b, h, w, _ = rgb.shape
    assert h % 2 == 0 and w % 2 == 0
    y = luma_oracle(rgb)
    sums = rgb.astype(np.int64).reshape(b, h // 2, 2, w // 2, 2, 3).sum(axis=(2, 4))
    cb, cr = chroma_oracle(sums)
    for plane in (y, cb, cr):
        assert plane.min(initial=16) >= 0 and plane.max(initial=16) <= 255
    return np.concatenate([y.reshape(b, -1), cb.reshape(b, -1), cr.reshape(b, -1)], axis=1).astype(np.uint8)


def known_colour_frame():
    """[1, 2, 10, 3]: the five known-answer colours, one 2 x 2 block each."""
    frame = np.zeros((1, 2, 10, 3), np.uint8)
    for i, (rgb, _) in enumerate(KNOWN.values()):
        frame[0, :, 2 * i: 2 * i + 2] = rgb
    return frame


def test_integer_oracle_known_answers():
    for name, (rgb, (y, cb, cr)) in KNOWN.items():
        px = np.array(rgb, np.uint8)
        assert int(luma_oracle(px)) == y, name
        got_cb, got_cr = chroma_oracle(4 * px.astype(np.int64))
        assert (int(got_cb), int(got_cr)) == (cb, cr), name
    planar = yuv420p_oracle(known_colour_frame())[0]
    assert planar.shape == (2 * 10 * 3 // 2,)
    want_y = np.repeat([v[1][0] for v in KNOWN.values()], 2)
    assert np.array_equal(planar[:10], want_y) and np.array_equal(planar[10:20], want_y)
    assert list(planar[20:25]) == [v[1][1] for v in KNOWN.values()] and list(planar[25:30]) == [v[1][2] for v in KNOWN.values()]


def test_integer_oracle_against_the_float64_definition():
    """4096 random pixels (luma) and 4096 random 2 x 2 blocks (chroma) against BT.601 in float64.  The definition is the standard's digital
    matrix as it is published, to three decimals, on R'G'B' in [0, 1] —
        Y = 16 + 65.481 R' + 128.553 G' + 24.966 B',  Cb = 128 - 37.797 R' - 74.203 G' + 112 B',  Cr = 128 + 112 R' - 93.786 G' - 18.214 B'
    — with the block's box average as the chroma input.  The integer formula is that matrix times 1000 over a common denominator, rounded
    half up, so every sample is within 0.5 (+ 1e-9 for the float64 evaluation) of the real value: no exemptions.
    Against the matrix derived from Kr = 0.299, Kb = 0.114 without the three-decimal rounding, each of the three coefficients of a row is
    off by at most 0.0005 and the inputs are in [0, 1]: the bound there is 0.5 + 0.0015 (the luma row is exact: 0.299 * 219 = 65.481)."""
    rng = np.random.default_rng(20260)
    px = rng.integers(0, 256, (4096, 3), dtype=np.uint8)
    f = px.astype(np.float64) / 255.0
    y_real = 16.0 + 65.481 * f[:, 0] + 128.553 * f[:, 1] + 24.966 * f[:, 2]
    err = np.abs(luma_oracle(px) - y_real)
    assert err.max() <= 0.5 + 1e-9, err.max()
    y_exact = 16.0 + 219.0 * (0.299 * f[:, 0] + 0.587 * f[:, 1] + 0.114 * f[:, 2])
    assert np.abs(luma_oracle(px) - y_exact).max() <= 0.5 + 1e-9

    blocks = rng.integers(0, 256, (4096, 4, 3), dtype=np.uint8)
    blocks[:8] = np.array([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255]],
                          np.uint8)[:, None, :]
    sums = blocks.astype(np.int64).sum(axis=1)
    mean = sums.astype(np.float64) / 4.0 / 255.0
    cb, cr = chroma_oracle(sums)
    cb_real = 128.0 - 37.797 * mean[:, 0] - 74.203 * mean[:, 1] + 112.0 * mean[:, 2]
    cr_real = 128.0 + 112.0 * mean[:, 0] - 93.786 * mean[:, 1] - 18.214 * mean[:, 2]
    assert np.abs(cb - cb_real).max() <= 0.5 + 1e-9 and np.abs(cr - cr_real).max() <= 0.5 + 1e-9
    luma_mean = 0.299 * mean[:, 0] + 0.587 * mean[:, 1] + 0.114 * mean[:, 2]
    cb_exact = 128.0 + 224.0 * (mean[:, 2] - luma_mean) / (2 * (1 - 0.114))
    cr_exact = 128.0 + 224.0 * (mean[:, 0] - luma_mean) / (2 * (1 - 0.299))
    assert np.abs(cb - cb_exact).max() <= 0.5 + 0.0015 and np.abs(cr - cr_exact).max() <= 0.5 + 0.0015
    assert cb.min() >= 16 and cb.max() <= 240 and cr.min() >= 16 and cr.max() <= 240


def _stand_in_ffmpeg(tmp_path, monkeypatch):
    """An executable named ``ffmpeg`` on PATH that records its argument vector and copies stdin to the output path (the technique of
    test_render_pipes_rawvideo_to_an_ffmpeg_process: there is no ffmpeg binary in the image)."""
    bindir = tmp_path / "bin"
    bindir.mkdir()
    fake = bindir / "ffmpeg"
    fake.write_text("#!/usr/bin/env python3\nimport json, sys\nargs = sys.argv[1:]\nout = args[-1]\n"
                    "json.dump(args, open(out + '.args.json', 'w'))\n"
                    "data = sys.stdin.buffer.read()\nopen(out, 'wb').write(data)\n")
    fake.chmod(fake.stat().st_mode | stat.S_IEXEC)
    monkeypatch.setenv("PATH", f"{bindir}:{os.environ['PATH']}")


def test_frame_sink_yuv420p_pipes_planar_frames_to_the_encoder(tmp_path, monkeypatch, built_lib):
    from maua_stylegan2_amd import render

    _stand_in_ffmpeg(tmp_path, monkeypatch)
    w, h, n = 6, 4, 3
    rng = np.random.default_rng(1)
    frames = rng.integers(0, 256, (n, w * h * 3 // 2), dtype=np.uint8)
    out = str(tmp_path / "clip.mp4")
    sink = render.FrameSink(out, w, h, 24, audio_file="song.wav", offset=1.5, duration=2.0, ffmpeg_preset="veryfast", pix_fmt="yuv420p")
    for frame in frames:
        sink.write(frame)
    for bad in (frames[0][:-1], np.zeros((h, w, 3), np.uint8), np.zeros(w * h * 3, np.uint8)):
        with pytest.raises(ValueError, match="yuv420p frame"):
            sink.write(bad)
    sink.close()
    assert sink.count == n
    args = json.load(open(out + ".args.json"))
    pipe = args.index("pipe:")
    assert args[:pipe + 1] == ["-hide_banner", "-y", "-v", "warning", "-f", "rawvideo", "-pix_fmt", "yuv420p", "-framerate", "24", "-s",
                               f"{w}x{h}", "-i", "pipe:"]
    output_side = args[pipe + 1:]
    joined = " ".join(output_side)
    for expect in ("-ss 1.5 -t 2.0 -guess_layout_max 0 -i song.wav", "-r 24 -vcodec libx264 -pix_fmt yuv420p -preset veryfast",
                   "-colorspace smpte170m", "-color_primaries smpte170m", "-color_trc smpte170m", "-color_range tv", "-b:a 320K -ac 2"):
        assert expect in joined, (expect, joined)
    assert args[-1] == out
    assert np.array_equal(np.fromfile(out, dtype=np.uint8), frames.reshape(-1))


def test_frame_sink_yuv420p_fallback_file_without_a_binary(tmp_path, monkeypatch, built_lib):
    from maua_stylegan2_amd import render

    monkeypatch.setattr(render.shutil, "which", lambda name: None)
    w, h, n = 10, 6, 4
    frames = np.arange(n * w * h * 3 // 2, dtype=np.int64).astype(np.uint8).reshape(n, -1)
    out = str(tmp_path / "clip.mp4")
    sink = render.FrameSink(out, w, h, 30, pix_fmt="yuv420p")
    for frame in frames:
        sink.write(frame)
    sink.close()
    assert not os.path.exists(out + ".rgb24")
    assert os.path.getsize(out + ".yuv420p") == n * h * w * 3 // 2
    assert np.array_equal(np.fromfile(out + ".yuv420p", dtype=np.uint8), frames.reshape(-1))
    with pytest.raises(ValueError, match="even"):
        render.FrameSink(None, 5, 4, 30, pix_fmt="yuv420p")
    with pytest.raises(ValueError, match="pixel format"):
        render.FrameSink(None, 4, 4, 30, pix_fmt="nv12")


def test_frame_sink_rgb24_default_arguments_are_unchanged(tmp_path, monkeypatch, built_lib):
    """The default path: the argument vector of the rgb24 sink, spelled out as it was before the pipe format existed."""
    from maua_stylegan2_amd import render

    _stand_in_ffmpeg(tmp_path, monkeypatch)
    w, h = 4, 2
    frame = np.arange(h * w * 3, dtype=np.uint8).reshape(h, w, 3)
    for k, (kwargs, middle, tail) in enumerate([
            (dict(), [], []),
            (dict(audio_file="song.wav", offset=0.5, duration=3.0), ["-ss", "0.5", "-t", "3.0", "-guess_layout_max", "0", "-i", "song.wav"],
             ["-b:a", "320K", "-ac", "2"])]):
        out = str(tmp_path / f"clip{k}.mp4")
        sink = render.FrameSink(out, w, h, 30, ffmpeg_preset="slow", **kwargs)
        assert sink.pix_fmt == "rgb24"
        sink.write(frame)
        sink.close()
        args = json.load(open(out + ".args.json"))
        assert args == (["-hide_banner", "-y", "-v", "warning", "-f", "rawvideo", "-pix_fmt", "rgb24", "-framerate", "30", "-s", f"{w}x{h}",
                         "-i", "pipe:"] + middle + ["-r", "30", "-vcodec", "libx264", "-pix_fmt", "yuv420p", "-preset", "slow"] + tail + [out])
        assert np.array_equal(np.fromfile(out, dtype=np.uint8), frame.reshape(-1))


def test_cli_flag_and_the_formats_way_into_the_render_loop(monkeypatch, built_lib):
    """``--pipe_pix_fmt {rgb24,yuv420p}``; generate() and render() keep the reference's parameter lists (tests/test_host_logic.py pins them),
    so the format reaches the render loop through the namespace / $MAUA_PIPE_PIX_FMT and render_shard's trailing keyword."""
    import inspect

    from maua_stylegan2_amd import generate_audiovisual as gav
    from maua_stylegan2_amd import render

    parser = gav.build_parser()
    assert parser.parse_args([]).pipe_pix_fmt == "rgb24"
    assert parser.parse_args(["--pipe_pix_fmt", "yuv420p"]).pipe_pix_fmt == "yuv420p"
    assert parser.parse_args(["--pipe_pix_fmt", "rgb24"]).pipe_pix_fmt == "rgb24"
    for bad in ("nv12", "yuv444p", ""):
        with pytest.raises(SystemExit):
            parser.parse_args(["--pipe_pix_fmt", bad])

    names = list(inspect.signature(render.render_shard).parameters)
    assert names[-1] == "pipe_pix_fmt" and names[-2] == "transport"
    assert "pipe_pix_fmt" not in inspect.signature(render.render).parameters
    assert "pipe_pix_fmt" not in inspect.signature(gav.generate).parameters

    monkeypatch.delenv("MAUA_PIPE_PIX_FMT", raising=False)
    assert render._pipe_pix_fmt(None) == "rgb24" and render._pipe_pix_fmt("yuv420p") == "yuv420p"
    monkeypatch.setenv("MAUA_PIPE_PIX_FMT", "yuv420p")
    assert render._pipe_pix_fmt(None) == "yuv420p" and render._pipe_pix_fmt("rgb24") == "rgb24"
    with pytest.raises(ValueError, match="pixel format"):
        render._pipe_pix_fmt("nv12")
    monkeypatch.delenv("MAUA_PIPE_PIX_FMT")

    # what generate() hands the body (every combination, and the positionals: tests/test_render_entries_host.py): the flag's default is
    # "not set" — the body then resolves the environment —, another format is passed on
    for name in ("MAUA_SUBFRAMES", "MAUA_DELIVER_SIZE"):
        monkeypatch.delenv(name, raising=False)
    for namespace, want in ((argparse.Namespace(), None), (argparse.Namespace(pipe_pix_fmt="rgb24"), None), (argparse.Namespace(pipe_pix_fmt="yuv420p"), "yuv420p")):
        assert gav._tail_options(namespace, None, None, None, None) == (want, None, None)


def test_transport_frame_shape_is_flat_for_the_planar_format(built_lib):
    """Every rank sizes its transport buffers from this function when its own block is empty: it must agree with what the others push."""
    from maua_stylegan2_amd import render

    class G:
        size = 1024

    shape = render._stream_frame_shape
    assert shape(G, 1024) == (1024, 1024, 3) and shape(G, 1024, "rgb24") == (1024, 1024, 3)
    assert shape(G, 1024, "yuv420p") == (1024 * 1024 * 3 // 2,)
    assert shape(G, 1920, "yuv420p") == (1920 * 1080 * 3 // 2,) and shape(G, 1080, "yuv420p") == (1920 * 1080 * 3 // 2,)
    G.size = 512
    assert shape(G, 512, "yuv420p") == (512 * 512 * 3 // 2,) and shape(G, 1920, "yuv420p") == (512 * 1024 * 3 // 2,)


def test_launcher_rejects_bad_arguments_without_a_device(built_lib):
    """Validation runs before any HIP call: odd or non-positive sizes, a negative batch and NULL buffers are refused; batch 0 succeeds."""
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    fake = 0x1000  # never dereferenced
    call = lambda b, h, w, src=fake, dst=fake: lib.maua_rgb_to_yuv420p_u8(src, dst, b, h, w, None)  # noqa: E731
    for b, h, w in [(1, 3, 4), (1, 4, 3), (1, 1, 1), (1, 0, 4), (1, 4, 0), (1, -2, 4), (-1, 4, 4), (0, 3, 4), (0, 4, 5)]:
        assert call(b, h, w) == -22, (b, h, w)
    assert call(1, 4, 4, src=None) == -22 and call(1, 4, 4, dst=None) == -22
    assert call(0, 4, 4) == 0 and call(0, 2, 2, src=None, dst=None) == 0
    assert "maua_rgb_to_yuv420p_u8" in _lib.exported_symbols() and len(_lib._SIGNATURES["maua_rgb_to_yuv420p_u8"][1]) == 6
