"""CPU: the Motion-JPEG pipe format without a device — the integer definition of the stream (tests/jpeg_ref.py, the oracle
tests/test_mjpeg_gpu.py compares csrc/jpeg.hip against byte for byte) against an independent decoder and encoder (Pillow / libjpeg), its
structure, the host-side entries of the C ABI, the AVI writer, the frame sink's mjpeg branch and the CLI."""
import argparse
import io
import json
import os
import struct

import numpy as np
import PIL.Image
import pytest

import jpeg_ref
from test_yuv420_host import _stand_in_ffmpeg

QUALITIES = (1, 50, 90, 95)
# PSNR of the reference's stream (decoded by Pillow) against Pillow's own encode of the same frame with the same tables, 4:2:0: same
# quantiser, so the difference is the rounding of the DCT and of the chroma average (libjpeg averages 2 x 2 chroma with an alternating
# bias of 1, 2; the definition here rounds half up) and, for frames that are no whole number of MCUs, of what fills the partial MCUs.
# Measured over the 5 pictures x 4 qualities below, per frame size (psnr_pil - psnr_ref, dB; negative: the reference is closer to the source):
#   256x256  -0.016 .. +0.179     56x120  -0.150 .. +0.029     24x40  -0.201 .. +0.011     16x16  -0.313 .. +0.273     8x8  -0.987 .. +0.922
# The spread grows as the pixel count falls — an 8 x 8 frame is one luma block and 16 real chroma samples, and at quality 1 (every divisor
# 255 x 8) one coefficient that rounds to 0 on one side and to 1 on the other moves the frame by most of a dB — and it is as wide in the
# reference's favour as against it: rounding noise, no bias.  Margin per size = its largest gap rounded up to 0.1 dB.
PSNR_MARGIN_DB = {(256, 256): 0.2, (56, 120): 0.1, (24, 40): 0.1, (16, 16): 0.3, (8, 8): 1.0}


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else float(10 * np.log10(255.0 ** 2 / mse))


def _cases():
    for h, w in jpeg_ref.SIZES:
        for name, rgb in jpeg_ref.inputs(h, w).items():
            yield name, h, w, rgb


def test_reference_streams_decode_in_pillow_with_the_scaled_tables_and_pillows_psnr():
    gaps, ratios = {}, {}
    for name, h, w, rgb in _cases():
        restart = (w + 15) // 16
        for q in QUALITIES:
            stream = jpeg_ref.encode(rgb, q, restart)
            im = PIL.Image.open(io.BytesIO(stream))
            im.load()
            assert im.size == (w, h) and im.mode == "RGB" and im.format == "JPEG"
            tables = jpeg_ref.scaled_tables(q)
            assert [list(im.quantization[i]) for i in (0, 1)] == tables, (name, h, w, q)
            buf = io.BytesIO()
            PIL.Image.fromarray(rgb).save(buf, "JPEG", qtables=tables, subsampling=2, restart_marker_blocks=restart)
            theirs = PIL.Image.open(io.BytesIO(buf.getvalue()))
            gap = _psnr(np.asarray(theirs), rgb) - _psnr(np.asarray(im), rgb)
            gaps[(name, h, w, q)] = gap
            ratios[(name, h, w, q)] = len(stream) / len(buf.getvalue())
    worst = max(gaps, key=gaps.get)
    print(f"largest PSNR gap {gaps[worst]:+.3f} dB at {worst}; smallest {min(gaps.values()):+.3f} dB")
    print(f"size against Pillow (same tables, same restart interval): {min(ratios.values()):.3f} .. {max(ratios.values()):.3f}, "
          f"256x256: " + ", ".join(f"{k[0]} q{k[3]} {v:.3f}" for k, v in ratios.items() if k[1] == 256 and k[3] in (90, 95)))
    for key, gap in gaps.items():
        assert gap <= PSNR_MARGIN_DB[key[1:3]], (key, gap)


def test_standard_huffman_tables_are_the_ones_libjpeg_writes():
    """The four DHT segments equal those of a Pillow encode (libjpeg writes the Annex K.3 tables unless asked to optimise)."""
    rgb = jpeg_ref.inputs(16, 16)["smooth"]
    buf = io.BytesIO()
    PIL.Image.fromarray(rgb).save(buf, "JPEG", subsampling=2)
    theirs = [p for m, p in jpeg_ref.walk(buf.getvalue())["segments"] if m == 0xC4]
    ours = [p for m, p in jpeg_ref.walk(jpeg_ref.encode(rgb, 75, 1))["segments"] if m == 0xC4]
    assert len(ours) == 4 and sorted(ours) == sorted(theirs)
    assert [p[0] for p in ours] == [0x00, 0x10, 0x01, 0x11]


def test_the_checkerboard_reaches_the_largest_size_categories():
    """At quality 95 the DC quantiser is 2: a swing between flat 0 and flat 255 blocks is a DC difference of 1020 (category 10, the largest a
    quality of at most 95 can produce; 11 needs a quantiser of 1), and the single-pixel checkerboard's highest AC coefficient is far
    beyond what the other pictures produce."""
    coef = jpeg_ref.coefficients(jpeg_ref.inputs(56, 120)["checker"], 95)
    luma_dc = coef[:, :4, 0].reshape(-1)
    assert int(np.abs(np.diff(luma_dc)).max()).bit_length() == 10
    assert int(np.abs(coef[:, :, 1:]).max()).bit_length() >= 8
    assert int(np.abs(coef).max()) <= 1023


@pytest.mark.parametrize("h,w,restart", [(16, 16, 1), (48, 64, 1), (48, 64, 4), (48, 64, 5), (48, 64, 65535), (24, 40, 2), (256, 256, 16)])
def test_stream_structure(h, w, restart):
    rgb = jpeg_ref.inputs(h, w)["noise"]
    stream = jpeg_ref.encode(rgb, 90, restart)
    info = jpeg_ref.walk(stream)
    assert [m for m, _ in info["segments"]] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert info["segments"][0][1][:5] == b"JFIF\0" and info["segments"][1][1][0] == 0 and info["segments"][2][1][0] == 1
    sof = info["segments"][3][1]
    assert struct.unpack(">BHHB", sof[:6]) == (8, h, w, 3) and sof[6:] == bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert info["dri"] == restart
    mcus = ((h + 15) // 16) * ((w + 15) // 16)
    assert len(info["rst"]) == -(-mcus // restart) - 1
    assert [m for _, m in info["rst"]] == [i % 8 for i in range(len(info["rst"]))]
    assert stream[-2:] == b"\xff\xd9" and info["entropy"][1] == len(stream) - 2
    assert stream[: info["entropy"][0]] == jpeg_ref.header(h, w, 90, restart)
    if (h, w) == (256, 256):
        assert info["stuffed"] >= 1  # (otherwise the noise frame does not test stuffing)
        worst = jpeg_ref.SEGMENT_BYTES_PER_MCU * restart + 16
        spans = np.diff([info["entropy"][0]] + [p for p, _ in info["rst"]] + [info["entropy"][1]])
        assert spans.max() < worst // 2  # (even noise stays far below the worst case the interval segments are sized for)


def test_walk_rejects_malformed_streams():
    stream = bytearray(jpeg_ref.encode(jpeg_ref.inputs(24, 40)["noise"], 90, 2))
    lo = jpeg_ref.walk(stream)["entropy"][0]
    bad = bytearray(stream)
    bad[lo: lo + 2] = b"\xff\x01"
    with pytest.raises(ValueError, match="unstuffed"):
        jpeg_ref.walk(bad)
    bad = bytearray(stream)
    first = jpeg_ref.walk(stream)["rst"][0][0]
    bad[first + 1] = 0xD3
    with pytest.raises(ValueError, match="out of order"):
        jpeg_ref.walk(bad)
    with pytest.raises(ValueError, match="behind EOI"):
        jpeg_ref.walk(bytes(stream) + b"\0")


def test_header_entry_equals_the_reference_and_rejects_bad_arguments(built_lib):
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    buf = np.full(1024, 0xA5, np.uint8)
    for h, w, q, ri in [(16, 16, 90, 1), (1080, 1920, 90, 120), (1, 1, 1, 65535), (65535, 65535, 95, 7), (24, 40, 50, 3), (7, 300, 49, 300)]:
        want = jpeg_ref.header(h, w, q, ri)
        buf[:] = 0xA5
        n = lib.maua_jpeg_header(h, w, q, ri, buf.ctypes.data, buf.size)
        assert n == len(want) == 629 and bytes(buf[:n]) == want, (h, w, q, ri)
        assert (buf[n:] == 0xA5).all()
        assert lib.maua_jpeg_header(h, w, q, ri, buf.ctypes.data, n) == n and lib.maua_jpeg_header(h, w, q, ri, buf.ctypes.data, n - 1) == -22
    call = lambda h=16, w=16, q=90, ri=1, p=buf.ctypes.data, cap=1024: lib.maua_jpeg_header(h, w, q, ri, p, cap)  # noqa: E731
    assert call() == 629
    for kw in (dict(q=0), dict(q=96), dict(q=-1), dict(ri=0), dict(ri=65536), dict(h=0), dict(w=0), dict(h=65536), dict(w=65536), dict(p=None),
               dict(cap=0), dict(cap=628)):
        assert call(**kw) == -22, kw


def test_workspace_size_is_a_pure_function_of_the_shape(built_lib):
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    for b, h, w, ri in [(1, 16, 16, 1), (3, 48, 64, 5), (8, 1024, 1024, 64), (8, 1080, 1920, 120), (2, 24, 40, 65535), (0, 16, 16, 1)]:
        n = lib.maua_jpeg_ws_bytes(b, h, w, ri)
        mcus = ((h + 15) // 16) * ((w + 15) // 16)
        intervals = -(-mcus // ri)
        coef = b * mcus * 6 * 64 * 2
        assert n >= coef and n == coef + b * intervals * (min(ri, mcus) * jpeg_ref.SEGMENT_BYTES_PER_MCU + 16) + b * intervals * 4
        assert all(lib.maua_jpeg_ws_bytes(b, h, w, ri) == n for _ in range(3))
    assert lib.maua_jpeg_ws_bytes(1, 0, 16, 1) == 0 and lib.maua_jpeg_ws_bytes(1, 16, 16, 0) == 0 and lib.maua_jpeg_ws_bytes(-1, 16, 16, 1) == 0


def test_launcher_rejects_bad_arguments_without_a_device(built_lib):
    """Validation runs before any HIP call (fake pointers, never dereferenced: a call that got past validation would fault here)."""
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    fake = 0x1000

    def call(rgb=fake, b=1, h=16, w=16, q=90, ri=1, header=fake, header_len=629, out=fake, slot=4096, ws=fake):
        return lib.maua_jpeg_encode_u8(rgb, b, h, w, q, ri, header, header_len, out, slot, ws, None)

    for kw in (dict(rgb=None), dict(header=None), dict(out=None), dict(ws=None), dict(h=0), dict(w=0), dict(h=-3), dict(q=0), dict(q=96),
               dict(ri=0), dict(ri=65536), dict(b=-1), dict(slot=16 + 629 + 1), dict(slot=0), dict(header_len=0), dict(ws=0x1008)):
        assert call(**kw) == -22, kw
    assert call(b=0) == 0 and call(b=0, rgb=None, out=None, ws=None, header=None) == 0
    assert call(b=0, q=0) == -22 and call(b=65536) == -38
    assert {"maua_jpeg_header", "maua_jpeg_ws_bytes", "maua_jpeg_encode_u8"} <= set(_lib.exported_symbols()) and _lib.ABI_VERSION == 8


def _frames(n, h=24, w=40, quality=90):
    """n distinct reference streams of odd and even lengths."""
    rgb = jpeg_ref.inputs(h, w)["smooth"]
    streams = [jpeg_ref.encode(np.roll(rgb, 3 * i, axis=1), quality, 3) for i in range(n)]
    assert len({len(s) & 1 for s in streams}) == 2 or n < 4, [len(s) for s in streams]
    return streams


def _check_avi(path, payloads, w, h, fps):
    info = jpeg_ref.avi_frames(path)
    assert info["frames"] == payloads
    assert info["avih"]["total_frames"] == len(payloads) and info["strh"]["length"] == len(payloads)
    assert (info["avih"]["width"], info["avih"]["height"], info["avih"]["streams"]) == (w, h, 1) and info["avih"]["flags"] & 0x10
    assert info["avih"]["us_per_frame"] == round(1e6 / fps)
    assert info["strh"]["type"] == b"vids" and info["strh"]["handler"] == b"MJPG"
    assert info["strh"]["scale"] == 1000000 and info["strh"]["rate"] == round(fps * 1000000)
    assert info["strf"] == dict(size=40, width=w, height=h, planes=1, bit_count=24, compression=b"MJPG", image_size=w * h * 3)
    assert len(info["idx1"]) == len(payloads)
    data = open(path, "rb").read()
    for (ckid, flags, offset, size), (at, chunk_size), payload in zip(info["idx1"], info["chunks"], payloads):
        assert ckid == b"00dc" and flags == 0x10 and size == chunk_size == len(payload)
        assert info["movi"] + offset == at and at % 2 == 0  # the index points at the chunk header; chunks are word-aligned
        assert data[at: at + 4] == b"00dc" and data[at + 8: at + 8 + size] == payload
    for payload in payloads:
        im = PIL.Image.open(io.BytesIO(payload))
        im.load()
        assert im.size == (w, h)


def test_avi_writer_round_trip(tmp_path):
    from maua_stylegan2_amd import avi

    payloads = _frames(6)
    assert any(len(p) & 1 for p in payloads)  # an odd payload: padding is exercised
    path = str(tmp_path / "clip.avi")
    writer = avi.MjpegAviWriter(path, 40, 24, 29.97)
    for p in payloads:
        writer.write(np.frombuffer(p, np.uint8))
    writer.close()
    writer.close()  # (twice is safe)
    assert writer.paths == [path] and writer.count == 6
    _check_avi(path, payloads, 40, 24, 29.97)
    empty = avi.MjpegAviWriter(str(tmp_path / "none"), 40, 24, 30)
    empty.close()
    assert empty.paths == [str(tmp_path / "none.avi")]
    _check_avi(empty.paths[0], [], 40, 24, 30)
    with pytest.raises(ValueError):
        avi.MjpegAviWriter(str(tmp_path / "bad.avi"), 40, 24, 0)


def test_avi_writer_rolls_over_before_the_riff_limit(tmp_path, monkeypatch):
    from maua_stylegan2_amd import avi

    payloads = _frames(12)
    limit = 4000
    monkeypatch.setattr(avi, "RIFF_LIMIT", limit)
    writer = avi.MjpegAviWriter(str(tmp_path / "clip.avi"), 40, 24, 30)
    for p in payloads:
        writer.write(p)
    writer.close()
    assert len(writer.paths) >= 3 and writer.count == 12
    assert writer.paths[:3] == [str(tmp_path / n) for n in ("clip.avi", "clip.002.avi", "clip.003.avi")]
    seen = []
    for path in writer.paths:
        assert os.path.getsize(path) <= limit
        part = jpeg_ref.avi_frames(path)["frames"]
        assert part
        _check_avi(path, part, 40, 24, 30)
        seen += part
    assert seen == payloads


def _slot(stream, slot_bytes, status=0, fill=0xA5):
    out = np.full(slot_bytes, fill, np.uint8)
    out[:16] = np.frombuffer(struct.pack("<IIQ", len(stream), status, 0), np.uint8)
    if not status:
        out[16: 16 + len(stream)] = np.frombuffer(stream, np.uint8)
    return out


def test_frame_sink_mjpeg_pipes_the_streams_to_the_encoder(tmp_path, monkeypatch, built_lib):
    from maua_stylegan2_amd import render

    _stand_in_ffmpeg(tmp_path, monkeypatch)
    w, h = 40, 24
    payloads = _frames(3)
    slot_bytes = render.mjpeg_slot_bytes(w, h)
    assert slot_bytes == 1024 + w * h * 3 // 2
    out = str(tmp_path / "clip.mp4")
    sink = render.FrameSink(out, w, h, 24, audio_file="song.wav", offset=1.5, duration=2.0, ffmpeg_preset="veryfast", pix_fmt="mjpeg", quality=90)
    for p in payloads:
        sink.write(_slot(p, slot_bytes))
    for bad in (_slot(payloads[0], slot_bytes)[:-1], np.zeros((h, w, 3), np.uint8), np.zeros(w * h * 3 // 2, np.uint8)):
        with pytest.raises(ValueError, match="mjpeg frame"):
            sink.write(bad)
    with pytest.raises(ValueError, match=r"frame 3 overflowed.*needs 5000 bytes.*quality 90"):
        sink.write(_slot(b"\0" * 5000, slot_bytes, status=1))
    sink.close()
    assert sink.count == 3
    args = json.load(open(out + ".args.json"))
    pipe = args.index("pipe:")
    assert args[:pipe + 1] == ["-hide_banner", "-y", "-v", "warning", "-f", "mjpeg", "-framerate", "24", "-i", "pipe:"]
    assert args[pipe + 1:] == ["-ss", "1.5", "-t", "2.0", "-guess_layout_max", "0", "-i", "song.wav", "-r", "24", "-vcodec", "libx264", "-pix_fmt",
                               "yuv420p", "-preset", "veryfast", "-b:a", "320K", "-ac", "2", out]
    assert open(out, "rb").read() == b"".join(payloads)  # no slot headers, no slot tails


def test_frame_sink_mjpeg_writes_an_avi_without_a_binary(tmp_path, monkeypatch, built_lib, capsys):
    from maua_stylegan2_amd import render

    monkeypatch.setattr(render.shutil, "which", lambda name: None)
    w, h = 40, 24
    payloads = _frames(5)
    slot_bytes = render.mjpeg_slot_bytes(w, h)
    out = str(tmp_path / "clip.mp4")
    sink = render.FrameSink(out, w, h, 30, audio_file="song.wav", offset=0, duration=1, pix_fmt="mjpeg")
    for p in payloads:
        sink.write(_slot(p, slot_bytes))
    with pytest.raises(ValueError, match="overflowed"):
        sink.write(_slot(b"", slot_bytes, status=1))
    sink.close()
    assert sink.count == 5 and not os.path.exists(out + ".rgb24") and not os.path.exists(out)
    _check_avi(out + ".avi", payloads, w, h, 30)
    said = capsys.readouterr().out
    assert f"ffmpeg -i {out}.avi" in said and "-i song.wav" in said and "-c:v copy" in said
    null = render.FrameSink(None, w, h, 30, pix_fmt="mjpeg")
    null.write(_slot(payloads[0], slot_bytes))
    assert null.count == 1


def test_cli_flag_quality_resolution_and_the_way_into_the_render_loop(monkeypatch, built_lib):
    import inspect

    from maua_stylegan2_amd import generate_audiovisual as gav
    from maua_stylegan2_amd import render

    assert render.PIPE_PIX_FMTS == ("rgb24", "yuv420p", "mjpeg")
    parser = gav.build_parser()
    args = parser.parse_args(["--pipe_pix_fmt", "mjpeg"])
    assert args.pipe_pix_fmt == "mjpeg" and args.mjpeg_quality == 90
    assert parser.parse_args(["--pipe_pix_fmt", "mjpeg", "--mjpeg_quality", "85"]).mjpeg_quality == 85
    assert parser.parse_args([]).pipe_pix_fmt == "rgb24"
    for bad in ("nv12", "mjpeg:85", ""):
        with pytest.raises(SystemExit):
            parser.parse_args(["--pipe_pix_fmt", bad])
    flags = [flag for flag, _ in gav.CLI_FLAGS]
    assert flags.index("--mjpeg_quality") == flags.index("--pipe_pix_fmt") + 1

    names = list(inspect.signature(render.render_shard).parameters)
    assert names[-2:] == ["transport", "pipe_pix_fmt"]
    assert "mjpeg_quality" not in inspect.signature(gav.generate).parameters and "quality" not in inspect.signature(render.render).parameters

    monkeypatch.delenv("MAUA_PIPE_PIX_FMT", raising=False)
    monkeypatch.delenv("MAUA_MJPEG_QUALITY", raising=False)
    assert render._pipe_pix_fmt("mjpeg") == "mjpeg" and render._pipe_pix_fmt("mjpeg:85") == "mjpeg" and render._pipe_pix_fmt(None) == "rgb24"
    with pytest.raises(ValueError, match="pixel format"):
        render._pipe_pix_fmt("nv12")
    with pytest.raises(ValueError, match="pixel format"):
        render._pipe_pix_fmt("mjpegs")
    assert render._mjpeg_quality("mjpeg") == 90 and render._mjpeg_quality("mjpeg:85") == 85
    monkeypatch.setenv("MAUA_MJPEG_QUALITY", "70")
    assert render._mjpeg_quality("mjpeg") == 70 and render._mjpeg_quality("mjpeg:85") == 85  # the suffix wins over the environment
    monkeypatch.setenv("MAUA_PIPE_PIX_FMT", "mjpeg:60")
    assert render._pipe_pix_fmt(None) == "mjpeg" and render._mjpeg_quality(None) == 60
    monkeypatch.delenv("MAUA_PIPE_PIX_FMT")
    for bad in ("mjpeg:0", "mjpeg:96", "mjpeg:-5", "mjpeg:high", "mjpeg:"):
        with pytest.raises(ValueError, match="quality"):
            render._mjpeg_quality(bad)
    monkeypatch.setenv("MAUA_MJPEG_QUALITY", "96")
    with pytest.raises(ValueError, match="quality"):
        render._mjpeg_quality("mjpeg")
    monkeypatch.delenv("MAUA_MJPEG_QUALITY")

    # what generate() hands the body (every combination, and the positionals: tests/test_render_entries_host.py): the quality travels
    # in the format's name, and only in mjpeg's
    for name in ("MAUA_SUBFRAMES", "MAUA_DELIVER_SIZE"):
        monkeypatch.delenv(name, raising=False)
    for pix_fmt, quality, want in (("mjpeg", 85, "mjpeg:85"), ("mjpeg", 90, "mjpeg:90"), ("mjpeg", None, "mjpeg"), ("yuv420p", 85, "yuv420p"), ("rgb24", 85, None)):
        namespace = argparse.Namespace(pipe_pix_fmt=pix_fmt, mjpeg_quality=quality)
        assert gav._tail_options(namespace, None, None, None, None) == (want, None, None)
        assert gav._pipe_format_of(namespace) == (want or "rgb24")


def test_transport_frame_shape_is_the_flat_slot(built_lib):
    from maua_stylegan2_amd import render

    class G:
        size = 1024

    shape = render._stream_frame_shape
    assert shape(G, 1024, "mjpeg") == (1024 + 1024 * 1024 * 3 // 2,) and shape(G, 1920, "mjpeg") == (1024 + 1920 * 1080 * 3 // 2,)
    assert shape(G, 1080, "mjpeg") == (1024 + 1920 * 1080 * 3 // 2,)
    G.size = 512
    assert shape(G, 1920, "mjpeg") == (1024 + 512 * 1024 * 3 // 2,) and shape(G, 512, "rgb24") == (512, 512, 3)
