"""Frame rendering loop — mirror of the reference's render.py:14-192 ``render(...)`` for MI355X.

Same signature and batch semantics (slice latents / noise / bend modulation / truncation on dim 0, call the generator
with ``input_is_latent=True``), different machinery:

  reference                                             here
  --------------------------------------------------    ------------------------------------------------------------
  pin + H2D of latents and up to 17 noise maps / batch    inputs are uploaded ONCE and stay resident in HBM (288 GB)
  eager generator call, ~200 launches per batch           hipGraph replay per batch (eager only when bends / rewrites /
                                                          randomize_noise make the batch non-capturable, or a tail batch)
  clamp/scale/permute on device, per-FRAME .cpu()         uint8 NHWC written by the last layer's epilogue, one async D2H per BATCH on a copy
  .numpy().astype(uint8), two Python threads + queues     stream into a 6-slot pinned ring (from its device-side twin), ordered sink thread
  DataParallel replicate/scatter/gather per forward       one process per GPU, contiguous frame shards, RCCL gather of
                                                          uint8 frames to rank 0 (maua_stylegan2_amd/sharding.py)

``render_frames`` is the one body of every entry point: ONE frame loop, whatever happens to a batch on the device and whatever carries the
frames to the sink.  Per batch it is ``delivery.push(tail(first, batch))``:
  the tail (_FrameTail)   everything between the generator's output and the frames as they leave the device, resolved and refused once,
                          before the sink is opened; the stages run on the producing stream, each only when its option is set, in the order
                          feedback -> lens -> grade (or the plain quantiser) -> temporal fold -> crop / resize -> yuv420p / mjpeg — the deep
                          formats end in frames_to_deep instead of the last three
  the delivery            an object per transport (_LocalRing on one GPU; _HostStore / _GatherStream under a process group) with
                          ``push(u8)`` — one deliverable batch, the producing stream current —, ``finish(frame_shape)`` — end of this
                          rank's frames, also when it had none — and ``close()`` — safe after a failure, and twice.
The entry points differ in their parameter lists and in what they read from the environment, nothing else: ``render`` (the reference's
parameter list) and ``render_shard`` take the fold and the delivery size from the environment, ``render_folded`` the delivery size;
``render_delivered``, ``render_graded``, ``render_lensed`` and ``render_fed`` read neither.  An unset ``pipe_pix_fmt`` is $MAUA_PIPE_PIX_FMT
for all of them.

Sinks: ffmpeg rawvideo pipe (same pixel format / codec arguments as render.py:58-91) when an ``ffmpeg`` binary exists,
otherwise raw rgb24 bytes to ``output_file`` (+ ".rgb24"), or a null sink for benchmarking (``output_file=None``).

The options of the tail, all off by default:
  pipe format ``yuv420p``   the frames are converted to planar YUV 4:2:0 on the device (frames_to_yuv420p) before they cross to the host /
                            to rank 0, 1.5 bytes per pixel instead of 3, and the encoder is fed what it would otherwise convert to itself
  ``mjpeg[:<quality>]``     every frame is encoded as one baseline JPEG on the device (frames_to_mjpeg) and travels in a fixed-size slot; the
                            sink writes the streams alone, to ``ffmpeg -f mjpeg`` or, without a binary, to a Motion-JPEG .avi (avi.py)
  deep formats              DEEP_PIX_FMTS: the lanes keep the fp32 image and frames_to_deep turns it into 16-bit packed RGB or 10-bit planar
                            BT.709 YUV, so no 8-bit quantiser sits between the generator and the encoder (libx265, 10 bits); the frames
                            travel as flat bytes like the yuv420p ones.  Not combinable with a temporal fold
  ``fold`` (TemporalFold)   temporal supersampling ($MAUA_SUBFRAMES): N rendered sub-frames per delivered frame, averaged on the device by
                            fold_frames before the spatial steps; the sink and the transports then count delivered frames
  ``resize`` (FrameResize)  delivery size ($MAUA_DELIVER_SIZE / _FILTER / _FIT): every delivered frame is resampled on the device
                            (resize_frames: Lanczos, bicubic, Hamming, bilinear or box; crop, pad or stretch) after the fold and before the
                            colour conversion, at 16 bits on the deep formats; the sink and the transports see the delivery size
  ``grade`` (ar.Grade)      the lanes keep the fp32 image and every rendered frame is graded by its row of the grade's table (grade_frames:
                            ASC CDL, a 3 x 3 matrix, a 3-D LUT) — the 8-bit formats continue with the frames the quantiser gives for the
                            graded image, the deep formats with the image graded in place
  ``lens`` (ar.Lens)        bloom, sharpen and vignette on the same fp32 image, per rendered frame by its row of the lens's table
                            (lens_frames), in front of the grade
  ``feedback`` (ar.Feedback)  the previous output frame fed back under every rendered frame (feedback_frames: a recurrence over the frames,
                            chained across the lanes' streams by events), in front of the lens.  One rank only.
"""
import collections
import contextlib
import ctypes
import gc
import os
import queue
import shutil
import subprocess
import threading

import numpy as np
import torch as th

from . import _lib, avi, sharding
from .audioreactive.feedback import Feedback
from .audioreactive.grade import Grade
from .audioreactive.lens import Lens
from .audioreactive.noise import NoiseSynth

th.set_grad_enabled(False)


def device_of(generator):
    """Device a generator lives on (StyleGAN2 mirror: its constant / latent input; StyleGAN1's G_style: any parameter)."""
    inp = getattr(getattr(generator, "input", None), "input", None)
    return inp.device if inp is not None else next(generator.parameters()).device


def _output_dims(out_size):
    if out_size == 512:
        return 512, 512
    if out_size == 1024:
        return 1024, 1024
    if out_size == 1920:
        return 1920, 1080
    if out_size == 1080:
        return 1080, 1920
    # (the generator's sizes, as in the reference; the VIDEO can have any size: --deliver_size, FrameResize)
    raise Exception("The only output sizes currently supported are: 512, 1024, 1080, or 1920")


# what travels to the sink: packed RGB (the reference's, default), planar 4:2:0 made on the device, or one JPEG per frame made on the device
PIPE_PIX_FMTS = ("rgb24", "yuv420p", "mjpeg")
MJPEG_DEFAULT_QUALITY = 90
# how a yuv420p pipe is tagged: the matrix / range csrc/yuv420.hip converts with (BT.601 limited range), so that players decode with it
YUV420P_TAGS = ["-colorspace", "smpte170m", "-color_primaries", "smpte170m", "-color_trc", "smpte170m", "-color_range", "tv"]
# the deep pipe formats: the fp32 image leaves the device at 16 bits per sample (packed RGB) or as planar 10-bit YUV (csrc/deep_frames.hip),
# never through the 8-bit quantiser; encoded as HEVC Main10.  The YUV ones carry the matrix / range of that conversion (BT.709 limited range)
DEEP_PIX_FMTS = ("rgb48le", "yuv420p10le", "yuv422p10le", "yuv444p10le")
DEEP_SUBSAMPLING = {"yuv420p10le": 420, "yuv422p10le": 422, "yuv444p10le": 444}
YUV_P10_TAGS = ["-colorspace", "bt709", "-color_primaries", "bt709", "-color_trc", "bt709", "-color_range", "tv"]


def deep_frame_bytes(pix_fmt, width, height):
    """Bytes of one ``width`` x ``height`` frame of a deep pipe format: 6 per pixel for rgb48le and 4:4:4, 4 for 4:2:2, 3 for 4:2:0."""
    return width * height * {"rgb48le": 6, "yuv444p10le": 6, "yuv422p10le": 4, "yuv420p10le": 3}[pix_fmt]


def _pipe_pix_fmt(pix_fmt):
    """A ``pipe_pix_fmt`` argument resolved: None -> $MAUA_PIPE_PIX_FMT -> rgb24.  ``mjpeg`` may carry its quality, ``mjpeg:<q>``
    (_mjpeg_quality reads it): the bare name is returned."""
    pix_fmt = pix_fmt or os.environ.get("MAUA_PIPE_PIX_FMT") or "rgb24"
    name = "mjpeg" if pix_fmt.startswith("mjpeg:") else pix_fmt
    if name not in PIPE_PIX_FMTS + DEEP_PIX_FMTS:
        raise ValueError(f"unknown pipe pixel format {pix_fmt!r} ({' | '.join(PIPE_PIX_FMTS + DEEP_PIX_FMTS)})")
    return name


def _mjpeg_quality(pix_fmt):
    """The JPEG quality of an mjpeg pipe: the suffix of ``mjpeg:<q>`` -> $MAUA_MJPEG_QUALITY -> 90; 1 .. 95."""
    pix_fmt = pix_fmt or os.environ.get("MAUA_PIPE_PIX_FMT") or ""
    text = pix_fmt[len("mjpeg:"):] if pix_fmt.startswith("mjpeg:") else os.environ.get("MAUA_MJPEG_QUALITY") or str(MJPEG_DEFAULT_QUALITY)
    try:
        quality = int(text)
    except ValueError:
        raise ValueError(f"mjpeg quality {text!r} is not an integer") from None
    if not 1 <= quality <= 95:
        raise ValueError(f"mjpeg quality {quality} outside 1 .. 95")
    return quality


def mjpeg_slot_bytes(w, h):
    """Bytes of the fixed-size slot an mjpeg frame travels in (16 bytes of slot header + the stream): the yuv420p frame plus 1 KiB.
    Uniform noise at quality 95 takes about 1.2 bytes per pixel, so no picture overflows the 1.5 in practice; one that does is reported by
    the sink (status 1 in the slot header)."""
    return 1024 + w * h * 3 // 2


class FrameSink:
    """Ordered consumer of uint8 [H, W, 3] frames (``pix_fmt="rgb24"``) or of flat planar I420 frames [H * W * 3 / 2]
    (``pix_fmt="yuv420p"``: converted, and for wide outputs resized, on the device — frames_to_yuv420p), or of flat mjpeg slots
    [mjpeg_slot_bytes] (``pix_fmt="mjpeg"``: one JPEG per frame behind a 16-byte slot header — frames_to_mjpeg; ``quality`` is only quoted
    in the error an overflowed slot raises), or of flat deep frames [deep_frame_bytes] (``pix_fmt`` in DEEP_PIX_FMTS: 16-bit little-endian
    samples as bytes — frames_to_deep; encoded with libx265 at 10 bits)."""

    def __init__(self, output_file, width, height, framerate, audio_file=None, offset=0, duration=None,
                 ffmpeg_preset="slow", pix_fmt="rgb24", quality=None):
        if pix_fmt not in PIPE_PIX_FMTS + DEEP_PIX_FMTS:
            raise ValueError(f"unknown pipe pixel format {pix_fmt!r} ({' | '.join(PIPE_PIX_FMTS + DEEP_PIX_FMTS)})")
        if (pix_fmt == "yuv420p" or pix_fmt in DEEP_PIX_FMTS) and (width % 2 or height % 2):
            raise ValueError(f"{pix_fmt} needs even dimensions, got {width}x{height}")
        self.w, self.h = width, height
        self.pix_fmt = pix_fmt
        self.quality = quality
        self.proc = None
        self.file = None
        self.count = 0
        if output_file is None:
            return
        if pix_fmt == "mjpeg" and shutil.which("ffmpeg") is None:
            # no encoder needed: the streams are a playable Motion-JPEG file as they are (audio is not muxed)
            self.file = avi.MjpegAviWriter(output_file, width, height, framerate)
            path = self.file.paths[0]
            audio = f" -ss {offset} -t {duration} -i {audio_file}" if audio_file is not None else ""
            mux = " -b:a 320K -ac 2" if audio_file is not None else ""
            print(f"ffmpeg binary not found: writing Motion-JPEG frames ({width}x{height}) to {path}\n"
                  f"  mux or transcode later with: ffmpeg -i {path}{audio} -c:v copy{mux} {output_file}")
            return
        if shutil.which("ffmpeg") is not None:
            if pix_fmt == "mjpeg":
                cmd = ["ffmpeg", "-hide_banner", "-y", "-v", "warning", "-f", "mjpeg", "-framerate", f"{framerate}", "-i", "pipe:"]
            else:
                cmd = ["ffmpeg", "-hide_banner", "-y", "-v", "warning", "-f", "rawvideo", "-pix_fmt", pix_fmt, "-framerate",
                       f"{framerate}", "-s", f"{width}x{height}", "-i", "pipe:"]
            if audio_file is not None:
                cmd += ["-ss", f"{offset}", "-t", f"{duration}", "-guess_layout_max", "0", "-i", audio_file]
            if pix_fmt in DEEP_PIX_FMTS:
                cmd += ["-r", f"{framerate}"] + self._deep_codec_args(pix_fmt, ffmpeg_preset)
            else:
                cmd += ["-r", f"{framerate}", "-vcodec", "libx264", "-pix_fmt", "yuv420p", "-preset", ffmpeg_preset]
            if pix_fmt == "yuv420p":
                cmd += YUV420P_TAGS
            if audio_file is not None:
                cmd += ["-b:a", "320K", "-ac", "2"]
            cmd += [output_file]
            self.proc = subprocess.Popen(cmd, stdin=subprocess.PIPE)
        else:
            ext = "." + pix_fmt
            path = output_file if output_file.endswith(ext) else output_file + ext
            audio = f" -ss {offset} -t {duration} -guess_layout_max 0 -i {audio_file}" if audio_file is not None else ""
            mux = " -b:a 320K -ac 2" if audio_file is not None else ""
            tags = " " + " ".join(YUV420P_TAGS) if pix_fmt == "yuv420p" else ""
            codec = f"-vcodec libx264 -pix_fmt yuv420p -preset {ffmpeg_preset}"
            if pix_fmt in DEEP_PIX_FMTS:
                codec = " ".join(self._deep_codec_args(pix_fmt, ffmpeg_preset))
            target = output_file[:-len(ext)] if output_file.endswith(ext) else output_file
            print(f"ffmpeg binary not found: writing raw {pix_fmt} frames ({width}x{height}) to {path}\n"
                  f"  encode later with: ffmpeg -f rawvideo -pix_fmt {pix_fmt} -framerate {framerate} -s {width}x{height} -i {path}{audio} "
                  f"-r {framerate} {codec}{tags}{mux} {target}")
            self.file = open(path, "wb")

    @staticmethod
    def _deep_codec_args(pix_fmt, ffmpeg_preset):
        """Output side of a deep pipe: HEVC at 10 bits (rgb48le is converted to 4:2:0 by ffmpeg itself and stays untagged, as rgb24 does: a
        tag would claim a matrix this side does not control; the YUV formats carry the matrix the device converted with)."""
        out_fmt = "yuv420p10le" if pix_fmt == "rgb48le" else pix_fmt
        args = ["-vcodec", "libx265", "-pix_fmt", out_fmt, "-tag:v", "hvc1", "-preset", ffmpeg_preset]
        return args + (YUV_P10_TAGS if pix_fmt != "rgb48le" else [])

    def write(self, frame):
        """frame: numpy uint8 [H, W, 3]; wide 2048-px outputs are cropped + resized as render.py:98-105.  A yuv420p sink takes the flat
        planar frame [H * W * 3 / 2] as it is: it was resized on the device before the conversion, neither PIL nor the crop applies.  An
        mjpeg sink takes the flat slot, checks its header and writes the stream alone."""
        if self.pix_fmt != "rgb24":  # a flat frame: its byte count and how the refusal names it (yuv420p's dtype is not looked at)
            if self.pix_fmt == "mjpeg":
                n_bytes, what = mjpeg_slot_bytes(self.w, self.h), "an mjpeg frame of {w}x{h} is a flat uint8 slot of {n} bytes, got {dtype} {shape}"
            elif self.pix_fmt == "yuv420p":
                n_bytes, what = self.w * self.h * 3 // 2, "a yuv420p frame of {w}x{h} is a flat array of {n} bytes, got shape {shape}"
            else:
                n_bytes = deep_frame_bytes(self.pix_fmt, self.w, self.h)
                what = "a " + self.pix_fmt + " frame of {w}x{h} is a flat uint8 array of {n} bytes, got {dtype} {shape}"
            if frame.ndim != 1 or frame.shape[0] != n_bytes or (self.pix_fmt != "yuv420p" and frame.dtype != np.uint8):
                raise ValueError(what.format(w=self.w, h=self.h, n=n_bytes, dtype=frame.dtype, shape=tuple(frame.shape)))
            frame = np.ascontiguousarray(frame)
            if self.pix_fmt == "mjpeg":  # the slot header: the stream's length and the encoder's status
                n, status = (int(v) for v in frame[:8].view("<u4"))
                if status != 0 or 16 + n > n_bytes:
                    raise ValueError(f"mjpeg frame {self.count} overflowed its slot: the stream needs {n} bytes, the slot holds {n_bytes - 16} "
                                     f"(quality {self.quality if self.quality is not None else 'unknown'}: lower it)")
                frame = frame[16: 16 + n]
            if self.proc is not None or self.file is not None:
                (self.proc.stdin if self.proc is not None else self.file).write(memoryview(frame).cast("B"))
            self.count += 1
            return
        # (a frame that already has the sink's size is written as it is: a delivery size of 2048 px is not the reference's wide output)
        if (frame.shape[1] == 2048 or frame.shape[0] == 2048) and (frame.shape[0], frame.shape[1]) != (self.h, self.w):
            import PIL.Image

            if frame.shape[1] == 2048:
                frame = np.array(PIL.Image.fromarray(frame[:, 112:-112, :]).resize((1920, 1080), PIL.Image.BILINEAR))
            else:
                frame = np.array(PIL.Image.fromarray(frame[112:-112, :, :]).resize((1080, 1920), PIL.Image.BILINEAR))
        assert frame.shape[1] == self.w and frame.shape[0] == self.h, (
            f"generator's output image size does not match specified output size: \n"
            f"got: {frame.shape[1]}x{frame.shape[0]}\t\tshould be {self.w}x{self.h}")
        if self.proc is not None or self.file is not None:
            # the frame's own bytes go to the pipe / file (a view of the pinned staging buffer): no tobytes() copy of 3 MiB per frame
            data = memoryview(np.ascontiguousarray(frame)).cast("B")
            (self.proc.stdin if self.proc is not None else self.file).write(data)
        self.count += 1

    def close(self):
        if self.proc is not None:
            self.proc.stdin.close()
            self.proc.wait()
        if self.file is not None:
            self.file.close()


class SinkWorker:
    """Ordered frame delivery OFF the thread that launches the graphs — the role of the reference's two daemon threads and
    queues (render.py:30-44,94-113: `make_video` / `split_batches`).  The launch thread hands over whole batches
    (``submit(wait, frames, count, release)``: ``wait()`` blocks until the batch's device-to-host copy has landed, ``frames[i]`` are
    its uint8 [H, W, 3] frames in a pinned staging slot, ``release()`` returns the slot to its ring) and never calls
    ``sink.write`` itself: a slow encoder fills the ring and then throttles the producer through the ring's free list, it does
    not sit between two graph launches.  Batches are written in submission order.  An exception of the sink is kept and
    re-raised on the launch thread (next ``submit`` or ``close``)."""

    def __init__(self, sink):
        self.sink = sink
        self.error = None
        self._work = queue.Queue()
        self._thread = threading.Thread(target=self._run, name="maua-sink", daemon=True)
        self._thread.start()

    def _run(self):
        while True:
            item = self._work.get()
            if item is None:
                return
            wait, frames, count, release = item
            try:
                if self.error is None:
                    if wait is not None:
                        wait()
                    for i in range(count):
                        self.sink.write(frames[i])
            except BaseException as exc:  # noqa: BLE001 - handed to the launch thread
                self.error = exc
            finally:
                if release is not None:
                    release()

    def _check(self):
        if self.error is not None:
            exc, self.error = self.error, None
            raise exc

    def submit(self, wait, frames, count, release=None):
        self._check()
        self._work.put((wait, frames, count, release))

    def feed(self, wait, frames, count, release=None):
        """``submit`` for a HELPER thread (the host transport's reader): never raises and never takes the sink's error off the worker —
        the error stays where the launch thread's next ``submit`` / ``close`` finds it.  Returns False once the sink has failed (the
        batch is dropped and its slot released: the helper can stop feeding)."""
        if self.error is not None:
            if release is not None:
                release()
            return False
        self._work.put((wait, frames, count, release))
        return True

    def close(self):
        """Wait until everything submitted has been written (or dropped after an error), then re-raise a sink error."""
        if self._thread.is_alive():
            self._work.put(None)
            self._thread.join()
        self._check()


def frames_to_uint8(images, out=None):
    """[B,3,H,W] fp32 device tensor -> [B,H,W,3] uint8 device tensor (render.py:40-43) via the HIP epilogue."""
    lib = _lib.load()
    images = _lib.require_cuda(images, "images")
    b, c, h, w = images.shape
    if c != 3:
        raise RuntimeError("frames must have 3 channels")
    if out is None:
        out = th.empty((b, h, w, 3), dtype=th.uint8, device=images.device)
    with th.cuda.device(images.device):
        _lib.check(lib.maua_frames_to_u8(images.data_ptr(), out.data_ptr(), b, h, w, _lib.stream_ptr(images.device)),
                   "maua_frames_to_u8")
    return out


def _cached(scratch, key, make):
    """``scratch[key]``, made on first use.  ``scratch`` is the dict a render hands to every stage of its tail for what the stage wants to
    find again on the next batch.  A stage keys its buffers by its INPUT buffer: the lanes' batches are in flight concurrently, so there
    is one output buffer per input buffer."""
    value = scratch.get(key)
    if value is None:
        value = scratch[key] = make()
    return value


def _scratch(scratch, key, shape, dtype, dev):
    """The reusable device buffer ``scratch[key]`` (_cached), allocated — not initialised — on first use."""
    return _cached(scratch, key, lambda: th.empty(shape, dtype=dtype, device=dev))


def _wide_output_box(out_size, h, w):
    """(x0, y0, cw, ch, ow, oh) of the built-in delivery of a 1920 / 1080 render's 2048-px frames — 112 px off both ends of the long side,
    then 1920x1080 / 1080x1920 —, None for every other frame."""
    if out_size == 1920 and w == 2048:
        return 112, 0, w - 224, h, 1920, 1080
    if out_size == 1080 and h == 2048:
        return 0, 112, w, h - 224, 1080, 1920
    return None


def _require_fp32_images(images, who):
    """What the stages on the fp32 image take, refused in ``who``'s name."""
    if images.dim() != 4 or images.shape[1] != 3 or images.dtype != th.float32 or not images.is_cuda or not images.is_contiguous():
        raise RuntimeError(f"{who} takes contiguous fp32 [b, 3, H, W] device images, got {images.dtype} {tuple(images.shape)} on {images.device}")


def crop_resize_for_delivery(u8, out_size, scratch):
    """The wide-output delivery of reference render.py:97-104 ON THE DEVICE: 2048-px frames of a 1920 / 1080 render are cropped
    (112 px off both ends of the long side) and resized to 1920x1080 / 1080x1920 by maua_crop_resize_u8 = PIL's bilinear resize —
    the reference does it per frame on the host with PIL, a few milliseconds each on rank 0's Python thread.
    Other frames pass through.  ``scratch``: the render's reusable buffers (_cached)."""
    b, h, w, _ = u8.shape
    box = _wide_output_box(out_size, h, w)
    if box is None:
        return u8
    x0, y0, cw, ch, ow, oh = box
    if ow < cw or oh < ch:
        return u8  # not the up-scale the device kernel reproduces: FrameSink.write falls back to PIL on the host
    out = _scratch(scratch, (u8.data_ptr(), b), (b, oh, ow, 3), th.uint8, u8.device)
    with th.cuda.device(u8.device):
        _lib.check(_lib.load().maua_crop_resize_u8(u8.data_ptr(), out.data_ptr(), b, h, w, x0, y0, cw, ch, ow, oh,
                                                   _lib.stream_ptr(u8.device)), "maua_crop_resize_u8")
    return out


def frames_to_yuv420p(u8, scratch):
    """uint8 [b, H, W, 3] device frames (frames_to_uint8 / crop_resize_for_delivery) -> planar YUV 4:2:0 [b, H * W * 3 // 2] uint8 on the
    device, on the current (= producing) stream: per frame the Y plane, then U, then V (I420: ffmpeg's rawvideo yuv420p), BT.601 limited
    range by maua_rgb_to_yuv420p_u8.  ``scratch``: the render's reusable buffers (_cached)."""
    if u8.dim() != 4 or u8.shape[3] != 3 or u8.dtype != th.uint8 or not u8.is_cuda:
        raise RuntimeError(f"frames_to_yuv420p takes uint8 [b, H, W, 3] device frames, got {u8.dtype} {tuple(u8.shape)} on {u8.device}")
    b, h, w, _ = u8.shape
    if h % 2 or w % 2:
        raise ValueError(f"yuv420p needs even frame dimensions, got {w}x{h}")
    u8 = u8.contiguous()
    out = _scratch(scratch, ("yuv420p", u8.data_ptr(), b, h, w), (b, h * w * 3 // 2), th.uint8, u8.device)
    with th.cuda.device(u8.device):
        _lib.check(_lib.load().maua_rgb_to_yuv420p_u8(u8.data_ptr(), out.data_ptr(), b, h, w, _lib.stream_ptr(u8.device)),
                   "maua_rgb_to_yuv420p_u8")
    return out


def frames_to_mjpeg(u8, scratch, quality):
    """uint8 [b, H, W, 3] device frames -> mjpeg slots [b, mjpeg_slot_bytes(W, H)] uint8 on the device, on the current (= producing) stream:
    per frame a 16-byte slot header (stream length, status) and one baseline JPEG at ``quality`` by maua_jpeg_encode_u8, one restart
    interval per MCU row.  ``scratch``: the render's reusable buffers (_cached): the slots and the workspace per input buffer — the lanes'
    batches are encoded concurrently on their own streams, a workspace cannot be shared between them — and the device copy of the JPEG
    header per (H, W, quality)."""
    if u8.dim() != 4 or u8.shape[3] != 3 or u8.dtype != th.uint8 or not u8.is_cuda:
        raise RuntimeError(f"frames_to_mjpeg takes uint8 [b, H, W, 3] device frames, got {u8.dtype} {tuple(u8.shape)} on {u8.device}")
    b, h, w, _ = u8.shape
    lib = _lib.load()
    u8 = u8.contiguous()
    dev = u8.device
    slot_bytes = mjpeg_slot_bytes(w, h)
    restart_mcus = (w + 15) // 16

    def device_header():
        host = np.empty(1024, np.uint8)
        n = lib.maua_jpeg_header(h, w, quality, restart_mcus, host.ctypes.data, host.size)
        if n <= 0:
            _lib.check(n, "maua_jpeg_header")
        return th.from_numpy(host[:n].copy()).to(dev)

    header = _cached(scratch, ("mjpeg-header", h, w, quality), device_header)
    out, ws = _cached(scratch, ("mjpeg", u8.data_ptr(), b, h, w, quality), lambda: (
        th.empty((b, slot_bytes), dtype=th.uint8, device=dev),
        th.empty(max(int(lib.maua_jpeg_ws_bytes(b, h, w, restart_mcus)), 16), dtype=th.uint8, device=dev)))
    with th.cuda.device(u8.device):
        _lib.check(lib.maua_jpeg_encode_u8(u8.data_ptr(), b, h, w, quality, restart_mcus, header.data_ptr(), header.numel(), out.data_ptr(),
                                           slot_bytes, ws.data_ptr(), _lib.stream_ptr(u8.device)), "maua_jpeg_encode_u8")
    return out


def frames_to_deep(images, out_size, pix_fmt, scratch, resize=None):
    """fp32 [b, 3, H, W] device images (the generator's output, before any quantiser) -> the frames of a deep pipe format (DEEP_PIX_FMTS) as
    flat bytes, uint8 [b, deep_frame_bytes], on the current (= producing) stream (csrc/deep_frames.hip states the arithmetic):
      no resize, a YUV format   maua_frames_to_yuv_p10_f32: one launch, the 16-bit codes never leave the registers
      no resize, rgb48le        maua_frames_to_u16
      2048-px wide outputs      maua_frames_to_u16, maua_crop_resize_u16 to 1920x1080 / 1080x1920 (the crop of crop_resize_for_delivery), then
                                maua_rgb48_to_yuv_p10 for a YUV format
      with ``resize``           maua_frames_to_u16 on the whole generated frame, maua_resample_u16 (resize_frames) to the delivery size, then
                                maua_rgb48_to_yuv_p10 for a YUV format: the resampler works on the 16-bit codes, nothing is re-quantised
    One path: the 16-bit master, the spatial step if there is one, the conversion for a YUV format; the first row is its shortcut.
    ``scratch``: the render's reusable buffers (_cached)."""
    if pix_fmt not in DEEP_PIX_FMTS:
        raise ValueError(f"{pix_fmt!r} is not a deep pipe format ({' | '.join(DEEP_PIX_FMTS)})")
    if images.dim() != 4 or images.shape[1] != 3 or images.dtype != th.float32 or not images.is_cuda:
        raise RuntimeError(f"frames_to_deep takes fp32 [b, 3, H, W] device images, got {images.dtype} {tuple(images.shape)} on {images.device}")
    b, _, h, w = images.shape
    box = None  # the spatial step: ``resize``, the built-in box of the wide outputs, or none — the frames leave at ow x oh
    if resize is not None:
        check_deliver_size(resize, pix_fmt)
        ow, oh = resize.size
    else:
        if h % 2 or w % 2:
            raise ValueError(f"{pix_fmt} needs even frame dimensions, got {w}x{h}")
        box = _wide_output_box(out_size, h, w)
        if box is not None and (box[4] < box[2] or box[5] < box[3]):
            raise ValueError(f"{pix_fmt}: a {w}x{h} frame cannot be delivered at --out_size {out_size}: the device resize only up-scales")
        ow, oh = box[4:] if box is not None else (w, h)
    images = images.contiguous()
    lib, dev, sub, ptr = _lib.load(), images.device, DEEP_SUBSAMPLING.get(pix_fmt), images.data_ptr()
    if b == 0:
        return th.empty((0, deep_frame_bytes(pix_fmt, ow, oh)), dtype=th.uint8, device=dev)
    with th.cuda.device(dev):
        st = _lib.stream_ptr(dev)
        if resize is None and box is None and sub is not None:
            out = _scratch(scratch, ("deep-yuv", ptr, b, h, w, sub), (b, deep_frame_bytes(pix_fmt, w, h) // 2), th.int16, dev)
            _lib.check(lib.maua_frames_to_yuv_p10_f32(ptr, out.data_ptr(), b, h, w, sub, st), "maua_frames_to_yuv_p10_f32")
            return out.view(th.uint8)
        master = _scratch(scratch, ("deep-u16", ptr, b, h, w), (b, h, w, 3), th.int16, dev)  # (uint16 bits in int16 tensors, here and below)
        _lib.check(lib.maua_frames_to_u16(ptr, master.data_ptr(), b, h, w, st), "maua_frames_to_u16")
        if resize is not None:
            master = resize_frames(master, resize, scratch)
        elif box is not None:
            resized = _scratch(scratch, ("deep-resize", ptr, b, oh, ow), (b, oh, ow, 3), th.int16, dev)
            _lib.check(lib.maua_crop_resize_u16(master.data_ptr(), resized.data_ptr(), b, h, w, *box, st), "maua_crop_resize_u16")
            master = resized
        if sub is None:
            return master.view(b, oh * ow * 3).view(th.uint8)
        out = _scratch(scratch, ("deep-yuv", ptr, b, oh, ow, sub), (b, deep_frame_bytes(pix_fmt, ow, oh) // 2), th.int16, dev)
        _lib.check(lib.maua_rgb48_to_yuv_p10(master.data_ptr(), out.data_ptr(), b, oh, ow, sub, st), "maua_rgb48_to_yuv_p10")
        return out.view(th.uint8)


def grade_frames(images, grade_rows, lut, scratch, out="u8"):
    """fp32 [b, 3, H, W] device images (the generator's output) graded on the current (= producing) stream by csrc/grade.hip: ASC CDL slope /
    offset / power, a 3 x 3 matrix with bias and a 3-D LUT (include/maua_hip.h states the arithmetic; audioreactive/grade.py's Grade builds
    the operands).  ``grade_rows``: float32 device rows [b, >= 24], one per frame of the batch (a view into a longer table is fine: the row
    stride is passed on); ``lut``: Grade.lut_table's padded table [N^3, 4] or None.
      out="u8"   -> uint8 [b, H, W, 3] by maua_grade_to_u8 (= frames_to_uint8 of the graded image), in a reusable buffer of ``scratch``
                    (_cached)
      out="f32"  -> ``images`` itself, graded in place by maua_grade_f32
    Frames whose row is the identity come out as they went in (as frames_to_uint8's for "u8")."""
    if out not in ("u8", "f32"):
        raise ValueError(f"unknown grade output {out!r} (u8 | f32)")
    _require_fp32_images(images, "grade_frames")
    b, _, h, w = images.shape
    dev = images.device
    if (grade_rows.dim() != 2 or grade_rows.shape[0] != b or grade_rows.shape[1] < 24 or grade_rows.dtype != th.float32 or grade_rows.device != dev
            or (b > 0 and grade_rows.stride(1) != 1) or (b > 1 and grade_rows.stride(0) < 24)):
        raise RuntimeError(f"grade_frames takes float32 rows [{b}, >= 24] on {dev}, got {grade_rows.dtype} {tuple(grade_rows.shape)} "
                           f"(strides {grade_rows.stride()}) on {grade_rows.device}")
    lut_n = 0
    if lut is not None:
        if lut.dim() != 2 or lut.shape[1] != 4 or lut.dtype != th.float32 or lut.device != dev or not lut.is_contiguous():
            raise RuntimeError(f"grade_frames takes the padded LUT [N^3, 4] float32 on {dev}, got {lut.dtype} {tuple(lut.shape)} on {lut.device}")
        lut_n = round(lut.shape[0] ** (1 / 3))
        if lut_n ** 3 != lut.shape[0]:
            raise RuntimeError(f"grade_frames: a LUT of {lut.shape[0]} entries is not a cube")
    stride = grade_rows.stride(0) if b > 1 else 24
    lib = _lib.load()
    if out == "f32":
        if b:
            with th.cuda.device(dev):
                _lib.check(lib.maua_grade_f32(images.data_ptr(), images.data_ptr(), b, h, w, grade_rows.data_ptr(), stride, _lib.ptr(lut), lut_n,
                                              _lib.stream_ptr(dev)), "maua_grade_f32")
        return images
    u8 = _scratch(scratch, ("grade-u8", images.data_ptr(), b, h, w), (b, h, w, 3), th.uint8, dev)
    if b:
        with th.cuda.device(dev):
            _lib.check(lib.maua_grade_to_u8(images.data_ptr(), u8.data_ptr(), b, h, w, grade_rows.data_ptr(), stride, _lib.ptr(lut), lut_n,
                                            _lib.stream_ptr(dev)), "maua_grade_to_u8")
    return u8


def _per_frame_table(what, n_rows, n_rendered):
    """The rule of the per-frame tables of a grade, a lens and a feedback: one row for every frame, or one row per rendered frame; anything
    else is refused.  Returns whether frame f reads row f (a one-row table: every frame reads row 0)."""
    if n_rows not in (1, n_rendered):
        raise ValueError(f"the {what}'s table has {n_rows} rows: it needs one row, or one per rendered frame ({n_rendered})")
    return n_rows != 1 or n_rendered == 1


def _batch_rows(table, per_frame, batch_size):
    """A [n, k] table (device tensor or numpy array) as the launches index it: a one-row table repeated to a batch, so that every launch
    finds a row per frame at the table's stride; a per-frame table as it is."""
    if per_frame:
        return table
    if isinstance(table, np.ndarray):
        return np.ascontiguousarray(np.broadcast_to(table, (max(batch_size, 1), table.shape[1])))
    return table.expand(max(batch_size, 1), table.shape[1]).contiguous()


class _TableOperands:
    """A render's grade, lens or feedback (``KIND``: its audioreactive class) on one device: the effect — under its own name, ``.grade`` /
    ``.lens`` / ``.feedback`` —, whether its table holds a row per rendered frame (_per_frame_table: a table that has neither one row nor
    ``n_rendered`` is refused), the tables per frame size (``sized``: a subclass builds them in ``_tables``) and the rows of a batch
    (``window``)."""

    KIND = None

    def __init__(self, effect, n_rendered, batch_size, dev):
        self.name = self.KIND.__name__.lower()
        if not isinstance(effect, self.KIND):
            raise TypeError(f"{self.name} must be an audioreactive {self.KIND.__name__}, got {type(effect).__name__}")
        setattr(self, self.name, effect)
        self.per_frame, self.batch_size, self.dev = _per_frame_table(self.name, effect.n_rows, n_rendered), batch_size, dev
        self._sized = {}

    def sized(self, h, w):
        """The tables for frames of h x w (``_tables``), built once per size."""
        if (h, w) not in self._sized:
            self._sized[(h, w)] = self._tables(h, w)
        return self._sized[(h, w)]

    def window(self, table, first, count):
        """The rows of the batch that starts at rendered frame ``first``: [first, first + count) of a per-frame table, else the first
        ``count`` of the one row repeated to a batch (_batch_rows)."""
        lo = first if self.per_frame else 0
        if lo < 0 or lo + count > table.shape[0]:
            raise RuntimeError(f"the frames {lo} .. {lo + count} are not inside the {table.shape[0]} rows of the {self.name}")
        return table[lo: lo + count]


class GradeOperands(_TableOperands):
    """A render's grade on one device: ``rows`` (the device row table, _batch_rows) and ``lut`` (the padded LUT, or None)."""

    KIND = Grade

    def __init__(self, grade, n_rendered, batch_size, dev):
        super().__init__(grade, n_rendered, batch_size, dev)
        self.rows, self.lut = _batch_rows(grade.rows(dev), self.per_frame, batch_size), grade.lut_table(dev)


class LensOperands(_TableOperands):
    """A render's lens on one device; per frame size — the plan rule needs the height — the device tables (_batch_rows)."""

    KIND = Lens

    def _tables(self, h, w):
        """(rows, d, bloom radius, bloom taps, sharpen radius, sharpen taps) for frames of h x w."""
        rows, d, rb, bt, rs, st = self.lens.operands(self.dev, h, w)
        rows, bt, st = (_batch_rows(t, self.per_frame, self.batch_size) for t in (rows, bt, st))
        return rows, d, rb, bt, rs, st


def lens_frames(images, lens_ops, first, count, scratch):
    """fp32 [b, 3, H, W] device images (the generator's output; b == count) through the lens of csrc/lens.hip, IN PLACE, on the current
    (= producing) stream: bloom (highlights extracted and averaged over d x d blocks, that map blurred by the frame's Gaussian, added back
    bilinearly), sharpen / soften (against a short Gaussian of the image) and vignette; include/maua_hip.h states the arithmetic,
    audioreactive/lens.py's Lens builds the operands.  ``lens_ops``: LensOperands; ``first``: the batch's first rendered frame (its rows
    are [first, first + count) of a per-frame table).  The bloom chain (extract, blur) is launched only when some row of the JOB has a
    bloom, the sharpen's blur only when some row has a sharpen, nothing at all for a lens that is the identity throughout; frames whose
    row is the identity come out as they went in, bit for bit.  The reduced maps and the soft image live in ``scratch`` (_cached)."""
    _require_fp32_images(images, "lens_frames")
    b, _, h, w = images.shape
    if b != count:
        raise RuntimeError(f"lens_frames: {b} images for {count} frames")
    lens = lens_ops.lens
    if b == 0 or lens.is_identity:
        return images
    dev = images.device
    rows, d, rb, btaps, rs, staps = lens_ops.sized(h, w)
    rows, btaps, staps = (lens_ops.window(t, first, b) for t in (rows, btaps, staps))
    lib = _lib.load()
    st = _lib.stream_ptr(dev)
    bloom = soft = None
    bh, bw = -(-h // d), -(-w // d)
    with th.cuda.device(dev):
        if lens.has_bloom:
            maps = _scratch(scratch, ("lens-bloom", images.data_ptr(), b, bh, bw), (2, b, 3, bh, bw), th.float32, dev)
            _lib.check(lib.maua_lens_extract_f32(images.data_ptr(), maps[0].data_ptr(), b, h, w, d, rows.data_ptr(), rows.stride(0), st),
                       "maua_lens_extract_f32")
            _lib.check(lib.maua_lens_blur_f32(maps[0].data_ptr(), maps[1].data_ptr(), b, 3, bh, bw, rb, btaps.data_ptr(), btaps.stride(0), st),
                       "maua_lens_blur_f32")
            bloom = maps[1]
        if lens.has_sharpen:
            soft = _scratch(scratch, ("lens-soft", images.data_ptr(), b, h, w), (b, 3, h, w), th.float32, dev)
            _lib.check(lib.maua_lens_blur_f32(images.data_ptr(), soft.data_ptr(), b, 3, h, w, rs, staps.data_ptr(), staps.stride(0), st),
                       "maua_lens_blur_f32")
        _lib.check(lib.maua_lens_apply_f32(images.data_ptr(), images.data_ptr(), b, h, w, rows.data_ptr(), rows.stride(0), _lib.ptr(bloom), bh, bw, d,
                                           _lib.ptr(soft), st), "maua_lens_apply_f32")
    return images


class FeedbackOperands(_TableOperands):
    """A render's feedback on one device, and what outlives a batch — the persistent ``state`` [3, H, W] (the last output frame; allocated
    by the render before the lanes start, NOT a lane buffer: a lane's image is overwritten by that lane's next replay while the following
    batch, on another lane, still has to read it), whether it holds a frame yet, and the event recorded behind the last batch's feedback
    (feedback_frames chains the lanes' streams on it)."""

    KIND = Feedback

    def __init__(self, feedback, n_rendered, batch_size, dev):
        super().__init__(feedback, n_rendered, batch_size, dev)
        self.state, self.state_valid, self.done = None, False, None

    def _tables(self, h, w):
        """(rows — float32 [n, 16] on the host, a one-row table repeated to a batch —, mode, border) for frames of h x w."""
        rows, mode, border = self.feedback.operands(h, w)
        return np.ascontiguousarray(_batch_rows(rows, self.per_frame, self.batch_size), np.float32), mode, border

    def allocate(self, h, w):
        """The state buffer for frames of h x w, on the current stream (the render's own, which the lanes' streams wait for when they
        start and which waits for them when they finish: the allocator may hand the block on only after that); a new size starts
        from black."""
        if self.state is None or tuple(self.state.shape) != (3, h, w):
            self.state, self.state_valid = th.empty((3, h, w), dtype=th.float32, device=self.dev), False
        return self.state


# (the names the lens and feedback operands were built by before they were classes: tests and tools call them, with these arguments.
# The tail names the classes themselves, looked up when it is loaded)
_lens_operands, _feedback_operands = LensOperands, FeedbackOperands


def feedback_frames(images, ops, first, count, scratch):
    """fp32 [b, 3, H, W] device images (the generator's output; b == count) through the frame feedback of csrc/feedback.hip, IN PLACE, on
    the current (= producing) stream: frame i of the batch is combined with the warped, scaled frame i - 1 of the RESULT, the batch's
    first frame with the last result of the previous batch (``ops.state``; black before the render's first frame); include/maua_hip.h
    states the arithmetic, audioreactive/feedback.py's Feedback builds the rows.  ``ops``: FeedbackOperands; ``first``: the batch's first
    rendered frame (its rows are [first, first + count) of a per-frame table).  Batches must arrive in frame order.  Nothing is launched
    for a feedback that is neutral throughout.  ``scratch`` is not used: the only buffer that outlives the call is the state.

    Cross-lane ordering.  Consecutive batches run on different lane streams, and this is a recurrence: before its launches a batch's
    stream waits for the event the previous batch recorded behind its own (``ops.done``), and records a new one behind them.  Why
    ``state`` is safe to overwrite when this batch's last launch does so: every access to it — the read by a batch's first launch, the
    write by its last — is one of the launches strung on that chain of events, batch after batch, and within a batch the launches are in
    stream order; so the only launch that reads the old state after the previous batch wrote it is this batch's first, which precedes
    this batch's last on the same stream, and the next reader waits for the event recorded after the write.  Nothing else reads it: the
    lens, the grade and the quantisers work on the lane's image."""
    _require_fp32_images(images, "feedback_frames")
    del scratch
    b, _, h, w = images.shape
    if b != count:
        raise RuntimeError(f"feedback_frames: {b} images for {count} frames")
    if b == 0 or ops.feedback.is_identity:
        return images
    dev = images.device
    rows, mode, border = ops.sized(h, w)
    rows = ops.window(rows, first, b)
    ops.allocate(h, w)  # (the render has done so on its own stream before the lanes started)
    lib = _lib.load()
    with th.cuda.device(dev):
        stream = th.cuda.current_stream(dev)
        if ops.done is not None:
            stream.wait_event(ops.done)
        _lib.check(lib.maua_feedback_f32(images.data_ptr(), images.data_ptr(), ops.state.data_ptr(), int(ops.state_valid), b, h, w,
                                         rows.ctypes.data, rows.strides[0] // 4, mode, border, _lib.stream_ptr(dev)), "maua_feedback_f32")
        ops.state_valid = True
        ops.done = stream.record_event()
    return images


MAX_SUBFRAMES = 16
SHUTTER_LIGHTS = ("encoded", "linear")


def shutter_weights(shutter, subframes):
    """The integer weights (0 .. 255, not all zero) of a shutter over ``subframes`` sub-frames: "box" (all ones), "tent"
    (w_i = min(i + 1, N - i)) or a comma-separated list of N integers — "1,1,0,0" is a 180 degree shutter."""
    n = subframes
    if shutter == "box":
        return (1,) * n
    if shutter == "tent":
        return tuple(min(i + 1, n - i) for i in range(n))
    try:
        weights = tuple(int(part) for part in str(shutter).split(","))
    except ValueError:
        raise ValueError(f"shutter {shutter!r} is neither box, tent nor a comma-separated list of integers") from None
    if len(weights) != n:
        raise ValueError(f"shutter {shutter!r} lists {len(weights)} weights for {n} sub-frames")
    if any(not 0 <= w <= 255 for w in weights):
        raise ValueError(f"shutter {shutter!r}: weights are integers in 0 .. 255")
    if not any(weights):
        raise ValueError(f"shutter {shutter!r}: the weights must not all be zero")
    return weights


class TemporalFold:
    """Temporal supersampling: ``subframes`` (1 .. 16) consecutive rendered frames are averaged into one delivered frame on the device
    (fold_frames) with the integer ``weights`` of ``shutter`` (shutter_weights), on the frames' encoded values (``light="encoded"``) or on
    linear light through the sRGB transfer function (``light="linear"``, srgb_fold_tables).  Sub-frames of weight zero are still rendered."""

    def __init__(self, subframes, shutter="box", light="encoded"):
        if isinstance(subframes, bool) or int(subframes) != subframes or not 1 <= int(subframes) <= MAX_SUBFRAMES:
            raise ValueError(f"subframes must be an integer in 1 .. {MAX_SUBFRAMES}, got {subframes!r}")
        if light not in SHUTTER_LIGHTS:
            raise ValueError(f"unknown shutter light {light!r} ({' | '.join(SHUTTER_LIGHTS)})")
        self.subframes = int(subframes)
        self.shutter = shutter
        self.light = light
        self.weights = shutter_weights(shutter, self.subframes)

    def __repr__(self):
        return f"TemporalFold({self.subframes}, shutter={self.shutter!r}, light={self.light!r})"


def _fold_from_env():
    """The fold of the entries that have no parameter for it (render, render_shard): $MAUA_SUBFRAMES, $MAUA_SHUTTER (box),
    $MAUA_SHUTTER_LIGHT (encoded).  $MAUA_SUBFRAMES unset, empty or 1: no fold."""
    text = os.environ.get("MAUA_SUBFRAMES")
    if not text:
        return None
    try:
        subframes = int(text)
    except ValueError:
        raise ValueError(f"$MAUA_SUBFRAMES {text!r} is not an integer") from None
    if subframes == 1:  # the plain render, whatever the other two say
        return None
    return TemporalFold(subframes, os.environ.get("MAUA_SHUTTER") or "box", os.environ.get("MAUA_SHUTTER_LIGHT") or "encoded")


def _subframes(fold):
    """Rendered frames per delivered frame: 1 without a fold."""
    return 1 if fold is None else fold.subframes


def srgb_fold_tables():
    """The two 256-entry uint16 tables of a linear-light fold, numpy, built in float64 from the piecewise sRGB transfer function (IEC
    61966-2-1): decode[v] = rint(65535 * srgb_to_linear(v / 255)) and encode_threshold[v] = the smallest 16-bit L whose
    rint(255 * linear_to_srgb(L / 65535)) is >= v.  The encoding is monotone in L, so max{v : encode_threshold[v] <= L} IS the encoding
    of L; encode(decode[v]) == v for every v (tests/test_temporal_fold_host.py)."""
    v = np.arange(256, dtype=np.float64) / 255.0
    decode = np.rint(65535.0 * np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)).astype(np.uint16)
    lin = np.arange(65536, dtype=np.float64) / 65535.0
    encoded = np.rint(255.0 * np.where(lin <= 0.0031308, 12.92 * lin, 1.055 * lin ** (1.0 / 2.4) - 0.055)).astype(np.int64)
    threshold = np.searchsorted(encoded, np.arange(256), side="left").astype(np.uint16)  # (encoded is non-decreasing and reaches 255)
    return decode, threshold


def check_fold_tables(decode, encode_threshold):
    """What csrc/temporal_fold.hip assumes of its tables: 256 uint16 entries each, encode_threshold[0] == 0, non-decreasing thresholds."""
    decode, encode_threshold = np.asarray(decode), np.asarray(encode_threshold)
    for name, table in (("decode", decode), ("encode_threshold", encode_threshold)):
        if table.shape != (256,) or table.dtype != np.uint16:
            raise ValueError(f"{name} must hold 256 uint16 entries, got {table.dtype} {tuple(table.shape)}")
    if encode_threshold[0] != 0 or np.any(np.diff(encode_threshold.astype(np.int64)) < 0):
        raise ValueError("encode_threshold must start at 0 and must not decrease")
    return decode, encode_threshold


_FOLD_TABLES = {}  # device index -> (decode, encode_threshold) of srgb_fold_tables on that device (uint16 bits in int16 tensors)


def _device_fold_tables(dev):
    index = dev.index if dev.index is not None else th.cuda.current_device()
    tables = _FOLD_TABLES.get(index)
    if tables is None:
        host = check_fold_tables(*srgb_fold_tables())
        tables = _FOLD_TABLES[index] = tuple(th.from_numpy(t.view(np.int16).copy()).to(dev) for t in host)
    return tables


def fold_frames(u8, fold, scratch):
    """uint8 [b, ...] device frames -> [b // N, ...] on the current (= producing) stream: frame g of the result is the weighted average of
    the frames g N .. g N + N - 1 (TemporalFold; maua_temporal_fold_u8 states the arithmetic).  ``scratch``: the render's reusable buffers
    (_cached)."""
    if u8.dim() < 2 or u8.dtype != th.uint8 or not u8.is_cuda:
        raise RuntimeError(f"fold_frames takes uint8 [b, ...] device frames, got {u8.dtype} {tuple(u8.shape)} on {u8.device}")
    n = fold.subframes
    b = u8.shape[0]
    if b % n:
        raise ValueError(f"a batch of {b} frames does not hold whole groups of {n} sub-frames")
    u8 = u8.contiguous()
    frame_bytes = int(np.prod(u8.shape[1:]))
    out = _scratch(scratch, ("fold", u8.data_ptr(), b, n, tuple(u8.shape[1:])), (b // n,) + tuple(u8.shape[1:]), th.uint8, u8.device)
    decode, threshold = _device_fold_tables(u8.device) if fold.light == "linear" else (None, None)
    weights = (ctypes.c_uint8 * n)(*fold.weights)
    with th.cuda.device(u8.device):
        _lib.check(_lib.load().maua_temporal_fold_u8(u8.data_ptr(), out.data_ptr(), b // n, n, frame_bytes, weights, _lib.ptr(decode),
                                                     _lib.ptr(threshold), _lib.stream_ptr(u8.device)), "maua_temporal_fold_u8")
    return out


RESIZE_FILTERS = ("lanczos", "bicubic", "hamming", "bilinear", "box")
RESIZE_FITS = ("crop", "pad", "stretch")


def parse_deliver_size(text):
    """``"WxH"`` (the --deliver_size flag, $MAUA_DELIVER_SIZE) or a (w, h) pair -> (w, h), both at least 1."""
    if isinstance(text, str):
        parts = text.lower().split("x")
        try:
            size = tuple(int(p) for p in parts)
        except ValueError:
            size = ()
        if len(size) != 2:
            raise ValueError(f"--deliver_size {text!r} is not WIDTHxHEIGHT (e.g. 1920x1080)")
    else:
        size = tuple(int(v) for v in text)
        if len(size) != 2:
            raise ValueError(f"a delivery size is (width, height), got {text!r}")
    if size[0] < 1 or size[1] < 1:
        raise ValueError(f"--deliver_size {size[0]}x{size[1]}: both sides must be at least 1")
    return size


class FrameResize:
    """Delivery at a size of the user's choice: every frame is resampled on the device (resize_frames; csrc/resample.hip = Pillow's
    ``Image.resize`` in integers) to ``size`` = (w, h) or "WxH" with ``filter`` (RESIZE_FILTERS) before the colour conversion.  ``fit`` says
    how a W x H source meets another aspect ratio, in integers (``geometry``):
      stretch  the whole source maps to the whole target
      crop     the centred box of the target's aspect ratio: W h > H w -> cw = clamp((H w + h // 2) // h, 1, W), ch = H; else
               ch = clamp((W h + w // 2) // w, 1, H), cw = W; x0 = (W - cw) // 2, y0 = (H - ch) // 2
      pad      the whole source into a centred window dw x dh of the target, one side the target's, the other (H w + W // 2) // W or
               (W h + H // 2) // H, both rounded down to even (at least 2), at the even offsets ((w - dw) // 2) & ~1, ((h - dh) // 2) & ~1;
               the border is RGB 0
    With a resize set the built-in 112-px crop of the 1920 / 1080 outputs is skipped: the source is the whole generated frame."""

    def __init__(self, size, filter="lanczos", fit="crop"):
        self.size = parse_deliver_size(size)
        if filter not in RESIZE_FILTERS:
            raise ValueError(f"unknown --deliver_filter {filter!r} ({' | '.join(RESIZE_FILTERS)})")
        if fit not in RESIZE_FITS:
            raise ValueError(f"unknown --deliver_fit {fit!r} ({' | '.join(RESIZE_FITS)})")
        self.filter, self.fit = filter, fit

    def __repr__(self):
        return f"FrameResize({self.size[0]}x{self.size[1]}, filter={self.filter!r}, fit={self.fit!r})"

    def key(self):
        return self.size + (self.filter, self.fit)

    def geometry(self, W, H):
        """(box, window) for a W x H source: the source box (x0, y0, x1, y1) and the target window (x, y, w, h) it is resampled into."""
        w, h = self.size
        if W < 1 or H < 1:
            raise ValueError(f"a {W}x{H} frame cannot be resized")
        if self.fit == "stretch":
            return (0, 0, W, H), (0, 0, w, h)
        if self.fit == "crop":
            if W * h > H * w:
                cw, ch = min(max((H * w + h // 2) // h, 1), W), H
            else:
                cw, ch = W, min(max((W * h + w // 2) // w, 1), H)
            x0, y0 = (W - cw) // 2, (H - ch) // 2
            return (x0, y0, x0 + cw, y0 + ch), (0, 0, w, h)
        if w < 2 or h < 2:
            raise ValueError(f"--deliver_fit pad needs a target of at least 2x2, got --deliver_size {w}x{h}")
        if W * h > H * w:
            dw, dh = w, (H * w + W // 2) // W
        else:
            dw, dh = (W * h + H // 2) // H, h
        dw, dh = max(min(dw, w) & ~1, 2), max(min(dh, h) & ~1, 2)
        return (0, 0, W, H), (((w - dw) // 2) & ~1, ((h - dh) // 2) & ~1, dw, dh)


def check_deliver_size(resize, pix_fmt):
    """yuv420p and the deep formats need even sides: refused with the flag's name, before anything is rendered."""
    if resize is not None and (pix_fmt == "yuv420p" or pix_fmt in DEEP_PIX_FMTS) and (resize.size[0] % 2 or resize.size[1] % 2):
        raise ValueError(f"--deliver_size {resize.size[0]}x{resize.size[1]}: --pipe_pix_fmt {pix_fmt} needs even sides")


def _resize_from_env():
    """The resize of the entries that have no parameter for it (render, render_shard, render_folded): $MAUA_DELIVER_SIZE (WxH),
    $MAUA_DELIVER_FILTER (lanczos), $MAUA_DELIVER_FIT (crop).  $MAUA_DELIVER_SIZE unset or empty: none, and the other two are not read."""
    text = os.environ.get("MAUA_DELIVER_SIZE")
    if not text:
        return None
    return FrameResize(text, os.environ.get("MAUA_DELIVER_FILTER") or "lanczos", os.environ.get("MAUA_DELIVER_FIT") or "crop")


_RESIZE_TABLES = {}  # (device index, W, H) + FrameResize.key() -> (box, window, (kx, bx, ksize_x), (ky, by, ksize_y)) with device tables


def _resize_tables(dev, W, H, resize):
    index = dev.index if dev.index is not None else th.cuda.current_device()
    key = (index, W, H) + resize.key()
    entry = _RESIZE_TABLES.get(key)
    if entry is None:
        box, window = resize.geometry(W, H)
        axes = []
        for n, in0, in1, m, name in ((W, box[0], box[2], window[2], "width"), (H, box[1], box[3], window[3], "height")):
            if m == n and in0 == 0 and in1 == n:
                axes.append((None, None, 0))  # the definition copies the axis
                continue
            rc, k, bounds = _lib.resample_coeffs(n, in0, in1, m, resize.filter)
            if rc == -38:
                raise ValueError(f"--deliver_size {resize.size[0]}x{resize.size[1]}: the {name} {in1 - in0} -> {m} needs more than "
                                 f"{_lib.RESAMPLE_MAX_TAPS} {resize.filter} taps; choose a larger size or a shorter filter (bilinear, box)")
            if rc <= 0:
                _lib.check(rc, "maua_resample_coeffs")
            axes.append((th.from_numpy(k).to(dev), th.from_numpy(bounds).to(dev), rc))
        entry = _RESIZE_TABLES[key] = (box, window, axes[0], axes[1])
    return entry


def resize_frames(frames, resize, scratch):
    """uint8 — or int16-viewed uint16 — [b, H, W, 3] device frames -> [b, h, w, 3] of the same type at ``resize.size`` on the current
    (= producing) stream, by maua_resample_u8 / maua_resample_u16 with ``resize``'s filter and fit.  The device tables are cached per
    (device, source size, setting).  ``scratch``: the render's reusable buffers (_cached), here the output and the workspace; a padded
    frame's border is zeroed when the buffer is allocated and never written again."""
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.dtype not in (th.uint8, th.int16) or not frames.is_cuda:
        raise RuntimeError(f"resize_frames takes uint8 or int16 [b, H, W, 3] device frames, got {frames.dtype} {tuple(frames.shape)} on "
                           f"{frames.device}")
    frames = frames.contiguous()
    b, H, W, _ = frames.shape
    dev = frames.device
    sz = 1 if frames.dtype == th.uint8 else 2
    box, (x, y, w, h), (kx, bx, ksx), (ky, by, ksy) = _resize_tables(dev, W, H, resize)
    ow, oh = resize.size
    lib = _lib.load()

    def buffers():
        n_ws = int(lib.maua_resample_ws_bytes(sz, b, H, W, w, h, ksx, ksy))
        return th.zeros((b, oh, ow, 3), dtype=frames.dtype, device=dev), th.empty(n_ws, dtype=th.uint8, device=dev) if n_ws else None

    out, ws = _cached(scratch, ("resize", frames.data_ptr(), b, H, W, sz) + resize.key(), buffers)
    if b == 0:
        return out
    fn = lib.maua_resample_u8 if sz == 1 else lib.maua_resample_u16
    with th.cuda.device(dev):
        _lib.check(fn(frames.data_ptr(), out.data_ptr(), b, H, W, oh, ow, x, y, w, h, _lib.ptr(kx), _lib.ptr(bx), ksx, _lib.ptr(ky), _lib.ptr(by),
                      ksy, _lib.ptr(ws), _lib.stream_ptr(dev)), "maua_resample_u8" if sz == 1 else "maua_resample_u16")
    return out


def _deliverable(u8, out_size, pix_fmt, scratch, quality=None, fold=None, resize=None):
    """A batch as it leaves the device: the sub-frames of a temporal fold averaged (on the generator's own frames, so that every later
    stage sees delivered frames only), wide frames cropped + resized — or, with ``resize`` (FrameResize), every frame resampled to the
    delivery size —, then — yuv420p — converted to planar 4:2:0 or — mjpeg — encoded."""
    if _subframes(fold) > 1:
        u8 = fold_frames(u8, fold, scratch)
    # (a resize of the user's replaces the built-in crop: its source is the whole generated frame)
    u8 = crop_resize_for_delivery(u8, out_size, scratch) if resize is None else resize_frames(u8, resize, scratch)
    if pix_fmt == "mjpeg":
        return frames_to_mjpeg(u8, scratch, MJPEG_DEFAULT_QUALITY if quality is None else quality)
    return frames_to_yuv420p(u8, scratch) if pix_fmt == "yuv420p" else u8


class parked_heap:
    """``with parked_heap():`` — no generation-2 collection on the thread that launches the graph replays: everything alive at entry moves
    to the collector's permanent generation (gc.freeze) and comes back at exit.  Re-entrant and shared between threads: the freeze is
    process-global, so the FIRST frame loop in parks the heap and the LAST one out thaws it (an unconditional unfreeze at the end of one
    render thawed the heap under a second render's loop), and a heap the embedding application froze itself (a pre-fork server:
    gc.get_freeze_count() > 0 at entry of the first loop) is left frozen."""

    _lock = threading.Lock()
    _users = 0
    _ours = False

    def __enter__(self):
        cls = parked_heap
        with cls._lock:
            if cls._users == 0:
                cls._ours = gc.get_freeze_count() == 0
                if cls._ours:
                    gc.freeze()
            cls._users += 1
        return self

    def __exit__(self, *exc):
        cls = parked_heap
        with cls._lock:
            cls._users -= 1
            if cls._users == 0 and cls._ours:
                gc.unfreeze()
                cls._ours = False
        return False


_RING_LOCKS = {}  # device index -> lock held by the single-GPU render loop while it uses that device's rings (two renders in two threads)
_PINNED_RING = {}  # device index -> pinned staging slots of the single-GPU render loop (reallocated when the frame shape changes)
_DEVICE_RING = {}  # device index -> their device-side twins (a batch leaves its lane's frame buffer before it crosses PCIe)
_RING_SLOTS = 6
_LANE_STREAMS = {}  # (device index, lane number) -> the stream that lane's forwards run on (_lane_stream)


def release_rings(device=None):
    """Free the pinned / device staging rings of the single-GPU render loop (6 x batch frames each, kept across renders by default) for
    ``device`` (index or torch.device; default: every device)."""
    index = None if device is None else (th.device(device).index if not isinstance(device, int) else device)
    for ring in (_PINNED_RING, _DEVICE_RING):
        for key in list(ring):
            if index is None or key == index:
                with _RING_LOCKS.setdefault(key, threading.Lock()):
                    del ring[key]


def _lane_stream(dev, k):
    # lane streams are kept per device: the caching allocator pools freed blocks per stream, so fresh streams on
    # every call would strand the staging buffers of the previous render
    stream = _LANE_STREAMS.get((dev.index, k))
    if stream is None:
        stream = _LANE_STREAMS[(dev.index, k)] = th.cuda.Stream(dev)
    return stream


UNSEEDED_GRAPH_MIN_FRAMES = 2048  # randomised renders without generator.noise_seed below this length keep the eager path (synthesize)


def _lane_is_stale(lane, weights_key, slots, seed, offset, synth_slots, synth_offset):
    """Whether a cached lane has to be captured again: its weights changed, or a kernel argument of one of its captured noise launches
    differs from what this render asks for — (seed, frame offset) of the random slots, the frame offset of the synthesised ones."""
    if lane.weights_key != weights_key:
        return True
    if slots and (lane.noise_seed, lane.noise_frame_offset) != (seed, offset):
        return True
    return bool(synth_slots) and lane.synth_frame_offset != synth_offset


def graph_lanes(generator, batch_size, n_lanes, bends=(), random=None, synth=None, frames="u8"):
    """``n_lanes`` captured forwards (GraphLane) of ``batch_size`` frames with uint8 frame output (``frames="f32"``: with the fp32 image
    [b, 3, H, W] as the output, no quantiser in the graph; cached next to the uint8 lanes), each on its own stream.
    Without bends they are cached on the generator and reused by every later render (a captured forward reads its inputs
    through a frame source, so nothing about a particular render is baked in); a changed weight drops the cache.  With bends the
    transforms' static operands are part of the graph: captured per call.  ``random`` = (slots, seed, frame offset): lanes that generate
    the noise maps of ``slots`` themselves (``Generator.capture_graph``'s random_slots); cached per slot set next to the static lanes, and
    captured again when the seed or the offset — kernel arguments of the captured noise launch — differ from the cached lane's.
    ``synth`` = (slots, frame offset): lanes that synthesise the maps of ``slots`` from NoiseSynth recipes (capture_graph's synth_slots); cached
    per slot set as well.  The recipes live in a device table that ``bind`` rewrites, so another render's recipes reuse the captured graph;
    only another frame offset (a shard's first frame, the one kernel argument of that launch) captures again."""
    dev = device_of(generator)
    slots, seed, offset = random if random else ((), 0, 0)
    slots = tuple(slots)
    synth_slots, synth_offset = (tuple(synth[0]), int(synth[1])) if synth else ((), 0)
    # only what the render asks for is passed on: StyleGAN1's capture_graph takes (batch, lane, frames_u8, bends) and nothing else
    extra = {}
    if slots:
        extra.update(random_slots=slots, noise_seed=seed, noise_frame_offset=offset)
    if synth_slots:
        extra.update(synth_slots=synth_slots, synth_frame_offset=synth_offset)
    key = generator.weights_key()
    cache = generator.__dict__.setdefault("_graph_lanes", {})
    lanes = []
    tap = bool(getattr(generator, "tap_float_image", False))  # (parity tests: such lanes also write the fp32 image — other kernels arguments)
    if frames not in ("u8", "f32"):
        raise ValueError(f"unknown frame kind {frames!r} (u8 | f32)")
    for k in range(n_lanes):
        stream = _lane_stream(dev, k)
        cache_key = (batch_size, k, tap) + ((slots,) if slots else ()) + ((("synth",) + synth_slots,) if synth_slots else ())
        if frames != "u8":  # (the uint8 lanes' key carries no frame kind)
            cache_key += (("frames", frames),)
        lane = None if bends else cache.get(cache_key)
        if lane is None or _lane_is_stale(lane, key, slots, seed, offset, synth_slots, synth_offset):
            stream.wait_stream(th.cuda.current_stream(dev))
            with th.cuda.stream(stream):
                lane = generator.capture_graph(batch_size, lane=k, frames_u8=frames == "u8", bends=bends, **extra)
            stream.synchronize()
            if not bends:
                cache[cache_key] = lane
        lanes.append((stream, lane))
    return lanes


def prepare(generator, batch_size, lanes=3, bends=False):
    """Everything of a render that does not depend on its inputs: weight packing, static buffers and — a captured forward reads
    its inputs through a frame source, so it needs none of them — the graph lanes themselves.  generate() calls this on the
    ranks that do not run the audio front end WHILE rank 0 runs it (multi-GPU jobs were front-end bound: the peers used to start
    loading / packing / capturing only after the scatter).  With bends the graphs are captured per render (the transforms'
    operands are part of them), so only the warm-up forward is done here."""
    if not hasattr(generator, "capture_graph") or (bends and not getattr(generator, "capturable_bends", True)):
        return 0
    if bends:
        dev = device_of(generator)
        zeros = th.zeros(batch_size, generator.n_latent, generator.style_dim, device=dev)
        generator(styles=zeros, noise=None, truncation=1.0, randomize_noise=False, input_is_latent=True)
        return 0
    return len(graph_lanes(generator, batch_size, lanes))


def _sequence_bends(bends, n_frames=None):
    """The render's bends with every modulated transform instantiated ONCE on the modulation of the whole sequence (the reference
    rebuilds it per batch from the batch's slice, render.py:151-158).  Returns (bends, capturable): capturable when every
    transform implements ``run_static`` (audioreactive/bend.py: picks the frame's parameters on the device) and — ``n_frames``
    given — its per-frame table has one row or one row per frame of the sequence: the captured kernel indexes it with
    frame0 + b unchecked, so anything else (a modulation shorter than the frame range, an un-modulated transform built with
    [batch, k] parameters) keeps the eager per-batch path, which slices and validates like the reference."""
    out, capturable = [], True
    for bend in bends:
        transform = bend["transform"](bend["modulation"]) if "modulation" in bend else bend["transform"]
        if not hasattr(transform, "run_static") or not getattr(transform, "capturable", True):
            return None, False
        rows = getattr(transform, "sequence_rows", None)
        if n_frames is not None and rows is not None and rows not in (1, n_frames):
            return None, False
        out.append({"layer": bend["layer"], "transform": transform})
    return out, capturable


# What a render's inputs decide before its first batch (_plan_render).  random / synth: graph_lanes' arguments of those names, or None;
# trunc_t: the per-frame truncation sequence, None for the exact identity; seq_bends: the bends as the graph lanes capture them
_Plan = collections.namedtuple("_Plan", "dev lo hi latents noise recipes synth truncation trunc_t bends rewrites original_weights random "
                                        "randomize_noise capturable seq_bends")


def _plan_render(generator, latents, noise, truncation, bends, rewrites, randomize_noise, use_graph, frame_range):
    """The part of ``synthesize`` that runs once: inputs made resident on the device, recipes and rewrites checked, and the decision
    between graph lanes and the eager path."""
    dev = device_of(generator)
    n_total = len(latents)
    lo, hi = frame_range if frame_range is not None else (0, n_total)
    latents = latents.to(dev, th.float32).contiguous()  # resident in HBM for the whole render
    # (a NoiseSynth recipe — audioreactive/noise.py — passes through as it is: its tensors are on the device already)
    noise = [nz if nz is None or isinstance(nz, NoiseSynth) else nz.to(dev, th.float32).contiguous() for nz in noise]
    recipes = {i: nz for i, nz in enumerate(noise) if isinstance(nz, NoiseSynth)}
    synth = None
    if recipes:
        offsets = {nz.offset for nz in recipes.values()}
        if len(offsets) != 1:
            raise RuntimeError(f"the NoiseSynth recipes of one render must share a frame offset, got {sorted(offsets)}")
        for i, nz in recipes.items():
            if nz.n_frames is not None and nz.n_frames != n_total:
                raise RuntimeError(f"noise[{i}]: the recipe's envelopes cover {nz.n_frames} frames, the render has {n_total}")
        synth = (tuple(recipes), offsets.pop())
    if isinstance(truncation, (int, float)):
        truncation = float(truncation)
        # a float != 1 (or a generator that carries a truncation latent) must reach the captured graph as well: it becomes a
        # per-frame truncation sequence filled with the constant (reference models/stylegan2.py:537-543 lerps every batch);
        # 1.0 without a truncation latent is the exact identity
        needs_lerp = truncation != 1.0 or getattr(generator, "truncation_latent", None) is not None
        trunc_t = th.full((n_total,), truncation, dtype=th.float32, device=dev) if needs_lerp else None
    else:
        trunc_t = truncation.to(dev, th.float32).contiguous()
    bends = list(bends or [])
    for bend in bends:
        if "modulation" in bend:
            bend["modulation"] = bend["modulation"].to(dev, th.float32).contiguous()
    # model rewriting (reference render.py:127-131,160-167, whose `.copy()` typo makes it unreachable there): per batch
    # the named parameter is replaced by transform(original weight), transform = rewrite(modulation[batch]).
    rewrites = dict(rewrites or {})
    param_dict = dict(generator.named_parameters())
    original_weights = {}
    for name, (rewrite, modulation) in rewrites.items():
        if name not in param_dict:
            raise KeyError(f"get_rewrites: generator has no parameter {name!r}")
        rewrites[name] = [rewrite, modulation.to(dev, th.float32).contiguous()]
        original_weights[name] = param_dict[name].detach().clone()
    # randomize_noise (reference models/stylegan2.py:262-265: fresh N(0,1) maps for the slots whose entry in `noise` is None): the map of
    # (seed, frame, slot) is a pure function (Generator.random_noise), generated inside the captured forward by the graph lanes and by one
    # launch per batch on the eager path, so every frame gets the same maps whichever path, batch size, lane or shard produces it.
    # Generators without `random_noise` (StyleGAN1) keep torch's generator on the eager path.
    random = None
    if randomize_noise and hasattr(generator, "random_noise"):
        slots = tuple(i for i, nz in enumerate(noise) if nz is None)
        seed = getattr(generator, "noise_seed", None)
        if seed is None:  # one draw per render from torch's CPU generator: torch.manual_seed makes a job repeatable
            seed = int(th.randint(0, 2 ** 63 - 1, (1,), dtype=th.int64).item())
        if slots:
            random = (slots, int(seed), int(getattr(generator, "noise_frame_offset", 0)))
    capturable = use_graph and not rewrites and hasattr(generator, "capture_graph") and (not randomize_noise or hasattr(generator, "random_noise"))
    if random is not None and getattr(generator, "noise_seed", None) is None and hi - lo < UNSEEDED_GRAPH_MIN_FRAMES:
        # the seed is an argument of the captured noise launch: a fresh seed per render means capturing the lanes again (~25 ms measured,
        # profiles/randnoise.md), more than the eager path costs such a render (~0.1 ms per batch).  Same maps, same frames either way.
        capturable = False
    seq_bends = []
    if capturable and bends:
        seq_bends, capturable = _sequence_bends(bends, n_total) if getattr(generator, "capturable_bends", True) else (None, False)
    return _Plan(dev, lo, hi, latents, noise, recipes, synth, truncation, trunc_t, bends, rewrites, original_weights, random,
                 randomize_noise, capturable, seq_bends)


def _set_parameter(generator, dotted_name, tensor):
    """``generator.<dotted_name> = Parameter(tensor)``: how a rewrite is applied to the module tree, and how it is taken back."""
    module = generator
    *path, leaf = dotted_name.split(".")
    for attr in path:
        module = getattr(module, attr)
    setattr(module, leaf, th.nn.Parameter(tensor, requires_grad=False))


def _eager_batch(generator, plan, n, m, stream, lane_streams, out, frames="u8"):
    """Frames [n, m) by one eager forward on ``stream`` (the current one): every batch of a render that is not capturable, the ragged tail
    batch of one that is.  ``lane_streams``: the captured lanes' streams, drained first.  Returns the uint8 frames, in ``out`` when it fits;
    ``frames="f32"``: the generator's fp32 image [b, 3, H, W] as it is."""
    b = m - n
    noise_batch = [None if nz is None or isinstance(nz, NoiseSynth) else (nz if nz.shape[0] == 1 else nz[n:m]) for nz in plan.noise]  # [1, ...] = one map for every frame
    for i, recipe in plan.recipes.items():  # the launch a graph lane makes for these frames, without a frame source
        noise_batch[i] = recipe.frames(n, b, i)
    if plan.random is not None:  # the same maps a graph lane generates for these frames
        slots, seed, offset = plan.random
        for i, nz in zip(slots, generator.random_noise(offset + n, b, seed, slots)):
            noise_batch[i] = nz
    bend_batch = []
    for bend in plan.bends:
        transform = bend["transform"](bend["modulation"][n:m]) if "modulation" in bend else bend["transform"]
        bend_batch.append({"layer": bend["layer"], "transform": transform})
    for name, (rewrite, modulation) in plan.rewrites.items():
        new_weight = rewrite(modulation[n:m])(plan.original_weights[name]).to(plan.dev, th.float32).contiguous()
        _set_parameter(generator, name, new_weight)
    for other in lane_streams:  # the eager tail batch shares lane 0's activations: let every lane drain first
        stream.wait_stream(other)
    images, _ = generator(styles=plan.latents[n:m], noise=noise_batch,
                          truncation=plan.truncation if plan.trunc_t is None else plan.trunc_t[n:m],
                          transform_dict_list=bend_batch, randomize_noise=plan.randomize_noise, input_is_latent=True)
    if frames == "f32":
        return images
    if out is None or out.shape[0] != b or out.shape[1:3] != images.shape[2:]:
        out = th.empty((b, images.shape[2], images.shape[3], 3), dtype=th.uint8, device=plan.dev)
    return frames_to_uint8(images, out)


def synthesize(generator, latents, noise, batch_size, truncation=1.0, bends=(), rewrites=None, randomize_noise=False,
               use_graph=True, frame_range=None, lanes=3, frames="u8"):
    """Generator -> uint8 frames for ``frame_range`` (default: all) of the sequence.  Yields (first_frame_index,
    uint8 device tensor [b, H, W, 3]) per batch, in order, with the producing stream current; the tensor stays valid
    until ``lanes`` further batches have been requested.  ``frames="f32"``: the fp32 image [b, 3, H, W] (values nominally in [-1, 1], not
    clamped) instead of the quantised frames — what the deep pipe formats are made from (frames_to_deep).

    hipGraph path: ``lanes`` graphs of ``batch_size`` frames (same weights, private activations) are replayed round-robin
    on their own streams, so consecutive batches overlap on the device — the small, latency-bound 4^2..32^2 layers and
    the last partial wave of every big launch of one batch run underneath the other batch's MFMA-bound layers.  The
    sequences (latents, noise maps, truncation, bend modulations) stay resident in HBM; a replay moves one frame index."""
    if frames not in ("u8", "f32"):
        raise ValueError(f"unknown frame kind {frames!r} (u8 | f32)")
    plan = _plan_render(generator, latents, noise, truncation, bends, rewrites, randomize_noise, use_graph, frame_range)
    caller_stream = th.cuda.current_stream(plan.dev)
    full_batches = (plan.hi - plan.lo) // batch_size
    if plan.capturable and full_batches >= 1:
        lane_state = graph_lanes(generator, batch_size, min(max(1, int(lanes)), full_batches), plan.seq_bends, plan.random, plan.synth, frames)
        for stream, lane in lane_state:
            lane.bind(plan.latents, plan.noise, plan.trunc_t)  # once per render: the pointers of the HBM-resident sequences
            stream.wait_stream(caller_stream)
    else:  # the eager path has lane 0's stream to itself
        lane_state = [(_lane_stream(plan.dev, 0), None)]
        lane_state[0][0].wait_stream(caller_stream)
    captured_streams = [stream for stream, lane in lane_state if lane is not None]
    eager_u8 = None
    try:
        for k, n in enumerate(range(plan.lo, plan.hi, batch_size)):
            m = min(n + batch_size, plan.hi)
            stream, lane = lane_state[k % len(lane_state)]
            with th.cuda.stream(stream):
                if lane is not None and m - n == batch_size:
                    lane.replay(n)
                    # (u8: the frame epilogue is part of the captured forward, fused into the last ToRGB)
                    yield n, lane.u8 if frames == "u8" else lane.image
                elif frames == "u8":
                    eager_u8 = _eager_batch(generator, plan, n, m, stream, captured_streams, eager_u8)
                    yield n, eager_u8
                else:
                    yield n, _eager_batch(generator, plan, n, m, stream, captured_streams, None, frames)
    finally:  # also when the consumer stops early (sink error, generator closed)
        for name, weight in plan.original_weights.items():  # leave the generator as it was found
            _set_parameter(generator, name, weight)
        for stream, lane in lane_state:
            caller_stream.wait_stream(stream)
            if lane is not None:
                lane.release()  # cached lanes outlive the render: they must not keep its sequences alive (or replay into them)


def render(generator, latents, noise, offset, duration, batch_size, out_size, output_file, audio_file=None,
           truncation=1.0, bends=[], rewrites={}, randomize_noise=False, ffmpeg_preset="slow"):
    """Drop-in for reference render.render (render.py:14-29).  With torch.distributed initialised (one process per
    GPU) every rank renders a contiguous shard of the frames and streams them, batch by batch, to rank 0's ordered sink
    (sharding.FrameStream).  The reference's parameter list has no room for the options of the tail: the pipe format, a temporal fold
    and a delivery size come from the environment (render_shard)."""
    return render_frames(generator, latents, noise, offset, duration, batch_size, out_size, output_file, audio_file, truncation, bends,
                         rewrites, randomize_noise, ffmpeg_preset, None, None, None, fold=_fold_from_env(), resize=_resize_from_env(),
                         grade=None, lens=None, feedback=None)


def _drain_quietly(worker):
    """``worker.close()`` while a render unwinds: whatever was submitted is written or dropped before the buffers it reads are let go."""
    with contextlib.suppress(BaseException):  # (a second failure while unwinding must not mask the first)
        worker.close()


class _LocalRing:
    """Single-GPU delivery.  Pinned staging ring: the D2H of batch k overlaps the replays of the next batches; the sink thread writes a
    slot and hands it back through ``free`` (the launch thread blocks in ``push`` only when the sink is _RING_SLOTS batches behind).  Holds the
    device's ring lock from construction to ``close``."""

    def __init__(self, dev, batch_size, worker):
        self.dev, self.batch_size, self.worker = dev, batch_size, worker
        self.copy_stream = th.cuda.Stream(dev)
        index = dev.index if dev.index is not None else th.cuda.current_device()  # torch.device("cuda") carries no index
        self.lock = _RING_LOCKS.setdefault(index, threading.Lock())
        self.lock.acquire()  # the rings are per device, not per render: a second render on this device (another thread) waits
        self.pinned = _PINNED_RING.setdefault(index, [None] * _RING_SLOTS)  # kept across renders: pinning 6 x 25 MB is ~40 ms
        self.staged = _DEVICE_RING.setdefault(index, [None] * _RING_SLOTS)
        self.free = queue.Queue()
        for i in range(_RING_SLOTS):
            self.free.put(i)

    def push(self, u8):
        slot = self.free.get()
        count = u8.shape[0]
        # slots hold a FULL batch; the tail batch of a render uses a prefix (re-pinning per shape cost 2 x 6.5 ms per render)
        if self.pinned[slot] is None or self.pinned[slot].shape[1:] != u8.shape[1:] or self.pinned[slot].shape[0] < max(count, self.batch_size):
            shape = (max(count, self.batch_size),) + tuple(u8.shape[1:])
            self.pinned[slot] = th.empty(shape, dtype=th.uint8).pin_memory()
            self.staged[slot] = th.empty(shape, dtype=th.uint8, device=self.dev)
        host, held = self.pinned[slot][:count], self.staged[slot][:count]
        # the lane's frame buffer is overwritten by its next replay: the batch moves to a device-side slot on the lane's own
        # stream (25 MB inside HBM: ~20 us) and crosses PCIe from there, so that no lane ever waits for a host copy
        # (waiting for it — 0.5 ms per batch on the lane — cost the render loop the whole gain of the three lanes)
        held.copy_(u8, non_blocking=True)
        produced = th.cuda.current_stream(self.dev).record_event()
        with th.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(produced)
            host.copy_(held, non_blocking=True)
            copied = self.copy_stream.record_event()
        self.worker.submit(copied.synchronize, host.numpy(), count, lambda s=slot: self.free.put(s))

    def finish(self, frame_shape):
        pass  # (the caller's worker.close() waits for the slots in flight)

    def close(self):
        if self.lock is not None:
            # the lock goes back only once the worker has drained: a ring slot must not reach the next render while the sink thread reads it
            _drain_quietly(self.worker)
            self.lock.release()
            self.lock = None


class _HostStore:
    """Transport "host": every rank copies its rounds to a pinned shared-memory segment over its own PCIe link; rank 0's sink thread
    reads the segments in global order (sharding.HostFrameStore) — no xGMI traffic, no funnel through rank 0's link."""

    def __init__(self, n_frames, batch_size, dev, rank, worker):
        self.n_frames, self.batch_size, self.dev, self.rank, self.worker = n_frames, batch_size, dev, rank, worker
        self.token = sharding.broadcast_object(f"{os.getpid():x}{int.from_bytes(os.urandom(4), 'little'):08x}" if rank == 0 else None)
        self.store = self.reader = None
        self.stop_reader = threading.Event()  # set when this rank's launch loop fails: the reader must not outlive the store
        self.pushed = 0

    def _opened(self, frame_shape):
        if self.store is None:
            self.store = sharding.HostFrameStore(self.n_frames, self.batch_size, tuple(frame_shape), self.dev, self.token)
            if self.rank == 0:
                self.reader = threading.Thread(target=self._read, args=(self.store,), name="maua-host-gather", daemon=True)
                self.reader.start()
        return self.store

    def _read(self, store):
        # (worker.feed, not submit: a sink error must stay on the worker for the LAUNCH thread — popped here it would end
        # this thread, clear itself, and the render would return a truncated video without an exception)
        for _, count, host in store.rounds_in_order(stop=self.stop_reader.is_set):
            if not self.worker.feed(None, host.numpy(), count, None):
                return

    def push(self, u8):
        self._opened(u8.shape[1:]).push(self.pushed, u8)
        self.pushed += 1

    def finish(self, frame_shape):
        self._opened(frame_shape).finish()
        if self.reader is not None:
            self.reader.join()
            self.worker.close()  # re-raises a sink error on the launch thread

    def close(self):
        if self.reader is not None and self.reader.is_alive():  # the launch loop failed: stop the reader BEFORE its segments go away
            self.stop_reader.set()
            self.reader.join()
        if self.store is not None:
            self.store.close()
            self.store = None


class _GatherStream:
    """Transport "gather" (sharding.FrameStream): one asynchronous gather per batch-round, issued as soon as the round's frames exist:
    the transfer of round k runs under the compute of rounds k+1.., rank 0 hands rounds to its sink thread as they land (its own block
    first — the blocks are contiguous — while the peers' frames accumulate in its HBM store)."""

    def __init__(self, n_frames, batch_size, dev, rank, worker):
        self.n_frames, self.batch_size, self.dev, self.rank, self.worker = n_frames, batch_size, dev, rank, worker
        self.stream = None
        self.pushed = 0

    def _opened(self, frame_shape):  # the frame shape is whatever the generator (and its layer-0 bends) produce
        if self.stream is None:
            self.stream = sharding.FrameStream(self.n_frames, self.batch_size, tuple(frame_shape), self.dev)
        return self.stream

    def _deliver(self, block):
        for _, count, host, release in self.stream.drain_rounds(block=block):
            self.worker.submit(None, host.numpy(), count, release)

    def push(self, u8):
        self._opened(u8.shape[1:]).push(self.pushed, u8)
        self.pushed += 1
        if self.rank == 0:
            self._deliver(False)

    def finish(self, frame_shape):
        self._opened(frame_shape).finish()  # a rank whose block is empty (more ranks than frames) still takes part in every round
        if self.rank == 0:
            self._deliver(True)
        else:
            self.stream.wait_all()

    def close(self):
        self.stream = None


FEEDBACK_ONE_RANK = ("a frame feedback is a recurrence over the frames: a shard's first frame needs the state its predecessor leaves behind, "
                     "which only a render that starts at frame 0 on its own has ({where}).  Render a feedback on one rank (one process, one GPU)")


def fold_shard_bounds(n_frames, subframes, rank, world):
    """[lo, hi) of a rank's block in RENDERED frames when every delivered frame is folded from ``subframes`` of them: the job is sharded in
    units of delivered frames (sharding.shard_bounds of n_frames / N), so that no group straddles two ranks."""
    lo, hi = sharding.shard_bounds(n_frames // subframes, rank, world)
    return subframes * lo, subframes * hi


def _generated_hw(generator, out_size):
    """(H, W) of the frames the generator produces for ``out_size``: 1920 / 1080 render 2048-px-wide / -high frames."""
    side = int(getattr(generator, "size", 0)) or _output_dims(out_size)[0]
    return (side, 2 * side) if out_size == 1920 else (2 * side, side) if out_size == 1080 else (side, side)


def _stream_frame_shape(generator, out_size, pix_fmt="rgb24", resize=None):
    """The shape of one frame as it travels from the device to the sink: [H, W, 3] of the generated frame (_generated_hw; 2048-px frames
    are cropped and resized to 1920x1080 / 1080x1920 on the device first, crop_resize_for_delivery) or, with ``resize`` (FrameResize), of
    its size whatever the generator's; [H * W * 3 // 2] for the planar ``pix_fmt`` "yuv420p", [mjpeg_slot_bytes] for "mjpeg",
    [deep_frame_bytes] for the deep formats."""
    if resize is not None:
        w, h = resize.size
    else:
        h, w = _generated_hw(generator, out_size)
        box = _wide_output_box(out_size, h, w)
        if box is not None:
            w, h = box[4:]
    if pix_fmt == "mjpeg":
        return (mjpeg_slot_bytes(w, h),)
    if pix_fmt in DEEP_PIX_FMTS:
        return (deep_frame_bytes(pix_fmt, w, h),)
    return (h * w * 3 // 2,) if pix_fmt == "yuv420p" else (h, w, 3)


class _FrameTail:
    """What happens to a batch between the generator and the delivery, decided once per render.  Constructed from the options alone —
    every refusal that needs no device, the sink's size, the frame kind the lanes are asked for —, then ``load``-ed with the render's frame
    count and position — the refusals and the operands of grade, lens and feedback on the device —, both before the sink is opened.
    ``tail(first, batch)`` then runs the stages on the current (= producing) stream and returns the batch as it leaves the device:

        feedback_frames -> lens_frames -> grade_frames, or the plain quantiser behind a feedback or lens without a grade
        8-bit formats: _deliverable (fold_frames -> crop or resize_frames -> frames_to_yuv420p / frames_to_mjpeg)
        deep formats:  frames_to_deep (the grade has worked in place on the fp32 image)

    A stage is launched only for an option that is set (and, inside the stage, only for a lens or feedback that is not the identity).
    ``scratch`` holds the stages' reusable buffers (_cached)."""

    def __init__(self, generator, out_size, pipe_pix_fmt, batch_size, fold, resize, grade, lens, feedback):
        self.width, self.height = _output_dims(out_size)
        if resize is not None:
            check_deliver_size(resize, _pipe_pix_fmt(pipe_pix_fmt))
            self.width, self.height = resize.size  # what the sink, the stream's frame shape and the transports see
        self.subframes = subframes = _subframes(fold)
        if batch_size % subframes:
            raise ValueError(f"--batch {batch_size} is not a multiple of --subframes {subframes}: a batch must hold whole groups of sub-frames "
                             f"(e.g. --batch {subframes * max(1, round(batch_size / subframes))})")
        self.pix_fmt = _pipe_pix_fmt(pipe_pix_fmt)
        self.quality = _mjpeg_quality(pipe_pix_fmt) if self.pix_fmt == "mjpeg" else None
        self.deep = self.pix_fmt in DEEP_PIX_FMTS
        if self.deep and subframes > 1:
            raise ValueError(f"--pipe_pix_fmt {self.pix_fmt} cannot be combined with --subframes {subframes}: the temporal fold is 8-bit only "
                             f"(it averages the uint8 frames); render at --subframes 1 or with an 8-bit pipe format")
        if self.deep and (self.width % 2 or self.height % 2):
            raise ValueError(f"{self.pix_fmt} needs even dimensions, got {self.width}x{self.height}")
        self.generator, self.out_size, self.batch_size = generator, out_size, batch_size
        self.fold, self.resize, self.grade, self.lens, self.feedback = fold, resize, grade, lens, feedback
        # the deep formats, the grade, the lens and the feedback work on the fp32 image: the lanes then run without their quantiser
        self.frames = "f32" if self.deep or grade is not None or lens is not None or feedback is not None else "u8"
        self.grade_ops = self.lens_ops = self.feedback_ops = None
        self.scratch = {}

    def load(self, n_rendered, first_frame, world):
        """The per-frame tables of ``n_rendered`` frames on the generator's device (``dev``), for a render that starts at ``first_frame``
        of a ``world``-rank job."""
        if self.feedback is not None and (world > 1 or first_frame > 0):
            raise ValueError(FEEDBACK_ONE_RANK.format(where=f"this shard starts at frame {first_frame} of a {world}-rank job"))
        self.dev = dev = device_of(self.generator)
        if self.grade is not None:
            self.grade_ops = GradeOperands(self.grade, n_rendered, self.batch_size, dev)
        if self.lens is not None:
            self.lens_ops = LensOperands(self.lens, n_rendered, self.batch_size, dev)
            self.lens_ops.sized(*_generated_hw(self.generator, self.out_size))  # (a bloom too wide for this frame height is refused here)
        if self.feedback is not None:
            self.feedback_ops = FeedbackOperands(self.feedback, n_rendered, self.batch_size, dev)
            if not self.feedback.is_identity:
                self.feedback_ops.sized(*_generated_hw(self.generator, self.out_size))
                self.feedback_ops.allocate(*_generated_hw(self.generator, self.out_size))  # (on this stream, before the lanes start)

    @property
    def frame_shape(self):
        return _stream_frame_shape(self.generator, self.out_size, self.pix_fmt, self.resize)

    def __call__(self, first, images):
        count, scratch = images.shape[0], self.scratch
        if self.feedback_ops is not None:  # (first of all: the state is the un-lensed image, the trail is glowed and graded with its picture)
            images = feedback_frames(images.contiguous(), self.feedback_ops, first, count, scratch)
        if self.lens_ops is not None:  # (in front of the grade: the glow is graded with the picture it belongs to)
            images = lens_frames(images.contiguous(), self.lens_ops, first, count, scratch)
        if self.grade_ops is not None:
            rows = self.grade_ops.window(self.grade_ops.rows, first, count)
            images = grade_frames(images.contiguous(), rows, self.grade_ops.lut, scratch, out="f32" if self.deep else "u8")
        elif self.frames == "f32" and not self.deep:  # (the quantiser every 8-bit render ends its forward with)
            _, _, h, w = images.shape
            images = frames_to_uint8(images, out=_scratch(scratch, ("lens-u8", images.data_ptr(), count, h, w), (count, h, w, 3), th.uint8, images.device))
        if self.deep:
            return frames_to_deep(images, self.out_size, self.pix_fmt, scratch, resize=self.resize)
        # (2048-px frames leave the device as 1920x1080 already)
        return _deliverable(images, self.out_size, self.pix_fmt, scratch, self.quality, self.fold, resize=self.resize)


def render_frames(generator, latents, noise, offset, duration, batch_size, out_size, output_file, audio_file, truncation,
                  bends, rewrites, randomize_noise, ffmpeg_preset, _shard, transport=None, pipe_pix_fmt=None, *, fold=None, resize=None,
                  grade=None, lens=None, feedback=None):
    """The body of every entry point below, and what generate() calls.  The reference's parameters, then ``_shard = (lo, hi, n_frames)``
    — set by generate() after sharding.scatter_frames: ``latents`` / ``noise`` / ``truncation`` / bend modulations already hold only this
    rank's block of the frames —, ``transport`` ("gather" | "host"; default $MAUA_FRAME_TRANSPORT, else gather) and ``pipe_pix_fmt``
    (PIPE_PIX_FMTS, "mjpeg:<quality>" or DEEP_PIX_FMTS; default $MAUA_PIPE_PIX_FMT, else rgb24 — what crosses to the host, to rank 0 and
    into the sink), then the options of the tail (_FrameTail; the environment is read for none of them):

      fold      TemporalFold: ``latents`` and every per-frame input hold ``fold.subframes`` rows per delivered frame, each batch is folded
                N:1 on the device, the sink runs at delivered frames / duration and the return value counts delivered frames.
                ``batch_size`` and the frame count (of the job and of every rank's block: ``_shard`` stays in rendered frames) must be
                multiples of N.  8-bit formats only
      resize    FrameResize: every delivered frame is resampled on the rank that rendered it — after the fold, before the colour
                conversion / the JPEG encoder; at 16 bits on the deep formats —, and the sink, the stream's frame shape and both
                multi-rank transports see that size.  The built-in 112-px crop of the 1920 / 1080 outputs is skipped: the source is the
                whole generated frame (2048 x 1024 for out_size 1920)
      grade     ar.Grade: every rendered frame is graded by its row of the grade's table — per sub-frame and before the fold —, then the
                8-bit formats go on as maua_grade_to_u8's frames, the deep formats as the image graded in place
      lens      ar.Lens: every rendered frame — the whole generated frame — passes through lens_frames in front of the grade
      feedback  ar.Feedback: every rendered frame passes through feedback_frames in front of the lens (the state is the un-lensed image,
                so a bloom is not fed back into itself).  One rank only: a job of more than one rank, or a ``_shard`` that does not start
                at frame 0, is refused before the sink is opened

    The tables of grade, lens and feedback hold one row, or one row per entry of ``latents`` (with ``_shard``: this rank's block);
    anything else is refused before the first batch."""
    tail = _FrameTail(generator, out_size, pipe_pix_fmt, batch_size, fold, resize, grade, lens, feedback)
    subframes = tail.subframes
    rank, world = sharding.rank_world()
    # multi-GPU frame transport: "gather" (default: RCCL gather of every round into rank 0's HBM) or "host" (per-rank D2H into shared memory)
    transport = transport or os.environ.get("MAUA_FRAME_TRANSPORT", "gather")
    if transport not in ("gather", "host"):
        raise ValueError(f"unknown frame transport {transport!r} (gather | host)")
    if _shard is None:
        n_frames = len(latents)
        lo, hi = fold_shard_bounds(n_frames, subframes, rank, world)  # (no process group: rank 0 of 1, every frame)
        frame_range = (lo, hi)
    else:
        lo, hi, n_frames = _shard
        frame_range = (0, hi - lo)
    if n_frames % subframes or lo % subframes or hi % subframes:
        raise ValueError(f"{n_frames} rendered frames (this rank's: {lo} .. {hi}) are not whole groups of {subframes} sub-frames")
    # what the sink and the transports count: delivered frames — n_frames and batch_size themselves without a fold
    n_out, batch_out = n_frames // subframes, batch_size // subframes
    tail.load(len(latents), lo, world)  # (refusals included: before the sink is opened, no file is created)
    sink = worker = None
    with contextlib.ExitStack() as unwind:  # (callbacks run last in, first out)
        if rank == 0:
            sink = FrameSink(output_file, tail.width, tail.height, n_out / duration, audio_file, offset, duration, ffmpeg_preset,
                             pix_fmt=tail.pix_fmt, quality=tail.quality)
            unwind.callback(sink.close)  # the encoder process / output file must not outlive a failed render: closed last, and always
            worker = SinkWorker(sink)
            unwind.callback(_drain_quietly, worker)
        if _shard is not None and hasattr(generator, "random_noise"):
            # the sequences of a scattered shard start at the job's frame `lo`: seeded noise is a function of the absolute frame
            generator.noise_frame_offset = lo
            unwind.callback(setattr, generator, "noise_frame_offset", 0)
        # The frame loop runs on the Python thread that launches every graph replay.  A generation-2 collection walks the ~170 k long-lived
        # objects of a process that has torch imported: 45-90 ms, i.e. 8-15 batches during which no replay is launched (measured: tools/gather_probe.py,
        # and as a 9 % hole in a 150-batch gathered bench region).  Park everything that is alive now in the permanent generation for the
        # duration of the loop: what the loop allocates is then all the collector ever walks.  (No full gc.collect() here: it would cost the same
        # 45-90 ms up front, as much as it saves on a 900-frame job; generate() has just run one, as the reference does.)
        with parked_heap():
            if not sharding.grouped():
                delivery = _LocalRing(tail.dev, batch_out, worker)
            else:
                delivery = (_HostStore if transport == "host" else _GatherStream)(n_out, batch_out, tail.dev, rank, worker)
            with contextlib.closing(delivery):
                # (lanes: synthesize's default, 3, on every path.  The frame kind is named only where it is not the default: the rank
                # tests stand in for synthesize with CPU functions of its original parameter list)
                kind = {} if tail.frames == "u8" else {"frames": tail.frames}
                for first, batch in synthesize(generator, latents, noise, batch_size, truncation, bends, rewrites, randomize_noise,
                                               frame_range=frame_range, **kind):
                    delivery.push(tail(first, batch))
                delivery.finish(tail.frame_shape)
                if worker is not None:
                    worker.close()  # every frame is written; re-raises a sink error on the launch thread
    return sink.count if sink is not None else 0


def render_shard(generator, latents, noise, offset, duration, batch_size, out_size, output_file, audio_file, truncation,
                 bends, rewrites, randomize_noise, ffmpeg_preset, _shard, transport=None, pipe_pix_fmt=None):
    """``render`` with ``_shard``, ``transport`` and ``pipe_pix_fmt`` (render_frames).  Like ``render`` it has no parameter for a temporal
    fold or a delivery size and takes them from the environment: $MAUA_SUBFRAMES, $MAUA_SHUTTER and $MAUA_SHUTTER_LIGHT (_fold_from_env;
    unset: none), $MAUA_DELIVER_SIZE, $MAUA_DELIVER_FILTER and $MAUA_DELIVER_FIT (_resize_from_env; unset: none)."""
    return render_frames(generator, latents, noise, offset, duration, batch_size, out_size, output_file, audio_file, truncation, bends,
                         rewrites, randomize_noise, ffmpeg_preset, _shard, transport, pipe_pix_fmt, fold=_fold_from_env(),
                         resize=_resize_from_env(), grade=None, lens=None, feedback=None)


def render_folded(generator, latents, noise, offset, duration, batch_size, out_size, output_file, audio_file, truncation,
                  bends, rewrites, randomize_noise, ffmpeg_preset, _shard, transport=None, pipe_pix_fmt=None, fold=None):
    """render_frames with an explicit ``fold`` (TemporalFold or None; the environment is not read for it) and the delivery size of the
    environment ($MAUA_DELIVER_SIZE, as render_shard)."""
    return render_frames(generator, latents, noise, offset, duration, batch_size, out_size, output_file, audio_file, truncation, bends,
                         rewrites, randomize_noise, ffmpeg_preset, _shard, transport, pipe_pix_fmt, fold=fold, resize=_resize_from_env(),
                         grade=None, lens=None, feedback=None)


def render_delivered(generator, latents, noise, offset, duration, batch_size, out_size, output_file, audio_file, truncation,
                     bends, rewrites, randomize_noise, ffmpeg_preset, _shard, transport=None, pipe_pix_fmt=None, fold=None, resize=None):
    """render_frames with ``fold`` and ``resize`` (FrameResize or None); the environment is read for neither, here and below."""
    return render_frames(generator, latents, noise, offset, duration, batch_size, out_size, output_file, audio_file, truncation, bends,
                         rewrites, randomize_noise, ffmpeg_preset, _shard, transport, pipe_pix_fmt, fold=fold, resize=resize, grade=None,
                         lens=None, feedback=None)


def render_graded(generator, latents, noise, offset, duration, batch_size, out_size, output_file, audio_file, truncation,
                  bends, rewrites, randomize_noise, ffmpeg_preset, _shard, transport=None, pipe_pix_fmt=None, fold=None, resize=None, grade=None):
    """render_frames with ``fold``, ``resize`` and a colour ``grade`` (audioreactive/grade.py's Grade, or None)."""
    return render_frames(generator, latents, noise, offset, duration, batch_size, out_size, output_file, audio_file, truncation, bends,
                         rewrites, randomize_noise, ffmpeg_preset, _shard, transport, pipe_pix_fmt, fold=fold, resize=resize, grade=grade,
                         lens=None, feedback=None)


def render_lensed(generator, latents, noise, offset, duration, batch_size, out_size, output_file, audio_file, truncation,
                  bends, rewrites, randomize_noise, ffmpeg_preset, _shard, transport=None, pipe_pix_fmt=None, fold=None, resize=None, grade=None,
                  lens=None):
    """render_frames with ``fold``, ``resize``, ``grade`` and a ``lens`` (audioreactive/lens.py's Lens, or None)."""
    return render_frames(generator, latents, noise, offset, duration, batch_size, out_size, output_file, audio_file, truncation, bends,
                         rewrites, randomize_noise, ffmpeg_preset, _shard, transport, pipe_pix_fmt, fold=fold, resize=resize, grade=grade,
                         lens=lens, feedback=None)


def render_fed(generator, latents, noise, offset, duration, batch_size, out_size, output_file, audio_file, truncation,
               bends, rewrites, randomize_noise, ffmpeg_preset, _shard, transport=None, pipe_pix_fmt=None, fold=None, resize=None, grade=None,
               lens=None, feedback=None):
    """render_frames with every option as an ordinary parameter: ``fold``, ``resize``, ``grade``, ``lens`` and a ``feedback``
    (audioreactive/feedback.py's Feedback, or None)."""
    return render_frames(generator, latents, noise, offset, duration, batch_size, out_size, output_file, audio_file, truncation, bends,
                         rewrites, randomize_noise, ffmpeg_preset, _shard, transport, pipe_pix_fmt, fold=fold, resize=resize, grade=grade,
                         lens=lens, feedback=feedback)

