"""GPU: the Motion-JPEG pipe format — maua_jpeg_encode_u8 (csrc/jpeg.hip) byte for byte against the integer restatement of
tests/jpeg_ref.py (slot header, stream, and the untouched slot behind the stream), its bounds, overflow, alignment and capture, and the
opt-in pipe format through render() on one rank, two played ranks and the host transport against the rgb24 delivery of the same job."""
import io
import os
import struct

import numpy as np
import PIL.Image
import pytest
import torch

import jpeg_ref
from maua_stylegan2_amd import seeding
from played_world import PlayedWorld
from redzone import CANARY_BITS, Guard

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

CANARY = np.frombuffer(struct.pack("<I", CANARY_BITS), np.uint8)


def _row(w):
    return (w + 15) // 16  # the render path's restart interval: one MCU row


def _encode(gpu, frames, quality, restart, slot_bytes=None):
    """maua_jpeg_encode_u8 on guarded windows (tests/redzone.py): returns the slots [b, slot_bytes] as numpy, canary where nothing was written.
    Asserts that nothing was written outside out / ws / header / rgb and that the frames and the header are unchanged."""
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    frames = np.ascontiguousarray(frames)
    b, h, w, _ = frames.shape
    slot_bytes = slot_bytes or 2048 + h * w * 3
    head = np.frombuffer(jpeg_ref.header(h, w, quality, restart), np.uint8).copy()
    guard = Guard(gpu)
    rgb = guard.inp(frames.reshape(-1), "rgb", torch.uint8)
    header = guard.inp(head, "header", torch.uint8)
    out = guard.out((b * slot_bytes,), "out", torch.uint8)
    ws_bytes = lib.maua_jpeg_ws_bytes(b, h, w, restart)
    ws = guard.out((ws_bytes,), "ws", torch.uint8)
    rc = lib.maua_jpeg_encode_u8(rgb.data_ptr(), b, h, w, quality, restart, header.data_ptr(), head.size, out.data_ptr(), slot_bytes,
                                 ws.data_ptr(), _lib.stream_ptr(gpu))
    assert rc == 0, rc
    guard.check()
    assert np.array_equal(rgb.cpu().numpy(), frames.reshape(-1)) and np.array_equal(header.cpu().numpy(), head)
    return out.cpu().numpy().reshape(b, slot_bytes)


def _assert_slots(slots, frames, quality, restart, base=0):
    """Every slot: header (length, status 0, zeros), the reference's stream, canary behind it.  ``base``: byte offset of the slots' first
    byte inside its guarded window (the canary pattern repeats every 4 bytes)."""
    b, slot_bytes = slots.shape
    for i in range(b):
        want = jpeg_ref.encode(frames[i], quality, restart)
        n = len(want)
        assert 16 + n <= slot_bytes
        assert bytes(slots[i, :16]) == struct.pack("<IIQ", n, 0, 0), (i, bytes(slots[i, :16]))
        got = bytes(slots[i, 16: 16 + n])
        if got != want:
            first = next(k for k in range(n) if got[k] != want[k])
            raise AssertionError(f"frame {i}: stream differs from the reference at byte {first} of {n}")
        tail = np.arange(base + i * slot_bytes + 16 + n, base + (i + 1) * slot_bytes)
        assert np.array_equal(slots[i, 16 + n:], CANARY[tail % 4]), f"frame {i}: bytes behind the stream were written"
    return True


@pytest.mark.parametrize("h,w", jpeg_ref.SIZES[:4] + [(48, 64), (21, 37)], ids=lambda v: str(v))
def test_streams_equal_the_reference_byte_for_byte(gpu, h, w):
    """The five pictures at every quality, as one batch of 3 and two batches of 1; (21, 37): odd sizes, rows off the dword grid."""
    pics = jpeg_ref.inputs(h, w)
    three = np.stack([pics["smooth"], pics["noise"], pics["checker"]])
    for q in (1, 50, 90, 95):
        _assert_slots(_encode(gpu, three, q, _row(w)), three, q, _row(w))
        for name in ("flat0", "flat255"):
            _assert_slots(_encode(gpu, pics[name][None], q, _row(w)), pics[name][None], q, _row(w))


@pytest.mark.parametrize("restart", [1, 4, 5, 65535])
def test_restart_intervals_at_48x64(gpu, restart):
    """12 MCUs in 3 rows of 4: an interval per MCU, per row, spanning rows without dividing the count, and one interval for everything."""
    pics = jpeg_ref.inputs(48, 64)
    frames = np.stack([pics["noise"], pics["smooth"], pics["checker"]])
    for q in (50, 95):
        _assert_slots(_encode(gpu, frames, q, restart), frames, q, restart)
    _assert_slots(_encode(gpu, frames[:1], 90, restart), frames[:1], 90, restart)


@pytest.mark.parametrize("restart", [16, 100, 65535])
def test_noise_at_quality_95_fills_long_intervals(gpu, restart):
    """256 x 256 noise at quality 95: long codes, heavy stuffing.  An interval of 16 MCUs is 96 blocks (one pass of the entropy kernel), of
    100 MCUs 600 blocks (three passes, the last interval shorter), 65535 -> all 1536 blocks in one workgroup (six passes with carried bits)."""
    frame = jpeg_ref.inputs(256, 256)["noise"][None]
    _assert_slots(_encode(gpu, frame, 95, restart), frame, 95, restart)


def test_more_intervals_than_one_pass_of_the_pack_kernel(gpu):
    """264 x 280: 17 x 18 MCUs, partial on both axes, the last group of an MCU row 2 MCUs wide; an interval per MCU = 306 intervals, more
    than the 256 the pack kernel scans at a time."""
    frame = jpeg_ref.inputs(264, 280)["smooth"][None]
    _assert_slots(_encode(gpu, frame, 50, 1), frame, 50, 1)


def test_overflow_is_reported_per_frame_and_stays_inside_the_slot(gpu):
    pics = jpeg_ref.inputs(56, 120)
    frames = np.stack([pics["flat0"], pics["noise"], pics["flat255"]])
    restart = _row(120)
    lengths = [len(jpeg_ref.encode(f, 90, restart)) for f in frames]
    slot_bytes = 16 + max(lengths[0], lengths[2]) + 64
    assert 16 + lengths[1] > slot_bytes >= 16 + 629 + 2
    slots = _encode(gpu, frames, 90, restart, slot_bytes=slot_bytes)  # (the red zones behind `out` stayed intact: _encode)
    _assert_slots(slots[[0]], frames[[0]], 90, restart)
    _assert_slots(slots[[2]], frames[[2]], 90, restart, base=2 * slot_bytes)
    assert bytes(slots[1, :16]) == struct.pack("<IIQ", lengths[1], 1, 0)
    tail = np.arange(slot_bytes + 16, 2 * slot_bytes)
    assert np.array_equal(slots[1, 16:], CANARY[tail % 4])  # nothing but the slot header


def test_unaligned_frames_and_slots_give_the_same_bytes(gpu):
    """rgb and out one byte off the dword grid (w % 4 == 0 would otherwise take the dword loads)."""
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    h, w, q = 24, 40, 90
    pics = jpeg_ref.inputs(h, w)
    frames = np.stack([pics["noise"], pics["smooth"]])
    slot_bytes = 1024 + h * w * 3 // 2 + 1  # (an odd slot size as well)
    head = np.frombuffer(jpeg_ref.header(h, w, q, _row(w)), np.uint8)
    src = torch.zeros(frames.size + 1, dtype=torch.uint8, device=gpu)
    src[1:].copy_(torch.from_numpy(frames.reshape(-1)))
    out = torch.full((2 * slot_bytes + 1 + 7,), 0xA5, dtype=torch.uint8, device=gpu)
    header = torch.from_numpy(head.copy()).to(gpu)
    ws = torch.empty(lib.maua_jpeg_ws_bytes(2, h, w, _row(w)), dtype=torch.uint8, device=gpu)
    assert src.data_ptr() % 4 == 0 and out.data_ptr() % 4 == 0
    rc = lib.maua_jpeg_encode_u8(src.data_ptr() + 1, 2, h, w, q, _row(w), header.data_ptr(), head.size, out.data_ptr() + 1, slot_bytes,
                                 ws.data_ptr(), _lib.stream_ptr(gpu))
    assert rc == 0
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert host[0] == 0xA5 and (host[1 + 2 * slot_bytes:] == 0xA5).all()
    for i in range(2):
        want = jpeg_ref.encode(frames[i], q, _row(w))
        slot = host[1 + i * slot_bytes: 1 + (i + 1) * slot_bytes]
        assert bytes(slot[:16]) == struct.pack("<IIQ", len(want), 0, 0) and bytes(slot[16: 16 + len(want)]) == want
        assert (slot[16 + len(want):] == 0xA5).all()


def _payloads(slots):
    slots = slots.cpu().numpy()
    out = []
    for slot in slots:
        n, status = struct.unpack("<II", bytes(slot[:8]))
        assert status == 0
        out.append(bytes(slot[16: 16 + n]))
    return out


def test_capturable_and_reuses_the_callers_scratch_buffers(gpu):
    """The three launches captured in a torch.cuda.graph and replayed on changed frames; slots, device header and workspace live in the
    caller's scratch dict and the second call allocates nothing."""
    from maua_stylegan2_amd import render

    h, w, q = 48, 64, 90
    inputs = [np.stack([np.roll(jpeg_ref.inputs(h, w)[name], s, axis=1) for name in ("noise", "smooth")]) for s in (0, 5, 9)]
    src = torch.from_numpy(inputs[0]).to(gpu)
    scratch = {}
    first = render.frames_to_mjpeg(src, scratch, q)
    assert first.dtype == torch.uint8 and tuple(first.shape) == (2, render.mjpeg_slot_bytes(w, h)) and len(scratch) == 2
    eager = [_payloads(first)]
    assert eager[0] == [jpeg_ref.encode(f, q, _row(w)) for f in inputs[0]]
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated(gpu)
    again = render.frames_to_mjpeg(src, scratch, q)
    assert again.data_ptr() == first.data_ptr() and len(scratch) == 2 and torch.cuda.memory_allocated(gpu) == allocated
    # another input buffer (another lane: its batch is encoded concurrently) gets slots and a workspace of its own, the header is shared
    other = render.frames_to_mjpeg(src.clone(), scratch, q)
    assert len(scratch) == 3 and other.data_ptr() != first.data_ptr() and _payloads(other) == eager[0]
    assert len({v[1].data_ptr() for k, v in scratch.items() if k[0] == "mjpeg"}) == 2
    del other
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = render.frames_to_mjpeg(src, scratch, q)
    assert out.data_ptr() == first.data_ptr() and len(scratch) == 3
    for frames in inputs[1:]:
        src.copy_(torch.from_numpy(frames).to(gpu))
        out.fill_(0xA5)
        graph.replay()
        torch.cuda.synchronize()
        replayed = _payloads(out)
        assert replayed == _payloads(render.frames_to_mjpeg(src, {}, q)) == [jpeg_ref.encode(f, q, _row(w)) for f in frames]
    empty = render.frames_to_mjpeg(torch.zeros((0, h, w, 3), dtype=torch.uint8, device=gpu), {}, q)
    assert tuple(empty.shape) == (0, render.mjpeg_slot_bytes(w, h))
    with pytest.raises(Exception, match="rejected"):
        render.frames_to_mjpeg(src, {}, 96)


@pytest.mark.parametrize("out_size,shape", [(1920, (1, 1024, 2048, 3)), (1080, (1, 2048, 1024, 3))])
def test_wide_output_is_delivered_as_a_1080p_stream(gpu, out_size, shape):
    """The delivery of a 1920 / 1080 render on a synthetic 2048-px frame (as tests/test_yuv420_gpu.py: the 1024^2 generator is too heavy
    here): crop + resize + encode on the device.  The stream says 1920 x 1080 (1080 x 1920), decodes, and — intervals being independent,
    one per MCU row — its first two intervals and its last (8 rows: a partial MCU row) equal the reference's for those rows of the rgb24
    delivery of the same frame."""
    from maua_stylegan2_amd import render

    frame = torch.from_numpy(np.random.default_rng(out_size).integers(0, 256, shape, dtype=np.uint8)).to(gpu)
    scratch = {}
    slots = render._deliverable(frame, out_size, "mjpeg", scratch, 90)
    rgb = render._deliverable(frame, out_size, "rgb24", scratch).cpu().numpy()[0]
    width, height = render._output_dims(out_size)
    assert rgb.shape == (height, width, 3) and tuple(slots.shape) == (1, render.mjpeg_slot_bytes(width, height))
    assert tuple(slots.shape[1:]) == render._stream_frame_shape(type("G", (), {"size": 1024}), out_size, "mjpeg")
    (stream,) = _payloads(slots)
    im = PIL.Image.open(io.BytesIO(stream))
    im.load()
    assert im.size == (width, height)
    info = jpeg_ref.walk(stream)
    rows = (height + 15) // 16
    assert info["dri"] == _row(width) and len(info["rst"]) == rows - 1
    assert stream[: info["entropy"][0]] == jpeg_ref.header(height, width, 90, _row(width))
    top = jpeg_ref.entropy_data(jpeg_ref.coefficients(rgb[:32], 90), _row(width))
    assert stream[info["entropy"][0]: info["rst"][1][0]] == top
    last = jpeg_ref.entropy_data(jpeg_ref.coefficients(rgb[(rows - 1) * 16:], 90), _row(width))
    assert stream[info["rst"][-1][0] + 2: info["entropy"][1]] == last
    sink = render.FrameSink(None, width, height, 30, pix_fmt="mjpeg")
    sink.write(slots.cpu().numpy()[0])
    assert sink.count == 1


# 5 captured batches + an eager tail batch of 1.  (Two ranks render 6 + 5 frames: with a batch of 2 every frame is rendered in a batch of the
# same size as on one rank — the generator's kernels are chosen per batch size, frames of different batch sizes need not agree to the bit.)
N_FRAMES, BATCH, SIZE, QUALITY = 11, 2, 64, 85


def _render(*args, **kwargs):
    """render_shard at the generator's own frame size, without an ffmpeg binary (as tests/test_yuv420_gpu.py)."""
    from maua_stylegan2_amd import render

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(render, "_output_dims", lambda out_size: (SIZE, SIZE))
        mp.setattr(render.shutil, "which", lambda name: None)
        return render.render_shard(*args, **kwargs)


@pytest.fixture(scope="module")
def job(gpu, tmp_path_factory):
    """The seeded generator, the rgb24 delivery of the job and the reference's stream of every frame (computed once)."""
    from maua_stylegan2_amd import render
    from maua_stylegan2_amd.models.stylegan2 import Generator

    g = Generator(SIZE, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(SIZE, seed=4), strict=True)
    g = g.to(gpu).eval()
    lat = seeding.seeded_latents(N_FRAMES, g.n_latent, seed=6)
    noise = seeding.seeded_noise(N_FRAMES, SIZE, seed=7)
    noise[-1] = None
    tmp = tmp_path_factory.mktemp("mjpeg")
    out = str(tmp / "rgb.mp4")
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("MAUA_PIPE_PIX_FMT", raising=False)
        mp.setattr(render, "_output_dims", lambda out_size: (SIZE, SIZE))
        mp.setattr(render.shutil, "which", lambda name: None)
        assert render.render(g, lat, noise, 0, N_FRAMES / 30, BATCH, SIZE, out) == N_FRAMES
    rgb = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(N_FRAMES, SIZE, SIZE, 3)
    assert rgb.std() > 5
    want = tuple(jpeg_ref.encode(frame, QUALITY, _row(SIZE)) for frame in rgb)
    assert len(set(want)) == N_FRAMES  # (distinct frames: the order is really checked)
    return g, lat, noise, want, tmp


def _assert_avi(path, want):
    info = jpeg_ref.avi_frames(path)
    assert len(info["frames"]) == len(want) and info["avih"]["total_frames"] == len(want)
    assert (info["avih"]["width"], info["avih"]["height"]) == (SIZE, SIZE) and info["strh"]["rate"] == 30 * info["strh"]["scale"]
    for i, (got, ref) in enumerate(zip(info["frames"], want)):
        assert got == ref, f"frame {i} differs from the reference's stream of the rgb24 frame"
        im = PIL.Image.open(io.BytesIO(got))
        im.load()
        assert im.size == (SIZE, SIZE)


def test_render_mjpeg_writes_an_avi_of_the_reference_streams(gpu, job, monkeypatch):
    """Through render() (the format and the quality arrive in $MAUA_PIPE_PIX_FMT) and through render_shard's keyword: same frame count and
    order as the rgb24 render, captured batches and the eager tail batch alike."""
    from maua_stylegan2_amd import render

    g, lat, noise, want, tmp = job
    monkeypatch.setattr(render, "_output_dims", lambda out_size: (SIZE, SIZE))
    monkeypatch.setattr(render.shutil, "which", lambda name: None)
    monkeypatch.setenv("MAUA_PIPE_PIX_FMT", f"mjpeg:{QUALITY}")
    out = str(tmp / "env.mp4")
    assert render.render(g, lat, noise, 0, N_FRAMES / 30, BATCH, SIZE, out) == N_FRAMES
    assert not os.path.exists(out + ".rgb24") and not os.path.exists(out)
    _assert_avi(out + ".avi", want)
    monkeypatch.delenv("MAUA_PIPE_PIX_FMT")
    monkeypatch.setenv("MAUA_MJPEG_QUALITY", str(QUALITY))
    out = str(tmp / "kw.mp4")
    assert _render(g, lat, noise, 0, N_FRAMES / 30, BATCH, SIZE, out, None, 1.0, [], {}, False, "slow", None, pipe_pix_fmt="mjpeg") == N_FRAMES
    _assert_avi(out + ".avi", want)


def test_two_played_ranks_deliver_the_one_rank_file(gpu, job, monkeypatch):
    """Two ranks played one after the other (tests/played_world.py): blocks of 6 + 5 frames travel as flat slots of mjpeg_slot_bytes, the
    file of rank 0 equals the one-rank file.  (Rank 0's recording pass has nothing in its peers' slots yet: whatever the uninitialised
    store holds there may or may not pass for a slot header, so that pass may end in the sink's overflow error.)"""
    from maua_stylegan2_amd import render

    g, lat, noise, want, tmp = job
    monkeypatch.delenv("MAUA_PIPE_PIX_FMT", raising=False)
    world = PlayedWorld(2)

    def play(rank, final):
        out = str(tmp / f"rank{rank}_{int(final)}.mp4")
        try:
            written = _render(g, lat, noise, 0, N_FRAMES / 30, BATCH, SIZE, out, None, 1.0, [], {}, False, "slow", None,
                              pipe_pix_fmt=f"mjpeg:{QUALITY}")
        except ValueError as exc:
            if rank != 0 or final or "overflowed" not in str(exc):
                raise
            written = None
        torch.cuda.synchronize()
        return out, written

    results = world.play(play)
    assert [written for _, written in results][1:] == [0, N_FRAMES]
    rounds = world.rounds[1]
    assert all(tuple(r.shape) == (BATCH, render.mjpeg_slot_bytes(SIZE, SIZE)) and r.dtype == torch.uint8 for r in rounds)
    assert len(rounds) == 3 and _payloads(torch.cat(rounds)[:5]) == list(want[6:])  # rank 1's block: frames 6 .. 10 in order
    _assert_avi(results[2][0] + ".avi", want)


class _GroupOfOne(PlayedWorld):
    """PlayedWorld plus the two collectives sharding.HostFrameStore issues when it opens its segment."""

    class ReduceOp:
        MAX = "max"

    def get_backend(self):
        return "gloo"

    def all_reduce(self, tensor, op=None, group=None, async_op=False):
        return None


def test_host_transport_carries_the_slots(gpu, job, monkeypatch):
    g, lat, noise, want, tmp = job
    monkeypatch.delenv("MAUA_PIPE_PIX_FMT", raising=False)
    out = str(tmp / "host.mp4")
    with _GroupOfOne(1).playing(0):
        written = _render(g, lat, noise, 0, N_FRAMES / 30, BATCH, SIZE, out, None, 1.0, [], {}, False, "slow", None, transport="host",
                          pipe_pix_fmt=f"mjpeg:{QUALITY}")
    assert written == N_FRAMES
    _assert_avi(out + ".avi", want)
