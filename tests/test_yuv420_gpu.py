"""GPU: planar YUV 4:2:0 delivery — maua_rgb_to_yuv420p_u8 (csrc/yuv420.hip) bit for bit against the integer oracle of
tests/test_yuv420_host.py, its bounds, argument checks and capture, and the opt-in pipe format through render() on one rank and on two
played ranks against the rgb24 delivery of the same job."""
import os

import numpy as np
import pytest
import torch

from maua_stylegan2_amd import seeding
from played_world import PlayedWorld
from test_yuv420_host import known_colour_frame, yuv420p_oracle

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# (batch, h, w): one block; rows off the dword grid, tail only; a full strip plus a tail; whole strips and the batch stride (vector path);
# 540 chroma columns; batch 8
SHAPES = [(1, 2, 2), (2, 4, 6), (3, 6, 10), (1, 8, 34), (2, 16, 64), (1, 4, 1080), (8, 2, 256)]
GUARD, FILL = 256, 0xA5


def _random_frames(shape, seed):
    b, h, w = shape
    frames = np.random.default_rng(seed).integers(0, 256, (b, h, w, 3), dtype=np.uint8)
    frames[0, :2, :2] = [(255, 255, 255), (0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255)][seed % 5]  # a saturated block in every input
    return frames


def _convert(frames, gpu):
    from maua_stylegan2_amd import render

    out = render.frames_to_yuv420p(torch.from_numpy(frames).to(gpu), {})
    assert out.dtype == torch.uint8 and tuple(out.shape) == (frames.shape[0], frames.shape[1] * frames.shape[2] * 3 // 2)
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_integer_oracle_bit_for_bit(gpu, shape):
    frames = _random_frames(shape, seed=sum(shape))
    assert np.array_equal(_convert(frames, gpu), yuv420p_oracle(frames))


def test_known_answer_colours_on_both_kernel_paths(gpu):
    known = known_colour_frame()  # [1, 2, 10, 3]: byte path
    wide = np.tile(known, (1, 1, 4, 1))  # [1, 2, 40, 3]: vector path
    for frames in (known, wide):
        got = _convert(frames, gpu)
        assert np.array_equal(got, yuv420p_oracle(frames))
    w = known.shape[2]
    got = _convert(known, gpu)[0]
    assert list(got[:w:2]) == [235, 16, 81, 145, 41] and list(got[2 * w: 2 * w + 5]) == [128, 128, 90, 54, 240]
    assert list(got[2 * w + 5:]) == [128, 128, 240, 34, 110]


@pytest.mark.parametrize("shape,skew", [((2, 4, 6), 0), ((1, 8, 34), 0), ((2, 16, 64), 0), ((1, 4, 16), 1)],
                         ids=["2x4x6", "1x8x34", "2x16x64-vector", "1x4x16-unaligned"])
def test_red_zone_every_byte_written_and_none_outside(gpu, shape, skew):
    """Output between two guards of 256 bytes of 0xA5, itself pre-filled with 0xA5; input at the very end of its allocation.  Afterwards the
    guards are intact and the body equals the oracle completely (= every byte was written).  ``skew`` = 1 moves the output off the 8-byte
    grid: a width the vector path would take goes through the byte path."""
    from maua_stylegan2_amd import _lib

    b, h, w = shape
    frames = _random_frames(shape, seed=7 + w)
    n_in, n_out = frames.size, b * h * w * 3 // 2
    holder = torch.empty(((n_in + 511) // 512) * 512, dtype=torch.uint8, device=gpu)  # (the allocator hands out multiples of 512 bytes)
    src = holder[holder.numel() - n_in:]
    src.copy_(torch.from_numpy(frames.reshape(-1)).to(gpu))
    buf = torch.full((GUARD + skew + n_out + GUARD,), FILL, dtype=torch.uint8, device=gpu)
    out = buf[GUARD + skew: GUARD + skew + n_out]
    rc = _lib.load().maua_rgb_to_yuv420p_u8(src.data_ptr(), out.data_ptr(), b, h, w, _lib.stream_ptr(gpu))
    assert rc == 0
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[: GUARD + skew] == FILL).all() and (host[GUARD + skew + n_out:] == FILL).all()
    assert np.array_equal(host[GUARD + skew: GUARD + skew + n_out].reshape(b, -1), yuv420p_oracle(frames))


def test_bad_arguments_launch_nothing_and_an_empty_batch_succeeds(gpu):
    from maua_stylegan2_amd import _lib, render

    lib = _lib.load()
    src = torch.zeros(4 * 8 * 8 * 3, dtype=torch.uint8, device=gpu)
    out = torch.full((4 * 8 * 8 * 3,), FILL, dtype=torch.uint8, device=gpu)
    for b, h, w in [(1, 3, 4), (1, 4, 3), (2, 5, 7), (1, 0, 4), (-1, 4, 4)]:
        assert lib.maua_rgb_to_yuv420p_u8(src.data_ptr(), out.data_ptr(), b, h, w, _lib.stream_ptr(gpu)) != 0, (b, h, w)
    for shape in [(1, 3, 4, 3), (1, 4, 3, 3), (2, 5, 7, 3)]:
        with pytest.raises(ValueError, match="even"):
            render.frames_to_yuv420p(torch.zeros(shape, dtype=torch.uint8, device=gpu), {})
    assert lib.maua_rgb_to_yuv420p_u8(src.data_ptr(), out.data_ptr(), 0, 4, 4, _lib.stream_ptr(gpu)) == 0
    torch.cuda.synchronize()
    assert bool((out == FILL).all())  # nothing was launched
    scratch = {}
    empty = render.frames_to_yuv420p(torch.zeros((0, 4, 4, 3), dtype=torch.uint8, device=gpu), scratch)
    assert tuple(empty.shape) == (0, 24)


def test_capturable_and_reuses_the_callers_scratch_buffer(gpu):
    """Captured in a torch.cuda.graph (stream-ordered, no allocation: the output lives in the caller's scratch dict) and replayed twice on
    changed input."""
    from maua_stylegan2_amd import render

    shape = (2, 16, 64)
    inputs = [_random_frames(shape, seed) for seed in (11, 12, 13)]
    src = torch.from_numpy(inputs[0]).to(gpu)
    scratch = {}
    first = render.frames_to_yuv420p(src, scratch)  # allocates the output
    assert np.array_equal(first.cpu().numpy(), yuv420p_oracle(inputs[0])) and len(scratch) == 1
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = render.frames_to_yuv420p(src, scratch)
    assert out.data_ptr() == first.data_ptr() and len(scratch) == 1
    for frames in inputs[1:]:
        src.copy_(torch.from_numpy(frames).to(gpu))
        out.fill_(FILL)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), yuv420p_oracle(frames))


@pytest.mark.parametrize("out_size,shape", [(1920, (1, 1024, 2048, 3)), (1080, (1, 2048, 1024, 3))])
def test_wide_output_is_delivered_as_planar_1080p(gpu, out_size, shape):
    """The delivery of a 1920 / 1080 render on a synthetic 2048-px frame (the 1024^2 generator the real route needs is too heavy for this
    file): crop + resize + conversion on the device = the oracle applied to the rgb24 delivery of the same frame, 1920 * 1080 * 3 / 2 bytes
    a frame, and the sink takes it as it is."""
    from maua_stylegan2_amd import render

    frame = torch.from_numpy(np.random.default_rng(out_size).integers(0, 256, shape, dtype=np.uint8)).to(gpu)
    scratch = {}
    planar = render._deliverable(frame, out_size, "yuv420p", scratch)
    rgb = render._deliverable(frame, out_size, "rgb24", scratch)
    width, height = render._output_dims(out_size)
    assert tuple(rgb.shape) == (1, height, width, 3) and tuple(planar.shape) == (1, 1920 * 1080 * 3 // 2)
    assert tuple(planar.shape[1:]) == render._stream_frame_shape(type("G", (), {"size": 1024}), out_size, "yuv420p")
    got = planar.cpu().numpy()
    assert np.array_equal(got, yuv420p_oracle(rgb.cpu().numpy()))
    sink = render.FrameSink(None, width, height, 30, pix_fmt="yuv420p")
    sink.write(got[0])
    assert sink.count == 1
    with pytest.raises(ValueError):
        sink.write(rgb.cpu().numpy()[0])


N_FRAMES, BATCH, SIZE = 7, 2, 64  # 3 captured batches + an eager tail batch of 1


def _render(*args, **kwargs):
    """render_shard at the generator's own frame size (render() only knows the reference's output sizes, 512 and up: the size table is
    stood in for, as tests/test_two_rank_gpu.py does for its 64-px generator)."""
    from maua_stylegan2_amd import render

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(render, "_output_dims", lambda out_size: (SIZE, SIZE))
        mp.setattr(render.shutil, "which", lambda name: None)  # the fallback file, whatever the box has installed
        return render.render_shard(*args, **kwargs)


@pytest.fixture(scope="module")
def job(gpu, tmp_path_factory):
    """The seeded generator and the rgb24 delivery of the job every end-to-end test below renders again as yuv420p (computed once)."""
    from maua_stylegan2_amd import render
    from maua_stylegan2_amd.models.stylegan2 import Generator

    g = Generator(SIZE, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(SIZE, seed=4), strict=True)
    g = g.to(gpu).eval()
    lat = seeding.seeded_latents(N_FRAMES, g.n_latent, seed=6)
    noise = seeding.seeded_noise(N_FRAMES, SIZE, seed=7)
    noise[-1] = None
    tmp = tmp_path_factory.mktemp("yuv420")
    out = str(tmp / "rgb.mp4")
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("MAUA_PIPE_PIX_FMT", raising=False)
        mp.setattr(render, "_output_dims", lambda out_size: (SIZE, SIZE))
        mp.setattr(render.shutil, "which", lambda name: None)
        assert render.render(g, lat, noise, 0, N_FRAMES / 30, BATCH, SIZE, out) == N_FRAMES  # the default path, through render() itself
    rgb = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(N_FRAMES, SIZE, SIZE, 3)
    assert rgb.std() > 5
    want = yuv420p_oracle(rgb)
    want.setflags(write=False)
    return g, lat, noise, want, tmp


def test_render_yuv420p_equals_the_oracle_on_the_rgb24_frames(gpu, job, monkeypatch):
    """A render with the planar pipe format writes the .yuv420p fallback file: same frame count and order as the rgb24 render of the same
    job, every byte the oracle's — captured batches and the eager tail batch alike.  Through render() (whose parameter list is the
    reference's: the format reaches it through $MAUA_PIPE_PIX_FMT) and through render_shard's keyword."""
    from maua_stylegan2_amd import render

    g, lat, noise, want, tmp = job
    monkeypatch.setattr(render, "_output_dims", lambda out_size: (SIZE, SIZE))
    monkeypatch.setattr(render.shutil, "which", lambda name: None)
    monkeypatch.setenv("MAUA_PIPE_PIX_FMT", "yuv420p")
    out = str(tmp / "env.mp4")
    assert render.render(g, lat, noise, 0, N_FRAMES / 30, BATCH, SIZE, out) == N_FRAMES
    assert not os.path.exists(out + ".rgb24") and os.path.getsize(out + ".yuv420p") == N_FRAMES * SIZE * SIZE * 3 // 2
    got = np.fromfile(out + ".yuv420p", dtype=np.uint8).reshape(N_FRAMES, -1)
    assert np.array_equal(got, want)
    assert len({got[i].tobytes() for i in range(N_FRAMES)}) == N_FRAMES  # (distinct frames: the order is really checked)
    monkeypatch.delenv("MAUA_PIPE_PIX_FMT")
    out = str(tmp / "kw.mp4")
    written = _render(g, lat, noise, 0, N_FRAMES / 30, BATCH, SIZE, out, None, 1.0, [], {}, False, "slow", None, pipe_pix_fmt="yuv420p")
    assert written == N_FRAMES
    assert np.array_equal(np.fromfile(out + ".yuv420p", dtype=np.uint8).reshape(N_FRAMES, -1), want)


def test_two_played_ranks_deliver_the_one_rank_file(gpu, job, monkeypatch):
    """Two ranks played one after the other through the product's multi-rank branch (tests/played_world.py: rank 0 recording, rank 1, rank 0
    delivering; the mirror of test_render_rank_shards_on_device_equal_single_rank): blocks of 4 + 3 frames, planar payloads of batch x 1.5
    bytes per pixel per round, arriving in order; the file of rank 0 equals the one-rank file bit for bit."""
    g, lat, noise, want, tmp = job
    monkeypatch.delenv("MAUA_PIPE_PIX_FMT", raising=False)
    world = PlayedWorld(2)

    def play(rank, final):
        out = str(tmp / f"rank{rank}_{int(final)}.mp4")
        written = _render(g, lat, noise, 0, N_FRAMES / 30, BATCH, SIZE, out, None, 1.0, [], {}, False, "slow", None, pipe_pix_fmt="yuv420p")
        torch.cuda.synchronize()
        return out, written

    results = world.play(play)
    assert [written for _, written in results] == [N_FRAMES, 0, N_FRAMES]
    rounds = world.rounds[1]
    assert len(rounds) == 2 and all(tuple(r.shape) == (BATCH, SIZE * SIZE * 3 // 2) and r.dtype == torch.uint8 for r in rounds)
    peer = torch.cat(rounds)[:3].cpu().numpy()  # rank 1's block: frames 4, 5, 6 in order
    assert np.array_equal(peer, want[4:])
    got = np.fromfile(results[2][0] + ".yuv420p", dtype=np.uint8).reshape(N_FRAMES, -1)
    assert np.array_equal(got, want)


class _GroupOfOne(PlayedWorld):
    """PlayedWorld plus the two collectives sharding.HostFrameStore issues when it opens its segment."""

    class ReduceOp:
        MAX = "max"

    def get_backend(self):
        return "gloo"

    def all_reduce(self, tensor, op=None, group=None, async_op=False):
        return None


def test_host_transport_carries_planar_frames(gpu, job, monkeypatch):
    """The shared-memory transport (render_shard(transport="host")) under a process group of one played rank: its segment is sized for the
    planar frame shape and the reader delivers the one-rank file."""
    g, lat, noise, want, tmp = job
    monkeypatch.delenv("MAUA_PIPE_PIX_FMT", raising=False)
    out = str(tmp / "host.mp4")
    with _GroupOfOne(1).playing(0):
        written = _render(g, lat, noise, 0, N_FRAMES / 30, BATCH, SIZE, out, None, 1.0, [], {}, False, "slow", None, transport="host",
                          pipe_pix_fmt="yuv420p")
    assert written == N_FRAMES
    assert np.array_equal(np.fromfile(out + ".yuv420p", dtype=np.uint8).reshape(N_FRAMES, -1), want)
