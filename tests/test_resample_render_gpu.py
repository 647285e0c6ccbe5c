"""GPU: delivery at a size of the user's choice through the render loop — render_delivered / render() with the three environment variables
/ generate() with the CLI flags and a plugin's OVERRIDE — on the seeded 64-px generator the delivery tests use.  Every render equals the
numpy twin (tests/resample_ref.py) applied to the frames of the plain render of the same job, followed by the existing twins of the
colour conversion / the JPEG encoder, bit for bit: 7 frames at batch 2 are three captured batches and an eager tail batch of one."""
import os

import numpy as np
import pytest
import torch

import deep_ref as dr
import jpeg_ref
import resample_ref as rr
from maua_stylegan2_amd import _lib, seeding
from played_world import PlayedWorld
from temporal_fold_ref import fold_video_ref
from test_yuv420_host import yuv420p_oracle

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

N_FRAMES, BATCH, SIZE = 7, 2, 64
ENV = ("MAUA_DELIVER_SIZE", "MAUA_DELIVER_FILTER", "MAUA_DELIVER_FIT", "MAUA_SUBFRAMES", "MAUA_PIPE_PIX_FMT", "MAUA_MJPEG_QUALITY")
TAIL = (None, 1.0, [], {}, False, "slow", None)  # audio_file .. _shard of render_shard's parameter list
# pipe format -> (size, filter, fit): every filter and every fit at least once; up-scales, down-scales and mixed
SETTINGS = {
    "rgb24": ((96, 54), "lanczos", "crop"),
    "yuv420p": ((80, 40), "bicubic", "pad"),
    "mjpeg": ((48, 80), "bilinear", "stretch"),
    "rgb48le": ((32, 48), "hamming", "crop"),
    "yuv420p10le": ((100, 36), "box", "pad"),
    "yuv444p10le": ((34, 22), "lanczos", "stretch"),
}


def _stand_ins(mp):
    """render() only knows the reference's output sizes, 512 and up: the size table is stood in for (as tests/test_yuv420_gpu.py does), and
    the sink writes its fallback file whatever the box has installed."""
    from maua_stylegan2_amd import render

    mp.setattr(render, "_output_dims", lambda out_size: (SIZE, SIZE))
    mp.setattr(render.shutil, "which", lambda name: None)
    for name in ENV:
        mp.delenv(name, raising=False)


def _delivered_render(*args, **kwargs):
    from maua_stylegan2_amd import render

    with pytest.MonkeyPatch.context() as mp:
        _stand_ins(mp)
        return render.render_delivered(*args, **kwargs)


@pytest.fixture(scope="module")
def job(gpu, tmp_path_factory):
    """The seeded generator, the job's inputs, the frames of its plain render and the fp32 images of the same lanes (once, read-only)."""
    from maua_stylegan2_amd import render
    from maua_stylegan2_amd.models.stylegan2 import Generator

    g = Generator(SIZE, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(SIZE, seed=4), strict=True)
    g = g.to(gpu).eval()
    lat = seeding.seeded_latents(N_FRAMES, g.n_latent, seed=6)
    noise = seeding.seeded_noise(N_FRAMES, SIZE, seed=7)
    noise[-1] = None
    tmp = tmp_path_factory.mktemp("resample")
    out = str(tmp / "plain.mp4")
    with pytest.MonkeyPatch.context() as mp:
        _stand_ins(mp)
        assert render.render(g, lat, noise, 0, N_FRAMES / 30, BATCH, SIZE, out) == N_FRAMES
    rgb = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(N_FRAMES, SIZE, SIZE, 3)
    assert rgb.std() > 5
    images = torch.cat([img.clone() for _, img in render.synthesize(g, lat, noise, BATCH, frames="f32")]).cpu().numpy()
    for a in (rgb, images):
        a.setflags(write=False)
    return dict(g=g, lat=lat, noise=noise, rgb=rgb, images=images, tmp=tmp)


def _expected(job, fmt, size, filt, fit):
    """The twin on the plain render's frames (8-bit formats) or on the 16-bit master of the lanes' fp32 images (deep formats), then the
    existing conversion twins: flat bytes per frame; for mjpeg the list of JPEG streams."""
    from maua_stylegan2_amd import render

    if fmt in render.DEEP_PIX_FMTS:
        master = rr.deliver(dr.frames_to_u16(job["images"]), size, filt, fit)
        if fmt == "rgb48le":
            return master.reshape(len(master), -1).astype("<u2").view(np.uint8)
        sub = {v: k for k, v in dr.FMT_OF.items()}[fmt]
        return dr.yuv_p10(master, sub).astype("<u2").view(np.uint8)
    frames = rr.deliver(job["rgb"], size, filt, fit)
    if fmt == "yuv420p":
        return yuv420p_oracle(frames)
    if fmt == "mjpeg":
        return [jpeg_ref.encode(f, render.MJPEG_DEFAULT_QUALITY, (size[0] + 15) // 16) for f in frames]
    return frames.reshape(len(frames), -1)


def _assert_file(out, fmt, want, size):
    if fmt == "mjpeg":
        info = jpeg_ref.avi_frames(out + ".avi")
        assert (info["avih"]["width"], info["avih"]["height"]) == size and len(info["frames"]) == len(want)
        assert all(got == ref for got, ref in zip(info["frames"], want))
        return
    got = np.fromfile(out + "." + fmt, dtype=np.uint8).reshape(len(want), -1)
    assert got.shape == want.shape and np.array_equal(got, want), (fmt, int((got != want).sum()))
    assert len({g.tobytes() for g in got}) == len(got)  # (pairwise distinct: the order is really checked)


@pytest.mark.parametrize("fmt", list(SETTINGS))
def test_render_delivered_equals_the_twin_on_the_plain_renders_frames(gpu, job, fmt):
    from maua_stylegan2_amd import render

    size, filt, fit = SETTINGS[fmt]
    resize = render.FrameResize(size, filt, fit)
    out = str(job["tmp"] / f"{fmt}.mp4")
    written = _delivered_render(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out, *TAIL, pipe_pix_fmt=fmt, resize=resize)
    assert written == N_FRAMES and not (fmt != "rgb24" and os.path.exists(out + ".rgb24"))
    _assert_file(out, fmt, _expected(job, fmt, size, filt, fit), size)
    if fit == "pad" and fmt == "yuv420p":  # the border of a padded frame is black: luma 16 in the bars left and right of the 40-px window
        luma = np.fromfile(out + ".yuv420p", dtype=np.uint8).reshape(N_FRAMES, -1)[:, :80 * 40].reshape(N_FRAMES, 40, 80)
        assert (luma[:, :, :20] == 16).all() and (luma[:, :, 60:] == 16).all() and luma[:, :, 20:60].std() > 5


def test_render_takes_the_resize_from_the_environment(gpu, job, monkeypatch):
    from maua_stylegan2_amd import render

    _stand_ins(monkeypatch)
    monkeypatch.setenv("MAUA_DELIVER_SIZE", "50x70")
    monkeypatch.setenv("MAUA_DELIVER_FILTER", "hamming")
    monkeypatch.setenv("MAUA_DELIVER_FIT", "stretch")
    out = str(job["tmp"] / "env.mp4")
    assert render.render(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out) == N_FRAMES
    _assert_file(out, "rgb24", _expected(job, "rgb24", (50, 70), "hamming", "stretch"), (50, 70))


def test_fold_then_resize(gpu, job):
    """With a temporal fold the resize sees delivered frames: 6 rendered frames, 2 per delivered frame, then 64^2 -> 48 x 36."""
    from maua_stylegan2_amd import render

    fold, resize = render.TemporalFold(2, "3,1"), render.FrameResize("48x36", "bicubic", "crop")
    out = str(job["tmp"] / "fold.mp4")
    noise = [None if nz is None else nz[:6] for nz in job["noise"]]
    assert _delivered_render(job["g"], job["lat"][:6], noise, 0, 3 / 30, BATCH, SIZE, out, *TAIL, pipe_pix_fmt="yuv420p", fold=fold, resize=resize) == 3
    want = yuv420p_oracle(rr.deliver(fold_video_ref(job["rgb"][:6], [3, 1]), (48, 36), "bicubic", "crop"))
    _assert_file(out, "yuv420p", want, (48, 36))


def test_default_render_never_reaches_the_resampler(gpu, job, monkeypatch):
    """Without a delivery size: the new entry and its wrapper raise if touched, and the render writes the bytes it always wrote."""
    from maua_stylegan2_amd import render

    def boom(*a, **kw):
        raise AssertionError("the resampler was reached by a render without a delivery size")

    _stand_ins(monkeypatch)
    lib = _lib.load()
    for name in ("maua_resample_u8", "maua_resample_u16", "maua_resample_coeffs", "maua_resample_ws_bytes"):
        monkeypatch.setattr(lib, name, boom)
    monkeypatch.setattr(render, "resize_frames", boom)
    for fmt, ext in ((None, "rgb24"), ("rgb48le", "rgb48le")):
        out = str(job["tmp"] / f"default_{ext}.mp4")
        assert render.render_shard(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out, *TAIL, pipe_pix_fmt=fmt) == N_FRAMES
        got = np.fromfile(out + "." + ext, dtype=np.uint8)
        want = job["rgb"].reshape(-1) if fmt is None else dr.deliver(job["images"], "rgb48le").reshape(-1)
        assert np.array_equal(got, want)


def test_resize_frames_scratch_border_and_refusals(gpu, job):
    from maua_stylegan2_amd import render

    frames = torch.from_numpy(job["rgb"][:2].copy()).to(gpu)
    resize = render.FrameResize("80x40", "lanczos", "pad")
    scratch = {}
    first = render.resize_frames(frames, resize, scratch)
    again = render.resize_frames(frames, resize, scratch)
    torch.cuda.synchronize()
    assert first.data_ptr() == again.data_ptr() and len(scratch) == 1 and tuple(first.shape) == (2, 40, 80, 3)
    assert np.array_equal(first.cpu().numpy(), rr.deliver(job["rgb"][:2], (80, 40), "lanczos", "pad"))
    first[:, :, :20].fill_(77)  # the border is zeroed at allocation only: a later call leaves it alone
    render.resize_frames(frames, resize, scratch)
    torch.cuda.synchronize()
    assert bool((first[:, :, :20] == 77).all()) and np.array_equal(first[:, :, 20:60].cpu().numpy(), rr.deliver(job["rgb"][:2], (80, 40), "lanczos", "pad")[:, :, 20:60])
    # 16-bit frames travel as int16 tensors, as the deep stages keep them
    master = dr.frames_to_u16(job["images"][:2])
    got = render.resize_frames(torch.from_numpy(master.view(np.int16)).to(gpu), render.FrameResize("30x50", "bicubic", "stretch"), scratch)
    torch.cuda.synchronize()
    assert got.dtype == torch.int16 and np.array_equal(got.cpu().numpy().view(np.uint16), rr.deliver(master, (30, 50), "bicubic", "stretch"))
    assert tuple(render.resize_frames(frames[:0], resize, {}).shape) == (0, 40, 80, 3)
    with pytest.raises(ValueError, match="--deliver_size 4x4.*taps"):
        render.resize_frames(frames, render.FrameResize("4x4", "lanczos", "stretch"), {})     # 16 : 1 with 3 lobes: 97 taps
    with pytest.raises(RuntimeError, match="uint8 or int16"):
        render.resize_frames(frames.float(), resize, {})
    with pytest.raises(ValueError, match="--deliver_size 33x21"):
        render.frames_to_deep(torch.from_numpy(job["images"][:2].copy()).to(gpu), SIZE, "yuv420p10le", {}, resize=render.FrameResize("33x21"))


def test_two_played_ranks_deliver_the_one_rank_file(gpu, job):
    """The multi-rank order of operations (tests/played_world.py: rank 0 recording, rank 1, rank 0 delivering): frames are resized on the
    rank that rendered them, the rounds travel at the delivery size, rank 0's file is the one-rank file."""
    from maua_stylegan2_amd import render

    size, filt, fit = (96, 54), "lanczos", "crop"
    resize = render.FrameResize(size, filt, fit)
    want = _expected(job, "rgb24", size, filt, fit)
    world = PlayedWorld(2)

    def play(rank, final):
        out = str(job["tmp"] / f"rank{rank}_{int(final)}.mp4")
        written = _delivered_render(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out, *TAIL, resize=resize)
        torch.cuda.synchronize()
        return out, written

    results = world.play(play)
    assert [written for _, written in results] == [N_FRAMES, 0, N_FRAMES]
    rounds = world.rounds[1]
    assert len(rounds) == 2 and all(tuple(r.shape) == (BATCH, 54, 96, 3) and r.dtype == torch.uint8 for r in rounds)
    assert np.array_equal(torch.cat(rounds)[:3].cpu().numpy().reshape(3, -1), want[4:])  # rank 1's block: frames 4, 5, 6 in order
    _assert_file(results[2][0], "rgb24", want, size)


def test_generate_with_the_cli_flags_and_with_a_plugins_override(gpu, job, tmp_path, monkeypatch):
    """main() with --deliver_size / --deliver_filter / --deliver_fit writes the twin of what it writes without them; a plugin's OVERRIDE
    beats the command line."""
    import random

    from maua_stylegan2_amd import audioreactive as ar
    from maua_stylegan2_amd import generate_audiovisual as gav

    g = job["g"]
    _stand_ins(monkeypatch)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(ar, "load_audio", lambda audio_file, offset, duration: (np.zeros(4000, np.float32), 8000, 0.5))
    monkeypatch.setattr(gav, "load_generator", lambda **kw: g)
    np.save("lat.npy", seeding.seeded_latents(5, g.n_latent, seed=11).numpy())
    plugin = '''import torch

def get_latents(selection, args):
    t = torch.arange(args.n_frames, dtype=torch.float32) / args.fps * 6.0
    lo, frac = t.floor().long() % len(selection), (t - t.floor())[:, None, None]
    return selection[lo] * (1 - frac) + selection[(lo + 1) % len(selection)] * frac

def get_noise(**kw):
    return None
'''
    (tmp_path / "plain_plugin.py").write_text(plugin)
    (tmp_path / "override_plugin.py").write_text(plugin + '\nOVERRIDE = dict(deliver_size="40x30", deliver_filter="box", deliver_fit="pad")\n')

    def run(name, plugin_file, *flags):
        random.seed(123), np.random.seed(123), torch.manual_seed(123), torch.cuda.manual_seed_all(123)
        out = str(tmp_path / name)
        gav.main(["--ckpt", "none.pt", "--audio_file", "stub.wav", "--audioreactive_file", str(tmp_path / plugin_file), "--latent_file", "lat.npy",
                  "--G_res", str(SIZE), "--out_size", str(SIZE), "--fps", "16", "--batch", "4", "--output_file", out, *flags])
        return out

    plain = np.fromfile(run("plain.mp4", "plain_plugin.py") + ".rgb24", dtype=np.uint8).reshape(-1, SIZE, SIZE, 3)
    assert plain.shape[0] == 8 and plain.std() > 5
    out = run("flags.mp4", "plain_plugin.py", "--deliver_size", "96x54", "--deliver_filter", "bicubic", "--deliver_fit", "crop")
    assert np.array_equal(np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(8, 54, 96, 3), rr.deliver(plain, (96, 54), "bicubic", "crop"))
    out = run("planar.mp4", "plain_plugin.py", "--deliver_size", "96x54", "--pipe_pix_fmt", "yuv420p")
    assert np.array_equal(np.fromfile(out + ".yuv420p", dtype=np.uint8).reshape(8, -1), yuv420p_oracle(rr.deliver(plain, (96, 54), "lanczos", "crop")))
    out = run("override.mp4", "override_plugin.py", "--deliver_size", "96x54", "--deliver_filter", "bicubic")
    assert np.array_equal(np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(8, 30, 40, 3), rr.deliver(plain, (40, 30), "box", "pad"))


def test_a_2048_wide_render_is_delivered_at_16_to_9(gpu, tmp_path):
    """``out_size`` 1920 on the smallest generator whose frames are 2048 px wide (the route of tests/test_deep_frames_gpu.py): with a
    delivery size the built-in 112-px crop is skipped, the source is the whole 2048 x 1024 frame, cropped to 16:9 by the fit."""
    from maua_stylegan2_amd import render
    from maua_stylegan2_amd.models.stylegan2 import Generator

    torch.manual_seed(11)
    with torch.device(gpu):
        g = Generator(1024, 512, 8, channel_multiplier=2, constant_input=True, output_size=1920)
    g = g.to(gpu).eval()
    n, batch = 2, 2
    lat = seeding.seeded_latents(n, g.n_latent, seed=8)
    noise = [None] * g.num_layers
    bends = [{"layer": 0, "transform": torch.nn.ReplicationPad2d((2, 2, 0, 0))}]
    (first, u8), = list(render.synthesize(g, lat, noise, batch, bends=bends))
    assert first == 0 and tuple(u8.shape) == (n, 1024, 2048, 3)
    plain = u8.cpu().numpy()
    resize = render.FrameResize("384x216", "lanczos", "crop")
    assert resize.geometry(2048, 1024) == ((114, 0, 1934, 1024), (0, 0, 384, 216)) and render._stream_frame_shape(g, 1920, "rgb24", resize) == (216, 384, 3)
    out = str(tmp_path / "wide.mp4")
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(render.shutil, "which", lambda name: None)
        for name in ENV:
            mp.delenv(name, raising=False)
        written = render.render_delivered(g, lat, noise, 0, n / 30, batch, 1920, out, None, 1.0, bends, {}, False, "slow", None, resize=resize)
    assert written == n
    got = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(n, 216, 384, 3)
    assert np.array_equal(got, rr.deliver(plain, (384, 216), "lanczos", "crop")) and got.std() > 1
