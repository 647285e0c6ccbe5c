"""GPU: a colour grade through the render loop — render_graded, generate() with a plugin's grade, the CLI flags and the shipped
examples/graded.py — on the seeded 64-px generator of tests/test_resample_render_gpu.py: 7 frames at batch 2 are three captured batches and
an eager tail batch of one.  Every file equals the existing conversion twins applied to what the device entries give for the lanes' fp32
images (tests/test_grade_gpu.py holds the entries themselves against the definition), bit for bit."""
import argparse
import random

import numpy as np
import pytest
import torch

import deep_ref as dr
import grade_ref as gr
import jpeg_ref
import resample_ref as rr
from maua_stylegan2_amd import _lib, seeding, sharding
from played_world import PlayedWorld
from temporal_fold_ref import fold_video_ref
from test_resample_render_gpu import BATCH, N_FRAMES, SIZE, TAIL, _assert_file, _stand_ins
from test_yuv420_host import yuv420p_oracle

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
FMTS = ("rgb24", "yuv420p", "mjpeg", "rgb48le", "yuv420p10le")


def _graded_render(*args, **kwargs):
    from maua_stylegan2_amd import render

    with pytest.MonkeyPatch.context() as mp:
        _stand_ins(mp)
        return render.render_graded(*args, **kwargs)


@pytest.fixture(scope="module")
def job(gpu, tmp_path_factory):
    """The seeded generator, the job's inputs, its plain frames and the lanes' fp32 images, two grades (one row per frame — identity rows,
    a power, a LUT — and one row) and what the device entries give for them (once, read-only)."""
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render
    from maua_stylegan2_amd.models.stylegan2 import Generator

    g = Generator(SIZE, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(SIZE, seed=4), strict=True)
    g = g.to(gpu).eval()
    lat = seeding.seeded_latents(N_FRAMES, g.n_latent, seed=6)
    noise = seeding.seeded_noise(N_FRAMES, SIZE, seed=7)
    noise[-1] = None
    tmp = tmp_path_factory.mktemp("grade")
    out = str(tmp / "plain.mp4")
    with pytest.MonkeyPatch.context() as mp:
        _stand_ins(mp)
        assert render.render(g, lat, noise, 0, N_FRAMES / 30, BATCH, SIZE, out) == N_FRAMES
    rgb = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(N_FRAMES, SIZE, SIZE, 3)
    images_dev = torch.cat([img.clone() for _, img in render.synthesize(g, lat, noise, BATCH, frames="f32")])
    images = images_dev.cpu().numpy()
    lut = gr.sample_lut(17, seed=3)
    flash = np.array([0.0, 0.8, 0.0, 0.3, -0.4, 0.0, 0.5])
    grades = {
        "per-frame": ar.Grade(N_FRAMES, exposure=flash, saturation=1 + flash, hue=40 * flash, gamma=1 + 0.5 * np.abs(flash), lut=lut, lut_mix=np.abs(flash)),
        "one-row": ar.Grade(contrast=1.2, pivot=0.4, white_balance=[1.1, 1.0, 0.9], saturation=0.7),
    }
    assert list(grades["per-frame"].identity) == [True, False, True, False, False, True, False] and grades["one-row"].n_rows == 1
    device = {}
    for name, grade in grades.items():
        rows = grade.rows(gpu)
        rows = rows if grade.n_rows == N_FRAMES else rows.expand(N_FRAMES, 24).contiguous()
        f32 = render.grade_frames(images_dev.clone(), rows, grade.lut_table(gpu), {}, out="f32")
        u8 = render.grade_frames(images_dev, rows, grade.lut_table(gpu), {}, out="u8")
        device[name] = (f32.cpu().numpy(), u8.cpu().numpy())
        # (the wrapper hands the entries what the twin is given: where power == 1 the bits are the twin's)
        plain_power = (grade.table[:, 6:9] == 1).all(axis=1) if grade.n_rows == N_FRAMES else np.full(N_FRAMES, bool((grade.table[:, 6:9] == 1).all()))
        twin = gr.grade(images, np.broadcast_to(grade.table, (N_FRAMES, 24)) if grade.n_rows == 1 else grade.table, grade.lut, np.float32)
        assert np.array_equal(device[name][0][plain_power].view(np.uint32), twin[plain_power].view(np.uint32))
        assert np.array_equal(device[name][1], gr.quant8(device[name][0]))
    assert np.array_equal(device["per-frame"][1][[0, 2, 5]], rgb[[0, 2, 5]]) and (device["per-frame"][1][1] != rgb[1]).mean() > 0.2
    for a in (rgb, images):
        a.setflags(write=False)
    return dict(g=g, lat=lat, noise=noise, rgb=rgb, images=images, images_dev=images_dev, tmp=tmp, grades=grades, device=device)


def _converted(fmt, f32, u8, size=(SIZE, SIZE)):
    """The existing conversion twins on graded frames: flat bytes per frame; for mjpeg the list of JPEG streams."""
    from maua_stylegan2_amd import render

    if fmt in render.DEEP_PIX_FMTS:
        return dr.deliver(f32, fmt)
    if fmt == "yuv420p":
        return yuv420p_oracle(u8)
    if fmt == "mjpeg":
        return [jpeg_ref.encode(f, render.MJPEG_DEFAULT_QUALITY, (size[0] + 15) // 16) for f in u8]
    return u8.reshape(len(u8), -1)


@pytest.mark.parametrize("fmt", FMTS)
def test_graded_render_writes_the_twins_of_the_device_entries_output(gpu, job, fmt):
    for name in ("per-frame", "one-row") if fmt in ("rgb24", "yuv420p10le") else ("per-frame",):
        out = str(job["tmp"] / f"{fmt}_{name}.mp4")
        written = _graded_render(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out, *TAIL, pipe_pix_fmt=fmt, grade=job["grades"][name])
        assert written == N_FRAMES
        _assert_file(out, fmt, _converted(fmt, *job["device"][name]), (SIZE, SIZE))


def test_an_identity_grade_writes_the_plain_renders_file(gpu, job):
    import maua_stylegan2_amd.audioreactive as ar

    for grade in (ar.Grade(), ar.Grade(N_FRAMES, exposure=np.zeros(N_FRAMES), lut=gr.sample_lut(3), lut_mix=0)):
        assert grade.is_identity
        out = str(job["tmp"] / f"identity{grade.n_rows}.mp4")
        assert _graded_render(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out, *TAIL, grade=grade) == N_FRAMES
        assert np.array_equal(np.fromfile(out + ".rgb24", dtype=np.uint8), job["rgb"].reshape(-1))
        assert _graded_render(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out, *TAIL, pipe_pix_fmt="rgb48le", grade=grade) == N_FRAMES
        assert np.array_equal(np.fromfile(out + ".rgb48le", dtype=np.uint8), dr.deliver(job["images"], "rgb48le").reshape(-1))


def test_default_render_never_reaches_the_grade_entries(gpu, job, monkeypatch):
    from maua_stylegan2_amd import render

    def boom(*a, **kw):
        raise AssertionError("the grade was reached by a render without one")

    _stand_ins(monkeypatch)
    lib = _lib.load()
    for name in ("maua_grade_f32", "maua_grade_to_u8"):
        monkeypatch.setattr(lib, name, boom)
    monkeypatch.setattr(render, "grade_frames", boom)
    for k, entry in enumerate((render.render_shard, render.render_delivered, render.render_graded)):
        for fmt, ext in ((None, "rgb24"), ("rgb48le", "rgb48le")):
            out = str(job["tmp"] / f"default{k}_{ext}.mp4")
            assert entry(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out, *TAIL, pipe_pix_fmt=fmt) == N_FRAMES
            want = job["rgb"].reshape(-1) if fmt is None else dr.deliver(job["images"], "rgb48le").reshape(-1)
            assert np.array_equal(np.fromfile(out + "." + ext, dtype=np.uint8), want)


def test_the_grade_is_applied_per_sub_frame_before_the_fold_and_before_the_resampler(gpu, job):
    from maua_stylegan2_amd import render

    grade = job["grades"]["per-frame"].slice(0, 6)
    u8 = job["device"]["per-frame"][1][:6]
    noise = [None if nz is None else nz[:6] for nz in job["noise"]]
    fold = render.TemporalFold(2, "3,1")
    out = str(job["tmp"] / "fold.mp4")
    assert _graded_render(job["g"], job["lat"][:6], noise, 0, 3 / 30, BATCH, SIZE, out, *TAIL, fold=fold, grade=grade) == 3
    folded = fold_video_ref(u8, [3, 1])
    assert np.array_equal(np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(3, SIZE, SIZE, 3), folded)
    assert not np.array_equal(folded, fold_video_ref(job["rgb"][:6], [3, 1]))
    # fold, then resize, then the colour conversion: all on graded sub-frames
    resize = render.FrameResize("48x36", "bicubic", "crop")
    assert _graded_render(job["g"], job["lat"][:6], noise, 0, 3 / 30, BATCH, SIZE, out, *TAIL, pipe_pix_fmt="yuv420p", fold=fold, resize=resize, grade=grade) == 3
    _assert_file(out, "yuv420p", yuv420p_oracle(rr.deliver(folded, (48, 36), "bicubic", "crop")), (48, 36))
    # a delivery size on a deep format: the graded fp32 image -> 16-bit master -> resampler
    resize = render.FrameResize("32x48", "hamming", "crop")
    grade = job["grades"]["per-frame"]
    assert _graded_render(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out, *TAIL, pipe_pix_fmt="rgb48le", resize=resize, grade=grade) == N_FRAMES
    master = rr.deliver(dr.frames_to_u16(job["device"]["per-frame"][0]), (32, 48), "hamming", "crop")
    _assert_file(out, "rgb48le", master.reshape(len(master), -1).astype("<u2").view(np.uint8), (32, 48))


def test_two_played_shards_concatenate_to_the_one_rank_file(gpu, job):
    """``_shard = (lo, hi, n)``: every rank holds its block of the per-frame inputs and of the grade (Grade.slice); rank 0's file is the
    one-rank file."""
    grade = job["grades"]["per-frame"]
    world = PlayedWorld(2)

    def play(rank, final):
        lo, hi = sharding.shard_bounds(N_FRAMES, rank, 2)
        noise = [None if nz is None else nz[lo:hi] for nz in job["noise"]]
        out = str(job["tmp"] / f"rank{rank}_{int(final)}.mp4")
        tail = TAIL[:-1] + ((lo, hi, N_FRAMES),)
        written = _graded_render(job["g"], job["lat"][lo:hi], noise, 0, N_FRAMES / 30, BATCH, SIZE, out, *tail, grade=grade.slice(lo, hi))
        torch.cuda.synchronize()
        return out, written

    results = world.play(play)
    assert [written for _, written in results] == [N_FRAMES, 0, N_FRAMES]
    _assert_file(results[2][0], "rgb24", _converted("rgb24", *job["device"]["per-frame"]), (SIZE, SIZE))


def test_a_table_of_the_wrong_length_is_refused_before_the_first_batch(gpu, job, monkeypatch):
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render

    def boom(*a, **kw):
        raise AssertionError("a batch was rendered")

    monkeypatch.setattr(render, "synthesize", boom)
    out = str(job["tmp"] / "refused.mp4")
    with pytest.raises(ValueError, match=r"5 rows.*\(7\)"):
        _graded_render(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out, *TAIL, grade=ar.Grade(exposure=np.zeros(5)))
    with pytest.raises(TypeError, match="Grade"):
        _graded_render(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out, *TAIL, grade="exposure=1")


# ------------------------------------------------------------------------------------------------ through generate()
PLUGIN = '''import numpy as np
import torch

import maua_stylegan2_amd.audioreactive as ar


def get_latents(selection, args):
    t = torch.arange(args.n_frames, dtype=torch.float32) / args.fps * 6.0
    lo, frac = t.floor().long() % len(selection), (t - t.floor())[:, None, None]
    return selection[lo] * (1 - frac) + selection[(lo + 1) % len(selection)] * frac


def get_noise(**kw):
    return None


def flash(args):
    return ar.Grade(args.n_frames, exposure=0.5 * (np.arange(args.n_frames) % 2), hue=np.linspace(0, 30, args.n_frames))
'''


class _Spy:
    """render.grade_frames with its operands recorded: what reached the entries, batch by batch."""

    def __init__(self, mp):
        from maua_stylegan2_amd import render

        self.images, self.rows, self.luts, self.kinds = [], [], [], []
        orig = render.grade_frames

        def spy(images, grade_rows, lut, scratch, out="u8"):
            self.images.append(images.detach().clone().cpu().numpy())
            self.rows.append(grade_rows[:, :24].detach().clone().cpu().numpy())
            self.luts.append(None if lut is None else lut.detach().clone().cpu().numpy())
            self.kinds.append(out)
            return orig(images, grade_rows, lut, scratch, out)

        mp.setattr(render, "grade_frames", spy)

    def expected_u8(self, lut=None):
        """The twin on everything recorded (power == 1 rows only: bit for bit)."""
        images, rows = np.concatenate(self.images), np.concatenate(self.rows)
        assert (rows[:, 6:9] == 1).all()
        return gr.quant8(gr.grade(images, rows, lut, np.float32)), rows


def test_generate_with_a_plugins_grade_and_with_the_cli_flags(gpu, job, tmp_path, monkeypatch):
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import generate_audiovisual as gav

    g = job["g"]
    _stand_ins(monkeypatch)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(ar, "load_audio", lambda audio_file, offset, duration: (np.zeros(4000, np.float32), 8000, 0.5))
    monkeypatch.setattr(gav, "load_generator", lambda **kw: g)
    np.save("lat.npy", seeding.seeded_latents(5, g.n_latent, seed=11).numpy())
    (tmp_path / "plain_plugin.py").write_text(PLUGIN)
    (tmp_path / "override_plugin.py").write_text(PLUGIN + "\nOVERRIDE = dict(grade=flash)\n")
    (tmp_path / "init_plugin.py").write_text(PLUGIN + "\ndef initialize(args):\n    args.grade = flash(args)\n    return args\n")
    lut = gr.sample_lut(5, seed=8)
    ar.save_cube(tmp_path / "look.cube", lut)

    def run(name, plugin_file, *flags):
        random.seed(123), np.random.seed(123), torch.manual_seed(123), torch.cuda.manual_seed_all(123)
        out = str(tmp_path / name)
        with pytest.MonkeyPatch.context() as mp:
            spy = _Spy(mp)
            gav.main(["--ckpt", "none.pt", "--audio_file", "stub.wav", "--audioreactive_file", str(tmp_path / plugin_file), "--latent_file", "lat.npy",
                      "--G_res", str(SIZE), "--out_size", str(SIZE), "--fps", "16", "--batch", "4", "--output_file", out, *flags])
        return out, spy

    out, spy = run("plain.mp4", "plain_plugin.py")
    plain = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(-1, SIZE, SIZE, 3)
    assert plain.shape[0] == 8 and plain.std() > 5 and not spy.kinds
    flash_rows = ar.Grade(8, exposure=0.5 * (np.arange(8) % 2), hue=np.linspace(0, 30, 8)).table
    for name, plugin_file in (("override.mp4", "override_plugin.py"), ("init.mp4", "init_plugin.py")):
        out, spy = run(name, plugin_file)
        want, rows = spy.expected_u8()
        got = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(8, SIZE, SIZE, 3)
        assert spy.kinds == ["u8", "u8"] and np.array_equal(rows, flash_rows) and np.array_equal(got, want)
        assert np.array_equal(got[0], plain[0]) and (got[1] != plain[1]).mean() > 0.3  # frame 0's row is the identity
    # the CLI flags alone: a one-row grade with a LUT; then attached to the plugin's LUT-less grade
    out, spy = run("flags.mp4", "plain_plugin.py", "--grade", "exposure=0.3,saturation=1.2,hue=15", "--grade_lut", str(tmp_path / "look.cube"), "--grade_lut_mix", "0.5")
    want, rows = spy.expected_u8(lut)
    one = ar.Grade(exposure=0.3, saturation=1.2, hue=15, lut_mix=0.5).table
    assert np.array_equal(rows, np.broadcast_to(one, (8, 24))) and np.array_equal(spy.luts[0], gr.pad_lut(lut))
    assert np.array_equal(np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(8, SIZE, SIZE, 3), want)
    out, spy = run("both.mp4", "init_plugin.py", "--grade_lut", str(tmp_path / "look.cube"), "--pipe_pix_fmt", "yuv420p")
    want, rows = spy.expected_u8(lut)
    both = flash_rows.copy()
    both[:, 21] = 1.0
    assert np.array_equal(rows, both) and np.array_equal(np.fromfile(out + ".yuv420p", dtype=np.uint8).reshape(8, -1), yuv420p_oracle(want))
    with pytest.raises(ValueError, match="cannot be combined"):
        run("refused.mp4", "init_plugin.py", "--grade", "hue=3")


def test_the_graded_example_plugin_through_generate(gpu, job, tmp_path, monkeypatch):
    """examples/graded.py: the default plugin's latents and noise, a grade of one row per frame from onsets, level and chroma; the file is
    the grade of the images that reached the entries, and the rows are finite, modulated and inside the plugin's ranges."""
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import generate_audiovisual as gav
    from maua_stylegan2_amd.audioreactive.examples import graded as plugin

    sr, fps, seconds = 22050, 16, 2
    t = np.arange(sr * seconds) / sr
    rng = np.random.default_rng(2)
    kick = np.sin(2 * np.pi * 60 * t) * np.exp(-((t % 0.5) * 12))  # four kicks a second apart by half a second
    chord = sum(np.sin(2 * np.pi * f * t) for f in (261.6, 329.6, 392.0)) * (t < 1) + sum(np.sin(2 * np.pi * f * t) for f in (293.7, 370.0, 440.0)) * (t >= 1)
    clip = (0.6 * kick + 0.15 * chord * (0.3 + 0.7 * (t / seconds)) + 0.02 * rng.standard_normal(t.size)).astype(np.float32)
    g = job["g"]
    _stand_ins(monkeypatch)
    monkeypatch.chdir(tmp_path)
    before = ar.signal.SMF
    monkeypatch.setattr(ar, "load_audio", lambda audio_file, offset, duration: (clip, sr, float(seconds)))
    monkeypatch.setattr(gav, "load_generator", lambda **kw: g)
    np.save("lat.npy", seeding.seeded_latents(12, g.n_latent, seed=11).numpy())
    random.seed(5), np.random.seed(5), torch.manual_seed(5), torch.cuda.manual_seed_all(5)
    spy = _Spy(monkeypatch)
    try:
        out = gav.generate(ckpt=None, audio_file="stub.wav", initialize=plugin.initialize, get_latents=plugin.get_latents, get_noise=plugin.get_noise,
                           latent_file="lat.npy", G_res=SIZE, out_size=SIZE, fps=fps, batch=4, output_file=str(tmp_path / "graded.mp4"),
                           args=argparse.Namespace(fps=fps, latent_count=12))
    finally:
        ar.set_SMF(before)
    n = fps * seconds
    want, rows = spy.expected_u8()
    got = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(-1, SIZE, SIZE, 3)
    assert got.shape[0] == n and rows.shape == (n, 24) and np.array_equal(got, want) and got.std() > 5
    assert np.isfinite(rows).all() and (rows[:, 0] >= 1).all() and (rows[:, 0] <= 2 ** plugin.FLASH_STOPS + 1e-6).all() and np.ptp(rows[:, 0]) > 0.1
    assert np.ptp(rows[:, 9]) > 0 and (rows[:, 21] == 1).all()  # (column 9: the first entry of hue . saturation)
