"""GPU: a frame feedback through the render loop — render_fed, generate() with a plugin's feedback, the --feedback flag and the shipped
examples/trails.py — on the seeded 64-px generator of tests/test_resample_render_gpu.py: 9 frames at batch 2 are four captured batches on
the three graph lanes and an eager tail batch of one, so the state crosses lanes, streams and the captured / eager boundary.

Every file is compared with the plain render's fp32 frames put through the float32 emulation of tests/feedback_ref.py ON THE HOST, then
through the existing twins of what follows (quantiser, lens, grade, fold, resampler, colour conversion): within one code value, with at most
0.1 % of the values differing (the kernel is expected to equal the emulation in every bit; the cap is the issue's)."""
import argparse
import os
import random

import numpy as np
import pytest
import torch

import deep_ref as dr
import feedback_ref as fr
import grade_ref as gr
import resample_ref as rr
from maua_stylegan2_amd import _lib, seeding
from temporal_fold_ref import fold_video_ref
from test_resample_render_gpu import SIZE, TAIL, _stand_ins

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
N_FRAMES, BATCH = 9, 2  # four full batches on three lanes and a partial last one
F32, F64 = np.float32, np.float64


def _fed_render(*args, **kwargs):
    from maua_stylegan2_amd import render

    with pytest.MonkeyPatch.context() as mp:
        _stand_ins(mp)
        return render.render_fed(*args, **kwargs)


def _emulated(images, feedback, dtype=F32):
    """The whole render's recurrence on the host: one run over all frames from black."""
    n, _, h, w = images.shape
    rows = feedback.rows(h, w)
    rows = np.broadcast_to(rows, (n, 16)) if feedback.n_rows == 1 else rows
    return fr.run(images, rows, feedback.mode, feedback.border, dtype=dtype)[0]


def _close(got, want, what=""):
    """Within one code value, at most 0.1 % of the values differing."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    print(f"{what}: {int((diff != 0).sum())} of {diff.size} values differ, largest difference {int(diff.max())}")
    assert diff.max() <= 1 and (diff != 0).mean() <= 1e-3, (what, int(diff.max()), float((diff != 0).mean()))


@pytest.fixture(scope="module")
def job(gpu, tmp_path_factory):
    """The seeded generator, the job's inputs, its plain frames and the lanes' fp32 images, and the feedbacks of the tests with their
    emulated results (once, read-only)."""
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render
    from maua_stylegan2_amd.models.stylegan2 import Generator

    g = Generator(SIZE, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(SIZE, seed=4), strict=True)
    g = g.to(gpu).eval()
    lat = seeding.seeded_latents(N_FRAMES, g.n_latent, seed=6)
    noise = seeding.seeded_noise(N_FRAMES, SIZE, seed=7)
    noise[-1] = None
    tmp = tmp_path_factory.mktemp("feedback")
    out = str(tmp / "plain.mp4")
    with pytest.MonkeyPatch.context() as mp:
        _stand_ins(mp)
        assert render.render(g, lat, noise, 0, N_FRAMES / 30, BATCH, SIZE, out) == N_FRAMES
    rgb = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(N_FRAMES, SIZE, SIZE, 3)
    images = torch.cat([img.clone() for _, img in render.synthesize(g, lat, noise, BATCH, frames="f32")]).cpu().numpy()
    kick = np.array([0.0, 0.9, 0.0, 0.0, 0.7, 0.0, 1.0, 0.3, 0.0])
    feedbacks = {
        # moving and still rows alternate inside and across batches; frame 5 is neutral
        "per-frame": ar.Feedback(N_FRAMES, gain=np.where(np.arange(N_FRAMES) == 5, 0.0, 0.85), zoom=1 + 0.06 * kick, rotate=4.0 * kick,
                                 translate=np.stack([0.02 * kick, -0.01 * kick], 1), tint=(1.0, 0.9, 0.8), mode="max", border="mirror"),
        "one-row": ar.Feedback(gain=0.7, dry=0.8, zoom=1.04, rotate=-2.0, mode="add", border="wrap", limit=1.25),
        "still": ar.Feedback(gain=0.6, mode="screen"),
    }
    assert list(feedbacks["per-frame"].rows(SIZE, SIZE)[:, 12]) == [1, 0, 1, 1, 0, 1, 0, 0, 1] and feedbacks["per-frame"].neutral[5]
    emulated = {}
    for name, fb in feedbacks.items():
        e32, e64 = _emulated(images, fb), _emulated(images, fb, F64)
        # on the CPU first: the float32 emulation and float64 stay within the cap the device is held to
        _close(gr.quant8(e32), gr.quant8(e64.astype(F32)), f"{name}: emulation against float64")
        emulated[name] = (e32, gr.quant8(e32))
        assert emulated[name][1].shape == rgb.shape and (emulated[name][1][1:] != rgb[1:]).mean() > 0.05  # (the trail is visible)
    for a in (rgb, images):
        a.setflags(write=False)
    return dict(g=g, lat=lat, noise=noise, rgb=rgb, images=images, tmp=tmp, feedbacks=feedbacks, emulated=emulated)


def _args(job, out):
    return (job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out)


@pytest.mark.parametrize("name", ("per-frame", "one-row", "still"))
def test_fed_render_is_the_emulated_recurrence_and_repeats_byte_for_byte(gpu, job, name):
    outs = []
    for k in range(2):
        out = str(job["tmp"] / f"{name}_{k}.mp4")
        assert _fed_render(*_args(job, out), *TAIL, feedback=job["feedbacks"][name]) == N_FRAMES
        outs.append(np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(N_FRAMES, SIZE, SIZE, 3))
    _close(outs[0], job["emulated"][name][1], name)
    assert np.array_equal(outs[0], outs[1])  # the cross-lane event chain: no batch ever read a state that was not finished
    # every frame after the first carries its predecessors: without recursion (the state taken from the plain frame) it would differ
    cur, fb = job["images"], job["feedbacks"][name]
    rows = np.broadcast_to(fb.rows(SIZE, SIZE), (N_FRAMES, 16)) if fb.n_rows == 1 else fb.rows(SIZE, SIZE)
    flat = gr.quant8(fr.run(cur, rows, fb.mode, fb.border, dtype=F32, defect="no recursion")[0])
    assert (flat[2:] != job["emulated"][name][1][2:]).mean() > 0.01


def test_a_neutral_feedback_writes_the_plain_renders_file_and_launches_nothing(gpu, job, monkeypatch):
    import maua_stylegan2_amd.audioreactive as ar

    def boom(*a, **kw):
        raise AssertionError("a neutral feedback reached the kernel")

    monkeypatch.setattr(_lib.load(), "maua_feedback_f32", boom)
    for fb in (ar.Feedback(), ar.Feedback(N_FRAMES, gain=np.zeros(N_FRAMES), zoom=1.1)):
        assert fb.is_identity
        out = str(job["tmp"] / f"neutral{fb.n_rows}.mp4")
        assert _fed_render(*_args(job, out), *TAIL, feedback=fb) == N_FRAMES
        assert np.array_equal(np.fromfile(out + ".rgb24", dtype=np.uint8), job["rgb"].reshape(-1))
        assert _fed_render(*_args(job, out), *TAIL, pipe_pix_fmt="rgb48le", feedback=fb) == N_FRAMES
        assert np.array_equal(np.fromfile(out + ".rgb48le", dtype=np.uint8), dr.deliver(job["images"], "rgb48le").reshape(-1))


def test_a_render_without_a_feedback_never_reaches_it(gpu, job, monkeypatch):
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render

    def boom(*a, **kw):
        raise AssertionError("the feedback was reached by a render without one")

    _stand_ins(monkeypatch)
    monkeypatch.setattr(_lib.load(), "maua_feedback_f32", boom)
    monkeypatch.setattr(render, "feedback_frames", boom)
    monkeypatch.setattr(render, "FeedbackOperands", boom)
    for k, (entry, kw) in enumerate(((render.render_shard, {}), (render.render_lensed, {}), (render.render_fed, {}),
                                     (render.render_fed, dict(lens=ar.Lens(vignette=0.3))))):
        out = str(job["tmp"] / f"default{k}.mp4")
        assert entry(*_args(job, out), *TAIL, **kw) == N_FRAMES
        if not kw:
            assert np.array_equal(np.fromfile(out + ".rgb24", dtype=np.uint8), job["rgb"].reshape(-1))


def test_feedback_then_lens_then_grade(gpu, job):
    """The trail is glowed and graded with the picture it belongs to; the state is the un-lensed image (were the lensed image fed back,
    frame 2 on would differ)."""
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render

    fb, name = job["feedbacks"]["per-frame"], "per-frame"
    lens, grade = ar.Lens(bloom=0.8, bloom_size=0.05, bloom_threshold=0.4, vignette=0.3), ar.Grade(offset=0.1, slope=0.9)
    fed = torch.from_numpy(job["emulated"][name][0]).to(gpu)
    ops = render._lens_operands(lens, N_FRAMES, N_FRAMES, fed.device)
    lensed = render.lens_frames(fed.clone(), ops, 0, N_FRAMES, {})
    rows = grade.rows(gpu).expand(N_FRAMES, 24).contiguous()
    want_u8 = render.grade_frames(lensed.clone(), rows, None, {}, out="u8").cpu().numpy()
    want_f32 = render.grade_frames(lensed.clone(), rows, None, {}, out="f32").cpu().numpy()
    out = str(job["tmp"] / "chain.mp4")
    assert _fed_render(*_args(job, out), *TAIL, grade=grade, lens=lens, feedback=fb) == N_FRAMES
    _close(np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(want_u8.shape), want_u8, "feedback + lens + grade")
    assert _fed_render(*_args(job, out), *TAIL, pipe_pix_fmt="yuv420p10le", grade=grade, lens=lens, feedback=fb) == N_FRAMES
    want = dr.deliver(want_f32, "yuv420p10le")
    _close(np.fromfile(out + ".yuv420p10le", dtype="<u2").reshape(N_FRAMES, -1), want.view("<u2"), "feedback + lens + grade, yuv420p10le")
    # lens alone behind the feedback, 8 bits: the quantiser of the lensed image
    assert _fed_render(*_args(job, out), *TAIL, lens=lens, feedback=fb) == N_FRAMES
    _close(np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(N_FRAMES, SIZE, SIZE, 3), gr.quant8(lensed.cpu().numpy()), "feedback + lens")


def test_deep_format_subframes_and_delivery_size(gpu, job):
    from maua_stylegan2_amd import render

    fb = job["feedbacks"]["one-row"]
    e32, u8 = job["emulated"]["one-row"]
    out = str(job["tmp"] / "combo.mp4")
    assert _fed_render(*_args(job, out), *TAIL, pipe_pix_fmt="yuv420p10le", feedback=fb) == N_FRAMES
    _close(np.fromfile(out + ".yuv420p10le", dtype="<u2").reshape(N_FRAMES, -1), dr.deliver(e32, "yuv420p10le").view("<u2"), "yuv420p10le")
    # --subframes 2 at batch 4: the recurrence runs per rendered sub-frame, the fold averages afterwards
    fold = render.TemporalFold(2, "3,1")
    noise = [None if nz is None else nz[:8] for nz in job["noise"]]
    assert _fed_render(job["g"], job["lat"][:8], noise, 0, 4 / 30, 4, SIZE, out, *TAIL, fold=fold, feedback=fb) == 4
    # (the generator's own bits depend on the batch size: the emulation starts from the images of batch-4 lanes)
    images4 = torch.cat([img.clone() for _, img in render.synthesize(job["g"], job["lat"][:8], noise, 4, frames="f32")]).cpu().numpy()
    _close(np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(4, SIZE, SIZE, 3), fold_video_ref(gr.quant8(_emulated(images4, fb)), [3, 1]), "subframes 2")
    # a delivery size: the recurrence runs at the generated size, the resampler afterwards
    resize = render.FrameResize("48x36", "bicubic", "crop")
    assert _fed_render(*_args(job, out), *TAIL, resize=resize, feedback=fb) == N_FRAMES
    got = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(N_FRAMES, 36, 48, 3)
    _close(got, rr.deliver(u8, (48, 36), "bicubic", "crop"), "deliver_size")


def test_a_shard_that_does_not_start_at_frame_zero_is_refused_before_any_file_is_created(gpu, job):
    fb = job["feedbacks"]["one-row"]
    out = str(job["tmp"] / "refused" / "shard.mp4")
    os.makedirs(os.path.dirname(out))
    noise = [None if nz is None else nz[4:] for nz in job["noise"]]
    tail = TAIL[:-1] + ((4, N_FRAMES, N_FRAMES),)
    with pytest.raises(ValueError, match="one rank"):
        _fed_render(job["g"], job["lat"][4:], noise, 0, N_FRAMES / 30, BATCH, SIZE, out, *tail, feedback=fb)
    assert os.listdir(os.path.dirname(out)) == []
    with pytest.raises(ValueError, match=r"5 rows.*\(9\)"):
        import maua_stylegan2_amd.audioreactive as ar

        _fed_render(*_args(job, out), *TAIL, feedback=ar.Feedback(gain=np.full(5, 0.5)))
    assert os.listdir(os.path.dirname(out)) == []


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


def trail(args):
    return ar.Feedback(args.n_frames, gain=0.8, zoom=1 + 0.05 * (np.arange(args.n_frames) % 3 == 1), rotate=3.0 * (np.arange(args.n_frames) % 2),
                       mode="max", border="replicate")
'''


class _Spy:
    """render.feedback_frames with the images that reached it recorded, batch by batch."""

    def __init__(self, mp):
        from maua_stylegan2_amd import render

        self.images, self.firsts, self.feedbacks = [], [], []
        orig = render.feedback_frames

        def spy(images, ops, first, count, scratch):
            self.images.append(images.detach().cpu().numpy().copy())
            self.firsts.append((first, count))
            self.feedbacks.append(ops.feedback)
            return orig(images, ops, first, count, scratch)

        mp.setattr(render, "feedback_frames", spy)

    def expected_u8(self, feedback):
        assert [f for f, _ in self.firsts] == list(np.cumsum([0] + [c for _, c in self.firsts[:-1]]))
        return gr.quant8(_emulated(np.concatenate(self.images), feedback))


def test_generate_with_a_plugins_feedback_and_with_the_cli_flag(gpu, job, tmp_path, monkeypatch):
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import generate_audiovisual as gav

    g = job["g"]
    _stand_ins(monkeypatch)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(ar, "load_audio", lambda audio_file, offset, duration: (np.zeros(4000, np.float32), 8000, 0.5))
    monkeypatch.setattr(gav, "load_generator", lambda **kw: g)
    np.save("lat.npy", seeding.seeded_latents(5, g.n_latent, seed=11).numpy())
    (tmp_path / "plain_plugin.py").write_text(PLUGIN)
    (tmp_path / "override_plugin.py").write_text(PLUGIN + "\nOVERRIDE = dict(feedback=trail)\n")
    (tmp_path / "init_plugin.py").write_text(PLUGIN + "\ndef initialize(args):\n    args.feedback = trail(args)\n    return args\n")

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
    assert plain.shape[0] == 8 and plain.std() > 5 and not spy.images
    trail = ar.Feedback(8, gain=0.8, zoom=1 + 0.05 * (np.arange(8) % 3 == 1), rotate=3.0 * (np.arange(8) % 2), mode="max", border="replicate")
    for name, plugin_file in (("override.mp4", "override_plugin.py"), ("init.mp4", "init_plugin.py")):
        out, spy = run(name, plugin_file)
        got = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(8, SIZE, SIZE, 3)
        assert spy.firsts == [(0, 4), (4, 4)] and all(np.array_equal(f.table, trail.table) and f.mode == "max" for f in spy.feedbacks)
        _close(got, spy.expected_u8(trail), name)
        assert (got[1:] != plain[1:]).mean() > 0.1
    spec = "gain=0.92,zoom=1.015,rotate=0.3,mode=max,border=mirror"
    one = ar.Feedback(gain=0.92, zoom=1.015, rotate=0.3, mode="max", border="mirror")
    out, spy = run("flag.mp4", "plain_plugin.py", "--feedback", spec)
    assert len(spy.feedbacks) == 2 and all(np.array_equal(f.table, one.table) and f.border == "mirror" for f in spy.feedbacks)
    _close(np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(8, SIZE, SIZE, 3), spy.expected_u8(one), "--feedback")
    with pytest.raises(ValueError, match="cannot be combined"):
        run("refused.mp4", "init_plugin.py", "--feedback", "gain=0.5")


def test_the_trails_example_plugin_through_generate(gpu, job, tmp_path, monkeypatch):
    """examples/trails.py on stubbed audio features: a feedback of one row per frame in max mode; the file is the emulated recurrence of
    the images that reached feedback_frames."""
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import generate_audiovisual as gav
    from maua_stylegan2_amd.audioreactive.examples import default
    from maua_stylegan2_amd.audioreactive.examples import trails as plugin

    fps, seconds = 16, 1
    n = fps * seconds
    g = job["g"]
    _stand_ins(monkeypatch)
    monkeypatch.chdir(tmp_path)
    kick = torch.zeros(n)
    kick[[2, 9]] = 1.0

    def fake_initialize(args):
        args.lo_onsets, args.hi_onsets = kick.clone(), torch.zeros(n)
        return args

    monkeypatch.setattr(default, "initialize", fake_initialize)
    monkeypatch.setattr(ar, "onsets", lambda audio, sr, n_frames, **kw: kick.clone())
    monkeypatch.setattr(ar, "rms", lambda audio, sr, n_frames, **kw: torch.linspace(0.1, 1.0, n_frames))
    monkeypatch.setattr(ar, "load_audio", lambda audio_file, offset, duration: (np.zeros(8000, np.float32), 8000, float(seconds)))
    monkeypatch.setattr(gav, "load_generator", lambda **kw: g)
    latents = seeding.seeded_latents(n, g.n_latent, seed=11)
    np.save("lat.npy", latents[:4].numpy())
    random.seed(5), np.random.seed(5), torch.manual_seed(5), torch.cuda.manual_seed_all(5)
    spy = _Spy(monkeypatch)
    out = gav.generate(ckpt=None, audio_file="stub.wav", initialize=plugin.initialize, get_latents=lambda selection, args: latents,
                       get_noise=lambda **kw: None, latent_file="lat.npy", G_res=SIZE, out_size=SIZE, fps=fps, batch=4,
                       output_file=str(tmp_path / "trails.mp4"), args=argparse.Namespace(fps=fps, latent_count=4))
    fb = spy.feedbacks[0]
    assert isinstance(fb, ar.Feedback) and fb.n_rows == n and fb.mode == "max" and all(f is fb for f in spy.feedbacks) and len(spy.firsts) == 4
    assert np.isclose(fb.table[2, 2], 1 + plugin.DRIFT + plugin.KICK_ZOOM) and (np.diff(fb.table[:, 0]) >= 0).all()
    got = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(-1, SIZE, SIZE, 3)
    assert got.shape[0] == n and got.std() > 5
    _close(got, spy.expected_u8(fb), "examples/trails.py")
