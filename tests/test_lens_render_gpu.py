"""GPU: a lens through the render loop — render_lensed, generate() with a plugin's lens, the --lens flag and the shipped examples/glow.py
— on the seeded 64-px generator of tests/test_resample_render_gpu.py: 7 frames at batch 2 are three captured batches and an eager tail
batch of one.  Every file equals the existing conversion twins applied to what render.lens_frames gives for the lanes' fp32 images
(tests/test_lens_gpu.py holds the entries and lens_frames against the definition), bit for bit."""
import argparse
import random

import numpy as np
import pytest
import torch

import deep_ref as dr
import grade_ref as gr
import lens_ref as lr
import resample_ref as rr
from maua_stylegan2_amd import _lib, seeding, sharding
from played_world import PlayedWorld
from temporal_fold_ref import fold_video_ref
from test_resample_render_gpu import BATCH, N_FRAMES, SIZE, TAIL, _assert_file, _stand_ins
from test_yuv420_host import yuv420p_oracle

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
FMTS = ("rgb24", "yuv420p", "yuv420p10le")
ENTRIES = ("maua_lens_extract_f32", "maua_lens_blur_f32", "maua_lens_apply_f32")


def _lensed_render(*args, **kwargs):
    from maua_stylegan2_amd import render

    with pytest.MonkeyPatch.context() as mp:
        _stand_ins(mp)
        return render.render_lensed(*args, **kwargs)


def _lensed(images_dev, lens, first=0):
    """render.lens_frames on a copy of the images -> numpy (the lens's own table decides per frame / one row)."""
    from maua_stylegan2_amd import render

    n = images_dev.shape[0]
    ops = render._lens_operands(lens, n if lens.n_rows == 1 else lens.n_rows, n, images_dev.device)
    return render.lens_frames(images_dev.clone(), ops, first, n, {}).cpu().numpy()


@pytest.fixture(scope="module")
def job(gpu, tmp_path_factory):
    """The seeded generator, the job's inputs, its plain frames and the lanes' fp32 images, two lenses (one row per frame — identity rows, a
    bloom on a reduced map, a sharpen, a vignette — and one row) and what lens_frames gives for them (once, read-only)."""
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render
    from maua_stylegan2_amd.models.stylegan2 import Generator

    g = Generator(SIZE, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(SIZE, seed=4), strict=True)
    g = g.to(gpu).eval()
    lat = seeding.seeded_latents(N_FRAMES, g.n_latent, seed=6)
    noise = seeding.seeded_noise(N_FRAMES, SIZE, seed=7)
    noise[-1] = None
    tmp = tmp_path_factory.mktemp("lens")
    out = str(tmp / "plain.mp4")
    with pytest.MonkeyPatch.context() as mp:
        _stand_ins(mp)
        assert render.render(g, lat, noise, 0, N_FRAMES / 30, BATCH, SIZE, out) == N_FRAMES
    rgb = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(N_FRAMES, SIZE, SIZE, 3)
    images_dev = torch.cat([img.clone() for _, img in render.synthesize(g, lat, noise, BATCH, frames="f32")])
    images = images_dev.cpu().numpy()
    kick = np.array([0.0, 0.9, 0.0, 0.4, 0.7, 0.0, 1.0])
    lenses = {
        "per-frame": ar.Lens(N_FRAMES, bloom=kick, bloom_size=0.15, bloom_threshold=0.45, bloom_knee=0.2, bloom_tint=(1, 0.8, 0.6), sharpen=0.6 * kick,
                             sharpen_radius=1.2, vignette=0.5 * kick),
        "one-row": ar.Lens(bloom=0.7, bloom_size=0.04, bloom_threshold=0.5, sharpen=-0.4, vignette=0.3, vignette_inner=0.3),
    }
    assert list(lenses["per-frame"].identity) == [True, False, True, False, False, True, False] and lenses["one-row"].n_rows == 1
    assert lenses["per-frame"].plan(SIZE, SIZE)[:2] == (2, 15) and lenses["one-row"].plan(SIZE, SIZE)[:2] == (1, 8)
    device = {}
    for name, lens in lenses.items():
        f32 = _lensed(images_dev, lens)
        device[name] = (f32, gr.quant8(f32))
        u8 = render.frames_to_uint8(torch.from_numpy(f32).to(gpu)).cpu().numpy()
        assert np.array_equal(u8, device[name][1])
        # (lens_frames hands the entries what the twin is given: within the chain's allowance of the definition)
        d, rb, bt, rs, st = lens.plan(SIZE, SIZE)
        rows = np.broadcast_to(lens.table, (N_FRAMES, 16)) if lens.n_rows == 1 else lens.table
        bt, st = (np.broadcast_to(t, (N_FRAMES, t.shape[1])) if lens.n_rows == 1 else t for t in (bt, st))
        allow, _ = lr.chain_allowance(images, rows, d, bt, st)
        assert (np.abs(f32.astype(np.float64) - lr.lens(images, rows, d, bt, st, np.float64)) <= allow).all()
    assert np.array_equal(device["per-frame"][0][[0, 2, 5]].view(np.uint32), images[[0, 2, 5]].view(np.uint32))
    assert np.array_equal(device["per-frame"][1][[0, 2, 5]], rgb[[0, 2, 5]]) and (device["per-frame"][1][1] != rgb[1]).mean() > 0.2
    for a in (rgb, images):
        a.setflags(write=False)
    return dict(g=g, lat=lat, noise=noise, rgb=rgb, images=images, images_dev=images_dev, tmp=tmp, lenses=lenses, device=device)


def _converted(fmt, f32, u8):
    """The existing conversion twins on lensed frames: flat bytes per frame."""
    from maua_stylegan2_amd import render

    if fmt in render.DEEP_PIX_FMTS:
        return dr.deliver(f32, fmt)
    if fmt == "yuv420p":
        return yuv420p_oracle(u8)
    return u8.reshape(len(u8), -1)


@pytest.mark.parametrize("fmt", FMTS)
def test_lensed_render_writes_the_twins_of_lens_frames_output(gpu, job, fmt):
    for name in ("per-frame", "one-row"):
        out = str(job["tmp"] / f"{fmt}_{name}.mp4")
        written = _lensed_render(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out, *TAIL, pipe_pix_fmt=fmt, lens=job["lenses"][name])
        assert written == N_FRAMES
        _assert_file(out, fmt, _converted(fmt, *job["device"][name]), (SIZE, SIZE))


def test_an_identity_lens_writes_the_plain_renders_file(gpu, job):
    import maua_stylegan2_amd.audioreactive as ar

    for lens in (ar.Lens(), ar.Lens(N_FRAMES, bloom=np.zeros(N_FRAMES), bloom_size=0.1, sharpen_radius=3.0)):
        assert lens.is_identity
        out = str(job["tmp"] / f"identity{lens.n_rows}.mp4")
        assert _lensed_render(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out, *TAIL, lens=lens) == N_FRAMES
        assert np.array_equal(np.fromfile(out + ".rgb24", dtype=np.uint8), job["rgb"].reshape(-1))
        assert _lensed_render(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out, *TAIL, pipe_pix_fmt="rgb48le", lens=lens) == N_FRAMES
        assert np.array_equal(np.fromfile(out + ".rgb48le", dtype=np.uint8), dr.deliver(job["images"], "rgb48le").reshape(-1))


def test_default_render_never_reaches_the_lens_entries(gpu, job, monkeypatch):
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render

    def boom(*a, **kw):
        raise AssertionError("the lens was reached by a render without one")

    _stand_ins(monkeypatch)
    lib = _lib.load()
    for name in ENTRIES:
        monkeypatch.setattr(lib, name, boom)
    monkeypatch.setattr(render, "lens_frames", boom)
    grade = ar.Grade(exposure=0.3)
    for k, (entry, kw) in enumerate(((render.render_shard, {}), (render.render_graded, {}), (render.render_lensed, {}), (render.render_lensed, dict(grade=grade)))):
        for fmt, ext in ((None, "rgb24"), ("rgb48le", "rgb48le")):
            out = str(job["tmp"] / f"default{k}_{ext}.mp4")
            assert entry(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out, *TAIL, pipe_pix_fmt=fmt, **kw) == N_FRAMES
            if not kw:
                want = job["rgb"].reshape(-1) if fmt is None else dr.deliver(job["images"], "rgb48le").reshape(-1)
                assert np.array_equal(np.fromfile(out + "." + ext, dtype=np.uint8), want)


def test_the_lens_comes_before_the_grade(gpu, job):
    """A bloom and a grade offset do not commute: the glow is extracted from the UNGRADED picture's highlights and graded with it."""
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render

    lens, grade = job["lenses"]["per-frame"], ar.Grade(offset=0.25, slope=0.8)
    rows = grade.rows(gpu).expand(N_FRAMES, 24).contiguous()
    lensed = torch.from_numpy(job["device"]["per-frame"][0]).to(gpu)
    want_u8 = render.grade_frames(lensed.clone(), rows, None, {}, out="u8").cpu().numpy()
    want_f32 = render.grade_frames(lensed.clone(), rows, None, {}, out="f32").cpu().numpy()
    other = gr.quant8(_lensed(render.grade_frames(job["images_dev"].clone(), rows, None, {}, out="f32"), lens))
    assert (other[1] != want_u8[1]).mean() > 0.05 and np.array_equal(other[0], want_u8[0])  # (frame 0's lens row is the identity)
    out = str(job["tmp"] / "both.mp4")
    assert _lensed_render(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out, *TAIL, grade=grade, lens=lens) == N_FRAMES
    _assert_file(out, "rgb24", want_u8.reshape(N_FRAMES, -1), (SIZE, SIZE))
    assert _lensed_render(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out, *TAIL, pipe_pix_fmt="yuv420p10le", grade=grade, lens=lens) == N_FRAMES
    _assert_file(out, "yuv420p10le", dr.deliver(want_f32, "yuv420p10le"), (SIZE, SIZE))


def test_the_lens_is_applied_per_sub_frame_before_the_fold_and_before_the_resampler(gpu, job):
    from maua_stylegan2_amd import render

    lens = job["lenses"]["per-frame"].slice(0, 6)
    u8 = job["device"]["per-frame"][1][:6]
    noise = [None if nz is None else nz[:6] for nz in job["noise"]]
    fold = render.TemporalFold(2, "3,1")
    out = str(job["tmp"] / "fold.mp4")
    assert _lensed_render(job["g"], job["lat"][:6], noise, 0, 3 / 30, BATCH, SIZE, out, *TAIL, fold=fold, lens=lens) == 3
    folded = fold_video_ref(u8, [3, 1])
    assert np.array_equal(np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(3, SIZE, SIZE, 3), folded)
    assert not np.array_equal(folded, fold_video_ref(job["rgb"][:6], [3, 1]))
    # fold, then resize, then the colour conversion: all on lensed sub-frames
    resize = render.FrameResize("48x36", "bicubic", "crop")
    assert _lensed_render(job["g"], job["lat"][:6], noise, 0, 3 / 30, BATCH, SIZE, out, *TAIL, pipe_pix_fmt="yuv420p", fold=fold, resize=resize, lens=lens) == 3
    _assert_file(out, "yuv420p", yuv420p_oracle(rr.deliver(folded, (48, 36), "bicubic", "crop")), (48, 36))
    # a delivery size on a deep format: the lensed fp32 image (the bloom's radius follows ITS height, not the delivery's) -> 16-bit master -> resampler
    resize = render.FrameResize("32x48", "hamming", "crop")
    lens = job["lenses"]["per-frame"]
    assert _lensed_render(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out, *TAIL, pipe_pix_fmt="rgb48le", resize=resize, lens=lens) == N_FRAMES
    master = rr.deliver(dr.frames_to_u16(job["device"]["per-frame"][0]), (32, 48), "hamming", "crop")
    _assert_file(out, "rgb48le", master.reshape(len(master), -1).astype("<u2").view(np.uint8), (32, 48))


def test_two_played_shards_concatenate_to_the_one_rank_file(gpu, job):
    """``_shard = (lo, hi, n)``: every rank holds its block of the per-frame inputs and of the lens (Lens.slice); rank 0's file is the
    one-rank file."""
    lens = job["lenses"]["per-frame"]
    world = PlayedWorld(2)

    def play(rank, final):
        lo, hi = sharding.shard_bounds(N_FRAMES, rank, 2)
        noise = [None if nz is None else nz[lo:hi] for nz in job["noise"]]
        out = str(job["tmp"] / f"rank{rank}_{int(final)}.mp4")
        tail = TAIL[:-1] + ((lo, hi, N_FRAMES),)
        written = _lensed_render(job["g"], job["lat"][lo:hi], noise, 0, N_FRAMES / 30, BATCH, SIZE, out, *tail, lens=lens.slice(lo, hi))
        torch.cuda.synchronize()
        return out, written

    results = world.play(play)
    assert [written for _, written in results] == [N_FRAMES, 0, N_FRAMES]
    _assert_file(results[2][0], "rgb24", _converted("rgb24", *job["device"]["per-frame"]), (SIZE, SIZE))


def test_two_played_shards_with_a_modulated_bloom_size_concatenate_to_the_one_rank_file(gpu, job):
    """bloom_size and sharpen_radius rise through the job, so the two blocks have different maxima of their own: planned alone, rank 0's
    block would take another reduction and other radii than the one-rank job.  Lens.slice keeps the table's plan_max, and the file is the
    one-rank file."""
    import maua_stylegan2_amd.audioreactive as ar

    lens = ar.Lens(N_FRAMES, bloom=0.8, bloom_size=np.linspace(0.02, 0.3, N_FRAMES), bloom_threshold=0.45, bloom_knee=0.2, sharpen=0.5,
                   sharpen_radius=np.linspace(0.4, 2.0, N_FRAMES))
    lo0, hi0 = sharding.shard_bounds(N_FRAMES, 0, 2)
    alone = ar.Lens.from_tables(lens.table[lo0:hi0], lens.bloom_size[lo0:hi0], lens.sharpen_sigma[lo0:hi0]).plan(SIZE, SIZE)
    whole = lens.plan(SIZE, SIZE)
    assert (whole[0], whole[1], whole[3]) == (4, 15, 6) and alone[0] != whole[0] and alone[3] != whole[3]
    assert lens.slice(lo0, hi0).plan(SIZE, SIZE)[:2] == whole[:2]
    f32 = _lensed(job["images_dev"], lens)
    one_rank = str(job["tmp"] / "modulated_one_rank.mp4")
    assert _lensed_render(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, one_rank, *TAIL, lens=lens) == N_FRAMES
    _assert_file(one_rank, "rgb24", gr.quant8(f32).reshape(N_FRAMES, -1), (SIZE, SIZE))
    world = PlayedWorld(2)

    def play(rank, final):
        lo, hi = sharding.shard_bounds(N_FRAMES, rank, 2)
        noise = [None if nz is None else nz[lo:hi] for nz in job["noise"]]
        out = str(job["tmp"] / f"modulated_rank{rank}_{int(final)}.mp4")
        tail = TAIL[:-1] + ((lo, hi, N_FRAMES),)
        written = _lensed_render(job["g"], job["lat"][lo:hi], noise, 0, N_FRAMES / 30, BATCH, SIZE, out, *tail, lens=lens.slice(lo, hi))
        torch.cuda.synchronize()
        return out, written

    results = world.play(play)
    assert [written for _, written in results] == [N_FRAMES, 0, N_FRAMES]
    assert np.array_equal(np.fromfile(results[2][0] + ".rgb24", dtype=np.uint8), np.fromfile(one_rank + ".rgb24", dtype=np.uint8))


def test_a_bloom_too_wide_for_the_frame_is_refused_before_the_first_batch(gpu, job, monkeypatch):
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render

    def boom(*a, **kw):
        raise AssertionError("the sink was opened or a batch was rendered")

    out = str(job["tmp"] / "too_wide.mp4")
    # a lens WITHOUT a bloom is not held to its bloom_size: nothing of the bloom chain would be launched
    assert _lensed_render(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out, *TAIL, lens=ar.Lens(vignette=0.3, bloom_size=5.0)) == N_FRAMES
    monkeypatch.setattr(render, "synthesize", boom)
    monkeypatch.setattr(render, "FrameSink", boom)
    with pytest.raises(ValueError, match=r"radius is \d+ taps.*serves 64"):
        _lensed_render(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out, *TAIL, lens=ar.Lens(bloom=0.5, bloom_size=5.0))


def test_a_table_of_the_wrong_length_is_refused_before_the_first_batch(gpu, job, monkeypatch):
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render

    def boom(*a, **kw):
        raise AssertionError("a batch was rendered")

    monkeypatch.setattr(render, "synthesize", boom)
    out = str(job["tmp"] / "refused.mp4")
    with pytest.raises(ValueError, match=r"5 rows.*\(7\)"):
        _lensed_render(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out, *TAIL, lens=ar.Lens(bloom=np.zeros(5)))
    with pytest.raises(TypeError, match="Lens"):
        _lensed_render(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out, *TAIL, lens="bloom=1")


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


def glow(args):
    return ar.Lens(args.n_frames, bloom=0.9 * (np.arange(args.n_frames) % 2), bloom_size=0.1, bloom_threshold=0.4, vignette=np.linspace(0, 0.4, args.n_frames))
'''


class _Spy:
    """render.lens_frames with its operands recorded: what reached it, batch by batch."""

    def __init__(self, mp):
        from maua_stylegan2_amd import render

        self.images, self.firsts, self.tables = [], [], []
        orig = render.lens_frames

        def spy(images, lens_ops, first, count, scratch):
            self.images.append(images.detach().clone())
            self.firsts.append((first, count))
            self.tables.append(np.array(lens_ops.lens.table))
            return orig(images, lens_ops, first, count, scratch)

        mp.setattr(render, "lens_frames", spy)

    def expected_u8(self, lens):
        """lens_frames with a lens built HERE on everything recorded (the rendered frames in order), quantised by the existing twin."""
        images = torch.cat(self.images)
        assert [f for f, _ in self.firsts] == list(np.cumsum([0] + [c for _, c in self.firsts[:-1]]))
        return gr.quant8(_lensed(images, lens))


def test_generate_with_a_plugins_lens_and_with_the_cli_flag(gpu, job, tmp_path, monkeypatch):
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import generate_audiovisual as gav

    g = job["g"]
    _stand_ins(monkeypatch)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(ar, "load_audio", lambda audio_file, offset, duration: (np.zeros(4000, np.float32), 8000, 0.5))
    monkeypatch.setattr(gav, "load_generator", lambda **kw: g)
    np.save("lat.npy", seeding.seeded_latents(5, g.n_latent, seed=11).numpy())
    (tmp_path / "plain_plugin.py").write_text(PLUGIN)
    (tmp_path / "override_plugin.py").write_text(PLUGIN + "\nOVERRIDE = dict(lens=glow)\n")
    (tmp_path / "init_plugin.py").write_text(PLUGIN + "\ndef initialize(args):\n    args.lens = glow(args)\n    return args\n")

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
    glow = ar.Lens(8, bloom=0.9 * (np.arange(8) % 2), bloom_size=0.1, bloom_threshold=0.4, vignette=np.linspace(0, 0.4, 8))
    for name, plugin_file in (("override.mp4", "override_plugin.py"), ("init.mp4", "init_plugin.py")):
        out, spy = run(name, plugin_file)
        got = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(8, SIZE, SIZE, 3)
        assert spy.firsts == [(0, 4), (4, 4)] and all(np.array_equal(t, glow.table) for t in spy.tables)
        assert np.array_equal(got, spy.expected_u8(glow))
        assert np.array_equal(got[0], plain[0]) and (got[1] != plain[1]).mean() > 0.3  # frame 0's row is the identity
    # the CLI flag alone: a one-row lens; on a deep format; next to a grade (lens first)
    spec = "bloom=0.8,bloom_size=0.03,bloom_threshold=0.6,sharpen=0.4,vignette=0.3"
    one = ar.Lens(bloom=0.8, bloom_size=0.03, bloom_threshold=0.6, sharpen=0.4, vignette=0.3)
    out, spy = run("flag.mp4", "plain_plugin.py", "--lens", spec)
    assert all(np.array_equal(t, one.table) for t in spy.tables) and len(spy.tables) == 2
    assert np.array_equal(np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(8, SIZE, SIZE, 3), spy.expected_u8(one))
    out, spy = run("deep.mp4", "init_plugin.py", "--pipe_pix_fmt", "yuv420p10le")
    lensed = _lensed(torch.cat(spy.images), glow)
    assert np.array_equal(np.fromfile(out + ".yuv420p10le", dtype=np.uint8).reshape(8, -1), dr.deliver(lensed, "yuv420p10le"))
    out, spy = run("graded.mp4", "init_plugin.py", "--grade", "exposure=0.4")
    from maua_stylegan2_amd import render

    rows = ar.Grade(exposure=0.4).rows(gpu).expand(8, 24).contiguous()
    want = render.grade_frames(torch.from_numpy(_lensed(torch.cat(spy.images), glow)).to(gpu), rows, None, {}, out="u8").cpu().numpy()
    assert np.array_equal(np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(8, SIZE, SIZE, 3), want)
    with pytest.raises(ValueError, match="cannot be combined"):
        run("refused.mp4", "init_plugin.py", "--lens", "vignette=0.3")


def test_the_glow_example_plugin_through_generate(gpu, job, tmp_path, monkeypatch):
    """examples/glow.py: the default plugin's latents and noise, a lens of one row per frame from the low onsets and the level; the file is
    lens_frames' output for the images that reached it, and the rows are finite, modulated and inside the plugin's ranges."""
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import generate_audiovisual as gav
    from maua_stylegan2_amd.audioreactive.examples import glow as plugin

    sr, fps, seconds = 22050, 16, 2
    t = np.arange(sr * seconds) / sr
    rng = np.random.default_rng(2)
    kick = np.sin(2 * np.pi * 60 * t) * np.exp(-((t % 0.5) * 12))  # four kicks half a second apart
    chord = sum(np.sin(2 * np.pi * f * t) for f in (261.6, 329.6, 392.0))
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
                           latent_file="lat.npy", G_res=SIZE, out_size=SIZE, fps=fps, batch=4, output_file=str(tmp_path / "glow.mp4"),
                           args=argparse.Namespace(fps=fps, latent_count=12))
    finally:
        ar.set_SMF(before)
    n = fps * seconds
    rows = spy.tables[0]
    assert rows.shape == (n, 16) and all(np.array_equal(t, rows) for t in spy.tables)
    lens = ar.Lens.from_tables(rows, np.full(n, plugin.BLOOM_SIZE), np.full(n, 1.0))
    assert np.allclose(rows[:, 2:5], rows[:, 2:3] * np.array(plugin.BLOOM_TINT) / plugin.BLOOM_TINT[0], atol=1e-6) and (rows[:, 5] == plugin.SHARPEN).all()
    assert (rows[:, 0] == np.float32(0.6)).all() and (rows[:, 1] == np.float32(0.15)).all()
    got = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(-1, SIZE, SIZE, 3)
    assert got.shape[0] == n and np.array_equal(got, spy.expected_u8(lens)) and got.std() > 5
    assert np.isfinite(rows).all() and (rows[:, 2] >= 0).all() and (rows[:, 2] <= plugin.BLOOM + 1e-6).all() and np.ptp(rows[:, 2]) > 0.1
    lo, hi = sorted(plugin.VIGNETTE)
    assert (rows[:, 6] >= lo - 1e-6).all() and (rows[:, 6] <= hi + 1e-6).all() and np.ptp(rows[:, 6]) > 0
