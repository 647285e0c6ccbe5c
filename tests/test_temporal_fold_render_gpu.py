"""GPU: temporal supersampling through the render loop — render_folded / render() with the three environment variables / generate() on the
seeded 64-px generator against the host-side fold (tests/temporal_fold_ref.py) of the plain render of the same rendered frames: 4
sub-frames per delivered frame, 7 delivered frames, batch 8 = 28 rendered frames in three captured batches and an eager tail of one group."""
import argparse
import os

import numpy as np
import pytest
import torch

from maua_stylegan2_amd import seeding
from played_world import PlayedWorld
from temporal_fold_ref import fold_video_ref
from test_yuv420_host import yuv420p_oracle

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SUB, N_OUT, BATCH, SIZE = 4, 7, 8, 64
N_RENDERED = SUB * N_OUT
ENV = ("MAUA_SUBFRAMES", "MAUA_SHUTTER", "MAUA_SHUTTER_LIGHT")
TAIL = (None, 1.0, [], {}, False, "slow", None)  # audio_file .. _shard of render_shard's parameter list


def _stand_ins(mp):
    """render() only knows the reference's output sizes, 512 and up: the size table is stood in for (as tests/test_yuv420_gpu.py does), and
    the sink writes its fallback file whatever the box has installed."""
    from maua_stylegan2_amd import render

    mp.setattr(render, "_output_dims", lambda out_size: (SIZE, SIZE))
    mp.setattr(render.shutil, "which", lambda name: None)
    for name in ENV + ("MAUA_PIPE_PIX_FMT",):
        mp.delenv(name, raising=False)


def _folded(*args, **kwargs):
    from maua_stylegan2_amd import render

    with pytest.MonkeyPatch.context() as mp:
        _stand_ins(mp)
        return render.render_folded(*args, **kwargs)


@pytest.fixture(scope="module")
def job(gpu, tmp_path_factory):
    """The seeded generator, the job's inputs and the 28 frames of its plain render (computed once, read-only)."""
    from maua_stylegan2_amd import render
    from maua_stylegan2_amd.models.stylegan2 import Generator

    g = Generator(SIZE, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(SIZE, seed=4), strict=True)
    g = g.to(gpu).eval()
    lat = seeding.seeded_latents(N_RENDERED, g.n_latent, seed=6)
    noise = seeding.seeded_noise(N_RENDERED, SIZE, seed=7)
    noise[-1] = None
    tmp = tmp_path_factory.mktemp("fold")
    out = str(tmp / "plain.mp4")
    with pytest.MonkeyPatch.context() as mp:
        _stand_ins(mp)
        assert render.render(g, lat, noise, 0, N_OUT / 30, BATCH, SIZE, out) == N_RENDERED  # no fold: every rendered frame is delivered
    rgb = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(N_RENDERED, SIZE, SIZE, 3)
    assert rgb.std() > 5
    rgb.setflags(write=False)
    return g, lat, noise, rgb, tmp


def _delivered(path, ext=".rgb24"):
    return np.fromfile(path + ext, dtype=np.uint8).reshape(N_OUT, -1)


def _assert_delivers(got, want):
    want = want.reshape(N_OUT, -1)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert len({got[i].tobytes() for i in range(N_OUT)}) == N_OUT  # (pairwise distinct: the order is really checked)


@pytest.mark.parametrize("shutter,light", [("box", "encoded"), ("tent", "linear")])
def test_render_folded_writes_the_fold_of_the_plain_render(gpu, job, shutter, light):
    from maua_stylegan2_amd import render

    g, lat, noise, rgb, tmp = job
    fold = render.TemporalFold(SUB, shutter, light)
    out = str(tmp / f"{shutter}_{light}.mp4")
    assert _folded(g, lat, noise, 0, N_OUT / 30, BATCH, SIZE, out, *TAIL, fold=fold) == N_OUT  # delivered frames are what is counted
    assert os.path.getsize(out + ".rgb24") == N_OUT * SIZE * SIZE * 3
    want = fold_video_ref(rgb, list(fold.weights), light)
    _assert_delivers(_delivered(out), want)
    assert not np.array_equal(want, rgb[::SUB]) and not np.array_equal(want, fold_video_ref(rgb, [1, 0, 0, 1], light))


def test_render_takes_the_fold_from_the_environment(gpu, job, monkeypatch):
    from maua_stylegan2_amd import render

    g, lat, noise, rgb, tmp = job
    _stand_ins(monkeypatch)
    monkeypatch.setenv("MAUA_SUBFRAMES", str(SUB))
    monkeypatch.setenv("MAUA_SHUTTER", "3,1,0,2")
    monkeypatch.setenv("MAUA_SHUTTER_LIGHT", "linear")
    out = str(tmp / "env.mp4")
    assert render.render(g, lat, noise, 0, N_OUT / 30, BATCH, SIZE, out) == N_OUT
    _assert_delivers(_delivered(out), fold_video_ref(rgb, [3, 1, 0, 2], "linear"))
    monkeypatch.setenv("MAUA_SUBFRAMES", "1")  # one sub-frame is the plain render, whatever the shutter says
    out = str(tmp / "env1.mp4")
    assert render.render(g, lat, noise, 0, N_OUT / 30, BATCH, SIZE, out) == N_RENDERED
    assert np.array_equal(np.fromfile(out + ".rgb24", dtype=np.uint8), rgb.reshape(-1))


def test_later_delivery_stages_see_folded_frames(gpu, job):
    """pipe_pix_fmt="yuv420p": the fold runs first, on the generator's own frames; the planar conversion sees 7 frames."""
    from maua_stylegan2_amd import render

    g, lat, noise, rgb, tmp = job
    out = str(tmp / "planar.mp4")
    fold = render.TemporalFold(SUB, "tent")
    assert _folded(g, lat, noise, 0, N_OUT / 30, BATCH, SIZE, out, *TAIL, pipe_pix_fmt="yuv420p", fold=fold) == N_OUT
    assert not os.path.exists(out + ".rgb24")
    _assert_delivers(_delivered(out, ".yuv420p"), yuv420p_oracle(fold_video_ref(rgb, [1, 2, 2, 1])))


def test_two_played_ranks_deliver_the_one_rank_file(gpu, job):
    """Two ranks played one after the other (tests/played_world.py): the job is sharded in delivered frames, 4 + 3 = 16 + 12 rendered; the
    peer's rounds hold batch / N = 2 delivered frames; rank 0's file is the one-rank file."""
    from maua_stylegan2_amd import render

    g, lat, noise, rgb, tmp = job
    fold = render.TemporalFold(SUB, "box", "linear")
    want = fold_video_ref(rgb, [1] * SUB, "linear")
    world = PlayedWorld(2)

    def play(rank, final):
        out = str(tmp / f"rank{rank}_{int(final)}.mp4")
        written = _folded(g, lat, noise, 0, N_OUT / 30, BATCH, SIZE, out, *TAIL, fold=fold)
        torch.cuda.synchronize()
        return out, written

    results = world.play(play)
    assert [written for _, written in results] == [N_OUT, 0, N_OUT]
    rounds = world.rounds[1]
    assert len(rounds) == 2 and all(tuple(r.shape) == (BATCH // SUB, SIZE, SIZE, 3) and r.dtype == torch.uint8 for r in rounds)
    peer = torch.cat(rounds)[:3].cpu().numpy()  # rank 1's block: delivered frames 4, 5, 6 in order
    assert np.array_equal(peer, want[4:])
    _assert_delivers(_delivered(results[2][0]), want)


def test_ragged_batches_and_frame_counts_are_refused_before_any_launch(gpu, job):
    from maua_stylegan2_amd import render

    g, lat, noise, rgb, tmp = job
    fold = render.TemporalFold(SUB)
    calls = []
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(render, "synthesize", lambda *a, **kw: calls.append(a) or iter(()))
        mp.setattr(render, "FrameSink", lambda *a, **kw: calls.append(a))
        with pytest.raises(ValueError, match="--batch 6 is not a multiple of --subframes 4"):
            _folded(g, lat, noise, 0, N_OUT / 30, 6, SIZE, str(tmp / "no.mp4"), *TAIL, fold=fold)
        with pytest.raises(ValueError, match="--batch 16"):
            _folded(g, lat, noise, 0, N_OUT / 30, BATCH, SIZE, str(tmp / "no.mp4"), *TAIL, fold=render.TemporalFold(16))
        with pytest.raises(ValueError, match="whole groups of 4"):
            _folded(g, lat[:26], [None if nz is None else nz[:26] for nz in noise], 0, N_OUT / 30, BATCH, SIZE, str(tmp / "no.mp4"), *TAIL, fold=fold)
    assert calls == [] and not os.path.exists(str(tmp / "no.mp4") + ".rgb24")


def test_generate_with_subframes_is_generate_at_the_sub_frame_rate_folded(gpu, job, tmp_path, monkeypatch):
    """generate(fps=8) with subframes = 2 writes the host-side fold of what generate(fps=16) writes: the same front end (args.fps = 16, the
    same n_frames), 2:1 fewer frames delivered.  Stubbed audio, callbacks that are functions of the frame's time; both runs start from the
    same random generators, as the other generate() tests seed theirs."""
    import random

    from maua_stylegan2_amd import audioreactive as ar
    from maua_stylegan2_amd import generate_audiovisual as gav

    g = job[0]
    _stand_ins(monkeypatch)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(ar, "load_audio", lambda audio_file, offset, duration: (np.zeros(4000, np.float32), 8000, 0.5))
    monkeypatch.setattr(gav, "load_generator", lambda **kw: g)
    np.save("lat.npy", seeding.seeded_latents(5, g.n_latent, seed=11).numpy())
    seen = []

    def get_latents(selection, args):
        seen.append((args.fps, args.n_frames, args.video_fps, args.subframes))
        t = torch.arange(args.n_frames, dtype=torch.float32) / args.fps * 6.0  # keyframes per second
        lo, frac = t.floor().long() % len(selection), (t - t.floor())[:, None, None]
        return selection[lo] * (1 - frac) + selection[(lo + 1) % len(selection)] * frac

    def run(name, fps, **fold):
        random.seed(123), np.random.seed(123), torch.manual_seed(123), torch.cuda.manual_seed_all(123)
        args = argparse.Namespace(fps=fps, latent_count=5, **fold)
        out = gav.generate(ckpt=None, audio_file="stub.wav", get_latents=get_latents, get_noise=lambda **kw: None, latent_file="lat.npy",
                           G_res=SIZE, out_size=SIZE, fps=fps, batch=4, output_file=str(tmp_path / name), args=args)
        return np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(-1, SIZE, SIZE, 3)

    fine = run("fine.mp4", 16, subframes=1)
    folded = run("folded.mp4", 8, subframes=2, shutter="box", shutter_light="encoded")
    assert seen == [(16, 8, 16, 1), (16, 8, 8, 2)]
    assert fine.shape[0] == 8 and folded.shape[0] == 4 and fine.std() > 5
    assert np.array_equal(folded, fold_video_ref(fine, [1, 1]))
    assert len({f.tobytes() for f in folded}) == 4 and not np.array_equal(folded, fine[::2])
    linear = run("linear.mp4", 8, subframes=2, shutter="3,1", shutter_light="linear")
    assert np.array_equal(linear, fold_video_ref(fine, [3, 1], "linear"))
