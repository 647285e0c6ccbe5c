"""GPU: every option of the render's tail in ONE render — feedback, lens, grade, temporal fold and delivery size together — on the seeded
64-px generator of tests/test_resample_render_gpu.py: 8 rendered frames at batch 4 are two captured batches on two graph lanes.

Each file is compared bit for bit with the public stage functions called by hand, in the documented order (feedback -> lens -> grade ->
fold -> resize -> colour conversion), on the batches of ``synthesize(..., frames="f32")``: both sides run the same kernels on the same
inputs, so there is no tolerance."""
import numpy as np
import pytest
import torch

from maua_stylegan2_amd import seeding
from test_resample_render_gpu import SIZE, TAIL, _stand_ins

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
N_FRAMES, BATCH = 8, 4
DELIVER = (80, 40)  # even sides, another aspect ratio than the generator's: a padded window


@pytest.fixture(scope="module")
def job(gpu):
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render
    from maua_stylegan2_amd.models.stylegan2 import Generator

    g = Generator(SIZE, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(SIZE, seed=4), strict=True)
    g = g.to(gpu).eval()
    lat = seeding.seeded_latents(N_FRAMES, g.n_latent, seed=6)
    noise = seeding.seeded_noise(N_FRAMES, SIZE, seed=7)
    noise[-1] = None
    kick = np.array([0.0, 0.9, 0.0, 0.0, 0.7, 0.0, 1.0, 0.3])
    # one table per rendered frame each: every stage has to pick the rows of its batch
    feedback = ar.Feedback(N_FRAMES, gain=0.8, zoom=1 + 0.06 * kick, rotate=4.0 * kick, tint=(1.0, 0.9, 0.8), mode="max", border="mirror")
    lens = ar.Lens(N_FRAMES, bloom=0.4 + 0.5 * kick, bloom_size=0.05, bloom_threshold=0.4, sharpen=0.5 * kick, vignette=0.3)
    grade = ar.Grade(N_FRAMES, offset=0.1 * kick, slope=0.9, power=1.1)
    assert not feedback.is_identity and not lens.is_identity and lens.has_bloom and lens.has_sharpen
    return dict(g=g, lat=lat, noise=noise, feedback=feedback, lens=lens, grade=grade, resize=render.FrameResize(DELIVER, "bicubic", "pad"))


def _by_hand(job, deliver, effects=None):
    """The stages called one after the other on every fp32 batch of the lanes; ``deliver(graded batch maker, scratch)`` ends the chain.
    ``effects``: per-frame feedback, lens and grade in place of the job's."""
    from maua_stylegan2_amd import render

    dev = render.device_of(job["g"])
    effects = effects or job
    feedback_ops = render._feedback_operands(effects["feedback"], N_FRAMES, BATCH, dev)
    lens_ops = render._lens_operands(effects["lens"], N_FRAMES, BATCH, dev)
    grade_ops = render.GradeOperands(effects["grade"], N_FRAMES, BATCH, dev)
    rows, lut = grade_ops.rows, grade_ops.lut
    assert grade_ops.per_frame and feedback_ops.per_frame and lens_ops.per_frame and rows.shape[0] == N_FRAMES
    scratch, out = {}, []
    for first, images in render.synthesize(job["g"], job["lat"], job["noise"], BATCH, frames="f32"):
        images, count = images.clone(), images.shape[0]
        images = render.feedback_frames(images, feedback_ops, first, count, scratch)
        images = render.lens_frames(images, lens_ops, first, count, scratch)
        out.append(deliver(lambda kind: render.grade_frames(images, rows[first: first + count], lut, scratch, out=kind), scratch).cpu().numpy().copy())
    assert len(out) == N_FRAMES // BATCH
    return np.concatenate(out)


def _render(job, out, effects=None, **kw):
    from maua_stylegan2_amd import render

    effects = effects or job
    with pytest.MonkeyPatch.context() as mp:
        _stand_ins(mp)
        return render.render_fed(job["g"], job["lat"], job["noise"], 0, N_FRAMES / 30, BATCH, SIZE, out, *TAIL, resize=job["resize"],
                                 grade=effects["grade"], lens=effects["lens"], feedback=effects["feedback"], **kw)


def test_all_five_options_in_one_rgb24_render(gpu, job, tmp_path):
    from maua_stylegan2_amd import render

    fold = render.TemporalFold(2, "3,1")
    want = _by_hand(job, lambda graded, scratch: render.resize_frames(render.fold_frames(graded("u8"), fold, scratch), job["resize"], scratch))
    out = str(tmp_path / "all.mp4")
    assert _render(job, out, fold=fold) == N_FRAMES // 2
    got = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(N_FRAMES // 2, DELIVER[1], DELIVER[0], 3)
    assert want.shape == got.shape and np.array_equal(got, want), int((got != want).sum())
    # (the window of the padded frame holds a picture, the bars left and right of it are black, and the frames differ: the order is checked)
    assert got[:, :, :20].max() == 0 and got[:, :, 60:].max() == 0 and got[:, :, 20:60].std() > 5
    assert len({f.tobytes() for f in got}) == len(got)


def test_feedback_lens_grade_and_delivery_size_in_one_yuv420p10le_render(gpu, job, tmp_path):
    from maua_stylegan2_amd import render

    fmt = "yuv420p10le"
    want = _by_hand(job, lambda graded, scratch: render.frames_to_deep(graded("f32"), SIZE, fmt, scratch, resize=job["resize"]))
    out = str(tmp_path / "deep.mp4")
    assert _render(job, out, pipe_pix_fmt=fmt) == N_FRAMES
    got = np.fromfile(out + "." + fmt, dtype=np.uint8).reshape(N_FRAMES, -1)
    assert want.shape == got.shape == (N_FRAMES, render.deep_frame_bytes(fmt, *DELIVER)) and np.array_equal(got, want), int((got != want).sum())
    assert len({f.tobytes() for f in got}) == len(got)


def test_one_row_tables_are_row_0_repeated_to_every_batch(gpu, job, tmp_path):
    """The three effects as ONE-ROW tables (row 0 of the job's per-frame tables): the render repeats the row to a batch and hands every
    batch — the second starts at ``first = 4`` — its first ``count`` rows.  Compared with the chain by hand on PER-FRAME tables that hold
    row 0 eight times, which picks its rows the other way: [first, first + count)."""
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render

    def rebuilt(effect, pick):  # (the effect's per-row tables through ``pick``; what belongs to the whole table — mode, border — kept)
        tables = effect.tables()
        return type(effect).from_tables(*(pick(t) if isinstance(t, np.ndarray) and t.shape[:1] == (N_FRAMES,) else t for t in tables[:3]))

    names = ("feedback", "lens", "grade")
    one = {k: rebuilt(job[k], lambda t: t[:1]) for k in names}
    repeated = {k: rebuilt(job[k], lambda t: np.repeat(t[:1], N_FRAMES, axis=0)) for k in names}
    assert all(one[k].n_rows == 1 and repeated[k].n_rows == N_FRAMES and not one[k].is_identity for k in names)
    assert isinstance(one["lens"], ar.Lens) and one["lens"].plan_max == repeated["lens"].plan_max
    want = _by_hand(job, lambda graded, scratch: render.resize_frames(graded("u8"), job["resize"], scratch), repeated)
    out = str(tmp_path / "one.mp4")
    assert _render(job, out, one) == N_FRAMES
    got = np.fromfile(out + ".rgb24", dtype=np.uint8).reshape(N_FRAMES, DELIVER[1], DELIVER[0], 3)
    assert want.shape == got.shape and np.array_equal(got, want), int((got != want).sum())
    assert len({f.tobytes() for f in got}) == len(got)
