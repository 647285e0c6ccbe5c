"""CPU: the frame feedback's definition (tests/feedback_ref.py) on known answers, the wrong variants the GPU case list must catch, the
float32 emulation against float64 and the allowance's ceiling, ar.Feedback / the --feedback flag / every refusal, the plumbing that
carries a feedback into generate(), the one-rank refusal, and the launch planner (host code) through ctypes."""
import argparse
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

import feedback_ref as fr

F32, F64 = np.float32, np.float64
BLACK = -1.0


def _frames(n, h, w, fill=BLACK):
    return np.full((n, 3, h, w), fill, F64)


def _rows(n, **kw):
    return np.stack([fr.make_row(**kw)] * n)


# ------------------------------------------------------------------------------------------------------------------ the definition
def test_a_still_trail_halves_exactly_in_unit_space_and_decays_to_black():
    cur = _frames(6, 3, 4)
    cur[0, :, 1, 2] = 1.0  # an impulse of display white on black, then black frames
    rows = _rows(6, gain=0.5, dry=0)
    rows[0] = fr.make_row(gain=0.5, dry=1)  # the impulse itself enters dry
    for T in (F64, F32):
        out, state = fr.run(cur, rows, "add", "zero", dtype=T)
        for k in range(6):
            assert np.array_equal(out[k, :, 1, 2], np.full(3, 2 * 2.0 ** -k - 1, T)), (T, k)  # unit value 2^-k
            assert np.array_equal(np.delete(out[k].reshape(3, -1), 6, axis=1), np.full((3, 11), BLACK, T))
        assert np.array_equal(state, out[-1])
    # under black frames the trail tends to -1 (black), not to 0 (grey): 40 more frames
    long = fr.run(_frames(40, 3, 4), _rows(40, gain=0.5, dry=0), "add", "zero", state=out[-1])[0]
    assert long[-1, 0, 1, 2] < -1 + 1e-9 and (long[:, 0, 1, 2] < 0).all()
    signed = fr.run(cur, rows, "add", "zero", defect="signed decay")[0]
    assert abs(signed[-1, 0, 1, 2]) < 0.1 and abs(signed[-1, 0, 0, 0]) < 0.1  # the wrong variant: everything decays to grey


def test_an_integer_translation_moves_an_impulse_by_whole_pixels():
    cur = _frames(3, 5, 7)
    cur[0, :, 2, 3] = 0.5
    # the inverse matrix: an output pixel reads its source 2 to the left and 1 below: the picture moves 2 right, 1 up per frame
    rows = _rows(3, matrix=(1, 0, -2, 0, 1, 1), gain=1, dry=0)
    rows[0] = fr.make_row(matrix=(1, 0, -2, 0, 1, 1), gain=1, dry=1)
    out = fr.run(cur, rows, "add", "zero")[0]
    for k, (y, x) in enumerate(((2, 3), (1, 5), (0, 7))):
        want = _frames(1, 5, 7)[0]
        if x < 7:
            want[:, y, x] = 0.5
        assert np.array_equal(out[k], want), k  # exactly; the third step leaves the frame
    assert not fr.make_row(matrix=(1, 0, -2, 0, 1, 1))[fr.STILL] and fr.make_row()[fr.STILL] == 1
    # the forward matrix (the wrong variant) moves it the other way
    wrong = fr.run(cur, rows, "add", "zero", defect="forward matrix")[0]
    assert wrong[1, 0, 3, 1] == 0.5 and wrong[1, 0, 1, 5] == BLACK


def test_zoom_two_about_the_centre_of_a_five_by_five_plane():
    prev = np.arange(25, dtype=F64).reshape(5, 5) / 16 - 1
    state = np.stack([prev] * 3)
    m = fr.inverse_matrix(2.0, 0.0, (0, 0), 5, 5)
    assert m == (0.5, -0.0, -0.0, 0.0, 0.5, -0.0)
    row = fr.make_row(matrix=m, gain=1, dry=0)
    out = fr.run(_frames(1, 5, 5), row[None], "add", "zero", state=state)[0][0, 0]
    # output (x, y) reads the source at 2 + (x - 2) / 2: the centre stays, the middle 3 x 3 of the old picture fills the frame
    assert out[2, 2] == prev[2, 2] and out[0, 0] == prev[1, 1] and out[4, 4] == prev[3, 3] and out[0, 4] == prev[1, 3]
    assert out[2, 1] == (prev[2, 1] + prev[2, 2]) / 2 and out[1, 1] == (prev[1, 1] + prev[1, 2] + prev[2, 1] + prev[2, 2]) / 4


def test_every_border_on_a_row_of_four():
    vals = np.array([0.0, 0.25, 0.5, 0.75])
    state = np.stack([vals[None]] * 3)  # [3, 1, 4]

    def sample(shift, border, defect=None, plane=state):
        h, w = plane.shape[1:]
        row = fr.make_row(matrix=(1, 0, shift, 0, 1, 0), gain=1, dry=0)
        return fr.run(_frames(1, h, w), row[None], "add", border, state=plane, defect=defect)[0][0, 0, 0]

    assert np.array_equal(sample(-2, "zero"), [BLACK, BLACK, 0.0, 0.25]) and np.array_equal(sample(2, "zero"), [0.5, 0.75, BLACK, BLACK])
    assert np.array_equal(sample(-2, "replicate"), [0.0, 0.0, 0.0, 0.25]) and np.array_equal(sample(5, "replicate"), [0.75] * 4)
    assert np.array_equal(sample(-2, "wrap"), [0.5, 0.75, 0.0, 0.25]) and np.array_equal(sample(-9, "wrap"), [0.75, 0.0, 0.25, 0.5])
    # mirror: period 2 (n - 1) = 6: ... 2 1 | 0 1 2 3 | 2 1 0 1 ...
    assert np.array_equal(sample(-2, "mirror"), [0.5, 0.25, 0.0, 0.25]) and np.array_equal(sample(2, "mirror"), [0.5, 0.75, 0.5, 0.25])
    assert np.array_equal(sample(6, "mirror"), vals) and not np.array_equal(sample(8, "mirror"), vals)
    # ... the wrong variant repeats the edge: period 2 n = 8
    assert np.array_equal(sample(-2, "mirror", "mirror 2n"), [0.25, 0.0, 0.0, 0.25]) and np.array_equal(sample(8, "mirror", "mirror 2n"), vals)
    # half a pixel: the mean of the neighbours; at the zero border half of the edge and half of black
    assert np.array_equal(sample(0.5, "replicate"), [0.125, 0.375, 0.625, 0.75]) and sample(0.5, "zero")[3] == (0.75 + BLACK) / 2
    assert sample(0.5, "wrap")[3] == (0.75 + 0.0) / 2 and sample(0.5, "mirror")[3] == (0.75 + 0.5) / 2
    # a plane of one element: every border but zero sees it everywhere
    one = np.full((3, 1, 1), 0.5)
    for border in ("replicate", "mirror", "wrap"):
        assert sample(3, border, plane=one)[0] == 0.5 and sample(-0.25, border, plane=one)[0] == 0.5
    assert sample(3, "zero", plane=one)[0] == BLACK and sample(-0.25, "zero", plane=one)[0] == 0.75 * 0.5 + 0.25 * BLACK


def test_max_screen_limit_and_the_neutral_row():
    cur = _frames(1, 1, 2)
    cur[0, :, 0, :] = [0.0, -0.5]  # unit 0.5, 0.25
    state = np.full((3, 1, 2), 0.5)  # unit 0.75
    run = lambda mode, **kw: fr.run(cur, fr.make_row(**kw)[None], mode, "replicate", state=state)[0][0, 0, 0]  # noqa: E731
    assert np.array_equal(run("max", gain=0.5, dry=1), 2 * np.maximum([0.5, 0.25], 0.375) - 1)
    assert np.array_equal(run("screen", gain=0.5, dry=1), 2 * (1 - (1 - np.array([0.5, 0.25])) * (1 - 0.375)) - 1)
    assert np.array_equal(run("screen", gain=2, dry=1), [1.0, 1.0])  # clamp01 of the trail: 1.5 -> 1
    assert np.array_equal(run("add", gain=1, dry=1, tint=(0.5, 1, 1)), 2 * (np.array([0.5, 0.25]) + 0.375) - 1)
    # a diverging add (gain 1, dry 1 on a white frame) is capped by the limit, in unit space
    white = _frames(12, 2, 2, 1.0)
    out = fr.run(white, _rows(12, gain=1, dry=1, limit=4), "add", "zero")[0]
    assert out[0, 0, 0, 0] == 1 and out[2, 0, 0, 0] == 5 and (out[3:] == 2 * 4 - 1).all()
    # neutral: the bits themselves, NaN payloads included; the frame still becomes the next one's state
    x = np.full((2, 3, 2, 2), -1, F32)
    x[0] = 0.25
    x[0, 1].view(np.uint32)[0, 1] = 0x7FC12345
    rows = np.stack([fr.make_row(gain=0, dry=1), fr.make_row(gain=0.5, dry=0)])
    assert fr.is_neutral(rows[0]) and not fr.is_neutral(rows[1]) and not fr.is_neutral(fr.make_row(gain=0, dry=0.5))
    out = fr.run(x, rows, "add", "zero", dtype=F32)[0]
    assert np.array_equal(out[0].view(np.uint32), x[0].view(np.uint32)) and out[0].view(np.uint32)[1, 0, 1] == 0x7FC12345
    assert (out[1, 0] == F32(2 * (0.5 * 0.625) - 1)).all() and (out[1, 2] == out[1, 0]).all()  # (channel 1 holds the NaN)


def test_the_state_is_carried_from_call_to_call():
    cur, rows = fr.case_operands((17, 33), 5, "zoomrot", False)
    whole = fr.run_calls(cur, rows, "add", "mirror")
    assert np.array_equal(fr.run_calls(cur, rows, "add", "mirror", splits=(2,)), whole)
    assert np.array_equal(fr.run_calls(cur, rows, "add", "mirror", splits=(1, 2, 4)), whole)
    lost = fr.run_calls(cur, rows, "add", "mirror", splits=(2,), defect="no carry")
    assert np.array_equal(lost[:2], whole[:2]) and np.abs(lost[2] - whole[2]).max() > 0.1


# ------------------------------------------------------------------------------------------------------------------ wrong variants, allowance
SPLIT = {5: (2,)}  # the GPU tests' state-carry case: two calls of 2 and 3 frames


def _caught(defect):
    """The cases (with mode and border) in which the wrong variant leaves the allowance."""
    hits = []
    for plane, batch, kind, dyadic in fr.cases():
        if plane[0] * plane[1] > 17 * 33 or dyadic:
            continue  # (the small real-operand planes are enough to tell them apart, and quick)
        for mode in fr.MODES:
            for border in fr.BORDERS:
                splits = SPLIT.get(batch)
                _, e64, allow = fr.case_reference(plane, batch, kind, dyadic, mode, border, splits)
                cur, rows = fr.case_operands(plane, batch, kind, dyadic)
                bad = fr.run_calls(cur, rows, mode, border, splits, F64, defect)
                if np.abs(bad - e64).max() > allow:
                    hits.append((plane, batch, kind, mode, border))
    return hits


@pytest.mark.parametrize("defect", fr.DEFECTS)
def test_the_case_list_tells_the_wrong_variant_apart(defect):
    hits = _caught(defect)
    assert hits, defect
    if defect == "mirror 2n":
        assert {h[4] for h in hits} == {"mirror"}
    if defect == "no carry":
        assert {h[1] for h in hits} == {5}  # only a case of more than one call can show it


def test_the_emulation_stays_under_the_derived_ceiling():
    worst = 0.0
    for plane, batch, kind, dyadic in fr.cases():
        if plane[0] * plane[1] > 17 * 33:
            continue
        cur, rows = fr.case_operands(plane, batch, kind, dyadic)
        assert all(float(r[fr.GAIN]) * float(np.abs(r[fr.TINT:fr.TINT + 3]).max()) <= 1 for r in rows)
        for mode in fr.MODES:
            for border in fr.BORDERS:
                e32, e64, allow = fr.case_reference(plane, batch, kind, dyadic, mode, border, SPLIT.get(batch))
                err = float(np.abs(e32.astype(F64) - e64).max())
                top = fr.ceiling(cur, rows, e64)
                assert err <= top, (plane, batch, kind, dyadic, mode, border, err, top)
                assert allow <= max(4 * top, 16 * fr.EPS * max(1.0, float(np.abs(e64).max())))
                if dyadic and batch == 1 and mode != "screen":
                    assert err == 0, (plane, kind, mode, border)  # one frame of sums and power-of-two products: every intermediate is representable
                worst = max(worst, err / top)
    print(f"largest emulation error / ceiling: {worst:.3f}")
    assert worst > 0


# ------------------------------------------------------------------------------------------------------------------ ar.Feedback
def test_feedback_builds_rows_matrices_and_still_flags(built_lib):
    import maua_stylegan2_amd.audioreactive as ar

    n, h, w = 5, 90, 160
    zoom, rot = np.array([1, 1.02, 0.5, 1, 2.0]), np.array([0, 3.0, -90, 0, 0.25])
    tr = np.array([[0, 0], [0.01, -0.02], [0, 0], [0, 0], [0.5, 0.25]])
    gain = torch.tensor([0.9, 0.8, 0.0, 0.5, 1.5])
    fb = ar.Feedback(gain=gain, dry=[1, 0.5, 1, 1, 1], zoom=zoom, rotate=rot, translate=tr, tint=(1, 0.5, 0.25), limit=2.0, mode="max", border="wrap")
    assert fb.n_rows == len(fb) == n and not fb.is_identity and list(fb.neutral) == [False, False, True, False, False]
    assert "5 rows" in repr(fb) and "max" in repr(fb) and "wrap" in repr(fb)
    rows, mode, border = fb.operands(h, w)
    assert rows.dtype == np.float32 and rows.shape == (n, 16) and rows.flags.c_contiguous and (mode, border) == (1, 3)
    assert fb.operands(h, w)[0] is rows and fb.rows(h, w) is rows
    for i in range(n):
        want = fr.inverse_matrix(zoom[i], rot[i], tr[i], h, w)
        assert np.array_equal(rows[i, :6], np.asarray(want, F64).astype(F32)), i
        # the float64 composition: forward map after inverse map is the identity
        th_ = math.radians(rot[i])
        fwd = zoom[i] * np.array([[math.cos(th_), math.sin(th_)], [-math.sin(th_), math.cos(th_)]])
        inv = np.array([[want[0], want[1]], [want[3], want[4]]])
        assert np.allclose(fwd @ inv, np.eye(2), atol=1e-15)
        assert np.allclose(fwd @ np.array([want[2], want[5]]) + tr[i] * (w, h), 0, atol=1e-12)
    assert np.array_equal(rows[:, 6], gain.numpy()) and np.array_equal(rows[:, 7:10], np.tile(F32([1, 0.5, 0.25]), (n, 1)))
    assert np.array_equal(rows[:, 10], F32([1, 0.5, 1, 1, 1])) and (rows[:, 11] == 2).all() and (rows[:, 13:] == 0).all()
    assert list(rows[:, 12]) == [1, 0, 0, 1, 0]  # still: exactly the identity
    # counter-clockwise on the screen: turned by +90 degrees, the pixel right of the centre shows what was below it ... its source
    quarter = ar.Feedback(rotate=90).rows(9, 9)[0]
    assert np.allclose(quarter[:6], (0, -1, 0, 1, 0, 0), atol=1e-7) and quarter[12] == 0
    # zoom > 1 magnifies: the source offset is smaller than the output's
    assert ar.Feedback(zoom=1.25).rows(8, 8)[0, 0] == F32(0.8)
    # translate in fractions of the frame: a quarter of 160 to the right reads 40 to the left
    assert ar.Feedback(translate=(0.25, 0)).rows(90, 160)[0, 2] == -40 and ar.Feedback(translate=(0, -0.1)).rows(90, 160)[0, 5] == 9
    # defaults: one neutral row; sequences as [n, 1]; n_frames alone stays one row
    assert ar.Feedback().is_identity and ar.Feedback().n_rows == 1 and ar.Feedback(7).n_rows == 1 and ar.Feedback(7, gain=0.5).n_rows == 1
    assert ar.Feedback(3, gain=np.ones((3, 1))).n_rows == 3 and ar.Feedback(tint=np.ones((4, 3))).n_rows == 4
    assert ar.FEEDBACK_ROW == 16


def test_feedback_slice_tables_and_gain_for(built_lib):
    import maua_stylegan2_amd.audioreactive as ar

    fb = ar.Feedback(gain=np.linspace(0, 0.9, 6), zoom=np.linspace(1, 1.1, 6), mode="screen", border="mirror")
    part = fb.slice(2, 5)
    assert part.n_rows == 3 and np.array_equal(part.table, fb.table[2:5]) and (part.mode, part.border) == ("screen", "mirror")
    assert np.array_equal(part.rows(32, 48), fb.rows(32, 48)[2:5])
    one = ar.Feedback(gain=0.5)
    assert one.slice(3, 9) is one
    for lo, hi in ((-1, 2), (2, 7), (3, 3), (4, 2)):
        with pytest.raises(ValueError):
            fb.slice(lo, hi)
    again = ar.Feedback.from_tables(fb.table, "screen", "mirror")
    assert np.array_equal(again.rows(20, 30), fb.rows(20, 30)) and again.table.shape == (6, 10)
    for bad in (fb.table[:, :9], -fb.table, fb.table[:0]):
        with pytest.raises(ValueError):
            ar.Feedback.from_tables(bad)
    assert ar.Feedback.gain_for(1.0, 30) == 0.5 ** (1 / 30) and abs(ar.Feedback.gain_for(0.5, 24) ** 12 - 0.5) < 1e-15
    for bad in ((0, 30), (1, 0), (-1, 30), (float("nan"), 30)):
        with pytest.raises(ValueError, match="gain_for"):
            ar.Feedback.gain_for(*bad)


@pytest.mark.parametrize("kwargs, message", [
    (dict(gain=-0.1), "gain must not be negative"),
    (dict(gain=[0.5, -1]), "gain must not be negative"),
    (dict(limit=0), "limit must be positive"),
    (dict(limit=-1), "limit must be positive"),
    (dict(zoom=0), "zoom must be positive"),
    (dict(zoom=[1, -2]), "zoom must be positive"),
    (dict(gain=float("nan")), "non-finite"),
    (dict(rotate=float("inf")), "non-finite"),
    (dict(tint=(1, float("nan"), 1)), "non-finite"),
    (dict(gain=1e39), "overflow float32"),
    (dict(gain=[0.5, 0.6], zoom=[1, 1, 1]), "zoom has 3 entries, gain says 2"),
    (dict(n_frames=4, gain=[0.5, 0.6]), "gain has 2 entries, n_frames says 4"),
    (dict(n_frames=0), "n_frames"),
    (dict(n_frames=2.5), "n_frames"),
    (dict(tint=(1, 1)), "tint of shape"),
    (dict(translate=0.1), "translate of shape"),
    (dict(gain=np.ones((2, 2))), "gain of shape"),
    (dict(mode="multiply"), "unknown mode"),
    (dict(border="clamp"), "unknown border"),
])
def test_feedback_refusals(built_lib, kwargs, message):
    import maua_stylegan2_amd.audioreactive as ar

    with pytest.raises(ValueError, match=message):
        ar.Feedback(**kwargs)


def test_the_feedback_flag_parses_and_resolves(built_lib):
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import generate_audiovisual as gav

    assert [f for f, _ in gav.FEEDBACK_FLAGS] == ["--feedback"]
    assert ar.feedback.SPEC_KEYS == ("gain", "dry", "zoom", "rotate", "translate", "tint", "limit", "mode", "border")
    base = ["--ckpt", "c.pt", "--audio_file", "a.wav"]
    assert gav.build_parser().parse_args(base).feedback_spec is None and gav._feedback_of(gav.build_parser().parse_args(base)) is None
    args = gav.build_parser().parse_args(base + ["--feedback", "gain=0.92,zoom=1.015,rotate=0.3,mode=max,border=mirror"])
    fb = gav._feedback_of(args)
    want = ar.Feedback(gain=0.92, zoom=1.015, rotate=0.3, mode="max", border="mirror")
    assert isinstance(fb, ar.Feedback) and np.array_equal(fb.table, want.table) and (fb.mode, fb.border) == ("max", "mirror")
    assert ar.feedback.parse_spec("tint=1:0.8:0.6, translate=0.01:0 ,dry=0.5") == dict(tint=[1, 0.8, 0.6], translate=[0.01, 0], dry=0.5)
    for bad in ("", "gain", "glare=1", "gain=1,gain=2", "gain=x", "gain=1:2", "tint=1", "translate=1:2:3", "mode=multiply", "border=3"):
        with pytest.raises(ValueError, match="--feedback"):
            ar.feedback.parse_spec(bad)
    # args.feedback: an ar.Feedback, a callable evaluated on the namespace, a string; next to --feedback it is refused
    plugin = ar.Feedback(gain=0.5)
    assert gav._feedback_of(argparse.Namespace(feedback=plugin)) is plugin
    assert gav._feedback_of(argparse.Namespace(feedback=lambda a: ar.Feedback(a.n_frames, gain=np.ones(a.n_frames)), n_frames=4)).n_rows == 4
    assert gav._feedback_of(argparse.Namespace(feedback="gain=0.25,mode=screen")).mode == "screen"
    assert gav._feedback_of(argparse.Namespace(feedback=lambda a: None)) is None
    with pytest.raises(ValueError, match="cannot be combined"):
        gav._feedback_of(argparse.Namespace(feedback=plugin, feedback_spec="gain=1"))
    for bad in (3, lambda a: 3):
        with pytest.raises(TypeError, match="ar.Feedback"):
            gav._feedback_of(argparse.Namespace(feedback=bad))


def test_main_keeps_the_effect_keys_out_of_generates_settings(monkeypatch, tmp_path, built_lib):
    """main() hands generate() its own parameters as keywords; the fold, the delivery and every effect's keys stay in ``args``."""
    from maua_stylegan2_amd import generate_audiovisual as gav

    seen, parameters = [], set(inspect.signature(gav.generate).parameters)
    monkeypatch.setattr(gav, "generate", lambda **kw: seen.append(kw))
    monkeypatch.setattr(gav, "load_plugin", lambda path: ({name: None for name in gav.CALLBACK_NAMES}, {"feedback": "gain=0.5", "lens": None}))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    gav.main(["--ckpt", "c.pt", "--audio_file", "a.wav", "--output_dir", str(tmp_path), "--grade", "hue=3", "--grade_lut", "k.cube", "--lens", "bloom=1",
              "--feedback", "gain=0.9", "--subframes", "2", "--deliver_size", "80x40", "--pipe_pix_fmt", "yuv420p"])
    (kw,) = seen
    kept = ("grade", "grade_spec", "grade_lut", "grade_lut_mix", "lens", "lens_spec", "feedback", "feedback_spec", "subframes", "shutter",
            "shutter_light", "deliver_size", "deliver_filter", "deliver_fit", "pipe_pix_fmt", "mjpeg_quality")
    assert not set(kept) & set(kw) and set(kw) <= parameters
    args = kw["args"]
    assert (kw["ckpt"], kw["audio_file"], kw["batch"]) == ("c.pt", "a.wav", 8)
    assert all(hasattr(args, key) for key in kept if key != "grade")  # (``args.grade`` exists only where a plugin sets it)
    assert (args.grade_spec, args.grade_lut, args.grade_lut_mix, args.lens_spec, args.feedback_spec) == ("hue=3", "k.cube", 1.0, "bloom=1", "gain=0.9")
    assert args.feedback == "gain=0.5" and args.lens is None and (args.subframes, args.deliver_size) == (2, "80x40")
    # ... and a plugin's OVERRIDE that sets ``grade`` reaches ``args``, not generate()
    monkeypatch.setattr(gav, "load_plugin", lambda path: ({name: None for name in gav.CALLBACK_NAMES}, {"grade": "hue=3"}))
    gav.main(["--ckpt", "c.pt", "--audio_file", "a.wav", "--output_dir", str(tmp_path)])
    assert "grade" not in seen[-1] and seen[-1]["args"].grade == "hue=3"


def test_surface_and_dispatch_without_a_feedback(monkeypatch, built_lib):
    from ctypes import c_int, c_void_p

    from maua_stylegan2_amd import _lib
    from maua_stylegan2_amd import generate_audiovisual as gav
    from maua_stylegan2_amd import render

    assert "feedback" not in inspect.signature(gav.generate).parameters
    lensed, fed = inspect.signature(render.render_lensed).parameters, inspect.signature(render.render_fed).parameters
    assert list(fed) == list(lensed) + ["feedback"] and fed["feedback"].default is None
    frames = inspect.signature(render.render_frames).parameters
    assert list(frames) == list(fed) and frames["feedback"].default is None and frames["feedback"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(render.feedback_frames).parameters) == ["images", "ops", "first", "count", "scratch"]
    P, I = c_void_p, c_int
    pinned = {"maua_feedback_f32": [P, P, P, I, I, I, I, P, I, I, I, P], "maua_feedback_plan": [I, I, I, P, I, P, P]}
    for name, argtypes in pinned.items():
        assert _lib._SIGNATURES[name] == (c_int, argtypes), name
    assert set(pinned) <= set(_lib.exported_symbols())
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "maua_hip.h")).read()
    for name in pinned:
        assert f"int {name}(" in header
    # with or without a feedback render_fed is one call of the body, which gets every option by keyword (the other entries and the
    # environment: tests/test_render_entries_host.py)
    seen = []
    args = ("G", "lat", [], 0, 1.0, 8, 512, None, None, 1.0, [], {}, False, "slow", None)
    monkeypatch.setattr(render, "render_frames", lambda *a, **kw: seen.append((a, kw)) or 6)
    none = dict(fold=None, resize=None, grade=None, lens=None, feedback=None)
    assert render.render_fed(*args) == 6 and seen[-1] == (args + (None, None), none)
    assert render.render_fed(*args, "host", "yuv420p", "F", "R", "GR", "L") == 6
    assert seen[-1] == (args + ("host", "yuv420p"), dict(fold="F", resize="R", grade="GR", lens="L", feedback=None))
    assert render.render_fed(*args, lens="L", feedback="FB") == 6 and seen[-1] == (args + (None, None), dict(none, lens="L", feedback="FB"))
    for entry in (render.render_shard, render.render_folded, render.render_delivered, render.render_graded, render.render_lensed):
        assert entry(*args) == 6 and seen[-1][1]["feedback"] is None  # the other entries reach the body without a feedback


def test_a_feedback_is_refused_on_more_than_one_rank_before_the_sink_opens(monkeypatch, tmp_path, built_lib):
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render

    opened = []
    monkeypatch.setattr(render, "FrameSink", lambda *a, **kw: opened.append(a) or (_ for _ in ()).throw(AssertionError("sink opened")))
    monkeypatch.setattr(render, "device_of", lambda g: (_ for _ in ()).throw(AssertionError("past the refusal")))
    fb = ar.Feedback(gain=0.5)
    out = str(tmp_path / "o.mp4")
    lat = torch.zeros(8, 2, 4)
    call = lambda shard: render.render_fed("G", lat, [], 0, 1.0, 4, 512, out, None, 1.0, [], {}, False, "slow", shard, feedback=fb)  # noqa: E731
    monkeypatch.setattr(render.sharding, "rank_world", lambda: (1, 2))
    with pytest.raises(ValueError, match="one rank") as e:
        call(None)
    assert "predecessor" in str(e.value) and "2-rank" in str(e.value)
    monkeypatch.setattr(render.sharding, "rank_world", lambda: (0, 2))
    with pytest.raises(ValueError, match="one rank"):
        call(None)
    # a played shard that does not start at frame 0
    monkeypatch.setattr(render.sharding, "rank_world", lambda: (0, 1))
    with pytest.raises(ValueError, match="starts at frame 8"):
        call((8, 16, 16))
    assert not opened and not os.path.exists(out)
    # rank 0 of 1 with lo == 0 passes the refusal (and reaches the stubbed device_of)
    with pytest.raises(AssertionError, match="past the refusal"):
        call((0, 8, 8))
    with pytest.raises(AssertionError, match="past the refusal"):
        call(None)


def test_render_refuses_a_table_of_the_wrong_length(built_lib):
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render

    ops = render._feedback_operands(ar.Feedback(gain=np.full(8, 0.5)), 8, 4, "cpu")
    assert ops.per_frame and ops.state is None and not ops.state_valid and ops.done is None
    one = render._feedback_operands(ar.Feedback(gain=0.5), 8, 4, "cpu")
    assert not one.per_frame and one.sized(6, 8)[0].shape == (4, 16) and one.sized(6, 8)[0].flags.c_contiguous
    with pytest.raises(ValueError, match="7 rows"):
        render._feedback_operands(ar.Feedback(gain=np.full(7, 0.5)), 8, 4, "cpu")
    with pytest.raises(TypeError, match="Feedback"):
        render._feedback_operands(object(), 8, 4, "cpu")


def test_the_trails_example_builds_a_valid_feedback(monkeypatch, built_lib):
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd.audioreactive.examples import default, trails

    n = 48
    kick = torch.zeros(n)
    kick[[3, 20]] = torch.tensor([1.0, 1.7])
    monkeypatch.setattr(default, "initialize", lambda args: args)
    monkeypatch.setattr(ar, "onsets", lambda audio, sr, n_frames, **kw: kick.clone())
    monkeypatch.setattr(ar, "rms", lambda audio, sr, n_frames, **kw: torch.linspace(0, 1.2, n_frames))
    args = trails.initialize(argparse.Namespace(audio=None, sr=8000, n_frames=n, duration=2.0))
    fb = args.feedback
    assert isinstance(fb, ar.Feedback) and fb.n_rows == n and fb.mode == "max" and not fb.is_identity
    t = fb.table
    assert np.isclose(t[0, 0], ar.Feedback.gain_for(trails.HALF_LIFE[0], 24)) and np.isclose(t[-1, 0], ar.Feedback.gain_for(trails.HALF_LIFE[1], 24))
    assert (np.diff(t[:, 0]) >= 0).all() and (t[:, 0] < 1).all()
    assert np.isclose(t[3, 2], 1 + trails.DRIFT + trails.KICK_ZOOM) and np.isclose(t[20, 2], t[3, 2]) and np.isclose(t[0, 2], 1 + trails.DRIFT)
    assert np.allclose(t[0, 6:9], trails.TINTS[0]) and not np.allclose(t[24, 6:9], trails.TINTS[0]) and (t[:, 6:9] <= 1).all()
    assert not fb.rows(64, 64)[:, 12].any()  # every frame moves


# ------------------------------------------------------------------------------------------------------------------ the planner
@pytest.fixture(scope="module")
def plan_fn(built_lib):
    fn = ctypes.CDLL(built_lib).maua_feedback_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]

    def plan(batch, h, w, rows, img=4096, stride=16):
        out = (ctypes.c_int * 8)()
        rows = None if rows is None else np.ascontiguousarray(rows, F32)
        rc = fn(batch, h, w, None if rows is None else rows.ctypes.data, stride, img, out)
        return rc, list(out)

    return plan


def test_the_planner_counts_launches_without_a_device(plan_fn):
    still, moving = fr.make_row(gain=0.5), fr.make_row(matrix=(1, 0, 1, 0, 1, 0), gain=0.5)
    rc, p = plan_fn(5, 64, 64, np.stack([still] * 5))
    assert rc == 0 and p[:6] == [1, 1, 1, 0b1, 0, 0] and p[6] == 4 and p[7] == 64  # one launch; 64 x 16 items in 4 workgroups
    rc, p = plan_fn(5, 64, 64, np.stack([moving] * 5))
    assert rc == 0 and p[:6] == [5, 0, 1, 0, 0, 0]
    rc, p = plan_fn(5, 64, 64, None)  # rows unknown: every frame counts as moving
    assert rc == 0 and p[:6] == [5, 0, 1, 0, 0, 0]
    rc, p = plan_fn(5, 64, 64, np.stack([still, still, moving, still, still]))
    assert rc == 0 and p[:6] == [3, 2, 1, 0b101, 0, 0]
    rc, p = plan_fn(5, 64, 64, np.stack([moving, still, moving, moving, still]))
    assert rc == 0 and p[:6] == [5, 2, 1, 0b10010, 0, 0]
    # a flag on a matrix that is not the identity is not believed; an identity without the flag takes the warp path
    liar = fr.make_row(matrix=(1, 0, 1, 0, 1, 0), gain=0.5, still=1)
    shy = fr.make_row(gain=0.5, still=0)
    assert plan_fn(3, 8, 8, np.stack([liar] * 3))[1][:2] == [3, 0] and plan_fn(3, 8, 8, np.stack([shy] * 3))[1][:2] == [3, 0]
    # a run longer than 64 frames is split; a wider row stride is honoured
    assert plan_fn(130, 4, 4, np.stack([still] * 130))[1][:2] == [3, 3]
    wide = np.zeros((4, 20), F32)
    wide[:, :16] = np.stack([still, moving, still, still])
    assert plan_fn(4, 4, 4, wide, stride=20)[1][:4] == [3, 2, 1, 0b101]
    # one moving frame may be followed by the copy of its result to the state
    assert plan_fn(1, 8, 8, moving[None])[1][:6] == [1, 0, 1, 0, 0, 1] and plan_fn(1, 8, 8, still[None])[1][:6] == [1, 1, 1, 1, 0, 0]
    # the scalar instance exactly when w % 4 != 0 or the pointer is skewed
    for w, img, vec in ((64, 4096, 1), (68, 4096, 1), (63, 4096, 0), (66, 4096, 0), (64, 4100, 0), (64, 4104, 0), (64, 4112, 1)):
        assert plan_fn(2, 8, w, None, img=img)[1][2] == vec, (w, img)
    # the grid: at most 2048 workgroups of 256 lanes
    assert plan_fn(1, 1024, 1024, None)[1][6] == 1024 and plan_fn(1, 2048, 2048, None)[1][6] == 2048 and plan_fn(1, 600, 600, None, img=4100)[1][6] == 1407
    for bad in ((0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, 0)):
        assert plan_fn(*bad, None)[0] == -22
    assert plan_fn(1, 4, 4, None, stride=15)[0] == -22 and plan_fn(1, 4, 4, None, img=None)[0] == -22
    assert plan_fn(1, 65536, 32768, None)[0] == -38
