"""CPU: what ar.Grade, ar.Lens and ar.Feedback share (audioreactive/frame_table.py) — the one rule of the constructors' arguments on the
table of calls that was recorded before the three copies became one, the empty-sequence refusal, ``tables()`` as the inverse of
``from_table(s)``, ``slice``, the shared broadcast of generate_audiovisual and each module's ``parse_spec``."""
import numpy as np
import pytest
import torch

import maua_stylegan2_amd.audioreactive as ar

ones, zeros = np.ones, np.zeros
CLASSES = {"Grade": ar.Grade, "Lens": ar.Lens, "Feedback": ar.Feedback}

# (class, positional arguments, keyword arguments, rows — or the text a ValueError must hold)
CALLS = [
    ("Grade", (), dict(slope=2), 1),
    ("Grade", (), dict(slope=ones(4)), 4),
    ("Grade", (), dict(slope=ones(3)), 1),  # a triple
    ("Grade", (), dict(slope=ones((3, 1))), 3),
    ("Grade", (), dict(exposure=ones(3)), 3),
    ("Grade", (), dict(exposure=ones((4, 2))), "Grade: exposure of shape"),
    ("Lens", (), dict(bloom_tint=1), "Lens: bloom_tint of shape"),
    ("Lens", (), dict(bloom_tint=ones(4)), "Lens: bloom_tint of shape"),
    ("Lens", (), dict(bloom_tint=ones((4, 3))), 4),
    ("Lens", (), dict(bloom=ones((4, 1))), 4),
    ("Lens", (), dict(bloom=ones((4, 2))), "Lens: bloom of shape"),
    ("Lens", (), dict(bloom=ones((2, 2, 2))), "Lens: bloom of shape"),
    ("Feedback", (), dict(tint=1), "Feedback: tint of shape"),
    ("Feedback", (), dict(translate=(0.1, 0)), 1),
    ("Feedback", (), dict(translate=zeros((5, 2))), 5),
    ("Feedback", (), dict(gain=ones(1)), 1),
    ("Feedback", (), dict(gain=ones((2, 2, 2))), "Feedback: gain of shape"),
    ("Feedback", (), dict(gain=ones(4), dry=ones(5)), "Feedback: dry has 5 entries, gain says 4"),
    ("Lens", (3,), dict(bloom=ones(4)), "Lens: bloom has 4 entries, n_frames says 3"),
    ("Lens", (7,), {}, 1),
] + [(name, (bad,), {}, f"{name}: n_frames") for name in CLASSES for bad in (0, True, 2.5)]


@pytest.mark.parametrize("name, args, kwargs, want", CALLS, ids=[f"{c[0]}{c[1]}-{','.join(c[2])}-{i}" for i, c in enumerate(CALLS)])
def test_what_the_constructors_accept_and_refuse(name, args, kwargs, want):
    if isinstance(want, int):
        made = CLASSES[name](*args, **kwargs)
        assert made.n_rows == len(made) == want and made.table.shape[0] == want and not made.table.flags.writeable
    else:
        with pytest.raises(ValueError) as e:
            CLASSES[name](*args, **kwargs)
        assert want in str(e.value) and str(e.value).startswith(name + ":")


def test_length_agreement_names_the_first_argument_of_the_agreed_length():
    # Grade's matrix joins the agreement last; "other" is the first sequence, or n_frames where that is given
    mats = np.stack([np.eye(3)] * 5)
    with pytest.raises(ValueError, match="Grade: matrix has 5 entries, hue says 4"):
        ar.Grade(hue=zeros(4), bias=zeros((4, 3)), matrix=mats)
    with pytest.raises(ValueError, match="Grade: matrix has 5 entries, n_frames says 4"):
        ar.Grade(4, matrix=mats)
    with pytest.raises(ValueError, match="Grade: bias has 3 entries, exposure says 2"):
        ar.Grade(exposure=zeros(2), slope=ones((2, 3)), bias=zeros((3, 1)))
    assert ar.Grade(5, matrix=mats, hue=torch.zeros(5, 1)).n_rows == 5 and ar.Grade(matrix=np.eye(3)).n_rows == 1
    for shape in ((4, 4), (3,), (2, 2, 3, 3), ()):
        with pytest.raises(ValueError, match="Grade: matrix of shape"):
            ar.Grade(matrix=ones(shape))
    # one row serves every frame, whatever n_frames says
    assert ar.Grade(9, slope=(1, 2, 3)).n_rows == ar.Feedback(9, tint=(1, 1, 1)).n_rows == 1


@pytest.mark.parametrize("name, kwargs", [("Grade", dict(exposure=ones(0))), ("Grade", dict(slope=ones((0, 3)))), ("Grade", dict(matrix=ones((0, 3, 3)))),
                                          ("Lens", dict(bloom=ones(0))), ("Lens", dict(bloom_tint=ones((0, 3)))), ("Feedback", dict(gain=[])),
                                          ("Feedback", dict(translate=ones((0, 2))))])
def test_an_empty_sequence_is_refused_by_name(name, kwargs):
    (argument,) = kwargs
    with pytest.raises(ValueError, match=f"^{name}: {argument} is empty"):
        CLASSES[name](**kwargs)


def _instances():
    lut = np.linspace(0, 1, 3 * 3 * 3 * 3, dtype=np.float32).reshape(3, 3, 3, 3)
    k = np.linspace(0, 1, 6)
    return {
        "Grade": (ar.Grade(exposure=k, slope=(1, 0.9, 0.8), lut=lut, lut_mix=0.5), ar.Grade(hue=20, lut=lut)),
        "Lens": (ar.Lens(bloom=k, bloom_size=0.01 + 0.04 * k, sharpen=0.3, sharpen_radius=0.5 + k), ar.Lens(vignette=0.3, bloom=0.2)),
        "Feedback": (ar.Feedback(gain=0.9 * k, zoom=1 + 0.1 * k, translate=(0.01, 0), mode="screen", border="mirror"), ar.Feedback(gain=0.5, mode="max")),
    }


def _same(a, b):
    assert type(a) is type(b) and len(a.tables()) == len(b.tables())
    for x, y in zip(a.tables(), b.tables()):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes() and x.shape == y.shape
        else:
            assert x == y
    return True


@pytest.mark.parametrize("name", list(CLASSES))
def test_tables_is_the_inverse_of_from_tables(name):
    for x in _instances()[name]:
        again = CLASSES[name].from_tables(*x.tables())
        assert _same(again, x) and again.is_identity == x.is_identity and repr(again) == repr(x)
        assert f"{x.n_rows} row{'s' if x.n_rows > 1 else ''}," in repr(x)
    per_frame, one = _instances()["Grade"]
    assert _same(ar.Grade.from_table(*per_frame.tables()), per_frame) and one.tables()[1] is one.lut
    lens = _instances()["Lens"][0]
    block = lens.slice(0, 2)  # (a block keeps the plan_max of the whole table, through tables() as well)
    assert block.plan_max == lens.plan_max == (0.05, 1.5) and ar.Lens.from_tables(*block.tables()).plan_max == lens.plan_max
    assert ar.Lens.from_tables(*block.tables()[:3]).plan_max != lens.plan_max


@pytest.mark.parametrize("name", list(CLASSES))
def test_slice(name):
    per_frame, one = _instances()[name]
    assert one.slice(3, 9) is one and one.slice(0, 0) is one
    part = per_frame.slice(2, 5)
    assert type(part) is CLASSES[name] and part.n_rows == 3 and np.array_equal(part.table, per_frame.table[2:5])
    for p, w in zip(part.tables(), per_frame.tables()):  # per-row tables are cut, what belongs to the whole table is kept
        if isinstance(w, np.ndarray):
            assert np.array_equal(p, w[2:5] if w.shape[0] == 6 else w)
        else:
            assert p == w
    assert _same(per_frame.slice(0, 6), per_frame)
    for lo, hi in ((-1, 2), (2, 7), (4, 2)):
        with pytest.raises(ValueError, match=f"{name}.slice: .* is not inside the 6 rows"):
            per_frame.slice(lo, hi)
    with pytest.raises(ValueError, match=f"{name}.slice: an empty slice"):
        per_frame.slice(3, 3)


@pytest.mark.parametrize("name", ["Grade", "Lens"])
def test_broadcast_effect_hands_every_rank_its_block(monkeypatch, built_lib, name):
    from maua_stylegan2_amd import generate_audiovisual as gav

    per_frame, one = _instances()[name]
    wire, calls = {}, []

    def broadcast_object(obj):
        calls.append(obj is not None)
        if obj is not None:
            wire["sent"] = obj
        return wire["sent"]

    monkeypatch.setattr(gav.sharding, "broadcast_object", broadcast_object)
    blocks = {}
    for rank, (lo, hi) in enumerate(((0, 4), (4, 6))):
        monkeypatch.setattr(gav.sharding, "rank_world", lambda rank=rank: (rank, 2))
        blocks[rank] = gav._broadcast_effect(name.lower(), per_frame if rank == 0 else None, lo, hi)
        assert _same(blocks[rank], per_frame.slice(lo, hi))
    assert calls == [True, False]  # one object per rank and job
    assert wire["sent"] is not None and len(wire["sent"]) == len(per_frame.tables())
    if name == "Grade":
        assert all(np.array_equal(b.lut, per_frame.lut) for b in blocks.values())
        assert _same(gav._broadcast_grade(None, 4, 6), blocks[1])
    else:
        assert blocks[0].plan_max == blocks[1].plan_max == per_frame.plan_max
        assert _same(gav._broadcast_lens(None, 4, 6), blocks[1])
    empty = gav._broadcast_effect(name.lower(), None, 6, 6)  # a rank without frames: one row, never applied
    assert empty.n_rows == 1 and _same(empty, per_frame.slice(0, 1))
    with pytest.raises(RuntimeError, match=f"the {name.lower()}'s table has 6 rows, this rank renders the frames 4 .. 8"):
        gav._broadcast_effect(name.lower(), None, 4, 8)
    monkeypatch.setattr(gav.sharding, "rank_world", lambda: (0, 2))
    assert _same(gav._broadcast_effect(name.lower(), one, 0, 3), one)
    monkeypatch.setattr(gav.sharding, "rank_world", lambda: (1, 2))
    assert _same(gav._broadcast_effect(name.lower(), None, 3, 6), one)  # a one-row table is kept as it is


def test_parse_spec_of_each_module():
    assert ar.grade.parse_spec(" exposure = 0.5 , bias=0.1:0:-0.1, slope=2,hue=-15,") == {"exposure": 0.5, "bias": [0.1, 0.0, -0.1], "slope": 2.0, "hue": -15.0}
    assert ar.lens.parse_spec("bloom_tint=1:0.8:0.6, bloom=1 ,sharpen_radius=2.5") == {"bloom_tint": [1.0, 0.8, 0.6], "bloom": 1.0, "sharpen_radius": 2.5}
    assert ar.feedback.parse_spec("tint=1:0.8:0.6, translate=0.01:0 ,dry=0.5,mode= max,border=wrap") == {
        "tint": [1.0, 0.8, 0.6], "translate": [0.01, 0.0], "dry": 0.5, "mode": "max", "border": "wrap"}
    assert all(isinstance(v, float) for v in ar.grade.parse_spec("hue=1,slope=2").values())
    refusals = {
        ar.grade: ("--grade", [("brightness=1", "not key=value"), ("exposure", "not key=value"), ("exposure=bright", "not a number"), ("hue=1:2:3", "hue takes one number$"),
                               ("slope=1:2", "one number or three"), ("hue=1,hue=2", "twice"), ("", "no parameter"), (" , ", "no parameter"), ("lut=x.cube", "not key=value")]),
        ar.lens: ("--lens", [("glare=1", "not key=value"), ("bloom", "not key=value"), ("bloom=x", "not a number"), ("bloom=1:2", "bloom takes one number$"),
                             ("bloom_tint=1", "bloom_tint takes three numbers joined by ':'"), ("bloom=1,bloom=2", "twice"), ("", "no parameter")]),
        ar.feedback: ("--feedback", [("glare=1", "not key=value"), ("gain", "not key=value"), ("gain=x", "not a number"), ("gain=1:2", "gain takes one number$"),
                                     ("tint=1", "tint takes three numbers"), ("translate=1:2:3", "translate takes two numbers"), ("gain=1,gain=2", "twice"),
                                     ("mode=multiply", "mode is one of add, max, screen, not 'multiply'"), ("border=3", "border is one of"), ("mode=1:2", "one of"),
                                     ("", "no parameter")]),
    }
    for module, (flag, cases) in refusals.items():
        for text, match in cases:
            with pytest.raises(ValueError, match=match) as e:
                module.parse_spec(text)
            assert str(e.value).startswith(f"{flag} {text!r}")
        # every key of SPEC_KEYS is understood, and named where a key is not
        with pytest.raises(ValueError, match=", ".join(module.SPEC_KEYS)):
            module.parse_spec("nothing=1")


def test_window_picks_the_rows_of_a_batch_and_refuses_what_lies_outside():
    from maua_stylegan2_amd import render

    cpu = torch.device("cpu")
    per_frame = render.GradeOperands(ar.Grade(exposure=np.arange(7.0)), 7, 4, cpu)
    assert per_frame.per_frame and per_frame.grade.n_rows == 7 and tuple(per_frame.rows.shape) == (7, 24)
    assert torch.equal(per_frame.window(per_frame.rows, 4, 3), per_frame.rows[4:7]) and per_frame.window(per_frame.rows, 7, 0).shape[0] == 0
    one = render.GradeOperands(ar.Grade(exposure=1), 7, 4, cpu)
    assert not one.per_frame and tuple(one.rows.shape) == (4, 24)  # the one row repeated to a batch
    assert torch.equal(one.window(one.rows, 4, 3), one.rows[:3]) and torch.equal(one.window(one.rows, 0, 4), one.rows)
    for ops, first, count in ((per_frame, 4, 4), (per_frame, -1, 2), (one, 0, 5)):
        with pytest.raises(RuntimeError, match="are not inside the . rows of the grade"):
            ops.window(ops.rows, first, count)
    # the same window serves the host rows of a feedback
    fb = render.FeedbackOperands(ar.Feedback(gain=np.full(8, 0.5)), 8, 4, cpu)
    rows = fb.sized(6, 8)[0]
    assert fb.window(rows, 4, 4).shape == (4, 16) and np.array_equal(fb.window(rows, 4, 4), rows[4:8]) and fb.sized(6, 8)[0] is rows
    with pytest.raises(RuntimeError, match="rows of the feedback"):
        fb.window(rows, 6, 4)
    # each subclass takes its own class alone, with one row or one per rendered frame
    for cls, name, other, five in ((render.GradeOperands, "Grade", ar.Lens(), ar.Grade(hue=zeros(5))), (render.LensOperands, "Lens", ar.Grade(), ar.Lens(bloom=zeros(5))),
                                   (render.FeedbackOperands, "Feedback", ar.Lens(), ar.Feedback(gain=zeros(5)))):
        with pytest.raises(TypeError, match=f"must be an audioreactive {name}, got {type(other).__name__}"):
            cls(other, 7, 4, cpu)
        with pytest.raises(ValueError, match=f"the {name.lower()}'s table has 5 rows.*one per rendered frame \\(7\\)"):
            cls(five, 7, 4, cpu)
