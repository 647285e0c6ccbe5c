"""Host: what reaches render.render_frames — the one body of the render — from each of its entry points and from generate().

One table: entry x environment x explicit arguments.  Every row asserts the 17 positionals and all five keyword options exactly, so the
table states which entry reads which environment variable, that an explicit argument beats the environment, that options nobody set
arrive as None, that ``mjpeg`` with a quality arrives as ``mjpeg:<q>`` and that a fold of one sub-frame arrives as no fold."""
import argparse
import inspect

import pytest

ARGS = ("G", "lat", ["nz"], 0.5, 2.0, 8, 512, "o.mp4", "a.wav", 1.0, [], {}, False, "slow")  # the reference's 14, in render_shard's order
OPTIONS = ("fold", "resize", "grade", "lens", "feedback")
ENV_NAMES = ("MAUA_PIPE_PIX_FMT", "MAUA_MJPEG_QUALITY", "MAUA_SUBFRAMES", "MAUA_SHUTTER", "MAUA_SHUTTER_LIGHT", "MAUA_DELIVER_SIZE",
             "MAUA_DELIVER_FILTER", "MAUA_DELIVER_FIT")
ENV = {"MAUA_PIPE_PIX_FMT": "yuv420p", "MAUA_SUBFRAMES": "2", "MAUA_SHUTTER": "3,1", "MAUA_DELIVER_SIZE": "64x36", "MAUA_DELIVER_FIT": "stretch"}
ENV_FOLD = (2, (3, 1), "encoded")
ENV_RESIZE = (64, 36, "lanczos", "stretch")


def _described(value):
    """Options compared by value: a TemporalFold / FrameResize built from the environment is a fresh object."""
    from maua_stylegan2_amd import render

    if isinstance(value, render.TemporalFold):
        return (value.subframes, value.weights, value.light)
    return value.key() if isinstance(value, render.FrameResize) else value


@pytest.fixture
def seam(monkeypatch, built_lib):
    """render.render_frames replaced by a recorder; the environment cleared."""
    from maua_stylegan2_amd import render

    seen = []
    monkeypatch.setattr(render, "render_frames", lambda *a, **kw: seen.append((a, {k: _described(v) for k, v in kw.items()})) or 5)
    for name in ENV_NAMES:
        monkeypatch.delenv(name, raising=False)
    return seen


def test_the_body_has_one_parameter_list(built_lib):
    from maua_stylegan2_amd import render

    params = inspect.signature(render.render_frames).parameters
    shard = list(inspect.signature(render.render_shard).parameters)
    assert list(params) == shard + list(OPTIONS) and len(shard) == 17
    assert all(params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default is None for name in OPTIONS)
    assert all(params[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for name in shard)
    assert not hasattr(render, "_render_shard")
    fed = list(inspect.signature(render.render_fed).parameters)
    assert fed == shard + list(OPTIONS)  # the widest entry takes the same names, as ordinary parameters


# entry, which of (fold, resize) it takes from the environment, the options it has a parameter for
ENTRIES = (
    ("render_shard", ("fold", "resize"), ()),
    ("render_folded", ("resize",), ("fold",)),
    ("render_delivered", (), ("fold", "resize")),
    ("render_graded", (), ("fold", "resize", "grade")),
    ("render_lensed", (), ("fold", "resize", "grade", "lens")),
    ("render_fed", (), ("fold", "resize", "grade", "lens", "feedback")),
)


def test_an_entry_passes_17_positionals_and_all_five_options(seam):
    """Every row of the table entry x environment (one test, so that it has one name: the rows are named in the failure message)."""
    for entry, from_env, own in ENTRIES:
        for env_set in (False, True):
            with pytest.MonkeyPatch.context() as mp:
                for name, value in ENV.items() if env_set else ():
                    mp.setenv(name, value)
                try:
                    _check_entry(seam, entry, from_env, own, env_set)
                except AssertionError as exc:
                    raise AssertionError(f"{entry}, environment {'set' if env_set else 'unset'}") from exc


def _check_entry(seam, entry, from_env, own, env_set):
    from maua_stylegan2_amd import render

    fn = getattr(render, entry)
    env_value = {"fold": ENV_FOLD, "resize": ENV_RESIZE}

    def expect(**explicit):
        want = dict.fromkeys(OPTIONS)
        for name in from_env:
            want[name] = env_value[name] if env_set else None
        want.update(explicit)
        return want

    # nothing but the reference's arguments and the shard: options nobody set arrive as None; transport and pipe_pix_fmt as None too
    # (the body resolves $MAUA_PIPE_PIX_FMT itself, for every entry)
    for shard in (None, (0, 3, 6)):
        assert fn(*ARGS, shard) == 5
        assert seam[-1] == (ARGS + (shard, None, None), expect())
    assert fn(*ARGS, None, "host", "mjpeg:80") == 5 and seam[-1] == (ARGS + (None, "host", "mjpeg:80"), expect())
    assert fn(*ARGS, None, pipe_pix_fmt="rgb48le") == 5 and seam[-1] == (ARGS + (None, None, "rgb48le"), expect())
    # every option the entry has a parameter for: the explicit argument arrives, whatever the environment says — None included
    values = {"fold": render.TemporalFold(4, "tent"), "resize": render.FrameResize("48x36", "box", "pad"), "grade": "GR", "lens": "L", "feedback": "FB"}
    for name in own:
        assert fn(*ARGS, None, **{name: values[name]}) == 5
        assert seam[-1] == (ARGS + (None, None, None), expect(**{name: _described(values[name])}))
        assert fn(*ARGS, None, **{name: None}) == 5 and seam[-1][1][name] is None
    everything = {name: values[name] for name in own}
    assert fn(*ARGS, (0, 8, 16), "gather", "yuv420p", *everything.values()) == 5  # ... positionally, in the order of the parameter list
    assert seam[-1] == (ARGS + ((0, 8, 16), "gather", "yuv420p"), expect(**{k: _described(v) for k, v in everything.items()}))
    # a fold of one sub-frame is passed on as it is given: the body counts its sub-frames (_subframes), 1 is the plain render
    if "fold" in own:
        one = render.TemporalFold(1, "box", "linear")
        assert fn(*ARGS, None, fold=one) == 5 and seam[-1][1]["fold"] == (1, (1,), "linear") and render._subframes(one) == 1


@pytest.mark.parametrize("env_set", (False, True), ids=("environment unset", "environment set"))
def test_render_keeps_the_references_parameter_list_and_reads_the_environment(seam, monkeypatch, env_set):
    from maua_stylegan2_amd import render

    if env_set:
        for name, value in ENV.items():
            monkeypatch.setenv(name, value)
    assert list(inspect.signature(render.render).parameters)[-1] == "ffmpeg_preset" and len(inspect.signature(render.render).parameters) == 14
    want = dict.fromkeys(OPTIONS)
    if env_set:
        want.update(fold=ENV_FOLD, resize=ENV_RESIZE)
    assert render.render(*ARGS) == 5 and seam[-1] == (ARGS + (None, None, None), want)
    # the reference's defaults, and its keyword call
    assert render.render("G", "lat", [], 0, 1.0, 8, 512, None) == 5
    assert seam[-1] == (("G", "lat", [], 0, 1.0, 8, 512, None, None, 1.0, [], {}, False, "slow", None, None, None), want)
    keywords = dict(zip(inspect.signature(render.render).parameters, ARGS))
    assert render.render(**keywords) == 5 and seam[-1] == (ARGS + (None, None, None), want)


def test_the_environment_fold_of_one_sub_frame_is_no_fold(seam, monkeypatch):
    from maua_stylegan2_amd import render

    monkeypatch.setenv("MAUA_SUBFRAMES", "1")
    monkeypatch.setenv("MAUA_SHUTTER", "tent")
    assert render.render_shard(*ARGS, None) == 5 and seam[-1][1] == dict.fromkeys(OPTIONS)
    assert render.render(*ARGS) == 5 and seam[-1][1] == dict.fromkeys(OPTIONS)
    monkeypatch.setenv("MAUA_SUBFRAMES", "two")
    with pytest.raises(ValueError, match="MAUA_SUBFRAMES"):
        render.render_shard(*ARGS, None)
    assert render.render_delivered(*ARGS, None) == 5  # (not read, so not refused)


# ------------------------------------------------------------------------------------------------------------------ generate()
def _namespace(**kw):
    return argparse.Namespace(**kw)


# namespace, (grade, lens, feedback), environment set -> (pipe_pix_fmt, fold, resize) as they reach the body
FOLD4 = ("fold4",)  # stands for the TemporalFold(4, "tent") the namespace asks for
NS_RESIZE = (48, 36, "box", "pad")
JOBS = (
    # a job without grade, lens, feedback or --deliver_size: the environment fills what the namespace leaves unset
    (dict(), (None, None, None), False, (None, None, None)),
    (dict(), (None, None, None), True, (None, ENV_FOLD, ENV_RESIZE)),
    (dict(pipe_pix_fmt="rgb24"), (None, None, None), False, (None, None, None)),  # the flag's default is "not set": $MAUA_PIPE_PIX_FMT decides
    (dict(pipe_pix_fmt="rgb24", mjpeg_quality=85), (None, None, None), True, (None, ENV_FOLD, ENV_RESIZE)),
    (dict(pipe_pix_fmt="yuv420p"), (None, None, None), False, ("yuv420p", None, None)),
    (dict(pipe_pix_fmt="yuv420p", mjpeg_quality=85), (None, None, None), True, ("yuv420p", ENV_FOLD, ENV_RESIZE)),
    (dict(pipe_pix_fmt="mjpeg", mjpeg_quality=85), (None, None, None), False, ("mjpeg:85", None, None)),
    (dict(pipe_pix_fmt="mjpeg", mjpeg_quality=90), (None, None, None), True, ("mjpeg:90", ENV_FOLD, ENV_RESIZE)),
    (dict(pipe_pix_fmt="mjpeg"), (None, None, None), False, ("mjpeg", None, None)),
    (dict(subframes=1, shutter="tent", shutter_light="linear"), (None, None, None), False, (None, None, None)),  # one sub-frame: no fold
    (dict(subframes=1, shutter="tent"), (None, None, None), True, (None, ENV_FOLD, ENV_RESIZE)),
    # ... a fold in the namespace beats the environment's, and the format is then passed on as the namespace has it
    (dict(subframes=4, shutter="tent"), (None, None, None), False, (None, FOLD4, None)),
    (dict(subframes=4, shutter="tent", pipe_pix_fmt="rgb24"), (None, None, None), True, ("rgb24", FOLD4, ENV_RESIZE)),
    (dict(subframes=4, shutter="tent", pipe_pix_fmt="mjpeg", mjpeg_quality=80), (None, None, None), True, ("mjpeg:80", FOLD4, ENV_RESIZE)),
    # a --deliver_size, a grade, a lens or a feedback: the namespace alone
    (dict(deliver_size="48x36", deliver_filter="box", deliver_fit="pad"), (None, None, None), True, (None, None, NS_RESIZE)),
    (dict(deliver_size="48x36", deliver_filter="box", deliver_fit="pad", pipe_pix_fmt="rgb24", subframes=4, shutter="tent"), (None, None, None),
     True, ("rgb24", FOLD4, NS_RESIZE)),
    (dict(pipe_pix_fmt="rgb24"), ("GR", None, None), True, ("rgb24", None, None)),
    (dict(pipe_pix_fmt="mjpeg", mjpeg_quality=70), (None, "L", None), True, ("mjpeg:70", None, None)),
    (dict(), (None, None, "FB"), True, (None, None, None)),
    (dict(subframes=4, shutter="tent", deliver_size="48x36", deliver_filter="box", deliver_fit="pad"), ("GR", "L", "FB"), True, (None, FOLD4, NS_RESIZE)),
)


def test_what_generate_takes_from_the_namespace_and_what_from_the_environment(seam):
    """Every row of JOBS (one test, so that it has one name: the row is quoted in the failure message)."""
    from maua_stylegan2_amd import generate_audiovisual as gav

    for namespace, rich, env_set, want in JOBS:
        with pytest.MonkeyPatch.context() as mp:
            for name, value in ENV.items() if env_set else ():
                mp.setenv(name, value)
            args = _namespace(**namespace)
            fold = gav._fold_of(args)
            assert (fold is None) == (namespace.get("subframes", 1) == 1), namespace
            pix_fmt, fold, resize = gav._tail_options(args, fold, *rich)
            described = (pix_fmt, FOLD4 if _described(fold) == (4, (1, 2, 2, 1), "encoded") else _described(fold), _described(resize))
            assert described == want, (namespace, rich, env_set)


def test_generate_makes_one_call_of_the_body(seam, monkeypatch, tmp_path):
    """The 15 positionals (the shard last), the format by keyword and all five options, for a plain job and for one with everything set."""
    import numpy as np
    import torch

    from maua_stylegan2_amd import audioreactive as ar
    from maua_stylegan2_amd import generate_audiovisual as gav

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(ar, "load_audio", lambda audio_file, offset, duration: (np.zeros(8, np.float32), 100, 2.0))
    monkeypatch.setattr(ar, "generate_latents", lambda *a, **kw: torch.zeros(3, 2, 4))
    monkeypatch.setattr(gav, "_cached_generator", lambda *a, **kw: ("G", True))
    monkeypatch.setattr(ar, "set_SMF", lambda v: None)
    common = dict(ckpt=None, audio_file="a.wav", get_latents=lambda selection, args: torch.zeros(args.n_frames, 2, 4), get_noise=lambda **kw: None,
                  fps=4, batch=8, out_size=512, G_res=512)

    def run(**extra):
        args = _namespace(**common, **extra, offset=0, duration=-1, latent_file=None, latent_count=3, noconst=False, latent_dim=4, n_mlp=2,
                          channel_multiplier=2, shuffle_latents=False)
        gav.generate(**common, output_file="o.mp4", args=args)
        return seam[-1]

    a, kw = run()
    assert len(a) == 15 and a[0] == "G" and len(a[1]) == 8 and a[3:9] == (0, 2.0, 8, 512, "o.mp4", "a.wav") and a[9:] == (1.0, [], {}, False, "slow", None)
    assert kw == dict(pipe_pix_fmt=None, fold=None, resize=None, grade=None, lens=None, feedback=None)
    grade, lens, feedback = ar.Grade(offset=0.1), ar.Lens(vignette=0.3), ar.Feedback(gain=0.5)
    a, kw = run(pipe_pix_fmt="mjpeg", mjpeg_quality=77, subframes=2, shutter="3,1", deliver_size="48x36", grade=grade, lens=lens, feedback=feedback)
    assert len(a) == 15 and len(a[1]) == 16 and a[4] == 2.0 and a[-1] is None
    assert kw == dict(pipe_pix_fmt="mjpeg:77", fold=(2, (3, 1), "encoded"), resize=(48, 36, "lanczos", "crop"), grade=grade, lens=lens, feedback=feedback)
