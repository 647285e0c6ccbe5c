"""CPU: the host side of the point and morphological network bends (audioreactive/bend.py: Ablate, Invert, ScalarMultiply,
BinaryThreshold, Erode, Dilate) — names, constructor validation, what the render loop's capturability test sees, and the agreement of
header, binding and library on the two entries (ABI 8).  No device call."""
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO

NAMES = ("Ablate", "Invert", "ScalarMultiply", "BinaryThreshold", "Erode", "Dilate")


def test_the_six_bends_are_exported():
    import maua_stylegan2_amd.audioreactive as ar

    for name in NAMES:
        cls = getattr(ar, name)
        assert issubclass(cls, ar.NetworkBend), name
    assert issubclass(ar.PointBend, torch.nn.Module) and issubclass(ar.MorphBend, torch.nn.Module)


def test_constructor_validation():
    import maua_stylegan2_amd.audioreactive as ar

    n = 6
    for cls in (ar.Erode, ar.Dilate):
        with pytest.raises(ValueError, match="radii"):
            cls(torch.full((n,), 17.0))
        with pytest.raises(ValueError, match="radii"):
            cls(torch.tensor([0.0, 2.0, -1.0]))
        with pytest.raises(ValueError, match="radii"):
            cls(torch.tensor([0.0, float("nan")]))
        cls(torch.tensor([0.0, 16.0, 16.4, 0.4]))  # rounds to 0 .. 16
        with pytest.raises(ValueError, match="sequence"):
            cls(torch.zeros(n, 2))
    for cls in (ar.ScalarMultiply, ar.BinaryThreshold, ar.Ablate):
        with pytest.raises(ValueError, match="sequence"):
            cls(torch.zeros(n, 2))
        with pytest.raises(ValueError, match="sequence"):
            cls(torch.tensor(1.0))
    with pytest.raises(ValueError):
        ar.PointBend("multiply", None, None)
    with pytest.raises(ValueError):
        ar.PointBend("blur", torch.ones(n), None)
    with pytest.raises(ValueError):
        ar.MorphBend("open", torch.ones(n), None)
    with pytest.raises(ValueError, match="whole numbers"):  # MorphBend takes radii, Erode / Dilate round a modulation to them
        ar.MorphBend("dilate", [2.7], None)
    assert ar.MorphBend("dilate", [2, 3], None).table.tolist() == [2, 3] and ar.MorphBend("erode", torch.tensor([1.0]), None).table.dtype == torch.int32
    assert not any(hasattr(ar, name) for name in ("POINT_OPS", "MORPH_OPS", "MAX_RADIUS"))
    # the channel list is checked against a channel count as soon as one is known
    with pytest.raises(RuntimeError, match="channels"):
        ar.PointBend("invert", None, [0, 8], n_channels=8)
    with pytest.raises(RuntimeError, match="channels"):
        ar.MorphBend("dilate", torch.ones(n), torch.tensor([-1]), n_channels=8)
    ar.PointBend("invert", None, [0, 7], n_channels=8)


def test_rounding_and_gating_of_the_modulation():
    import maua_stylegan2_amd.audioreactive as ar

    radii = ar.Dilate(torch.tensor([0.4, 0.6, 2.5, 3.5, 15.7])).sequential.table
    assert radii.dtype == torch.int32 and radii.tolist() == [0, 1, 2, 4, 16]  # torch.round: halves to even
    gate = ar.Ablate(torch.tensor([0.0, 0.5, 0.51, 1.0])).sequential
    assert gate.op == ar.bend._POINT_OPS["multiply"] and gate.table.tolist() == [1.0, 1.0, 0.0, 0.0]
    assert ar.Ablate().sequential.op == ar.bend._POINT_OPS["ablate"] and ar.Ablate().sequential.table is None
    assert ar.Erode(torch.ones(3)).sequential.op == 0 and ar.Dilate(torch.ones(3)).sequential.op == 1


def test_capturable_and_sequence_rows():
    import maua_stylegan2_amd.audioreactive as ar

    n = 9
    env = torch.linspace(0.0, 3.0, n)
    static = [ar.Invert(), ar.Invert(channels=[1, 2]), ar.Ablate(channels=torch.tensor([0]))]
    per_frame = [ar.Ablate(env), ar.ScalarMultiply(env, channels=[0, 3]), ar.BinaryThreshold(env), ar.Erode(env), ar.Dilate(env, channels=[5])]
    for t in static + per_frame:
        assert t.capturable and hasattr(t, "run_static") and hasattr(t.sequential, "run_static"), type(t).__name__
    assert [t.sequence_rows for t in static] == [1, 1, 1]
    assert [t.sequence_rows for t in per_frame] == [n] * 5
    assert ar.ScalarMultiply(env[:1]).sequence_rows == 1


def test_the_render_loop_finds_them_capturable():
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render

    n = 12
    env = torch.linspace(0.0, 2.0, n)
    idx = [0, 2, 4]
    bends = [{"layer": 3, "modulation": env, "transform": lambda m: ar.ScalarMultiply(m, channels=idx)},
             {"layer": 5, "modulation": env, "transform": lambda m: ar.Dilate(m, channels=idx)},
             {"layer": 5, "modulation": env, "transform": lambda m: ar.Erode(m)},
             {"layer": 4, "modulation": env, "transform": lambda m: ar.BinaryThreshold(m, channels=idx)},
             {"layer": 4, "modulation": env, "transform": lambda m: ar.Ablate(m, channels=idx)},
             {"layer": 2, "transform": ar.Invert()},
             {"layer": 1, "transform": ar.Ablate(channels=idx)}]
    seq, ok = render._sequence_bends(bends, n)
    assert ok and len(seq) == len(bends)
    assert [b["layer"] for b in seq] == [3, 5, 5, 4, 4, 2, 1]
    assert [b["transform"].sequence_rows for b in seq] == [n] * 5 + [1, 1]
    assert seq[5]["transform"] is bends[5]["transform"]  # a static module is used as it is
    for bend in bends[:5]:  # a table of another length than the sequence never reaches a captured forward
        assert render._sequence_bends([bend], n + 1) == (None, False)
        assert render._sequence_bends([dict(bend, modulation=env[: n - 2])], n) == (None, False)
    for bend in bends[5:]:
        assert render._sequence_bends([bend], n + 1)[1]


def _header():
    return open(os.path.join(REPO, "include", "maua_hip.h")).read()


def test_header_binding_and_library_agree_on_abi_8(built_lib):
    from maua_stylegan2_amd import _lib
    from maua_stylegan2_amd.audioreactive import bend

    text = _header()
    assert re.search(r"#define\s+MAUA_BEND_MAX_RADIUS\s+16\b", text) and bend._MAX_RADIUS == 16
    assert re.search(r"maua_abi_version\(void\);\s*/\*\s*8:", text)
    assert _lib.ABI_VERSION == 8
    lib = ctypes.CDLL(built_lib)
    lib.maua_abi_version.restype = ctypes.c_int
    assert lib.maua_abi_version() == 8
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("maua_bend_point_f32", 11), ("maua_bend_morph_f32", 12)):
        decl = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)", code)
        assert decl, f"{name} is not declared in include/maua_hip.h"
        assert len(decl.group(1).split(",")) == n_args
        assert name in _lib.exported_symbols() and len(_lib._SIGNATURES[name][1]) == n_args
        assert hasattr(lib, name), f"{name} is not exported by the library"


def test_entries_reject_bad_arguments_without_gpu(built_lib):
    """Argument validation runs before any HIP call."""
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    fake = 0x1000  # never dereferenced: every call below is refused
    fake2 = 0x2000

    def point(x=fake, y=fake2, batch=2, channels=4, hw=16, op=2, param=fake, rows=2, src=None):
        return lib.maua_bend_point_f32(x, y, batch, channels, hw, op, param, rows, None, src, None)

    def morph(x=fake, y=fake2, batch=2, channels=4, h=4, w=4, op=1, radius=fake, rows=2, src=None):
        return lib.maua_bend_morph_f32(x, y, batch, channels, h, w, op, radius, rows, None, src, None)

    assert point(x=None) == -22 and point(y=None) == -22 and point(batch=0) == -22 and point(batch=65) == -22
    assert point(channels=0) == -22 and point(hw=0) == -22 and point(hw=-4) == -22 and point(hw=1 << 29) == -22
    assert point(op=-1) == -22 and point(op=4) == -22
    assert point(op=2, param=None) == -22 and point(op=3, param=None) == -22  # multiply and threshold need their parameter
    assert point(rows=0) == -22 and point(rows=3) == -22                       # without a frame source: one row, or one per sample
    assert morph(x=None) == -22 and morph(y=None) == -22 and morph(radius=None) == -22
    assert morph(y=fake) == -22                                                # in place
    assert morph(batch=0) == -22 and morph(batch=65) == -22 and morph(channels=0) == -22 and morph(h=0) == -22 and morph(w=-1) == -22
    assert morph(op=2) == -22 and morph(op=-1) == -22 and morph(rows=0) == -22 and morph(rows=3) == -22
    assert morph(h=1 << 15, w=1 << 14) == -22                                  # a plane of 2 GiB
