"""CPU: the host side of the padding bend (audioreactive/bend.py: Pad; include/maua_hip.h: maua_bend_pad_f32) — the entry is declared,
bound and exported under the unchanged ABI 8, the class's shape rule and refusals, what the render loop's capturability test sees, and
the pads of the shipped wide plugin.  No device call."""
import argparse
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO

N_ARGS = 15


def test_header_binding_and_library_agree_on_the_entry_under_abi_8(built_lib):
    from maua_stylegan2_amd import _lib

    text = open(os.path.join(REPO, "include", "maua_hip.h")).read()
    assert re.search(r"maua_abi_version\(void\);\s*/\*\s*8:", text) and _lib.ABI_VERSION == 8
    lib = ctypes.CDLL(built_lib)
    lib.maua_abi_version.restype = ctypes.c_int
    assert lib.maua_abi_version() == 8
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+maua_bend_pad_f32\s*\(([^)]*)\)", code)
    assert decl, "maua_bend_pad_f32 is not declared in include/maua_hip.h"
    assert len(decl.group(1).split(",")) == N_ARGS
    assert "maua_bend_pad_f32" in _lib.exported_symbols() and len(_lib._SIGNATURES["maua_bend_pad_f32"][1]) == N_ARGS
    assert hasattr(lib, "maua_bend_pad_f32"), "maua_bend_pad_f32 is not exported by the library"


def test_entry_rejects_bad_arguments_without_gpu(built_lib):
    """Argument validation runs before any HIP call."""
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    fake, fake2 = 0x1000, 0x2000  # never dereferenced: every call below is refused

    def pad(x=fake, y=fake2, batch=2, channels=4, h=4, w=4, pads=(2, 2, 0, 0), mode=1, value=0.0, noise=None, noise_channels=0):
        return lib.maua_bend_pad_f32(x, y, batch, channels, h, w, *pads, mode, value, noise, noise_channels, None)

    assert pad(x=None) == -22 and pad(y=None) == -22 and pad(y=fake) == -22
    assert pad(batch=0) == -22 and pad(batch=65) == -22 and pad(channels=0) == -22 and pad(channels=65536) == -22
    assert pad(h=0) == -22 and pad(w=0) == -22 and pad(w=-3) == -22
    for k in range(4):  # a negative pad, whichever side
        assert pad(pads=tuple(-1 if i == k else 1 for i in range(4))) == -22
    assert pad(mode=-1) == -22 and pad(mode=4) == -22
    for k in range(4):  # reflect: pad >= axis; circular: pad > axis
        assert pad(mode=2, pads=tuple(4 if i == k else 0 for i in range(4))) == -22
        assert pad(mode=3, pads=tuple(5 if i == k else 0 for i in range(4))) == -22
    assert pad(noise=fake, noise_channels=2) == -22 and pad(noise=fake, noise_channels=0) == -22
    assert pad(h=1 << 14, w=1 << 14, pads=(1 << 14, 0, 0, 0)) == -22  # a padded plane of 2 GiB and more


def test_pad_is_exported_with_the_static_bend_protocol():
    import maua_stylegan2_amd.audioreactive as ar

    assert issubclass(ar.Pad, torch.nn.Module)
    p = ar.Pad((2, 2, 0, 0))
    assert p.capturable is True and p.sequence_rows is None and hasattr(p, "run_static") and hasattr(p, "static_shape")
    assert (p.padding, p.mode, p.value, p.noise) == ((2, 2, 0, 0), "replicate", 0.0, None)
    assert not any(hasattr(ar, name) for name in ("PAD_MODES",))


def test_static_shape():
    import maua_stylegan2_amd.audioreactive as ar

    assert ar.Pad((2, 2, 0, 0)).static_shape((8, 512, 4, 4)) == (8, 512, 4, 8)
    assert ar.Pad((0, 0, 2, 2)).static_shape((8, 512, 4, 4)) == (8, 512, 8, 4)
    assert ar.Pad((1, 2, 3, 4), mode="constant", value=-1.0).static_shape(torch.Size((1, 3, 5, 7))) == (1, 3, 12, 10)
    assert ar.Pad((0, 0, 0, 0)).static_shape((2, 2, 1, 1)) == (2, 2, 1, 1)
    assert ar.Pad((3, 3, 3, 3), mode="reflect").static_shape((1, 1, 4, 4)) == (1, 1, 10, 10)     # the limit: pad = axis - 1
    assert ar.Pad((4, 4, 4, 4), mode="circular").static_shape((1, 1, 4, 4)) == (1, 1, 12, 12)    # the limit: pad = axis
    for k in range(4):
        with pytest.raises(RuntimeError, match="reflect"):
            ar.Pad(tuple(4 if i == k else 0 for i in range(4)), mode="reflect").static_shape((1, 1, 4, 4))
        with pytest.raises(RuntimeError, match="circular"):
            ar.Pad(tuple(5 if i == k else 0 for i in range(4)), mode="circular").static_shape((1, 1, 4, 4))
    ar.Pad((40, 0, 0, 9), mode="replicate").static_shape((1, 1, 1, 1))  # replicate and constant have no limit
    ar.Pad((40, 0, 0, 9), mode="constant").static_shape((1, 1, 1, 1))


def test_constructor_refusals():
    import maua_stylegan2_amd.audioreactive as ar

    for padding in ((2, 2), (2, 2, 0, 0, 0), (2, 2, 0, 0.5)):
        with pytest.raises(ValueError, match="padding"):
            ar.Pad(padding)
    for k in range(4):
        with pytest.raises(ValueError, match="negative"):
            ar.Pad(tuple(-1 if i == k else 2 for i in range(4)))
    for mode in ("replication", "zeros", None, 1):
        with pytest.raises(ValueError, match="mode"):
            ar.Pad((2, 2, 0, 0), mode=mode)
    with pytest.raises(ValueError, match="noise"):
        ar.Pad((2, 2, 0, 0), noise=torch.zeros(8))
    with pytest.raises(ValueError, match="noise"):
        ar.Pad((2, 2, 0, 0), noise=torch.zeros(2, 1, 4, 8))  # one static plane, not one per sample
    assert ar.Pad((2, 2, 0, 0), noise=torch.zeros(1, 1, 4, 8)).noise.shape == (1, 4, 8)
    assert ar.Pad((2, 2, 0, 0), noise=torch.zeros(4, 8)).noise.shape == (1, 4, 8)
    assert ar.Pad((2, 2, 0, 0), noise=torch.zeros(1, 5, 4, 8, dtype=torch.float64)).noise.dtype == torch.float32
    assert ar.Pad((2, 2, 0, 0), mode="constant", value=float("-inf")).value == float("-inf")
    with pytest.raises(RuntimeError, match="CUDA"):  # no CPU fallback
        ar.Pad((2, 2, 0, 0))(torch.zeros(1, 2, 4, 4))


def test_the_render_loop_finds_pad_capturable_and_the_torch_pad_not():
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render

    n = 12
    pad = ar.Pad((2, 2, 0, 0))
    seq, ok = render._sequence_bends([{"layer": 0, "transform": pad}], n)
    assert ok and len(seq) == 1 and seq[0]["layer"] == 0 and seq[0]["transform"] is pad
    assert render._sequence_bends([{"layer": 0, "transform": torch.nn.ReplicationPad2d((2, 2, 0, 0))}], n) == (None, False)
    both = torch.nn.Sequential(torch.nn.ReplicationPad2d((2, 2, 0, 0)), ar.AddNoise(torch.zeros(1, 1, 4, 8)))
    assert render._sequence_bends([{"layer": 0, "transform": both}], n) == (None, False)  # no torch module is recognised or translated
    env = torch.linspace(0.0, 2.0, n)
    seq, ok = render._sequence_bends([{"layer": 0, "transform": pad},
                                      {"layer": 3, "modulation": env, "transform": lambda m: ar.ScalarMultiply(m)}], n)
    assert ok and [b["transform"].sequence_rows for b in seq] == [None, n]


def test_manipulation_layer_sizes_the_captured_buffer_with_static_shape():
    """The one line of protocol: under capture the output buffer of a bend has ``static_shape(x.shape)`` where the transform has that
    method and ``x.shape`` otherwise; the eager branch goes through ``forward``."""
    from maua_stylegan2_amd.models.stylegan2 import ManipulationLayer

    asked = []

    class Widen:
        def static_shape(self, shape):
            return shape[:3] + (2 * shape[3],)

        def run_static(self, x, out, src):
            return out

    class Same:
        def run_static(self, x, out, src):
            return out

    def bufs(name, shape):
        asked.append((name, shape))
        return torch.zeros(shape)

    bends = [{"layer": 0, "transform": Widen()}, {"layer": 1, "transform": Widen()}, {"layer": 0, "transform": Same()}]
    out = ManipulationLayer(0).run(torch.zeros(2, 3, 4, 4), bends, bufs, "const", src=object())
    assert asked == [("const.bend0", (2, 3, 4, 8)), ("const.bend2", (2, 3, 4, 8))] and out.shape == (2, 3, 4, 8)


@pytest.mark.parametrize("out_size,pads,plane", [(1920, (2, 2, 0, 0), (4, 8)), (1080, (0, 0, 2, 2), (8, 4))])
def test_wide_plugin_bends(out_size, pads, plane):
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd.audioreactive.examples import default, wide

    assert wide.initialize is default.initialize and wide.get_latents is default.get_latents and wide.get_noise is default.get_noise
    bends = wide.get_bends(argparse.Namespace(out_size=out_size))
    assert len(bends) == 1 and bends[0]["layer"] == 0 and "modulation" not in bends[0]
    t = bends[0]["transform"]
    assert isinstance(t, ar.Pad) and t.padding == pads and t.mode == "replicate"
    assert t.static_shape((8, 512, 4, 4)) == (8, 512) + plane
    assert tuple(t.noise.shape) == (1,) + plane and 0 < float(t.noise.abs().max()) < 0.2
    again = wide.get_bends(argparse.Namespace(out_size=out_size))[0]["transform"]
    assert torch.equal(again.noise, t.noise)  # seeded: the same plane on every rank of a sharded job
    with pytest.raises(ValueError, match="1920 or 1080"):
        wide.get_bends(argparse.Namespace(out_size=1024))
