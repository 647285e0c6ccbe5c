"""GPU: maua_bend_pad_f32 (include/maua_hip.h, csrc/bend_ops.hip) through the C ABI against torch.nn.functional.pad on the CPU (+ the
noise add: one fp32 add, so the result is bit-defined and the comparison is ``torch.equal``).  Every buffer of a call sits between red
zones (tests/redzone.py), every output element must be written, and a second launch must give the same bits.  The shapes are the smallest
at which the kernel has separate code: the 16-byte path (padded width a multiple of 4, aligned rows) and the element path (any other
width, an unaligned output), one thread block and several, a last quad that is cut by the end of the plane.  ``ar.Pad`` on top."""
import pytest
import torch
import torch.nn.functional as F

from maua_stylegan2_amd import seeding
from redzone import Guard

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

MODES = ("constant", "replicate", "reflect", "circular")  # `mode` 0 .. 3 of the entry
INF = float("inf")


def lib():
    from maua_stylegan2_amd import _lib

    return _lib.load()


def stream(dev):
    from maua_stylegan2_amd import _lib

    return _lib.stream_ptr(dev)


def feature_map(shape, tag="x"):
    """Seeded N(0,1) map with zeros of both signs and a few large values."""
    x = torch.from_numpy(seeding.seeded_array(51, f"{tag}{tuple(shape)}", shape)).float()
    flat = x.view(-1)
    flat[::7] = 0.0
    flat[3::14] = -0.0
    flat[5::31] *= 1e6
    return x


def reference(x, pads, mode, value, noise):
    y = F.pad(x, pads, mode="constant", value=value) if mode == "constant" else F.pad(x, pads, mode=mode)
    return y if noise is None else y + noise[None]


def same(got, want):
    """torch.equal, with a NaN equal to a NaN at the same place."""
    if not torch.equal(got.isnan(), want.isnan()):
        return False
    zero = torch.zeros(())
    return torch.equal(torch.where(got.isnan(), zero, got), torch.where(want.isnan(), zero, want))


def call(x, y, pads, mode, value, noise, gpu):
    b, c, h, w = x.shape
    return lib().maua_bend_pad_f32(x.data_ptr(), y.data_ptr(), b, c, h, w, *pads, MODES.index(mode), value,
                                   None if noise is None else noise.data_ptr(), 0 if noise is None else noise.shape[0], stream(gpu))


# (id, shape [B, C, h, w], pads (left, right, top, bottom), mode, fill value, noise channels: 0 none / 1 / "C")
CASES = []
for _mode in MODES:  # the two layer-0 pads of a 2:1 render, every mode (padded widths 8 and 4: the 16-byte path)
    CASES.append((f"{_mode}-landscape", (3, 2, 4, 4), (2, 2, 0, 0), _mode, 0.75, 0))
    CASES.append((f"{_mode}-portrait", (3, 2, 4, 4), (0, 0, 2, 2), _mode, 0.75, 0))
CASES += [
    # widths that leave the 16-byte path, as the issue lists them (padded widths 7 and 6) and with the padded widths it names (8 and 7)
    ("four-unequal-pads-w7", (1, 3, 5, 4), (1, 2, 0, 1), "replicate", 0.0, 0),
    ("four-unequal-pads-w6", (2, 1, 4, 3), (3, 0, 1, 1), "constant", -2.5, 0),
    ("four-unequal-pads-w8", (1, 3, 4, 5), (1, 2, 0, 1), "reflect", 0.0, 0),
    ("four-unequal-pads-w7-circular", (2, 1, 3, 4), (3, 0, 1, 1), "circular", 0.0, 0),
    ("reflect-at-its-limit", (2, 3, 4, 5), (4, 4, 3, 3), "reflect", 0.0, 0),         # pad = axis - 1
    ("circular-at-its-limit", (2, 3, 4, 5), (5, 5, 4, 4), "circular", 0.0, 0),       # pad = axis
    ("one-pixel-replicate", (2, 3, 1, 1), (3, 2, 1, 4), "replicate", 0.0, 0),
    ("one-pixel-constant", (2, 3, 1, 1), (3, 2, 1, 4), "constant", 1.5, 0),
    ("no-pads", (2, 3, 3, 5), (0, 0, 0, 0), "replicate", 0.0, 1),
    ("fill-minus-inf", (1, 2, 4, 4), (2, 2, 1, 0), "constant", -INF, 1),
    ("nan-carried-through", (1, 2, 4, 4), (2, 2, 0, 0), "replicate", 0.0, "C"),
    ("512-channels", (4, 512, 4, 4), (2, 2, 0, 0), "replicate", 0.0, 0),
    ("vector-path-64", (1, 2, 64, 64), (32, 32, 32, 32), "reflect", 0.0, 0),
    ("noise-1-channel", (3, 2, 4, 4), (2, 2, 0, 0), "replicate", 0.0, 1),
    ("noise-C-channels", (3, 5, 4, 4), (2, 2, 0, 0), "replicate", 0.0, "C"),
    ("noise-1-channel-element-path", (2, 3, 5, 4), (1, 2, 0, 1), "circular", 0.0, 1),
    ("noise-C-channels-element-path", (2, 3, 5, 4), (1, 2, 0, 1), "constant", 0.25, "C"),
]


def operands(case):
    name, shape, pads, mode, value, nch = case
    x = feature_map(shape)
    if name == "nan-carried-through":
        x[0, 1, 2, 0] = float("nan")  # a border pixel: replicated into the pad
        x[0, 0, 1, 2] = INF
    b, c, h, w = shape
    oh, ow = h + pads[2] + pads[3], w + pads[0] + pads[1]
    noise = None
    if nch:
        noise = 0.05 * torch.from_numpy(seeding.seeded_array(52, f"noise{name}", (c if nch == "C" else 1, oh, ow))).float()
    return x, noise, (b, c, oh, ow)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_pad_equals_torch_pad(gpu, case):
    name, shape, pads, mode, value, nch = case
    x, noise, out_shape = operands(case)
    want = reference(x, pads, mode, value, noise)
    assert tuple(want.shape) == out_shape
    g = Guard(gpu)
    xd = g.inp(x, "x")
    nd = None if noise is None else g.inp(noise, "noise")
    first, second = g.out(out_shape, "y"), g.out(out_shape, "y2")
    assert call(xd, first, pads, mode, value, nd, gpu) == 0
    assert call(xd, second, pads, mode, value, nd, gpu) == 0
    nonfinite = ("y", "y2") if name in ("fill-minus-inf", "nan-carried-through") else ()
    g.check(written=("y", "y2"), nonfinite_ok=nonfinite)
    assert same(first.cpu(), want), name
    assert torch.equal(first.view(torch.int32), second.view(torch.int32)), "two launches, two results"
    assert torch.equal(xd.cpu().view(torch.int32), x.view(torch.int32)), "the input was written"
    if name == "nan-carried-through":
        got = first.cpu()
        assert int(got.isnan().sum()) == 3 and bool(got[0, 1, 2, :3].isnan().all()) and int(got.isinf().sum()) == 1


def test_output_rows_that_are_not_16_byte_aligned(gpu):
    """A padded width of 8 whose rows start 4 bytes past a 16-byte boundary: the element path, same values."""
    shape, pads = (2, 2, 4, 4), (2, 2, 0, 0)
    x = feature_map(shape)
    noise = 0.05 * torch.from_numpy(seeding.seeded_array(52, "unaligned", (1, 4, 8))).float()
    want = reference(x, pads, "replicate", 0.0, noise)
    g = Guard(gpu)
    xd, nd = g.inp(x, "x"), g.inp(noise, "noise")
    raw = g.out((want.numel() + 1,), "y")
    raw[0] = 0.0  # the float in front of the map belongs to the window, not to the map
    y = raw[1:].view(want.shape)
    assert y.data_ptr() % 16 == 4
    assert call(xd, y, pads, "replicate", 0.0, nd, gpu) == 0
    g.check(written=("y",))
    assert float(raw[0]) == 0.0 and torch.equal(y.cpu(), want)
    # ... and an unaligned noise plane under an aligned output
    nraw = g.inp(torch.cat([torch.zeros(1), noise.reshape(-1)]), "noise1")
    y2 = g.out(want.shape, "y2")
    assert call(xd, y2, pads, "replicate", 0.0, nraw[1:].view(noise.shape), gpu) == 0
    g.check(written=("y", "y2"))
    assert torch.equal(y2.cpu(), want)


REFUSALS = [
    ("negative-left", dict(pads=(-1, 2, 0, 0))),
    ("negative-bottom", dict(pads=(0, 0, 0, -2))),
    ("reflect-pad-equals-axis", dict(pads=(4, 0, 0, 0), mode=2)),
    ("reflect-pad-equals-axis-rows", dict(pads=(0, 0, 0, 4), mode=2)),
    ("circular-pad-above-axis", dict(pads=(0, 5, 0, 0), mode=3)),
    ("circular-pad-above-axis-rows", dict(pads=(0, 0, 5, 0), mode=3)),
    ("unknown-mode", dict(mode=4)),
    ("negative-mode", dict(mode=-1)),
    ("null-input", dict(x=None)),
    ("null-output", dict(y=None)),
    ("empty-batch", dict(batch=0)),
    ("empty-channels", dict(channels=0)),
    ("empty-rows", dict(h=0)),
    ("empty-columns", dict(w=0)),
    ("in-place", dict(y="x")),
    ("noise-of-two-channels", dict(noise_channels=2)),
]


@pytest.mark.parametrize("name,change", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_launch_nothing(gpu, name, change):
    g = Guard(gpu)
    x = g.inp(feature_map((2, 3, 4, 4)), "x")
    noise = g.inp(torch.zeros(1, 12, 12), "noise")
    y = g.out((2, 3, 12, 12), "y")  # room for the largest padded map below
    kw = dict(x=x.data_ptr(), y=y.data_ptr(), batch=2, channels=3, h=4, w=4, pads=(2, 2, 0, 0), mode=1, noise_channels=1)
    kw.update(change)
    if kw["y"] == "x":
        kw["y"] = kw["x"]
    rc = lib().maua_bend_pad_f32(kw["x"], kw["y"], kw["batch"], kw["channels"], kw["h"], kw["w"], *kw["pads"], kw["mode"], 0.0,
                                 noise.data_ptr(), kw["noise_channels"], stream(gpu))
    assert rc == -22
    assert g.untouched("y")
    g.check()


@pytest.mark.parametrize("name", ["reflect-at-its-limit", "noise-C-channels-element-path"])
def test_pad_module_forward_and_run_static(gpu, name):
    import maua_stylegan2_amd.audioreactive as ar

    case = next(c for c in CASES if c[0] == name)
    _, shape, pads, mode, value, _ = case
    x, noise, out_shape = operands(case)
    want = reference(x, pads, mode, value, noise)
    pad = ar.Pad(pads, mode=mode, value=value, noise=None if noise is None else noise[None])
    xd = x.to(gpu)
    got = pad(xd)
    assert tuple(got.shape) == out_shape and torch.equal(got.cpu(), want)
    out = torch.full(out_shape, float("nan"), device=gpu)
    assert pad.run_static(xd, out, None) is out and torch.equal(out.cpu(), want)
    if noise is not None:  # uploaded once per device
        assert len(pad._dev) == 1 and pad._noise_plane(xd, out_shape) is pad._noise_plane(xd, out_shape)
    with pytest.raises(RuntimeError, match="output buffer"):
        pad.run_static(xd, torch.empty(shape, device=gpu), None)


def test_pad_module_names_both_shapes_of_a_noise_mismatch(gpu):
    import maua_stylegan2_amd.audioreactive as ar

    pad = ar.Pad((2, 2, 0, 0), noise=torch.zeros(1, 1, 4, 4))  # the size of the map before the pad
    with pytest.raises(RuntimeError, match=r"\(1, 4, 4\).*\(2, 512, 4, 8\)"):
        pad(torch.zeros(2, 512, 4, 4, device=gpu))
    with pytest.raises(RuntimeError, match=r"\(3, 4, 8\).*\(2, 512, 4, 8\)"):
        ar.Pad((2, 2, 0, 0), noise=torch.zeros(3, 4, 8))(torch.zeros(2, 512, 4, 4, device=gpu))
