"""GPU: the coordinate-remap bends inside a render.  A seeded 32-px generator with a per-frame ``ar.Swirl`` on half of the channels of
layer id 3 (8 x 8) and a per-frame ``ar.Displace`` on layer id 5 (16 x 16): the captured forward on three graph lanes equals the eager
per-batch path byte for byte, the frames differ from the unbent render, a frame range renders the same bytes as those frames of the
whole render, and the shipped examples/liquid.py plugin returns capturable bends."""
import argparse

import numpy as np
import pytest
import torch

import remap_ref as rr
from maua_stylegan2_amd import seeding

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SIZE, N, BS, LANES = 32, 14, 4, 3  # 3 graph batches on 3 lanes + an eager tail of 2 frames


@pytest.fixture(scope="module")
def world(gpu):
    from maua_stylegan2_amd.models.stylegan2 import Generator

    g = Generator(SIZE, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(SIZE, seed=60, rgb_gain=0.3), strict=True)
    g = g.to(gpu).eval()
    lat = seeding.seeded_latents(N, g.n_latent, seed=61)
    noise = [torch.from_numpy(seeding.seeded_array(62, f"sq{i}", (N, 1, r, r))) if r <= 16 else None
             for i, r in enumerate(seeding.noise_sizes(SIZE))]
    return g, lat, noise


def bends():
    import maua_stylegan2_amd.audioreactive as ar

    frame = torch.arange(N, dtype=torch.float32)
    half = list(range(0, 512, 2))
    field = torch.from_numpy(rr.field_bank())
    liquid = torch.stack([1.5 + torch.sin(frame / 2.0), 0.35 * frame], 1)  # amplitude in pixels, loop position (wraps past frame 4 of the bank)
    return [{"layer": 3, "modulation": 150.0 * torch.cos(frame / 3.0), "transform": lambda m: ar.Swirl(m, radius=3.0, channels=half)},
            {"layer": 5, "modulation": liquid, "transform": lambda m: ar.Displace(m, field, border="clamp")}]


def render_frames(g, lat, noise, spec, use_graph, frame_range=None, taps=None):
    """uint8 frames [N, SIZE, SIZE, 3] (zeros outside ``frame_range``) and the first frames of the batches that came out of a graph lane."""
    from maua_stylegan2_amd import render

    frames = np.zeros((N, SIZE, SIZE, 3), np.uint8)
    replays = []
    for k, (first, u8) in enumerate(render.synthesize(g, lat, noise, BS, bends=spec, use_graph=use_graph, lanes=LANES, frame_range=frame_range)):
        frames[first: first + u8.shape[0]] = u8.cpu().numpy()
        if taps and u8.shape[0] == BS:
            assert taps[k % len(taps)].u8 is u8, "a full batch must come out of a graph lane"
            replays.append(first)
    return frames, replays


def test_captured_swirl_and_displace_equal_the_eager_path(gpu, world):
    from maua_stylegan2_amd import render

    g, lat, noise = world
    seq, ok = render._sequence_bends([dict(b, modulation=b["modulation"].to(gpu)) for b in bends()], N)
    assert ok and [b["transform"].sequence_rows for b in seq] == [N, N]

    taps = {}
    orig_capture = g.capture_graph

    def capture(batch, lane=0, **kw):  # graphs with bends are per render (not cached on the generator): keep the lanes here
        assert len(kw["bends"]) == 2 and all(hasattr(b["transform"], "run_static") for b in kw["bends"])
        assert [type(b["transform"]).__name__ for b in kw["bends"]] == ["Swirl", "Displace"]
        taps[lane] = orig_capture(batch, lane=lane, **kw)
        return taps[lane]

    g.capture_graph = capture
    try:
        graphed, replays = render_frames(g, lat, noise, bends(), True, taps=taps)
        assert sorted(taps) == [0, 1, 2] and replays == [0, BS, 2 * BS]
        n_captured = len(taps)
        eager, _ = render_frames(g, lat, noise, bends(), False)
        assert len(taps) == n_captured, "use_graph=False must not capture"
        # byte for byte
        assert np.array_equal(graphed, eager)
        # a frame range: two full batches at frame0 = 5 and 9 read their rows through the frame source
        taps.clear()
        part, replays = render_frames(g, lat, noise, bends(), True, frame_range=(5, 13), taps=taps)
        assert replays == [5, 9] and sorted(taps) == [0, 1]
        assert np.array_equal(part[5:13], graphed[5:13]) and not part[:5].any() and not part[13:].any()
    finally:
        g.capture_graph = orig_capture
    # the bends do something, each of them, on every frame
    plain, _ = render_frames(g, lat, noise, [], True)
    assert graphed.std() > 5 and plain.std() > 5
    changed = [float(np.abs(graphed[i].astype(np.int16) - plain[i]).mean()) for i in range(N)]
    print(f"[swirl + displace at 32^2] mean |bent - plain| per frame (grey levels): {min(changed):.2f} .. {max(changed):.2f}")
    assert min(changed) > 0, "every frame must differ from the unbent render"
    for one in bends():
        alone, _ = render_frames(g, lat, noise, [one], True)
        assert not np.array_equal(alone, plain) and not np.array_equal(alone, graphed)


def test_the_liquid_plugin_returns_capturable_bends(gpu, world):
    """examples/liquid.py: ``get_bends`` on stand-in audio features gives three capturable bends whose tables cover the sequence; the 32-px
    generator renders with the two that sit on layers it has, on the graph lanes."""
    from maua_stylegan2_amd import render
    from maua_stylegan2_amd.audioreactive.examples import liquid

    g, lat, noise = world
    t = torch.arange(N, dtype=torch.float32)
    args = argparse.Namespace(n_frames=N, rms=0.5 + 0.5 * torch.sin(t / 4.0), lo_onsets=torch.relu(torch.cos(t)) ** 2,
                              hi_onsets=torch.relu(torch.sin(1.7 * t)) ** 2)
    for name in ("initialize", "get_latents", "get_noise", "get_bends"):
        assert callable(getattr(liquid, name)), name
    np.random.seed(0)  # (the Perlin lattice draws its gradients from numpy's generator)
    spec = liquid.get_bends(args)
    assert [b["layer"] for b in spec] == [liquid.LIQUID_LAYER, liquid.SWIRL_LAYER, liquid.KALEIDOSCOPE_LAYER]
    assert all(b["modulation"].shape[0] == N for b in spec) and tuple(spec[0]["modulation"].shape) == (N, 2)
    seq, ok = render._sequence_bends([dict(b, modulation=b["modulation"].to(gpu)) for b in spec], N)
    assert ok and [type(b["transform"]).__name__ for b in seq] == ["Displace", "Swirl", "Kaleidoscope"]
    assert all(b["transform"].capturable and b["transform"].sequence_rows == N for b in seq)
    field = seq[0]["transform"].sequential.field
    assert tuple(field.shape) == (liquid.FIELD_FRAMES, 2, liquid.FIELD_SIZE, liquid.FIELD_SIZE) and bool(torch.isfinite(field).all())
    position = spec[0]["modulation"][:, 1]
    assert bool((position[1:] > position[:-1]).all()), "the loop position only moves forward"
    usable = [b for b in spec if b["layer"] <= 7]  # layer ids of a 32-px generator: 0 .. 7
    assert len(usable) == 2
    graphed, _ = render_frames(g, lat, noise, usable, True)
    eager, _ = render_frames(g, lat, noise, usable, False)
    plain, _ = render_frames(g, lat, noise, [], True)
    assert np.array_equal(graphed, eager) and not np.array_equal(graphed, plain)
