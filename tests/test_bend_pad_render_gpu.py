"""GPU: 2:1 renders on the graph lanes.  A seeded 32-px generator built for 1920 (1080) output has 2:1 noise buffers; the layer-0
``ar.Pad`` widens its 4 x 4 constant to 4 x 8 (8 x 4) inside the captured forward, a per-frame ``ar.Translate`` scrolls the 16 x 32
(32 x 16) map of layer id 4 as examples/tauceti.py does, and the frames are 32 x 64 (64 x 32).  Captured forward == eager per-batch path
byte for byte == oracle, whose layer 0 is ``Sequential(ReplicationPad2d, AddNoise)`` in torch.  And ``generate()`` with the shipped
examples/wide.py plugin."""
import numpy as np
import pytest
import torch

import wide_seeding
from maua_stylegan2_amd import seeding

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SIZE, N, BS, LANES = 32, 14, 4, 3  # 3 graph batches on 3 lanes + an eager tail of 2 frames


def inputs(out_size, n):
    """Latents, per-frame noise up to the 16-px level (the 32-px level reads the checkpoint's 2:1 buffers), the pad's noise plane, the
    scroll of layer id 4 and its canvas noise."""
    shapes = wide_seeding.noise_shapes(SIZE, out_size)
    lat = seeding.seeded_latents(n, 8, seed=31)
    noise = [torch.from_numpy(seeding.seeded_array(32, f"wide{i}", (n, 1) + hw)) if min(hw) <= 16 else None for i, hw in enumerate(shapes)]
    pads = (2, 2, 0, 0) if out_size == 1920 else (0, 0, 2, 2)
    plane = 0.025 * torch.from_numpy(seeding.seeded_array(33, "pad_noise", (1, 1, 4 + pads[2] + pads[3], 4 + pads[0] + pads[1])))
    h, w = shapes[3]  # layer id 4 = convs.2 = noise slot 3
    shift = torch.stack([torch.linspace(0.0, 1.5 * w, n), torch.zeros(n)], 1)  # scrolls by more than one width: the stacked pads
    canvas = 0.05 * torch.from_numpy(seeding.seeded_array(34, "canvas_noise", (1, 1, h, 5 * w)))
    return lat, noise, pads, plane, (h, w), shift, canvas


def oracle_bends(pads, plane, hw, shift, canvas):
    """{layer id: torch callable} on the frames whose rows of ``shift`` are given; ``plane`` / ``shift`` None: without that part."""
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd.audioreactive import bend
    from oracle import signal_oracle

    h, w = hw
    layer0 = torch.nn.ReplicationPad2d(pads) if plane is None else torch.nn.Sequential(torch.nn.ReplicationPad2d(pads), ar.AddNoise(plane))
    if shift is None:
        return {0: layer0}

    def translate(t):
        chain = [(int(w / 2), int(w / 2), 0, 0), (w, w, 0, 0), (w, 0, 0, 0)]
        return torch.from_numpy(signal_oracle.affine_reflect_warp(t.numpy(), bend._inverse_maps_translate(shift).numpy(), chain,
                                                                  canvas.numpy())).float()

    return {0: layer0, 4: translate}


def unsaturated_checkpoint(out_size, lat, noise, o_bends, seed=30, target_std=0.35):
    """Seeded wide checkpoint whose bent frames can SHOW an error (few values on the uint8 clamp): the image is linear in the ToRGB weights
    and biases, so one oracle forward at gain 1 gives the gain that brings its standard deviation to ``target_std``."""
    sd = wide_seeding.wide_state_dict(SIZE, out_size, seed)
    img = wide_seeding.oracle_forward(sd, lat[:2], [None if nz is None else nz[:2] for nz in noise], o_bends)
    return wide_seeding.wide_state_dict(SIZE, out_size, seed, rgb_gain=float(target_std / float(img.std())))


def render_both_ways(g, lat, noise, bends, n, n_lanes, frame_hw):
    """Frames of the graph path and of the eager path, the fp32 images the lanes tapped, the lanes, and the replayed first frames."""
    from maua_stylegan2_amd import render

    taps, replays = {}, []
    orig_capture = g.capture_graph

    def capture(batch, lane=0, **kw):  # graphs with bends are per render (not cached on the generator): keep the lanes here
        assert len(kw["bends"]) == 2 and all(hasattr(b["transform"], "run_static") for b in kw["bends"])
        taps[lane] = orig_capture(batch, lane=lane, **kw)
        return taps[lane]

    def run(use_graph):
        frames = np.zeros((n,) + frame_hw + (3,), np.uint8)
        images = {}
        k = 0
        for first, u8 in render.synthesize(g, lat, noise, BS, bends=bends(), use_graph=use_graph, lanes=n_lanes):
            assert tuple(u8.shape[1:]) == frame_hw + (3,)
            frames[first: first + u8.shape[0]] = u8.cpu().numpy()
            if use_graph and u8.shape[0] == BS:
                lane = taps[k % n_lanes]
                assert lane.u8 is u8, "a full batch must come out of a graph lane"
                replays.append(first)
                if lane.image is not None:
                    torch.cuda.current_stream().synchronize()
                    images[first] = lane.image.cpu().clone()
            k += 1
        return frames, images

    g.capture_graph = capture
    try:
        graphed, images = run(True)
    finally:
        g.capture_graph = orig_capture
    n_captured = len(taps)
    eager, _ = run(False)
    assert len(taps) == n_captured, "use_graph=False must not capture"
    return graphed, eager, images, taps, replays


def test_captured_pad_and_translate_at_1920_equal_eager_and_oracle(gpu):
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render
    from oracle import stylegan2_oracle as so

    lat, noise, pads, plane, hw, shift, canvas = inputs(1920, N)
    sd = unsaturated_checkpoint(1920, lat, noise, oracle_bends(pads, plane, hw, shift[:2], canvas))
    g = wide_seeding.build_wide(SIZE, 1920, sd, gpu)
    g.tap_float_image = True  # the captured forward leaves its fp32 image next to the uint8 frames

    def bends():
        return [{"layer": 0, "transform": ar.Pad(pads, noise=plane.clone())},
                {"layer": 4, "modulation": shift.clone(), "transform": lambda m: ar.Translate(m, hw[0], hw[1], canvas)}]

    seq, ok = render._sequence_bends([dict(b, modulation=b["modulation"].to(gpu)) if "modulation" in b else b for b in bends()], N)
    assert ok and [b["transform"].sequence_rows for b in seq] == [None, N]

    graphed, eager, images, taps, replays = render_both_ways(g, lat, noise, bends, N, LANES, (SIZE, 2 * SIZE))
    # (a) the render ran captured: three lanes were captured with both bends and replayed for the three full batches
    assert sorted(taps) == [0, 1, 2] and replays == [0, BS, 2 * BS]
    assert all(tuple(lane.u8.shape) == (BS, SIZE, 2 * SIZE, 3) for lane in taps.values())
    # (b) byte for byte
    assert np.array_equal(graphed, eager)

    # (c) the fp32 image of the second batch (frame0 = 4: the scroll's rows are picked through the frame source) against the oracle
    lo, hi = BS, 2 * BS
    noise_o = [None if nz is None else nz[lo:hi] for nz in noise]
    want = wide_seeding.oracle_forward(sd, lat[lo:hi], noise_o, oracle_bends(pads, plane, hw, shift[lo:hi], canvas))
    plain = wide_seeding.oracle_forward(sd, lat[lo:hi], noise_o, oracle_bends(pads, None, hw, None, None))  # the bare ReplicationPad2d
    assert tuple(want.shape) == (BS, 3, SIZE, 2 * SIZE) and tuple(images[lo].shape) == tuple(want.shape)
    err = float((images[lo] - want).abs().max())
    moved = float((want - plain).abs().mean())
    clamped = seeding.clamped_fraction(want)
    print(f"[pad + translate at 32 x 64, frames {lo}..{hi - 1}] image std {float(want.std()):.3f}, max |hip - oracle| = {err:.3e} (float, "
          f"full frames), clamped values {100 * clamped:.1f} %, noise plane + scroll move the image by {moved:.3f} on average")
    # (d)
    assert moved > 0, "the bends must change the frames for this test to mean anything"
    assert err < 1e-3, err
    assert np.array_equal(so.frames_to_uint8(images[lo]), graphed[lo:hi]), "frames != cast of the tapped float image"
    diff = np.abs(graphed[lo:hi].astype(np.int16) - so.frames_to_uint8(want).astype(np.int16))
    assert diff.max() <= 1


def test_captured_pad_and_translate_at_1080_equal_eager(gpu):
    """Portrait: pads (0, 0, 2, 2), 64 x 32 frames; two full batches on two lanes + an eager tail of one frame."""
    import maua_stylegan2_amd.audioreactive as ar

    n, n_lanes = 2 * BS + 1, 2
    lat, noise, pads, plane, hw, shift, canvas = inputs(1080, n)
    assert pads == (0, 0, 2, 2) and hw == (32, 16)
    g = wide_seeding.build_wide(SIZE, 1080, wide_seeding.wide_state_dict(SIZE, 1080, 35, rgb_gain=0.2), gpu)

    def bends():
        return [{"layer": 0, "transform": ar.Pad(pads, noise=plane.clone())},
                {"layer": 4, "modulation": shift.clone(), "transform": lambda m: ar.Translate(m, hw[0], hw[1], canvas)}]

    graphed, eager, _, taps, replays = render_both_ways(g, lat, noise, bends, n, n_lanes, (2 * SIZE, SIZE))
    assert sorted(taps) == [0, 1] and replays == [0, BS]
    assert all(tuple(lane.u8.shape) == (BS, 2 * SIZE, SIZE, 3) for lane in taps.values())
    assert np.array_equal(graphed, eager)
    assert graphed.std() > 5 and not np.array_equal(graphed[0], graphed[BS])


def test_captured_pad_and_translate_at_1080_equal_eager_range_and_oracle(gpu):
    """The portrait twin of the 1920 test: ``ar.Pad((0, 0, 2, 2))`` on layer 0, the per-frame scroll on the 32 x 16 map of layer id 4,
    64 x 32 frames.  Three lanes == the eager path == a render of a frame range that starts inside a batch, byte for byte; the second
    batch against the oracle: the tapped fp32 image inside 1e-3, the frames within one grey level."""
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render
    from oracle import stylegan2_oracle as so

    lat, noise, pads, plane, hw, shift, canvas = inputs(1080, N)
    assert pads == (0, 0, 2, 2) and hw == (32, 16)
    sd = unsaturated_checkpoint(1080, lat, noise, oracle_bends(pads, plane, hw, shift[:2], canvas), seed=36)
    g = wide_seeding.build_wide(SIZE, 1080, sd, gpu)
    g.tap_float_image = True

    def bends():
        return [{"layer": 0, "transform": ar.Pad(pads, noise=plane.clone())},
                {"layer": 4, "modulation": shift.clone(), "transform": lambda m: ar.Translate(m, hw[0], hw[1], canvas)}]

    graphed, eager, images, taps, replays = render_both_ways(g, lat, noise, bends, N, LANES, (2 * SIZE, SIZE))
    assert sorted(taps) == [0, 1, 2] and replays == [0, BS, 2 * BS]
    assert all(tuple(lane.u8.shape) == (BS, 2 * SIZE, SIZE, 3) for lane in taps.values())
    assert np.array_equal(graphed, eager)
    assert graphed.std() > 5 and not np.array_equal(graphed[0], graphed[BS])

    # a frame range that starts inside a batch of the full render: two captured batches (frames 3 .. 10) and an eager tail (11 .. 12)
    lo, hi = 3, 13
    ranged = np.zeros((hi - lo, 2 * SIZE, SIZE, 3), np.uint8)
    firsts = []
    for first, u8 in render.synthesize(g, lat, noise, BS, bends=bends(), use_graph=True, lanes=LANES, frame_range=(lo, hi)):
        firsts.append(first)
        ranged[first - lo: first - lo + u8.shape[0]] = u8.cpu().numpy()
    assert firsts == [lo, lo + BS, lo + 2 * BS]
    assert np.array_equal(ranged, graphed[lo:hi])

    lo, hi = BS, 2 * BS
    noise_o = [None if nz is None else nz[lo:hi] for nz in noise]
    want = wide_seeding.oracle_forward(sd, lat[lo:hi], noise_o, oracle_bends(pads, plane, hw, shift[lo:hi], canvas))
    plain = wide_seeding.oracle_forward(sd, lat[lo:hi], noise_o, oracle_bends(pads, None, hw, None, None))
    assert tuple(want.shape) == (BS, 3, 2 * SIZE, SIZE) and tuple(images[lo].shape) == tuple(want.shape)
    err = float((images[lo] - want).abs().max())
    moved = float((want - plain).abs().mean())
    print(f"[pad + translate at 64 x 32, frames {lo}..{hi - 1}] image std {float(want.std()):.3f}, max |hip - oracle| = {err:.3e} (float, "
          f"full frames), clamped values {100 * seeding.clamped_fraction(want):.1f} %, noise plane + scroll move the image by {moved:.3f} on average")
    assert moved > 0, "the bends must change the frames for this test to mean anything"
    assert seeding.clamped_fraction(want) < 0.25
    assert err < 1e-3, err
    assert np.array_equal(so.frames_to_uint8(images[lo]), graphed[lo:hi]), "frames != cast of the tapped float image"
    diff = np.abs(graphed[lo:hi].astype(np.int16) - so.frames_to_uint8(want).astype(np.int16))
    assert diff.max() <= 1


def test_capture_refuses_a_widening_bend_on_a_generator_built_square(gpu):
    """A captured forward reads its noise through slots bound to maps of the generator's noise buffers' shape and sizes the uint8 frames
    from them: with a layer-0 ``ar.Pad`` on a generator built WITHOUT ``output_size`` both would be half of what the layers read and
    write.  The capture raises at conv1, before any layer runs, as the eager forward does on the checkpoint's square buffers."""
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd.models.stylegan2 import Generator

    size, batch = 16, 2
    g = Generator(size, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(size, seed=37), strict=True)
    g = g.to(gpu).eval()
    lat = seeding.seeded_latents(batch, g.n_latent, seed=38).to(gpu)
    bends = [{"layer": 0, "transform": ar.Pad((2, 2, 0, 0))}]
    with pytest.raises(RuntimeError, match="does not match feature map"):
        g(styles=lat, noise=None, randomize_noise=False, input_is_latent=True, transform_dict_list=bends)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for frames_u8 in (False, True):
            with pytest.raises(RuntimeError, match="noise slot 0 holds 4 x 4 maps"):
                g.capture_graph(batch, bends=bends, frames_u8=frames_u8)
    stream.synchronize()
    # the same generator without the bend still captures and replays
    with torch.cuda.stream(stream):
        lane = g.capture_graph(batch, frames_u8=True)
        lane.bind(lat, [None] * g.num_layers)
        lane.replay(0)
        stream.synchronize()
    assert tuple(lane.u8.shape) == (batch, size, size, 3) and float(lane.u8.float().std()) > 1
    lane.release()


def test_generate_with_the_wide_plugin_renders_1920_on_the_lanes(gpu, tmp_path, monkeypatch):
    """``generate(out_size=1920)`` with examples/wide.py on stand-in audio features: the layer-0 bend is captured (the full batch comes
    from a graph lane) and every delivered frame has the shape ``render`` itself names for that output size."""
    import sys

    from conftest import GOLDEN

    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import generate_audiovisual as gav
    from maua_stylegan2_amd import render
    from maua_stylegan2_amd.audioreactive.examples import wide

    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import plugin_stubs as stubs

    monkeypatch.chdir(tmp_path)
    size, n, fps, batch = 1024, 6, 6, 4
    torch.save({"g_ema": seeding.seeded_state_dict(size, seed=0)}, "seeded1024.pt")
    np.save("selection.npy", seeding.seeded_array(42, "selection", (12, 18, 512)))
    feats = stubs.Features(n, fps)
    monkeypatch.setattr(ar, "onsets", feats.onsets)
    monkeypatch.setattr(ar, "chroma", feats.chroma)
    monkeypatch.setattr(ar, "load_audio", feats.load_audio)
    monkeypatch.setattr(torch, "randn", stubs.SeededRandn(46))
    monkeypatch.setenv("MAUA_GENERATOR_CACHE", "0")
    shapes, held, captured = [], {}, []

    class KeepingSink(render.FrameSink):
        def __init__(self, output_file, width, height, *a, **k):
            self.count, self.w, self.h = 0, width, height

        def write(self, frame):
            shapes.append(tuple(frame.shape))
            held["last"] = np.array(frame, copy=True)
            self.count += 1

        def close(self):
            pass

    monkeypatch.setattr(render, "FrameSink", KeepingSink)
    real_load = gav.load_generator

    def load_generator(**kw):
        g = held["g"] = real_load(**kw)
        orig_capture = g.capture_graph

        def capture(batch_, lane=0, **ckw):
            captured.append((lane, [type(b["transform"]).__name__ for b in ckw["bends"]]))
            return orig_capture(batch_, lane=lane, **ckw)

        g.capture_graph = capture
        return g

    monkeypatch.setattr(gav, "load_generator", load_generator)
    gav.generate(ckpt="seeded1024.pt", audio_file="clip.wav", initialize=wide.initialize, get_latents=wide.get_latents,
                 get_noise=wide.get_noise, get_bends=wide.get_bends, latent_file="selection.npy", G_res=size, out_size=1920, fps=fps,
                 batch=batch, output_file=str(tmp_path / "o.mp4"))
    assert captured == [(0, ["Pad"])]  # one full batch of 4 -> one lane; the tail of 2 is eager
    want_shape = render._stream_frame_shape(held["g"], 1920)
    assert want_shape == (1080, 1920, 3)
    assert shapes == [want_shape] * n
    assert held["last"].std() > 5
