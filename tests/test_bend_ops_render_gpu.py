"""GPU: the point and morphological bends inside a render — captured forward == eager per-batch path == oracle.  A seeded 64^2
generator with a per-frame ScalarMultiply on layer id 3 (half of the channels), a per-frame Dilate on layer id 5 and a static Invert on
layer id 2; the oracle generator takes the torch expressions of the same transforms as callables at the same layer ids."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from maua_stylegan2_amd import seeding

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SIZE, N, BS, LANES = 64, 14, 4, 3  # 3 graph batches on 3 lanes + an eager tail of 2 frames


def inputs():
    lat = seeding.seeded_latents(N, 10, seed=21)
    noise = [torch.from_numpy(seeding.seeded_array(22, f"sq{i}", (N, 1, r, r))) if r <= 32 else None
             for i, r in enumerate(seeding.noise_sizes(SIZE))]
    envelope = 0.5 + torch.sin(torch.arange(N) / 3.0) ** 2   # 0.5 .. 1.5
    radius = 1.5 + 1.5 * torch.cos(torch.arange(N) / 2.0)      # rounds to 0 .. 3
    half = list(range(0, 512, 2))
    return lat, noise, envelope, radius, half


def oracle_bends(envelope, radius, half):
    """{layer id: torch callable} on the frames whose modulation rows are given."""
    def multiply(t):
        out = t.clone()
        out[:, half] = t[:, half] * envelope.view(-1, 1, 1, 1)
        return out

    def dilate(t):
        return torch.cat([F.max_pool2d(t[i: i + 1], 2 * r + 1, 1, r) for i, r in enumerate(torch.round(radius).int().tolist())])

    return {3: multiply, 5: dilate, 2: lambda t: 1 - t}


def unsaturated_checkpoint(lat, noise, envelope, radius, half, seed=20, target_std=0.35):
    """Seeded checkpoint whose bent frames can SHOW an error (few values on the uint8 clamp): the image is linear in the ToRGB weights
    and biases, so one oracle forward at gain 1 gives the gain that brings its standard deviation to ``target_std``."""
    from oracle import stylegan2_oracle as so

    sd = seeding.seeded_state_dict(SIZE, seed=seed)
    noise2 = [sd[f"noises.noise_{i}"] if nz is None else nz[:2] for i, nz in enumerate(noise)]
    img = so.generator_forward(sd, lat[:2], noise2, bends=oracle_bends(envelope[:2], radius[:2], half))
    return seeding.seeded_state_dict(SIZE, seed=seed, rgb_gain=float(target_std / float(img.std())))


def test_captured_point_and_morph_bends_equal_eager_and_oracle(gpu):
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render
    from maua_stylegan2_amd.models.stylegan2 import Generator
    from oracle import stylegan2_oracle as so

    lat, noise, envelope, radius, half = inputs()
    sd = unsaturated_checkpoint(lat, noise, envelope, radius, half)
    g = Generator(SIZE, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(sd, strict=True)
    g = g.to(gpu).eval()
    g.tap_float_image = True  # the captured forward leaves its fp32 image next to the uint8 frames

    def bends():
        return [{"layer": 3, "modulation": envelope.clone(), "transform": lambda m: ar.ScalarMultiply(m, channels=half)},
                {"layer": 5, "modulation": radius.clone(), "transform": lambda m: ar.Dilate(m)},
                {"layer": 2, "transform": ar.Invert()}]

    seq, ok = render._sequence_bends([dict(b, modulation=b["modulation"].to(gpu)) if "modulation" in b else b for b in bends()], N)
    assert ok and [b["transform"].sequence_rows for b in seq] == [N, N, 1]

    taps = {}
    replays = []
    orig_capture = g.capture_graph

    def capture(batch, lane=0, **kw):  # graphs with bends are per render (not cached on the generator): keep the lanes here
        assert len(kw["bends"]) == 3 and all(hasattr(b["transform"], "run_static") for b in kw["bends"])
        taps[lane] = orig_capture(batch, lane=lane, **kw)
        return taps[lane]

    def run(use_graph):
        frames = np.zeros((N, SIZE, SIZE, 3), np.uint8)
        images = {}
        k = 0
        for first, u8 in render.synthesize(g, lat, noise, BS, bends=bends(), use_graph=use_graph, lanes=LANES):
            frames[first: first + u8.shape[0]] = u8.cpu().numpy()
            if use_graph and u8.shape[0] == BS:
                lane = taps[k % LANES]
                assert lane.u8 is u8 and lane.image is not None, "a full batch must come out of a graph lane"
                replays.append(first)
                torch.cuda.current_stream().synchronize()
                images[first] = lane.image.cpu().clone()
            k += 1
        return frames, images

    g.capture_graph = capture
    graphed, images = run(True)
    g.capture_graph = orig_capture
    # (c) the render ran captured: three lanes were captured with the three bends and replayed for the three full batches
    assert sorted(taps) == [0, 1, 2] and replays == [0, BS, 2 * BS]
    n_captured = len(taps)
    eager, _ = run(False)
    assert len(taps) == n_captured, "use_graph=False must not capture"
    # (a) byte for byte
    assert np.array_equal(graphed, eager)

    # (b) the fp32 image of the second batch (frame0 = 4: the per-frame rows are picked through the frame source) against the oracle
    lo, hi = BS, 2 * BS
    noise_o = [sd[f"noises.noise_{i}"] if nz is None else nz[lo:hi] for i, nz in enumerate(noise)]
    want = so.generator_forward(sd, lat[lo:hi], noise_o, bends=oracle_bends(envelope[lo:hi], radius[lo:hi], half))
    plain = so.generator_forward(sd, lat[lo:hi], noise_o)
    err = float((images[lo] - want).abs().max())
    moved = float((want - plain).abs().mean())
    clamped = seeding.clamped_fraction(want)
    print(f"[bends at 64^2, frames {lo}..{hi - 1}] image std {float(want.std()):.3f}, max |hip - oracle| = {err:.3e} (float, full frames), "
          f"clamped values {100 * clamped:.1f} %, the bends move the image by {moved:.3f} on average")
    assert moved > 0, "the bends must change the frames for this test to mean anything"
    assert err < 1e-3, err
    assert np.array_equal(so.frames_to_uint8(images[lo]), graphed[lo:hi]), "frames != cast of the tapped float image"
    diff = np.abs(graphed[lo:hi].astype(np.int16) - so.frames_to_uint8(want).astype(np.int16))
    assert diff.max() <= 1


def test_bends_on_layers_the_style_fold_would_claim(gpu):
    """The 32^2 and 64^2 layers of this generator hand their maps over pre-multiplied by the next convolution's styles (the style fold)
    unless a bend reads them: with a per-frame Erode on layer id 6 and a ScalarMultiply on layer id 7 the producers must store the plain
    maps.  Captured == eager byte for byte, and the eager fp32 image of frames 4 .. 7 agrees with the oracle."""
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render
    from maua_stylegan2_amd.models.stylegan2 import Generator
    from oracle import stylegan2_oracle as so

    lat, noise, envelope, radius, half = inputs()
    radius = radius * 2.0 / 3.0  # rounds to 0 .. 2

    def o_bends(lo, hi):
        def erode(t):
            out = t.clone()
            for i, r in enumerate(torch.round(radius[lo:hi]).int().tolist()):
                out[i, half] = -F.max_pool2d(-t[i: i + 1, half], 2 * r + 1, 1, r)[0]
            return out

        return {6: erode, 7: lambda t: t * envelope[lo:hi].view(-1, 1, 1, 1)}

    sd = seeding.seeded_state_dict(SIZE, seed=23)
    noise2 = [sd[f"noises.noise_{i}"] if nz is None else nz[:2] for i, nz in enumerate(noise)]
    gain = 0.35 / float(so.generator_forward(sd, lat[:2], noise2, bends=o_bends(0, 2)).std())
    sd = seeding.seeded_state_dict(SIZE, seed=23, rgb_gain=gain)
    g = Generator(SIZE, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(sd, strict=True)
    g = g.to(gpu).eval()
    assert g.style_fold

    def bends():
        return [{"layer": 6, "modulation": radius.clone(), "transform": lambda m: ar.Erode(m, channels=half)},
                {"layer": 7, "modulation": envelope.clone(), "transform": lambda m: ar.ScalarMultiply(m)}]

    def run(use_graph):
        frames = np.zeros((N, SIZE, SIZE, 3), np.uint8)
        for first, u8 in render.synthesize(g, lat, noise, BS, bends=bends(), use_graph=use_graph, lanes=LANES):
            frames[first: first + u8.shape[0]] = u8.cpu().numpy()
        return frames

    graphed = run(True)
    assert np.array_equal(graphed, run(False))
    lo, hi = BS, 2 * BS
    batch_bends = [{"layer": b["layer"], "transform": b["transform"](b["modulation"][lo:hi].to(gpu))} for b in bends()]
    noise_d = [None if nz is None else nz[lo:hi].to(gpu) for nz in noise]
    image, _ = g(styles=lat[lo:hi].to(gpu), noise=noise_d, truncation=1.0, transform_dict_list=batch_bends, randomize_noise=False,
                 input_is_latent=True)
    noise_o = [sd[f"noises.noise_{i}"] if nz is None else nz[lo:hi] for i, nz in enumerate(noise)]
    want = so.generator_forward(sd, lat[lo:hi], noise_o, bends=o_bends(lo, hi))
    err = float((image.cpu() - want).abs().max())
    moved = float((want - so.generator_forward(sd, lat[lo:hi], noise_o)).abs().mean())
    print(f"[bends on folded layers, frames {lo}..{hi - 1}] image std {float(want.std()):.3f}, max |hip - oracle| = {err:.3e}, "
          f"the bends move the image by {moved:.3f} on average")
    assert moved > 0 and err < 1e-3, (moved, err)
    diff = np.abs(graphed[lo:hi].astype(np.int16) - so.frames_to_uint8(want).astype(np.int16))
    assert diff.max() <= 1
