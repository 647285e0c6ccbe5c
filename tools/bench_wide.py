"""Side measurement of 2:1 renders (``--out_size 1920``) on one MI355X — the figures of profiles/bend_pad.md.

    python tools/bench_wide.py [--size 1024] [--frames 240] [--batch 8] [--rounds 5] [--out FILE.json]

1. maua_bend_pad_f32 alone, HIP events round 20 launches: the layer-0 launch of a render and pads on large maps.
2. render.synthesize of a generator built for 1920 output on three lanes, alternating per round:
   "lanes"  — the layer-0 bend is ``ar.Pad((2, 2, 0, 0), noise=...)``: captured, three graph lanes;
   "eager"  — the layer-0 bend is ``Sequential(ReplicationPad2d((2, 2, 0, 0)), AddNoise(...))``: a torch module without ``run_static``, so
              the render takes the eager per-batch path on one lane, which is all such a render could do before ``ar.Pad`` existed;
   "plain"  — the square render of a generator of the same size without bends (cached lanes), for scale: a wide frame has twice the pixels.
   A bent render captures its graph lanes per render, and that capture is inside the "lanes" figure.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import maua_stylegan2_amd.audioreactive as ar  # noqa: E402
from maua_stylegan2_amd import _lib, render, seeding  # noqa: E402
from maua_stylegan2_amd.models.stylegan2 import Generator  # noqa: E402

torch.set_grad_enabled(False)


def time_kernel(dev, reps=20):
    rows = []
    cases = [((8, 512, 4, 4), (2, 2, 0, 0), "replicate", 1), ((8, 512, 4, 4), (0, 0, 2, 2), "replicate", 1),
             ((8, 512, 64, 64), (32, 32, 0, 0), "reflect", 0), ((8, 128, 256, 256), (128, 128, 0, 0), "replicate", 0),
             ((8, 32, 1024, 1024), (512, 512, 0, 0), "reflect", 1), ((8, 32, 1024, 1021), (1, 1, 0, 0), "circular", 0)]
    for shape, pads, mode, nch in cases:
        out_shape = shape[:2] + (shape[2] + pads[2] + pads[3], shape[3] + pads[0] + pads[1])
        module = ar.Pad(pads, mode=mode, noise=torch.randn((nch,) + out_shape[2:]) if nch else None)
        x = torch.randn(shape, device=dev)
        y = torch.empty(out_shape, device=dev)
        module.run_static(x, y, None)  # uploads the noise plane
        torch.cuda.synchronize(dev)
        start, stop = _lib.HipEvent(), _lib.HipEvent()
        start.record()
        for _ in range(reps):
            module.run_static(x, y, None)
        stop.record()
        torch.cuda.synchronize(dev)
        ms = start.elapsed_ms(stop) / reps
        moved = 4 * (x.numel() + y.numel())  # the source once, the padded map once (the noise plane stays in cache)
        rows.append({"shape": list(shape), "pads": list(pads), "mode": mode, "noise_channels": nch, "ms": ms, "bytes": moved,
                     "TB_per_s": moved / ms / 1e9})
        print(f"pad {str(shape):22s} {str(pads):18s} {mode:10s} noise {nch}: {ms * 1e3:9.1f} us  {moved / 1e6:9.1f} MB  "
              f"{moved / ms / 1e9:6.2f} TB/s", flush=True)
    return rows


def time_render(dev, size, n, batch, rounds):
    weights = {k: v for k, v in seeding.seeded_state_dict(size, seed=0).items() if not k.startswith("noises.")}
    torch.manual_seed(0)  # the 2:1 noise buffers are drawn at construction
    wide = Generator(size, 512, 8, channel_multiplier=2, constant_input=True, output_size=1920)
    square = Generator(size, 512, 8, channel_multiplier=2, constant_input=True)
    for g in (wide, square):
        missing, unexpected = g.load_state_dict(weights, strict=False)
        assert not unexpected and all(k.startswith("noises.") for k in missing)
    wide, square = wide.to(dev).eval(), square.to(dev).eval()
    lat = seeding.seeded_latents(n, wide.n_latent, seed=1).to(dev)
    noise = [None] * wide.num_layers
    plane = 0.025 * torch.randn(1, 1, 4, 8)
    specs = {"lanes": lambda: [{"layer": 0, "transform": ar.Pad((2, 2, 0, 0), noise=plane)}],
             "eager": lambda: [{"layer": 0, "transform": torch.nn.Sequential(torch.nn.ReplicationPad2d((2, 2, 0, 0)), ar.AddNoise(plane))}],
             "plain": lambda: []}

    def run(name):
        g = square if name == "plain" else wide
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        shape = None
        for _, u8 in render.synthesize(g, lat, noise, batch, bends=specs[name](), lanes=3):
            shape = tuple(u8.shape[1:])
        torch.cuda.synchronize(dev)
        return n / (time.perf_counter() - t0), shape

    shapes = {name: run(name)[1] for name in specs}  # warm-up: packs the weights, captures the plain lanes
    out = {name: [] for name in specs}
    for _ in range(rounds):
        for name in specs:
            out[name].append(run(name)[0])
        print(f"render {size} px, {n} frames, batch {batch}: " + ", ".join(f"{name} {out[name][-1]:.1f} frames/s" for name in specs), flush=True)
    median = {name: sorted(v)[rounds // 2] for name, v in out.items()}
    out["frame_shapes"] = {name: list(s) for name, s in shapes.items()}
    out["median"] = median
    out["lanes_over_eager"] = median["lanes"] / median["eager"]
    out["lanes_over_plain"] = median["lanes"] / median["plain"]
    print(f"medians: lanes {median['lanes']:.1f}, eager {median['eager']:.1f}, plain {median['plain']:.1f} frames/s; "
          f"lanes / eager {out['lanes_over_eager']:.3f}, lanes / plain {out['lanes_over_plain']:.3f} (twice the pixels: 0.5 expected)")
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wide.py needs an MI355X: there is no CPU path to time")
    dev = torch.device("cuda:0")
    _lib.load()
    result = {"device": _lib.device_info()["name"], "kernel": time_kernel(dev),
              "render": time_render(dev, args.size, args.frames, args.batch, args.rounds)}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
