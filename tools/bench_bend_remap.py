"""Side measurement of the coordinate-remap bends (csrc/bend_remap.hip) on one MI355X — the figures of profiles/bend_remap.md.

    python tools/bench_bend_remap.py [--size 1024] [--frames 240] [--batch 8] [--rounds 3] [--reps 200] [--out FILE.json]

1. maua_bend_remap_f32 alone, each of the five ops, on the feature maps a 1024^2 render bends (batch 8): HIP events (maua_event_*) round
   ``--reps`` launches after a warm-up, ``--rounds`` times, the median.  In the same process and on the same maps: the affine warp
   (maua_affine_reflect_warp_mapped_f32 as ``ar.Rotate`` launches it, the comparable gather) and the point bend (maua_bend_point_f32,
   scalar multiply on every channel: the device's copy rate).  Bytes: one read and one write of the map.
2. render.synthesize at ``--size`` on three graph lanes: plain against the same render with a per-frame Swirl on half of the channels of
   layer id 6 (32 x 32) and a per-frame Displace on layer id 10 (128 x 128), alternating, ``--rounds`` times each.  A bent render captures its graph lanes per
   render (a plain one reuses cached lanes), and that capture is inside the bent figure.
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

SHAPES = [(8, 512, 32, 32), (8, 256, 128, 128), (8, 128, 256, 256)]


def flow_field(frames=16, size=32, seed=5):
    return torch.from_numpy(seeding.seeded_array(seed, "flow", (frames, 2, size, size)))


def kernel_cases(shape):
    """(name, module with run_static) for a map of ``shape``: one parameter row for every sample."""
    b, c, h, w = shape
    one = lambda v: torch.tensor([v], dtype=torch.float32)  # noqa: E731
    return [("remap: mirror", ar.Mirror(one(30.0), offset=0.1 * w)),
            ("remap: kaleidoscope", ar.Kaleidoscope(one(25.0), sectors=6)),
            ("remap: swirl", ar.Swirl(one(120.0), radius=0.3 * w)),
            ("remap: ripple", ar.Ripple(one(0.05 * w), wavelength=0.2 * w, phase=0.3)),
            ("remap: displace", ar.Displace(torch.tensor([[0.05 * w, 3.4]]), flow_field())),
            ("remap: swirl, every other channel", ar.Swirl(one(120.0), radius=0.3 * w, channels=list(range(0, c, 2)))),
            ("affine warp (ar.Rotate)", ar.Rotate(one(20.0), h, w)),
            ("point: scalar multiply", ar.ScalarMultiply(one(1.5)))]


def time_kernels(dev, reps, rounds):
    rows = []
    for shape in SHAPES:
        x = torch.from_numpy(seeding.seeded_array(6, f"x{shape}", shape)).to(dev)
        y = torch.empty_like(x)
        moved = 2 * x.numel() * 4
        for name, module in kernel_cases(shape):
            for _ in range(5):  # uploads the operands, loads the code object
                module.run_static(x, y, None)
            torch.cuda.synchronize(dev)
            times = []
            for _ in range(rounds):
                start, stop = _lib.HipEvent(), _lib.HipEvent()
                start.record()
                for _ in range(reps):
                    module.run_static(x, y, None)
                stop.record()
                torch.cuda.synchronize(dev)
                times.append(start.elapsed_ms(stop) / reps)
            ms = sorted(times)[rounds // 2]
            rows.append({"kernel": name, "shape": list(shape), "us": ms * 1e3, "us_rounds": [t * 1e3 for t in times], "bytes": moved,
                         "TB_per_s": moved / ms / 1e9})
            print(f"{name:36s} {str(shape):22s} {ms * 1e3:9.1f} us  ({min(times) * 1e3:.1f} .. {max(times) * 1e3:.1f})  {moved / 1e6:8.1f} MB  "
                  f"{moved / ms / 1e9:6.2f} TB/s", flush=True)
    return rows


def time_render(dev, size, n, batch, rounds):
    g = Generator(size, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(size, seed=0), strict=True)
    g = g.to(dev).eval()
    lat = seeding.seeded_latents(n, g.n_latent, seed=1).to(dev)
    noise = [None] * g.num_layers
    frame = torch.arange(n, dtype=torch.float32)
    half = list(range(0, 512, 2))
    field = flow_field()

    def bends():
        return [{"layer": 6, "modulation": 90.0 * torch.sin(frame / 5.0), "transform": lambda m: ar.Swirl(m, radius=10.0, channels=half)},
                {"layer": 10, "modulation": torch.stack([2.0 + torch.cos(frame / 7.0), 0.3 * frame], 1),
                 "transform": lambda m: ar.Displace(m, field)}]

    def run(spec):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in render.synthesize(g, lat, noise, batch, bends=spec, lanes=3):
            pass
        torch.cuda.synchronize(dev)
        return n / (time.perf_counter() - t0)

    run([]), run(bends())  # warm-up: packs the weights, captures the plain lanes
    out = {"plain": [], "bends": []}
    for _ in range(rounds):
        out["plain"].append(run([]))
        out["bends"].append(run(bends()))
        print(f"render {size}^2, {n} frames, batch {batch}: plain {out['plain'][-1]:.1f} frames/s, swirl + displace {out['bends'][-1]:.1f} frames/s",
              flush=True)
    out["relative"] = sorted(out["bends"])[rounds // 2] / sorted(out["plain"])[rounds // 2]
    print(f"bends / plain (medians): {out['relative']:.3f}   (the bent render captures its graphs per render: that is part of its time)")
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bend_remap.py needs an MI355X: there is no CPU path to time")
    dev = torch.device("cuda:0")
    _lib.load()
    result = {"device": _lib.device_info()["name"], "kernels": time_kernels(dev, args.reps, args.rounds),
              "render": time_render(dev, args.size, args.frames, args.batch, args.rounds)}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
