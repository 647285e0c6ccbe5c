"""Side measurement of the point and morphological bends (csrc/bend_ops.hip) on one MI355X — sections 2 and 3 of profiles/bend_ops.md.

    python tools/bench_bend_ops.py [--size 1024] [--frames 240] [--batch 8] [--rounds 3] [--out FILE.json]

1. The two kernels alone, HIP events round 20 launches each, on feature maps of the sizes a 1024^2 render bends (batch 8): time, the
   bytes the op has to move (one read and one write of the map) and the rate that implies.
2. render.synthesize at ``--size`` on three graph lanes: plain against the same render with a per-frame ScalarMultiply (half of the
   channels of layer id 3), a per-frame Dilate (layer id 5) and a static Invert (layer id 2), alternating, ``--rounds`` times each.
   bench.py's ``--bends`` switch times the affine bends; this is the same comparison for the new ones.  A bent render captures its
   graph lanes per render (a plain one reuses cached lanes), and that capture is inside the bent figure: the ratio is a whole-render
   ratio, not comparable with bench.py's steady-state "0.99 x plain" of the affine bends.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from maua_stylegan2_amd import _lib, render, seeding  # noqa: E402
from maua_stylegan2_amd.audioreactive import bend  # noqa: E402
from maua_stylegan2_amd.models.stylegan2 import Generator  # noqa: E402

torch.set_grad_enabled(False)


def time_kernels(dev, reps=20):
    rows = []
    shapes = [(8, 512, 16, 16), (8, 512, 64, 64), (8, 128, 256, 256), (8, 32, 1024, 1024), (8, 32, 540, 960)]
    cases = [("point: scalar multiply", lambda n: bend.PointBend("multiply", torch.full((n,), 1.5), None)),
             ("point: invert, every third channel", lambda n: bend.PointBend("invert", None, list(range(0, 32, 3)))),
             ("morph: dilate r = 1", lambda n: bend.MorphBend("dilate", torch.full((n,), 1), None)),
             ("morph: dilate r = 3", lambda n: bend.MorphBend("dilate", torch.full((n,), 3), None)),
             ("morph: erode r = 16", lambda n: bend.MorphBend("erode", torch.full((n,), 16), None))]
    for shape in shapes:
        x = torch.randn(shape, device=dev)
        y = torch.empty_like(x)
        for name, make in cases:
            module = make(shape[0])
            module.run_static(x, y, None)  # uploads the operands
            torch.cuda.synchronize(dev)
            start, stop = _lib.HipEvent(), _lib.HipEvent()
            start.record()
            for _ in range(reps):
                module.run_static(x, y, None)
            stop.record()
            torch.cuda.synchronize(dev)
            ms = start.elapsed_ms(stop) / reps
            moved = 2 * x.numel() * 4  # one read and one write of the map (a copied-through channel moves the same bytes)
            rows.append({"kernel": name, "shape": list(shape), "ms": ms, "bytes": moved, "TB_per_s": moved / ms / 1e9})
            print(f"{name:38s} {str(shape):22s} {ms * 1e3:9.1f} us  {moved / 1e6:9.1f} MB  {moved / ms / 1e9:6.2f} TB/s", flush=True)
        # the device's own copy of the same bytes, for scale
        start, stop = _lib.HipEvent(), _lib.HipEvent()
        y.copy_(x)
        torch.cuda.synchronize(dev)
        start.record()
        for _ in range(reps):
            y.copy_(x)
        stop.record()
        torch.cuda.synchronize(dev)
        ms = start.elapsed_ms(stop) / reps
        rows.append({"kernel": "device copy", "shape": list(shape), "ms": ms, "bytes": 2 * x.numel() * 4, "TB_per_s": 2 * x.numel() * 4 / ms / 1e9})
        print(f"{'device copy (torch copy_)':38s} {str(shape):22s} {ms * 1e3:9.1f} us  {2 * x.numel() * 4 / 1e6:9.1f} MB  {2 * x.numel() * 4 / ms / 1e9:6.2f} TB/s", flush=True)
    return rows


def time_render(dev, size, n, batch, rounds):
    g = Generator(size, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(size, seed=0), strict=True)
    g = g.to(dev).eval()
    lat = seeding.seeded_latents(n, g.n_latent, seed=1).to(dev)
    noise = [None] * g.num_layers
    frame = torch.arange(n, dtype=torch.float32)
    half = list(range(0, 512, 2))

    def bends():
        return [{"layer": 3, "modulation": 0.5 + torch.sin(frame / 3.0) ** 2, "transform": lambda m: bend.ScalarMultiply(m, channels=half)},
                {"layer": 5, "modulation": 1.5 + 1.5 * torch.cos(frame / 2.0), "transform": lambda m: bend.Dilate(m)},
                {"layer": 2, "transform": bend.Invert()}]

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
        print(f"render {size}^2, {n} frames, batch {batch}: plain {out['plain'][-1]:.1f} frames/s, bends {out['bends'][-1]:.1f} frames/s", flush=True)
    out["relative"] = sorted(out["bends"])[rounds // 2] / sorted(out["plain"])[rounds // 2]
    print(f"bends / plain (medians): {out['relative']:.3f}   (the bent render captures its graphs per render: that is part of its time)")
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bend_ops.py needs an MI355X: there is no CPU path to time")
    dev = torch.device("cuda:0")
    _lib.load()
    result = {"device": _lib.device_info()["name"], "kernels": time_kernels(dev),
              "render": time_render(dev, args.size, args.frames, args.batch, args.rounds)}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
