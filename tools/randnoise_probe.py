"""frames/s of render.synthesize on the 1024^2 bench generator with static and with randomised noise, and the isolated time of the
noise launch (maua_randn_frames_f32).  Prints one JSON line.

    python tools/randnoise_probe.py [--repo DIR] [--steps 20] [--warmup 5] [--batch 8] [--lanes 3] [--noise bench|none]

A step is one synthesize() over 15 batches (bench.py's step); the timed region is bracketed by device events on the calling stream, as
bench.py brackets its own.  ``--repo DIR`` imports the package from another checkout (the parent commit, for the baseline of
profiles/randnoise.md: there ``randomize_noise`` takes the eager one-lane path).  ``--noise bench``: per-frame sequences up to 256^2 and
None above, as bench.py's workload (randomised: the 512^2 / 1024^2 maps are generated); ``none``: every slot None (all 17 generated).
Modes: static; random = randomize_noise with a fixed generator.noise_seed (graph lanes cached across renders); random_unseeded = a fresh
seed per render (the lanes are captured again for every render: the seed is an argument of the captured launch)."""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--lanes", type=int, default=3)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batches-per-step", type=int, default=15)
    ap.add_argument("--noise", choices=("bench", "none"), default="bench")
    ap.add_argument("--modes", default="static,random,random_unseeded")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo))

    import torch

    from maua_stylegan2_amd import _lib, render, seeding
    from maua_stylegan2_amd.models.stylegan2 import Generator

    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    g = Generator(args.size, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(args.size, seed=0))
    g = g.to(dev).eval()
    n = args.batches_per_step * args.batch
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000)
    lat = torch.randn(n, g.n_latent, 512, device=dev, generator=gen)
    sizes = seeding.noise_sizes(args.size)
    noise = [torch.randn(n, 1, s, s, device=dev, generator=gen) if (s <= 256 and args.noise == "bench") else None for s in sizes]
    has_new = hasattr(g, "random_noise")
    out = {"repo": os.path.abspath(args.repo), "counter_based": has_new, "device": _lib.device_info()["name"], "batch": args.batch,
           "lanes": args.lanes, "frames_per_step": n, "steps": args.steps, "noise": args.noise}

    def step(randomize):
        for _first, _u8 in render.synthesize(g, lat, noise, args.batch, randomize_noise=randomize, lanes=args.lanes):
            pass

    for mode in args.modes.split(","):
        randomize = mode != "static"
        if has_new:
            g.noise_seed = 0x5EED if mode == "random" else None
        for _ in range(args.warmup):
            step(randomize)
        torch.cuda.synchronize(dev)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        wall = time.perf_counter()
        start.record()
        for _ in range(args.steps):
            step(randomize)
        stop.record()
        stop.synchronize()
        ms = start.elapsed_time(stop)
        out[mode] = {"frames_per_s": round(args.steps * n / (ms * 1e-3), 1), "ms_per_batch": round(ms / (args.steps * args.batches_per_step), 4),
                     "wall_s": round(time.perf_counter() - wall, 3)}
    if has_new:
        g.noise_seed = None
        # the launch alone: every noise layer of one batch, then only the layers `--noise bench` leaves to the generator
        for name, slots in (("launch_all_slots_us", None), ("launch_none_slots_us", [i for i, nz in enumerate(noise) if nz is None])):
            for _ in range(3):
                maps = g.random_noise(0, args.batch, 1, slots)
            table = g._randn_table(list(range(g.num_layers)) if slots is None else slots, maps)
            lib, st = _lib.load(), _lib.stream_ptr(dev)
            reps = 50
            torch.cuda.synchronize(dev)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for r in range(reps):
                _lib.check(lib.maua_randn_frames_f32(table.data_ptr(), len(maps), args.batch, 1, 8 * r, None, st), "maua_randn_frames_f32")
            stop.record()
            stop.synchronize()
            out[name] = round(start.elapsed_time(stop) * 1e3 / reps, 2)
            out[name.replace("_us", "_mb")] = round(sum(m.numel() for m in maps) * 4 / 1e6, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
