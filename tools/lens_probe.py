"""The cost of the lens effects on one MI355X: each entry's own time (csrc/lens.hip) on one batch beside a device copy of the same bytes —
extract at every reduction, the blur at the (map, radius) pairs the plan rule yields for bloom_size 0.01, 0.03 and 0.1 at 1024 px and for
the sharpen, a full-resolution blur at radius 64 to say how slow that is, apply with and without its terms — and the delivered frame rate
of rgb24 and yuv420p10le renders with a bloom, with a bloom and a sharpen, and without a lens (the bench configuration: 1024^2, batch 8,
three graph lanes, HBM-resident inputs, null sink).  Modelled on tools/grade_probe.py.

The parent process never touches the device: every step runs in one child process of its own under its own time limit, and a step that
fails, aborts or runs out of time ends the probe (nothing further is started on the device).
    python tools/lens_probe.py [--frames 448] [--alternations 3] [--md profiles/lens.md] [--json out.json]"""
import argparse
import gc
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT_S = {"kernels": 300, "rates": 480}
BLOOM_SIZES = (0.01, 0.03, 0.1)
SHARPEN_SIGMA = 1.0
RATE_FORMATS = ("rgb24", "yuv420p10le")
N_COLD = 6  # x 2 x 100 MB at 8 frames of 1024^2: well beyond the 256 MiB Infinity Cache


# ---------------------------------------------------------------------------------------------------------------- the steps (child processes)
def step_kernels(args):
    """Every entry on one batch, on the same buffers every call ("hot": what a batch the last layer has just written looks like) and
    rotating over more buffers than the Infinity Cache holds ("cold"), beside a device copy of the same bytes read + written.  Every frame
    has its own non-identity row and its own taps; the image is uniform noise over [-1.1, 1.1]."""
    import math

    import numpy as np
    import torch

    import maua_stylegan2_amd.audioreactive as ar
    from deep_delivery_probe import graph_time_ms
    from maua_stylegan2_amd import _lib

    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    lib = _lib.load()
    size, batch = args.size, args.batch
    st = lambda: _lib.stream_ptr(dev)  # noqa: E731
    imgs = [torch.rand(batch, 3, size, size, device=dev) * 2.2 - 1.1 for _ in range(N_COLD)]
    fulls = [torch.empty(batch, 3, size, size, device=dev) for _ in range(N_COLD)]
    k = np.arange(batch)
    lens = ar.Lens(batch, bloom=0.5 + 0.05 * k, bloom_threshold=0.6, sharpen=0.3 + 0.02 * k, vignette=0.2 + 0.01 * k)
    rows = lens.operands(dev, size, size)[0]
    result = {}
    counter = {"k": 0}

    def measure(name, moved, call, note=""):
        """call(i): one launch on buffer set i."""
        half = moved // 2
        n_sets = N_COLD if moved > (8 << 20) else 1
        src = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(n_sets)]
        dst = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(n_sets)]

        def rotate(f):
            def run():
                counter["k"] += 1
                f(counter["k"] % N_COLD)
            return run

        row = {"bytes_read_plus_written": moved, "note": note}
        modes = [("hot", lambda: call(0), lambda: dst[0].copy_(src[0]))]
        if n_sets > 1:
            modes.append(("cold", rotate(call), rotate(lambda i: dst[i].copy_(src[i]))))
        for temp, kern, copy in modes:
            k_ms = statistics.median(graph_time_ms(kern, 32) for _ in range(5))
            c_ms = statistics.median(graph_time_ms(copy, 32) for _ in range(5))
            row[temp] = {"kernel_us": k_ms * 1e3, "kernel_GBps": moved / (k_ms * 1e-3) / 1e9, "copy_us": c_ms * 1e3, "copy_GBps": 2 * half / (c_ms * 1e-3) / 1e9}
        result[name] = row
        print(f"{name}: " + ", ".join(f"{t} {row[t]['kernel_us']:.1f} us (copy {row[t]['copy_us']:.1f})" for t, _, _ in modes), file=sys.stderr, flush=True)

    px = batch * 3 * size * size
    # extract at every reduction
    for d in (1, 2, 4, 8):
        m = -(-size // d)
        outs = [torch.empty(batch, 3, m, m, device=dev) for _ in range(N_COLD)]
        measure(f"extract d={d}", 4 * (px + batch * 3 * m * m),
                lambda i, d=d, outs=outs: _lib.check(lib.maua_lens_extract_f32(imgs[i].data_ptr(), outs[i].data_ptr(), batch, size, size, d, rows.data_ptr(), 16, st()),
                                                     "maua_lens_extract_f32"))
    # the blur at the plan rule's (map, radius) pairs, the sharpen's, and the slowest the entry accepts
    blurs = []
    for frac in BLOOM_SIZES:
        d, rb, bt, _, _ = ar.Lens(batch, bloom=1, bloom_size=frac * (1 - 0.02 * k / batch)).plan(size, size)
        blurs.append((f"blur bloom_size {frac}: {-(-size // d)}^2 (d={d}) R={rb}", -(-size // d), rb, bt))
    rs = int(math.ceil(3 * SHARPEN_SIGMA))
    blurs.append((f"blur sharpen sigma {SHARPEN_SIGMA}: {size}^2 R={rs}", size, rs, ar.lens.gaussian_taps(np.full(batch, SHARPEN_SIGMA), rs)))
    blurs.append((f"blur full resolution, the widest: {size}^2 R=64", size, 64, ar.lens.gaussian_taps(np.full(batch, 64 / 3.0), 64)))
    for name, m, radius, taps in blurs:
        taps = torch.from_numpy(np.ascontiguousarray(taps)).to(dev)
        srcs = imgs if m == size else [torch.rand(batch, 3, m, m, device=dev) for _ in range(N_COLD)]
        dsts = fulls if m == size else [torch.empty(batch, 3, m, m, device=dev) for _ in range(N_COLD)]
        measure(name, 8 * batch * 3 * m * m,
                lambda i, m=m, radius=radius, taps=taps, srcs=srcs, dsts=dsts: _lib.check(
                    lib.maua_lens_blur_f32(srcs[i % len(srcs)].data_ptr(), dsts[i % len(dsts)].data_ptr(), batch, 3, m, m, radius, taps.data_ptr(), radius + 1, st()),
                    "maua_lens_blur_f32"))
    # apply: every term, the bloom alone (d = 4), the vignette alone
    m = size // 4
    bloom = torch.rand(batch, 3, m, m, device=dev)
    for name, use_bloom, use_soft in (("apply bloom (d=4) + sharpen + vignette", True, True), ("apply bloom (d=4) + vignette", True, False), ("apply vignette", False, False)):
        moved = 4 * (2 * px + (px if use_soft else 0) + (bloom.numel() if use_bloom else 0))
        measure(name, moved,
                lambda i, b=use_bloom, s=use_soft: _lib.check(
                    lib.maua_lens_apply_f32(imgs[i].data_ptr(), fulls[i].data_ptr(), batch, size, size, rows.data_ptr(), 16, bloom.data_ptr() if b else None, m, m, 4,
                                            imgs[(i + 1) % N_COLD].data_ptr() if s else None, st()), "maua_lens_apply_f32"))
    return {"device": torch.cuda.get_device_name(0), "size": size, "batch": batch, "kernel_one_batch": result}


def step_rates(args):
    import numpy as np
    import torch

    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render, seeding
    from maua_stylegan2_amd.models.stylegan2 import Generator

    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    size, batch = args.size, args.batch
    n = (args.frames // batch) * batch
    g = Generator(size, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(size, seed=0))
    g = g.to(dev).eval()
    lat = torch.randn(n, g.n_latent, 512, device=dev)
    noise = [torch.randn(n, 1, r, r, device=dev) if r <= 256 else None for r in seeding.noise_sizes(size)]
    t = np.arange(n) / 30.0
    kick = 0.05 + np.clip(np.sin(2 * np.pi * 2 * t), 0, 1) ** 4  # (never 0: every frame pays for its glow)
    lenses = {"no lens": None,
              "bloom": ar.Lens(n, bloom=kick, bloom_size=0.03, bloom_threshold=0.6, vignette=0.3 - 0.2 * kick),
              "bloom + sharpen": ar.Lens(n, bloom=kick, bloom_size=0.03, bloom_threshold=0.6, vignette=0.3 - 0.2 * kick, sharpen=0.4, sharpen_radius=SHARPEN_SIGMA)}

    def delivered(pix_fmt, lens):
        gc.collect()
        torch.cuda.synchronize()
        start = time.perf_counter()
        # output_file=None: the null sink — every frame still lands in pinned host memory and passes through the ordered sink thread
        written = render.render_lensed(g, lat, noise, 0, n / 30.0, batch, size, None, None, 1.0, [], {}, False, "slow", None, pipe_pix_fmt=pix_fmt, lens=lens)
        torch.cuda.synchronize()
        assert written == n
        return n / (time.perf_counter() - start)

    configs = [(fmt, name) for fmt in RATE_FORMATS for name in lenses]
    for fmt, name in configs:
        delivered(fmt, lenses[name])  # captures the lanes of both frame kinds, sizes the rings
    rates = {f"{fmt} {name}": [] for fmt, name in configs}
    for k in range(args.alternations):
        for fmt, name in (configs if k % 2 == 0 else configs[::-1]):
            # (the staging rings are re-made when the frame shape changes: every configuration is rendered twice, the warm render counts)
            delivered(fmt, lenses[name])
            rates[f"{fmt} {name}"].append(delivered(fmt, lenses[name]))
        print(f"alternation {k}: " + " | ".join(f"{name} {v[-1]:.0f}/s" for name, v in rates.items()), file=sys.stderr, flush=True)
    spread = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": [round(x, 1) for x in v]}  # noqa: E731
    return {"device": torch.cuda.get_device_name(0), "size": size, "batch": batch, "lanes": 3, "frames_per_render": n,
            "alternations": args.alternations, "frames_per_s": {k: spread(v) for k, v in rates.items()}}


STEPS = {"kernels": step_kernels, "rates": step_rates}


# ---------------------------------------------------------------------------------------------------------------- the parent
def run_step(name, args):
    """One child process, one time limit.  Returns the step's result, or None when it failed (the caller then starts nothing more)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--frames", str(args.frames), "--size", str(args.size), "--batch", str(args.batch),
           "--alternations", str(args.alternations)]
    try:
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=STEP_LIMIT_S[name], text=True)
    except subprocess.TimeoutExpired:
        print(f"step {name}: no result within {STEP_LIMIT_S[name]} s", file=sys.stderr)
        return None
    if proc.returncode != 0:
        print(f"step {name}: exit status {proc.returncode}", file=sys.stderr)
        return None
    return json.loads(proc.stdout.strip().splitlines()[-1])


def markdown(result):
    lines = ["# Lens effects: kernel time and delivered rate", "",
             "Written by `tools/lens_probe.py` (one child process and one time limit per step; medians, with the range of the runs)."]
    kernels = result.get("kernels")
    if kernels:
        lines += ["", f"## One batch through each entry ({kernels['device']}, {kernels['batch']} frames of {kernels['size']}^2, one non-identity row and one "
                  "half-kernel per frame, uniform-noise image), beside a device copy of the same bytes", "",
                  "| entry | MB read + written | hot: kernel us (GB/s) | hot: copy us (GB/s) | cold: kernel us (GB/s) | cold: copy us (GB/s) |",
                  "|---|---|---|---|---|---|"]
        for name, row in kernels["kernel_one_batch"].items():
            cells = [f"{row[t][k + '_us']:.1f} ({row[t][k + '_GBps']:.0f})" if t in row else "-" for t in ("hot", "cold") for k in ("kernel", "copy")]
            lines.append(f"| {name} | {row['bytes_read_plus_written'] / 1e6:.1f} | " + " | ".join(cells) + " |")
        lines += ["", "(Maps of a few MB are measured hot only: they never leave the caches between the extract that writes them and the blur.)"]
    rates = result.get("rates")
    if rates:
        fps = rates["frames_per_s"]
        lines += ["", f"## Delivered frames per second ({rates['device']}, {rates['size']}^2, batch {rates['batch']}, {rates['lanes']} lanes, "
                  f"{rates['frames_per_render']} frames per render, {rates['alternations']} alternations, null sink; bloom_size 0.03, sharpen sigma "
                  f"{SHARPEN_SIGMA} px, a non-identity row on every frame)", "",
                  "| render | frames/s (median) | min .. max | vs no lens |", "|---|---|---|---|"]
        for name, s in fps.items():
            base = fps[name.split(" ")[0] + " no lens"]["median"]
            lines.append(f"| {name} | {s['median']:.0f} | {s['min']:.0f} .. {s['max']:.0f} | {s['median'] / base:.3f} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=448, help="frames per timed render (whole batches)")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="run one step in this process and print its JSON (what the parent starts)")
    ap.add_argument("--md", type=str, default=None, help="write the tables here (e.g. profiles/lens.md)")
    ap.add_argument("--json", type=str, default=None, help="also write the raw result here")
    args = ap.parse_args()
    if args.step:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("lens_probe measures on the device: no GPU visible")
        print(json.dumps(STEPS[args.step](args)))
        return 0
    result = {}
    for name in ("kernels", "rates"):
        result[name] = run_step(name, args)
        if result[name] is None:  # a failed step ends the probe: nothing more is started on the device
            break
    result = {k: v for k, v in result.items() if v is not None}
    print(json.dumps(result))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    if args.md and result:
        with open(args.md, "w") as f:
            f.write(markdown(result))
    return 0 if len(result) == 2 else 1


if __name__ == "__main__":
    sys.exit(main())
