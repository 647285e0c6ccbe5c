"""The device resampler (csrc/resample.hip) on one MI355X: each instance's own time at 1024^2 -> 1920x1080, -> 3840x2160 and -> 512^2 beside a
device copy of the same bytes in + out; the delivered frame rate of those renders (1024^2, batch 8, three graph lanes, null sink: the
bench configuration through render_delivered) beside the plain rgb24 render; and Pillow's resize of one such frame on the host.  Modelled
on tools/deep_delivery_probe.py.

The parent process never touches the device: every step runs in one child process of its own under its own time limit, and a step that
fails, aborts or runs out of time ends the probe (nothing further is started on the device).
    python tools/resample_probe.py [--frames 224] [--alternations 3] [--md profiles/resample.md] [--json out.json]"""
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
TARGETS = ((1920, 1080), (3840, 2160), (512, 512))
STEP_LIMIT_S = {"kernels": 240, "rates": 420, "pillow": 120}


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "runs": [round(v, 1) for v in values]}


def graph_time_ms(fn, iters):
    """Mean device time of one ``fn()``: ``iters`` calls captured into one graph, replayed once to warm and once between two events."""
    import torch

    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(iters):
            fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    graph.replay()
    torch.cuda.synchronize()
    start.record()
    graph.replay()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


# ---------------------------------------------------------------------------------------------------------------- the steps (child processes)
def step_kernels(args):
    """One batch through resize_frames per target, sample type and filter, on the same buffers every call ("hot": a batch the last layer
    has just written) and rotating over more buffers than the Infinity Cache holds ("cold"), beside a device copy of the bytes in + out."""
    import torch

    from maua_stylegan2_amd import _lib, render

    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    size, batch = args.size, args.batch
    result = {}
    for (w, h) in TARGETS:
        for dtype, sz in ((torch.uint8, 1), (torch.int16, 2)):
            for filt in ("lanczos", "bilinear"):
                resize = render.FrameResize((w, h), filt, "crop")
                moved = batch * 3 * sz * (size * size + w * h)  # (the whole source counted, although a crop reads less)
                n_cold = max(2, min(12, int(1.5 * 2 ** 30 // moved)))
                srcs = [torch.randint(0, 255, (batch, size, size, 3), device=dev).to(dtype) for _ in range(n_cold)]
                scratch = {}
                box, window, (kx, bx, ksx), (ky, by, ksy) = render._resize_tables(dev, size, size, resize)
                _, plan, fields = _lib.planned_resample(sz, batch, size, size, h, w, *window, ksx, ksy)
                counter = {"k": 0}

                def hot():
                    render.resize_frames(srcs[0], resize, scratch)

                def cold():
                    counter["k"] += 1
                    render.resize_frames(srcs[counter["k"] % n_cold], resize, scratch)

                half = moved // 2
                copy_src = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(n_cold)]
                copy_dst = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(n_cold)]

                def copy_hot():
                    copy_dst[0].copy_(copy_src[0])

                def copy_cold():
                    counter["k"] += 1
                    copy_dst[counter["k"] % n_cold].copy_(copy_src[counter["k"] % n_cold])

                for _ in range(n_cold):  # every output buffer and workspace exists before anything is captured
                    cold()
                row = {"plan": plan + " " + " ".join(f"{k}={v}" for k, v in sorted(fields.items())), "taps": [ksx, ksy], "bytes_in_plus_out": moved}
                for temp, kern, copy in (("hot", hot, copy_hot), ("cold", cold, copy_cold)):
                    iters = 24 if temp == "hot" else n_cold * 2
                    k_ms = statistics.median(graph_time_ms(kern, iters) for _ in range(5))
                    c_ms = statistics.median(graph_time_ms(copy, iters) for _ in range(5))
                    row[temp] = {"kernel_us": k_ms * 1e3, "kernel_GBps": moved / (k_ms * 1e-3) / 1e9, "copy_us": c_ms * 1e3,
                                 "copy_GBps": 2 * half / (c_ms * 1e-3) / 1e9}
                name = f"{size}^2 -> {w}x{h} {'u8' if sz == 1 else 'u16'} {filt}"
                result[name] = row
                print(f"{name}: {row['plan']}: hot {row['hot']['kernel_us']:.1f} us (copy {row['hot']['copy_us']:.1f}), cold "
                      f"{row['cold']['kernel_us']:.1f} us (copy {row['cold']['copy_us']:.1f})", file=sys.stderr, flush=True)
                del srcs, scratch, copy_src, copy_dst
                gc.collect()
                torch.cuda.empty_cache()
    return {"device": torch.cuda.get_device_name(0), "size": size, "batch": batch, "kernel_one_batch": result}


def step_rates(args):
    import torch

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
    jobs = [("rgb24 plain", None, None)] + [(f"rgb24 {w}x{h} lanczos", None, render.FrameResize((w, h))) for w, h in TARGETS]
    jobs += [("yuv420p 1920x1080 lanczos", "yuv420p", render.FrameResize((1920, 1080))),
             ("yuv420p10le 1920x1080 lanczos", "yuv420p10le", render.FrameResize((1920, 1080)))]

    def delivered(pix_fmt, resize):
        gc.collect()
        torch.cuda.synchronize()
        t = time.perf_counter()
        written = render.render_delivered(g, lat, noise, 0, n / 30.0, batch, size, None, None, 1.0, [], {}, False, "slow", None,
                                          pipe_pix_fmt=pix_fmt, resize=resize)
        torch.cuda.synchronize()
        assert written == n
        return n / (time.perf_counter() - t)

    rates = {name: [] for name, _, _ in jobs}
    for k in range(args.alternations):
        for name, pix_fmt, resize in (jobs if k % 2 == 0 else jobs[::-1]):
            delivered(pix_fmt, resize)  # (the staging rings are re-made when the frame shape changes: the second, warm render is the figure)
            rates[name].append(delivered(pix_fmt, resize))
        print(f"alternation {k}: " + " | ".join(f"{name} {v[-1]:.0f}/s" for name, v in rates.items()), file=sys.stderr, flush=True)
    return {"device": torch.cuda.get_device_name(0), "size": size, "batch": batch, "lanes": 3, "frames_per_render": n,
            "alternations": args.alternations, "frames_per_s": {k: spread(v) for k, v in rates.items()}}


def step_pillow(args):
    """Pillow's own resize of one frame on the host (one thread): what a per-frame host resize costs next to 0.7 ms of synthesis."""
    import numpy as np
    from PIL import Image

    frame = Image.fromarray(np.random.default_rng(0).integers(0, 256, (args.size, args.size, 3), dtype=np.uint8))
    result = {}
    for (w, h) in TARGETS:
        for name, flt in (("lanczos", Image.LANCZOS), ("bilinear", Image.BILINEAR)):
            times = []
            for _ in range(7):
                t = time.perf_counter()
                frame.resize((w, h), flt)
                times.append((time.perf_counter() - t) * 1e3)
            result[f"{args.size}^2 -> {w}x{h} {name}"] = spread(times)
    return {"pillow_ms_per_frame": result}


STEPS = {"kernels": step_kernels, "rates": step_rates, "pillow": step_pillow}


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
    lines = ["# Delivery at any size: the resampler's time and the delivered rate", "",
             "Written by `tools/resample_probe.py` (one child process and one time limit per step; medians, with the range of the runs)."]
    kernels = result.get("kernels")
    if kernels:
        lines += ["", f"## One batch through the resampler ({kernels['device']}, {kernels['batch']} frames of {kernels['size']}^2, fit crop), beside a "
                  "device copy of the same bytes in + out", "",
                  "| geometry | plan | taps x, y | MB in + out | hot: kernel us (GB/s) | hot: copy us (GB/s) | cold: kernel us (GB/s) | cold: copy us (GB/s) |",
                  "|---|---|---|---|---|---|---|---|"]
        for name, row in kernels["kernel_one_batch"].items():
            cells = [f"{row[t][k + '_us']:.1f} ({row[t][k + '_GBps']:.0f})" for t in ("hot", "cold") for k in ("kernel", "copy")]
            lines.append(f"| {name} | {row['plan']} | {row['taps'][0]}, {row['taps'][1]} | {row['bytes_in_plus_out'] / 1e6:.1f} | " + " | ".join(cells) + " |")
    rates = result.get("rates")
    if rates:
        fps = rates["frames_per_s"]
        base = fps["rgb24 plain"]["median"]
        lines += ["", f"## Delivered frames per second ({rates['device']}, {rates['size']}^2, batch {rates['batch']}, {rates['lanes']} lanes, "
                  f"{rates['frames_per_render']} frames per render, {rates['alternations']} alternations, null sink)", "",
                  "| render | frames/s (median) | min .. max | vs plain rgb24 |", "|---|---|---|---|"]
        for name, s in fps.items():
            lines.append(f"| {name} | {s['median']:.0f} | {s['min']:.0f} .. {s['max']:.0f} | {s['median'] / base:.3f} |")
    pillow = result.get("pillow")
    if pillow:
        lines += ["", "## Pillow's resize of one frame on the host (one thread)", "", "| geometry | ms per frame (median) | min .. max |", "|---|---|---|"]
        for name, s in pillow["pillow_ms_per_frame"].items():
            lines.append(f"| {name} | {s['median']:.1f} | {s['min']:.1f} .. {s['max']:.1f} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=224, help="frames per timed render (whole batches)")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="run one step in this process and print its JSON (what the parent starts)")
    ap.add_argument("--md", type=str, default=None, help="write the tables here (e.g. profiles/resample.md)")
    ap.add_argument("--json", type=str, default=None, help="also write the raw result here")
    args = ap.parse_args()
    if args.step:
        if args.step != "pillow":
            import torch

            if not torch.cuda.is_available():
                raise SystemExit("resample_probe measures on the device: no GPU visible")
        print(json.dumps(STEPS[args.step](args)))
        return 0
    result = {}
    for name in ("kernels", "rates", "pillow"):
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
    return 0 if len(result) == 3 else 1


if __name__ == "__main__":
    sys.exit(main())
