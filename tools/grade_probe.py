"""The cost of a colour grade on one MI355X: the grade kernel's own time (csrc/grade.hip, both entries, without a LUT and with 17^3, 33^3
and 65^3 tables) on one batch beside a device copy of the same bytes, and the delivered frame rate of a graded rgb24 and a graded
yuv420p10le render beside the ungraded ones (the bench configuration: 1024^2, batch 8, three graph lanes, HBM-resident inputs, null sink).
Modelled on tools/deep_delivery_probe.py.

The parent process never touches the device: every step runs in one child process of its own under its own time limit, and a step that
fails, aborts or runs out of time ends the probe (nothing further is started on the device).
    python tools/grade_probe.py [--frames 448] [--alternations 3] [--md profiles/grade.md] [--json out.json]"""
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
STEP_LIMIT_S = {"kernels": 240, "rates": 420}
LUT_SIZES = (0, 17, 33, 65)
RATE_FORMATS = ("rgb24", "yuv420p10le")


def _film_look(rgb):
    """A smooth, clearly non-linear table: an S-curve and a little cross-talk."""
    import numpy as np

    curve = rgb * rgb * (3 - 2 * rgb)
    return np.clip(0.85 * curve + 0.15 * curve[..., ::-1], 0, 1)


# ---------------------------------------------------------------------------------------------------------------- the steps (child processes)
def step_kernels(args):
    """Both entries on one batch, rotating over more buffers than the 256 MiB Infinity Cache holds ("cold") and on the same buffers every
    call ("hot": what a batch the last layer has just written looks like), beside a device copy of the same bytes read + written.  Every
    frame has its own non-identity row (power 1: the common modulated grade); the image is uniform noise over [-1.1, 1.1], i.e. the LUT
    gathers are as scattered as they can be — a picture's neighbouring pixels share cells."""
    import numpy as np
    import torch

    import maua_stylegan2_amd.audioreactive as ar
    from deep_delivery_probe import graph_time_ms
    from maua_stylegan2_amd import _lib

    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    lib = _lib.load()
    size, batch = args.size, args.batch
    px = batch * size * size
    n_cold = 12
    imgs = [torch.rand(batch, 3, size, size, device=dev) * 2.2 - 1.1 for _ in range(n_cold)]
    outs = [torch.empty(px * 3, dtype=torch.float32, device=dev) for _ in range(n_cold)]
    k = np.arange(batch)
    result = {}
    counter = {"k": 0}
    for entry, out_bytes in (("maua_grade_f32", 12), ("maua_grade_to_u8", 3)):
        for n in LUT_SIZES:
            grade = ar.Grade(batch, exposure=0.1 + 0.05 * k, saturation=1.2, hue=10.0 + k, lut=ar.lut_from_function(_film_look, n) if n else None)
            rows, lut = grade.rows(dev), grade.lut_table(dev)
            moved = px * (12 + out_bytes)
            fn = getattr(lib, entry)

            def call(i, fn=fn, rows=rows, lut=lut, n=n, entry=entry):
                _lib.check(fn(imgs[i].data_ptr(), outs[i].data_ptr(), batch, size, size, rows.data_ptr(), 24, _lib.ptr(lut), n, _lib.stream_ptr(dev)), entry)

            half = moved // 2
            copy_src = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(n_cold)]
            copy_dst = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(n_cold)]

            def rotate(f):
                def run():
                    counter["k"] += 1
                    f(counter["k"] % n_cold)
                return run

            row = {"bytes_read_plus_written": moved, "lut_bytes": 16 * n ** 3}
            for temp, kern, copy in (("hot", lambda: call(0), lambda: copy_dst[0].copy_(copy_src[0])),
                                     ("cold", rotate(call), rotate(lambda i: copy_dst[i].copy_(copy_src[i])))):
                k_ms = statistics.median(graph_time_ms(kern, 48) for _ in range(5))
                c_ms = statistics.median(graph_time_ms(copy, 48) for _ in range(5))
                row[temp] = {"kernel_us": k_ms * 1e3, "kernel_GBps": moved / (k_ms * 1e-3) / 1e9, "copy_us": c_ms * 1e3,
                             "copy_GBps": 2 * half / (c_ms * 1e-3) / 1e9}
            name = f"{entry[5:]} {'no LUT' if not n else f'{n}^3'}"
            result[name] = row
            del copy_src, copy_dst
            print(f"{name}: hot {row['hot']['kernel_us']:.1f} us (copy {row['hot']['copy_us']:.1f}), cold {row['cold']['kernel_us']:.1f} us "
                  f"(copy {row['cold']['copy_us']:.1f})", file=sys.stderr, flush=True)
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
    flash = np.clip(np.sin(2 * np.pi * 2 * t), 0, 1) ** 4
    grades = {"ungraded": None,
              "graded": ar.Grade(n, exposure=0.8 * flash, saturation=1 + 0.3 * np.sin(t), hue=20 * np.sin(0.5 * t)),
              "graded + 33^3 LUT": ar.Grade(n, exposure=0.8 * flash, saturation=1 + 0.3 * np.sin(t), hue=20 * np.sin(0.5 * t),
                                            lut=ar.lut_from_function(_film_look, 33))}

    def delivered(pix_fmt, grade):
        gc.collect()
        torch.cuda.synchronize()
        start = time.perf_counter()
        # output_file=None: the null sink — every frame still lands in pinned host memory and passes through the ordered sink thread
        written = render.render_graded(g, lat, noise, 0, n / 30.0, batch, size, None, None, 1.0, [], {}, False, "slow", None, pipe_pix_fmt=pix_fmt,
                                       grade=grade)
        torch.cuda.synchronize()
        assert written == n
        return n / (time.perf_counter() - start)

    configs = [(fmt, name) for fmt in RATE_FORMATS for name in grades]
    for fmt, name in configs:
        delivered(fmt, grades[name])  # captures the lanes of both frame kinds, sizes the rings
    rates = {f"{fmt} {name}": [] for fmt, name in configs}
    for k in range(args.alternations):
        for fmt, name in (configs if k % 2 == 0 else configs[::-1]):
            # (the staging rings are re-made when the frame shape changes: every configuration is rendered twice, the warm render counts)
            delivered(fmt, grades[name])
            rates[f"{fmt} {name}"].append(delivered(fmt, grades[name]))
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
    lines = ["# Colour grading: kernel time and delivered rate", "",
             "Written by `tools/grade_probe.py` (one child process and one time limit per step; medians, with the range of the runs)."]
    kernels = result.get("kernels")
    if kernels:
        lines += ["", f"## One batch through each entry ({kernels['device']}, {kernels['batch']} frames of {kernels['size']}^2, one non-identity row per "
                  "frame, uniform-noise image), beside a device copy of the same bytes", "",
                  "| entry | MB read + written | LUT KB | hot: kernel us (GB/s) | hot: copy us (GB/s) | cold: kernel us (GB/s) | cold: copy us (GB/s) |",
                  "|---|---|---|---|---|---|---|"]
        for name, row in kernels["kernel_one_batch"].items():
            cells = [f"{row[t][k + '_us']:.1f} ({row[t][k + '_GBps']:.0f})" for t in ("hot", "cold") for k in ("kernel", "copy")]
            lines.append(f"| {name} | {row['bytes_read_plus_written'] / 1e6:.1f} | {row['lut_bytes'] / 1024:.0f} | " + " | ".join(cells) + " |")
    rates = result.get("rates")
    if rates:
        fps = rates["frames_per_s"]
        lines += ["", f"## Delivered frames per second ({rates['device']}, {rates['size']}^2, batch {rates['batch']}, {rates['lanes']} lanes, "
                  f"{rates['frames_per_render']} frames per render, {rates['alternations']} alternations, null sink)", "",
                  "| render | frames/s (median) | min .. max | vs ungraded |", "|---|---|---|---|"]
        for name, s in fps.items():
            base = fps[name.split(" ")[0] + " ungraded"]["median"]
            lines.append(f"| {name} | {s['median']:.0f} | {s['min']:.0f} .. {s['max']:.0f} | {s['median'] / base:.3f} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=448, help="frames per timed render (whole batches)")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="run one step in this process and print its JSON (what the parent starts)")
    ap.add_argument("--md", type=str, default=None, help="write the tables here (e.g. profiles/grade.md)")
    ap.add_argument("--json", type=str, default=None, help="also write the raw result here")
    args = ap.parse_args()
    if args.step:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("grade_probe measures on the device: no GPU visible")
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
