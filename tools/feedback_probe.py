"""The cost of the frame feedback on one MI355X: the entry's own time (csrc/feedback.hip, maua_feedback_f32) on one batch, in place as the
render calls it — the still path (one launch that walks the batch in registers) and the warp path (one dependent launch per frame) at
each border rule — beside a device copy of the same bytes, and the delivered frame rate of rgb24 renders with a still feedback, with a
warped feedback and with none (the bench configuration: 1024^2, batch 8, three graph lanes, HBM-resident inputs, null sink).  Modelled on
tools/lens_probe.py.

The parent process never touches the device: every step runs in one child process of its own under its own time limit, and a step that
fails, aborts or runs out of time ends the probe (nothing further is started on the device).
    python tools/feedback_probe.py [--frames 448] [--alternations 3] [--md profiles/feedback_probe.md] [--json out.json]"""
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
N_COLD = 6  # x 100 MB at 8 frames of 1024^2: well beyond the 256 MiB Infinity Cache
BORDERS = ("zero", "replicate", "mirror", "wrap")


# ---------------------------------------------------------------------------------------------------------------- the steps (child processes)
def step_kernels(args):
    """One call of the entry on one batch, in place, from a valid state: on the same buffer every call ("hot": what a batch the last layer
    has just written looks like) and rotating over more buffers than the Infinity Cache holds ("cold"), beside a device copy of the bytes
    the call must move — still: the state and every frame read once, every frame and the state written once; warp: per frame the frame and
    its predecessor read once (the four taps of neighbouring lanes share cache lines) and the frame written, the state read and written
    once.  Mode max, gain 0.8: applied over and over the values stay put."""
    import ctypes

    import numpy as np
    import torch

    import maua_stylegan2_amd.audioreactive as ar
    from deep_delivery_probe import graph_time_ms
    from maua_stylegan2_amd import _lib

    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    lib = _lib.load()
    size, batch = args.size, args.batch
    imgs = [torch.rand(batch, 3, size, size, device=dev) * 2.2 - 1.1 for _ in range(N_COLD)]
    state = torch.rand(3, size, size, device=dev) * 2 - 1
    frame = 3 * size * size * 4
    result, counter = {}, {"k": 0}

    def measure(name, moved, feedback, note=""):
        rows, mode, border = feedback.operands(size, size)
        rows = np.ascontiguousarray(np.broadcast_to(rows, (batch, 16)) if rows.shape[0] == 1 else rows)
        plan = (ctypes.c_int * 8)()
        _lib.check(lib.maua_feedback_plan(batch, size, size, rows.ctypes.data, 16, imgs[0].data_ptr(), ctypes.addressof(plan)), "maua_feedback_plan")

        def call(i):
            _lib.check(lib.maua_feedback_f32(imgs[i].data_ptr(), imgs[i].data_ptr(), state.data_ptr(), 1, batch, size, size, rows.ctypes.data, 16, mode, border,
                                             _lib.stream_ptr(dev)), "maua_feedback_f32")

        half = moved // 2
        src = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(N_COLD)]
        dst = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(N_COLD)]

        def rotate(f):
            def run():
                counter["k"] += 1
                f(counter["k"] % N_COLD)
            return run

        row = {"bytes_read_plus_written": moved, "launches": plan[0], "still_launches": plan[1], "note": note}
        for temp, kern, copy in (("hot", lambda: call(0), lambda: dst[0].copy_(src[0])), ("cold", rotate(call), rotate(lambda i: dst[i].copy_(src[i])))):
            k_ms = statistics.median(graph_time_ms(kern, 16) for _ in range(5))
            c_ms = statistics.median(graph_time_ms(copy, 16) for _ in range(5))
            row[temp] = {"kernel_us": k_ms * 1e3, "kernel_GBps": moved / (k_ms * 1e-3) / 1e9, "copy_us": c_ms * 1e3, "copy_GBps": 2 * half / (c_ms * 1e-3) / 1e9}
        result[name] = row
        print(f"{name}: " + ", ".join(f"{t} {row[t]['kernel_us']:.1f} us (copy {row[t]['copy_us']:.1f})" for t in ("hot", "cold")), file=sys.stderr, flush=True)

    measure("still path (one launch)", (2 * batch + 2) * frame, ar.Feedback(gain=0.8, mode="max"))
    k = np.arange(batch)
    for border in BORDERS:
        fb = ar.Feedback(batch, gain=0.8, zoom=1.01 + 0.002 * k, rotate=0.3 + 0.05 * k, translate=(0.002, -0.001), mode="max", border=border)
        measure(f"warp path, border {border} ({batch} launches)", (3 * batch + 2) * frame, fb)
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
    kick = 0.05 + np.clip(np.sin(2 * np.pi * 2 * t), 0, 1) ** 4  # (never 0: every frame moves)
    feedbacks = {"no feedback": None,
                 "still feedback": ar.Feedback(n, gain=0.7 + 0.2 * kick, mode="max"),
                 "warped feedback": ar.Feedback(n, gain=0.7 + 0.2 * kick, zoom=1 + 0.03 * kick, rotate=0.3, mode="max", border="mirror")}

    def delivered(feedback):
        gc.collect()
        torch.cuda.synchronize()
        start = time.perf_counter()
        # output_file=None: the null sink — every frame still lands in pinned host memory and passes through the ordered sink thread
        written = render.render_fed(g, lat, noise, 0, n / 30.0, batch, size, None, None, 1.0, [], {}, False, "slow", None, pipe_pix_fmt="rgb24", feedback=feedback)
        torch.cuda.synchronize()
        assert written == n
        return n / (time.perf_counter() - start)

    for name in feedbacks:
        delivered(feedbacks[name])  # captures the lanes of both frame kinds, sizes the rings
    rates = {name: [] for name in feedbacks}
    order = list(feedbacks)
    for k in range(args.alternations):
        for name in (order if k % 2 == 0 else order[::-1]):
            delivered(feedbacks[name])  # (every configuration is rendered twice, the warm render counts)
            rates[name].append(delivered(feedbacks[name]))
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
    lines = ["# Frame feedback: kernel time and delivered rate", "",
             "Written by `tools/feedback_probe.py` (one child process and one time limit per step; medians, with the range of the runs)."]
    kernels = result.get("kernels")
    if kernels:
        lines += ["", f"## One call of maua_feedback_f32 ({kernels['device']}, {kernels['batch']} frames of {kernels['size']}^2, in place, a valid state, "
                  "mode max, uniform-noise image), beside a device copy of the same bytes", "",
                  "| rows | launches | MB read + written | hot: entry us (GB/s) | hot: copy us (GB/s) | cold: entry us (GB/s) | cold: copy us (GB/s) |",
                  "|---|---|---|---|---|---|---|"]
        for name, row in kernels["kernel_one_batch"].items():
            cells = [f"{row[t][k + '_us']:.1f} ({row[t][k + '_GBps']:.0f})" for t in ("hot", "cold") for k in ("kernel", "copy")]
            lines.append(f"| {name} | {row['launches']} | {row['bytes_read_plus_written'] / 1e6:.1f} | " + " | ".join(cells) + " |")
        lines += ["", "(The warp path's bytes count a frame's predecessor once: the four taps of neighbouring lanes share cache lines.  Its launches "
                  "depend on one another, so the entry's time holds the gaps between them as well.)"]
    rates = result.get("rates")
    if rates:
        fps = rates["frames_per_s"]
        lines += ["", f"## Delivered frames per second ({rates['device']}, {rates['size']}^2, batch {rates['batch']}, {rates['lanes']} lanes, "
                  f"{rates['frames_per_render']} frames per render, {rates['alternations']} alternations, rgb24, null sink; a non-neutral row on every frame)", "",
                  "| render | frames/s (median) | min .. max | vs no feedback |", "|---|---|---|---|"]
        base = fps["no feedback"]["median"]
        for name, s in fps.items():
            lines.append(f"| {name} | {s['median']:.0f} | {s['min']:.0f} .. {s['max']:.0f} | {s['median'] / base:.3f} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=448, help="frames per timed render (whole batches)")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="run one step in this process and print its JSON (what the parent starts)")
    ap.add_argument("--md", type=str, default=None, help="write the tables here (e.g. profiles/feedback_probe.md)")
    ap.add_argument("--json", type=str, default=None, help="also write the raw result here")
    args = ap.parse_args()
    if args.step:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("feedback_probe measures on the device: no GPU visible")
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
