"""Delivered frame rate of the deep pipe formats beside rgb24 and yuv420p, and the deep kernels' own time, on one MI355X: the bench
configuration (1024^2, batch 8, three graph lanes, HBM-resident inputs) rendered through the product's single-GPU delivery loop (device
ring -> pinned host ring -> ordered null sink), every format in the same call, alternating; then each kernel of csrc/deep_frames.hip on
one batch beside a device copy that moves the same number of bytes.  Modelled on tools/delivery_probe.py.

The parent process never touches the device: every step runs in one child process of its own under its own time limit, and a step that
fails, aborts or runs out of time ends the probe (nothing further is started on the device).
    python tools/deep_delivery_probe.py [--frames 448] [--alternations 3] [--md profiles/deep_delivery.md] [--json out.json]"""
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
FORMATS_8 = ("rgb24", "yuv420p")
STEP_LIMIT_S = {"rates": 420, "kernels": 180}


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "runs": [round(v, 1) for v in values]}


# ---------------------------------------------------------------------------------------------------------------- the steps (child processes)
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
    formats = FORMATS_8 + render.DEEP_PIX_FMTS

    def synthesized(frames):
        gc.collect()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in render.synthesize(g, lat, noise, batch, **({} if frames == "u8" else {"frames": frames})):
            pass
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t)

    def delivered(pix_fmt):
        gc.collect()
        torch.cuda.synchronize()
        t = time.perf_counter()
        # output_file=None: the null sink — every frame still lands in pinned host memory and passes through the ordered sink thread
        written = render.render_shard(g, lat, noise, 0, n / 30.0, batch, size, None, None, 1.0, [], {}, False, "slow", None, pipe_pix_fmt=pix_fmt)
        torch.cuda.synchronize()
        assert written == n
        return n / (time.perf_counter() - t)

    for kind in ("u8", "f32"):
        synthesized(kind)  # captures the lanes of both frame kinds
    # The staging rings are re-made when the frame shape changes, i.e. by the first render after a change of format: a job renders in ONE
    # format, so every format is rendered twice in a row and the second, warm render is the figure (as tools/delivery_probe.py does).
    rates = {fmt: [] for fmt in formats}
    rates.update(synthesized_u8=[], synthesized_f32=[])
    for k in range(args.alternations):
        order = formats if k % 2 == 0 else formats[::-1]
        for fmt in order:
            delivered(fmt)
            rates[fmt].append(delivered(fmt))
        rates["synthesized_u8"].append(synthesized("u8"))
        rates["synthesized_f32"].append(synthesized("f32"))
        print(f"alternation {k}: " + " | ".join(f"{name} {v[-1]:.0f}/s" for name, v in rates.items()), file=sys.stderr, flush=True)
    bytes_per_frame = {fmt: int(render._stream_frame_shape(g, size, fmt)[0]) if fmt != "rgb24" else size * size * 3 for fmt in formats}
    return {"device": torch.cuda.get_device_name(0), "size": size, "batch": batch, "lanes": 3, "frames_per_render": n,
            "alternations": args.alternations, "frames_per_s": {k: spread(v) for k, v in rates.items()}, "bytes_per_frame": bytes_per_frame}


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


def step_kernels(args):
    """Each deep kernel on one batch, rotating over more buffers than the 256 MiB Infinity Cache holds ("cold") and on the same buffers
    every call ("hot": what a batch the last layer has just written looks like), beside a device copy of the same bytes read + written."""
    import torch

    from maua_stylegan2_amd import _lib

    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    lib = _lib.load()
    size, batch = args.size, args.batch
    px = batch * size * size
    n_cold = 12
    imgs = [torch.rand(batch, 3, size, size, device=dev) * 2.2 - 1.1 for _ in range(n_cold)]
    masters = [torch.randint(-32768, 32767, (batch, size, size, 3), dtype=torch.int16, device=dev) for _ in range(n_cold)]
    wide = torch.randint(-32768, 32767, (batch // 4 or 1, 1024, 2048, 3), dtype=torch.int16, device=dev)
    outs = [torch.empty(px * 3, dtype=torch.int16, device=dev) for _ in range(n_cold)]
    wide_out = torch.empty((wide.shape[0], 1080, 1920, 3), dtype=torch.int16, device=dev)

    def sub_samples(sub):
        return {420: px * 3 // 2, 422: px * 2, 444: px * 3}[sub]

    def call(name, *a):
        _lib.check(getattr(lib, name)(*a, _lib.stream_ptr(dev)), name)

    kernels = {"frames_to_u16": (lambda i: call("maua_frames_to_u16", imgs[i].data_ptr(), outs[i].data_ptr(), batch, size, size), px * 12 + px * 6)}
    for sub in (420, 422, 444):
        kernels[f"frames_to_yuv_p10_f32 {sub}"] = (lambda i, s=sub: call("maua_frames_to_yuv_p10_f32", imgs[i].data_ptr(), outs[i].data_ptr(), batch, size,
                                                                        size, s), px * 12 + 2 * sub_samples(sub))
        kernels[f"rgb48_to_yuv_p10 {sub}"] = (lambda i, s=sub: call("maua_rgb48_to_yuv_p10", masters[i].data_ptr(), outs[i].data_ptr(), batch, size, size, s),
                                              px * 6 + 2 * sub_samples(sub))
    wide_bytes = wide.shape[0] * (1024 * 1824 + 1080 * 1920) * 6
    kernels["crop_resize_u16 1824x1024 -> 1920x1080"] = (lambda i: call("maua_crop_resize_u16", wide.data_ptr(), wide_out.data_ptr(), wide.shape[0], 1024,
                                                                        2048, 112, 0, 1824, 1024, 1920, 1080), wide_bytes)
    result = {}
    counter = {"k": 0}
    for name, (fn, moved) in kernels.items():
        half = moved // 2
        copy_src = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(n_cold)]
        copy_dst = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(n_cold)]

        def rotate(f):
            def run():
                counter["k"] += 1
                f(counter["k"] % n_cold)
            return run

        row = {"bytes_read_plus_written": moved}
        for temp, kern, copy in (("hot", lambda: fn(0), lambda: copy_dst[0].copy_(copy_src[0])),
                                 ("cold", rotate(fn), rotate(lambda i: copy_dst[i].copy_(copy_src[i])))):
            k_ms = statistics.median(graph_time_ms(kern, 48) for _ in range(5))
            c_ms = statistics.median(graph_time_ms(copy, 48) for _ in range(5))
            row[temp] = {"kernel_us": k_ms * 1e3, "kernel_GBps": moved / (k_ms * 1e-3) / 1e9, "copy_us": c_ms * 1e3,
                         "copy_GBps": 2 * half / (c_ms * 1e-3) / 1e9}
        result[name] = row
        del copy_src, copy_dst
        print(f"{name}: hot {row['hot']['kernel_us']:.1f} us (copy {row['hot']['copy_us']:.1f}), cold {row['cold']['kernel_us']:.1f} us "
              f"(copy {row['cold']['copy_us']:.1f})", file=sys.stderr, flush=True)
    return {"device": torch.cuda.get_device_name(0), "size": size, "batch": batch, "kernel_one_batch": result}


STEPS = {"rates": step_rates, "kernels": step_kernels}


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
    lines = ["# Deep frame delivery: delivered rate and kernel time", "",
             "Written by `tools/deep_delivery_probe.py` (one child process and one time limit per step; medians, with the range of the runs)."]
    rates = result.get("rates")
    if rates:
        fps = rates["frames_per_s"]
        base = fps["rgb24"]["median"]
        lines += ["", f"## Delivered frames per second ({rates['device']}, {rates['size']}^2, batch {rates['batch']}, {rates['lanes']} lanes, "
                  f"{rates['frames_per_render']} frames per render, {rates['alternations']} alternations, null sink)", "",
                  "| format | bytes per frame | frames/s (median) | min .. max | vs rgb24 |", "|---|---|---|---|---|"]
        for name, s in fps.items():
            size = rates["bytes_per_frame"].get(name, "(stay in HBM)")
            lines.append(f"| {name} | {size} | {s['median']:.0f} | {s['min']:.0f} .. {s['max']:.0f} | {s['median'] / base:.3f} |")
    kernels = result.get("kernels")
    if kernels:
        lines += ["", f"## One batch through each kernel ({kernels['device']}, {kernels['batch']} frames of {kernels['size']}^2; the resize on "
                  "2048-px frames), beside a device copy of the same bytes", "",
                  "| kernel | MB read + written | hot: kernel us (GB/s) | hot: copy us (GB/s) | cold: kernel us (GB/s) | cold: copy us (GB/s) |",
                  "|---|---|---|---|---|---|"]
        for name, row in kernels["kernel_one_batch"].items():
            cells = [f"{row[t][k + '_us']:.1f} ({row[t][k + '_GBps']:.0f})" for t in ("hot", "cold") for k in ("kernel", "copy")]
            lines.append(f"| {name} | {row['bytes_read_plus_written'] / 1e6:.1f} | " + " | ".join(cells) + " |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=448, help="frames per timed render (whole batches)")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="run one step in this process and print its JSON (what the parent starts)")
    ap.add_argument("--md", type=str, default=None, help="write the table here (e.g. profiles/deep_delivery.md)")
    ap.add_argument("--json", type=str, default=None, help="also write the raw result here")
    args = ap.parse_args()
    if args.step:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("deep_delivery_probe measures on the device: no GPU visible")
        print(json.dumps(STEPS[args.step](args)))
        return 0
    result = {}
    for name in ("rates", "kernels"):
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
