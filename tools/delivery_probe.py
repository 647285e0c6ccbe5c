"""Delivered frame rate of the two pipe formats, A/B in one process on one MI355X: the bench configuration (1024^2, batch 8, three graph
lanes, HBM-resident inputs) rendered through render.synthesize and the product's single-GPU delivery loop (device ring -> pinned host ring
-> ordered null sink) as rgb24 and as yuv420p, alternating; plus render.synthesize alone (frames left in HBM), the conversion kernel's own
time and bytes/s, and a device copy that moves the same number of bytes for comparison.
    python tools/delivery_probe.py [--frames 896] [--alternations 8] [--json out.json]"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maua_stylegan2_amd import render, seeding  # noqa: E402
from maua_stylegan2_amd.models.stylegan2 import Generator  # noqa: E402


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "runs": [round(v, 1) for v in values]}


def graph_time_ms(fn, iters):
    """Mean device time of one ``fn()``: ``iters`` calls captured into one graph (the host's launch rate is then out of the picture — a
    Python call takes about as long as this kernel runs), the graph replayed once to warm and once between two HIP events."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=896, help="frames per timed render (whole batches)")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--alternations", type=int, default=8)
    ap.add_argument("--json", type=str, default=None, help="also write the result here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("delivery_probe measures on the device: no GPU visible")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    size, batch = args.size, args.batch
    n = (args.frames // batch) * batch
    g = Generator(size, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(size, seed=0))
    g = g.to(dev).eval()
    lat = torch.randn(n, g.n_latent, 512, device=dev)
    noise = [torch.randn(n, 1, r, r, device=dev) if r <= 256 else None for r in seeding.noise_sizes(size)]

    def synthesized():
        gc.collect()  # (generate() collects once before it renders: no timed region inherits the previous one's garbage)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in render.synthesize(g, lat, noise, batch):
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

    synthesized()  # captures the lanes
    for fmt in render.PIPE_PIX_FMTS:  # pins the rings of both frame shapes once, loads the kernel
        delivered(fmt)
        delivered(fmt)
    # The staging rings are kept per device and re-made when the frame shape changes, i.e. by the first render after a change of format: a job
    # renders in ONE format, so every alternation renders each format twice and the second, warm render is the figure ("switch": the first).
    rates = {"synthesized": [], "rgb24": [], "yuv420p": [], "rgb24_switch": [], "yuv420p_switch": []}
    for k in range(args.alternations):
        order = ("rgb24", "yuv420p") if k % 2 == 0 else ("yuv420p", "rgb24")
        for fmt in order:
            rates[fmt + "_switch"].append(delivered(fmt))
            rates[fmt].append(delivered(fmt))
        rates["synthesized"].append(synthesized())
        print(f"alternation {k} ({' then '.join(order)}): rgb24 {rates['rgb24'][-1]:.0f}/s (after the switch {rates['rgb24_switch'][-1]:.0f}) | "
              f"yuv420p {rates['yuv420p'][-1]:.0f}/s (after the switch {rates['yuv420p_switch'][-1]:.0f}) | synthesized "
              f"{rates['synthesized'][-1]:.0f}/s", flush=True)

    # the kernel alone on one batch, and a device copy of the same number of bytes (read + written).  "hot": the same 38 MB every call
    # (they stay in the 256 MiB Infinity Cache, as a batch the last layer has just written does); "cold": rotating over more buffers than
    # the cache holds
    px = batch * size * size
    bytes_moved = px * 3 + px * 3 // 2
    n_cold = 16
    srcs = [torch.randint(0, 256, (batch, size, size, 3), dtype=torch.uint8, device=dev) for _ in range(n_cold)]
    scratch = {}
    half = bytes_moved // 2
    copy_src = [torch.randint(0, 256, (half,), dtype=torch.uint8, device=dev) for _ in range(n_cold)]
    copy_dst = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(n_cold)]
    counter = {"k": 0, "c": 0}

    def kernel_hot():
        render.frames_to_yuv420p(srcs[0], scratch)

    def kernel_cold():
        counter["k"] += 1
        render.frames_to_yuv420p(srcs[counter["k"] % n_cold], scratch)

    def copy_hot():
        copy_dst[0].copy_(copy_src[0])

    def copy_cold():
        counter["c"] += 1
        copy_dst[counter["c"] % n_cold].copy_(copy_src[counter["c"] % n_cold])

    for s in srcs:
        render.frames_to_yuv420p(s, scratch)  # allocates the outputs outside the timed loops
    kernel = {}
    for name, kern, copy in (("hot", kernel_hot, copy_hot), ("cold", kernel_cold, copy_cold)):
        k_ms = statistics.median(graph_time_ms(kern, 96) for _ in range(5))
        c_ms = statistics.median(graph_time_ms(copy, 96) for _ in range(5))
        kernel[name] = {"kernel_us": k_ms * 1e3, "kernel_GBps": bytes_moved / (k_ms * 1e-3) / 1e9, "copy_us": c_ms * 1e3,
                        "copy_GBps": 2 * half / (c_ms * 1e-3) / 1e9, "kernel_fraction_of_copy_rate": c_ms / k_ms}
    result = {"device": torch.cuda.get_device_name(0), "size": size, "batch": batch, "lanes": 3, "frames_per_render": n,
              "alternations": args.alternations, "frames_per_s": {k: spread(v) for k, v in rates.items()},
              "bytes_per_batch_read_plus_written": bytes_moved, "kernel_one_batch": kernel}
    a, b = result["frames_per_s"]["rgb24"], result["frames_per_s"]["yuv420p"]
    result["yuv420p_minus_rgb24_median"] = b["median"] - a["median"]
    result["rgb24_spread"] = a["max"] - a["min"]
    print(json.dumps(result))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
