"""Cost of temporal supersampling, A/B in one process on one MI355X: the bench configuration (1024^2, batch 8, three graph lanes,
HBM-resident inputs) rendered through the product's single-GPU delivery loop (device ring -> pinned host ring -> ordered null sink) plainly
and with a fold of N sub-frames, alternating, as synthesised frames/s; the fold kernel's own time per batch by HIP events in both light
modes for N in 2, 4, 8 (launched eagerly, and captured into one graph) next to a device copy of the same number of bytes in the same process; and the delivered bytes per synthesised frame.
    python tools/temporal_fold_probe.py [--frames 960] [--subframes 8] [--alternations 4] [--json out.json]"""
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


def event_time_us(fn, launches):
    """Mean device time of one ``fn()`` between two HIP events around ``launches`` back-to-back calls, in microseconds (the calls are
    queued faster than they run once the queue is primed: a warm-up of the same length runs first)."""
    for _ in range(launches):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / launches


def graph_time_us(fn, launches):
    """The same mean with the ``launches`` calls captured into one graph and the replay between the two events: the host's call rate (a
    ctypes call takes about as long as this kernel runs) is then out of the picture."""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(launches):
            fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    graph.replay()
    torch.cuda.synchronize()
    start.record()
    graph.replay()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=960, help="synthesised frames per timed render (whole batches)")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--subframes", type=int, default=8)
    ap.add_argument("--alternations", type=int, default=4)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--json", type=str, default=None, help="also write the result here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("temporal_fold_probe measures on the device: no GPU visible")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    size, batch = args.size, args.batch
    n = (args.frames // batch) * batch
    g = Generator(size, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(size, seed=0))
    g = g.to(dev).eval()
    lat = torch.randn(n, g.n_latent, 512, device=dev)
    noise = [torch.randn(n, 1, r, r, device=dev) if r <= 256 else None for r in seeding.noise_sizes(size)]
    folds = {"plain": None, "folded": render.TemporalFold(args.subframes), "folded_linear": render.TemporalFold(args.subframes, "tent", "linear")}

    def rendered(name):
        """Synthesised frames/s of one render (null sink: every delivered frame still lands in pinned host memory and passes through
        the ordered sink thread)."""
        fold = folds[name]
        gc.collect()
        torch.cuda.synchronize()
        t = time.perf_counter()
        written = render.render_folded(g, lat, noise, 0, n / 30.0, batch, size, None, None, 1.0, [], {}, False, "slow", None, fold=fold)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        assert written == n // (fold.subframes if fold else 1)
        return n / dt

    for name in folds:  # captures the lanes, pins the rings of both batch sizes once, loads the kernels
        rendered(name)
        rendered(name)
    plain_twice = [rendered("plain"), rendered("plain")]  # the spread of the plain render, before anything is compared with it
    print(f"plain, twice: {plain_twice[0]:.0f} and {plain_twice[1]:.0f} synthesised frames/s", flush=True)
    # (the staging rings are re-made when the batch shape changes, i.e. by the first render after a switch: every alternation renders each
    # variant twice and the second, warm render is the figure)
    rates = {name: [] for name in folds}
    for k in range(args.alternations):
        order = list(folds) if k % 2 == 0 else list(folds)[::-1]
        for name in order:
            rendered(name)
            rates[name].append(rendered(name))
        print(f"alternation {k}: " + " | ".join(f"{name} {rates[name][-1]:.0f}/s" for name in folds), flush=True)

    # the kernel alone on one batch of frames, and a device copy that reads and writes the same number of bytes
    frames = torch.randint(0, 256, (batch, size, size, 3), dtype=torch.uint8, device=dev)
    kernel = {}
    for sub in (2, 4, 8):
        if batch % sub:
            continue
        moved = frames.numel() + frames.numel() // sub
        copy_src = torch.randint(0, 256, (moved // 2,), dtype=torch.uint8, device=dev)
        copy_dst = torch.empty_like(copy_src)
        copy_us = event_time_us(lambda: copy_dst.copy_(copy_src), args.launches)
        copy_graph_us = graph_time_us(lambda: copy_dst.copy_(copy_src), args.launches)
        for light in render.SHUTTER_LIGHTS:
            fold, scratch = render.TemporalFold(sub, "tent", light), {}
            render.fold_frames(frames, fold, scratch)  # allocates the output, uploads the tables
            us = event_time_us(lambda: render.fold_frames(frames, fold, scratch), args.launches)
            graph_us = graph_time_us(lambda: render.fold_frames(frames, fold, scratch), args.launches)
            kernel[f"N{sub}_{light}"] = {"kernel_us": us, "kernel_GBps": moved / us / 1e3, "copy_us": copy_us, "copy_GBps": moved / copy_us / 1e3,
                                        "kernel_us_in_a_graph": graph_us, "kernel_GBps_in_a_graph": moved / graph_us / 1e3,
                                        "copy_us_in_a_graph": copy_graph_us, "bytes_read_plus_written": moved}
            print(f"fold N={sub} {light}: {us:.1f} us per batch eagerly, {graph_us:.1f} us in a graph ({moved / graph_us / 1e3:.0f} GB/s); "
                  f"copy_ of the same bytes {copy_us:.1f} / {copy_graph_us:.1f} us", flush=True)
    frame_bytes = size * size * 3
    result = {"device": torch.cuda.get_device_name(0), "size": size, "batch": batch, "lanes": 3, "synthesised_frames_per_render": n,
              "subframes": args.subframes, "alternations": args.alternations, "plain_twice_before": plain_twice,
              "synthesised_frames_per_s": {k: spread(v) for k, v in rates.items()}, "launches_per_kernel_time": args.launches,
              "kernel_one_batch": kernel,
              "delivered_bytes_per_synthesised_frame": {"plain": frame_bytes, "folded": frame_bytes / args.subframes}}
    plain = result["synthesised_frames_per_s"]["plain"]
    result["plain_spread"] = plain["max"] - plain["min"]
    for name in ("folded", "folded_linear"):
        result[f"{name}_minus_plain_median"] = result["synthesised_frames_per_s"][name]["median"] - plain["median"]
    print(json.dumps(result))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
