"""The Motion-JPEG pipe format on one MI355X (profiles/mjpeg.md): the encoder's device time for a batch of 8 RENDERED frames at 1024^2 and
at 1920x1080 (quality 90) next to maua_rgb_to_yuv420p_u8 timed the same way, the mean stream size, and the delivered frame rate of a
1024^2 render to the null sink as rgb24, yuv420p and mjpeg, alternating in one process.
    python tools/mjpeg_probe.py [--frames 896] [--alternations 4] [--json out.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mjpeg_probe.py --kernels-only     (the three kernels' own times)"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from delivery_probe import graph_time_ms, spread  # noqa: E402
from maua_stylegan2_amd import render, seeding  # noqa: E402
from maua_stylegan2_amd.models.stylegan2 import Generator  # noqa: E402

QUALITY = 90


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=896)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--alternations", type=int, default=4)
    ap.add_argument("--kernels-only", action="store_true", help="a few eager calls of both conversions and nothing else (for a kernel trace)")
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mjpeg_probe measures on the device: no GPU visible")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    size, batch = args.size, args.batch
    n = (args.frames // batch) * batch
    g = Generator(size, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(size, seed=0))
    g = g.to(dev).eval()
    torch.manual_seed(0)
    lat = torch.randn(n, g.n_latent, 512, device=dev)
    noise = [torch.randn(n, 1, r, r, device=dev) if r <= 256 else None for r in seeding.noise_sizes(size)]

    # rendered frames: the first batches of the job; the wide case from the same pictures, mirrored to 2048 px and delivered as 1920x1080
    batches = []
    for _, u8 in render.synthesize(g, lat[: 4 * batch], [m[: 4 * batch] if m is not None else None for m in noise], batch):
        batches.append(u8.clone())
    square = batches[0]
    wide = render.crop_resize_for_delivery(torch.cat([square, square.flip(2)], dim=2).contiguous(), 1920, {}).clone()
    assert tuple(wide.shape) == (batch, 1080, 1920, 3)
    scratch = {}
    result = {"device": torch.cuda.get_device_name(0), "quality": QUALITY, "batch": batch, "encode": {}}
    if args.kernels_only:
        for _ in range(5):
            for frames in (square, wide):
                render.frames_to_mjpeg(frames, scratch, QUALITY)
                render.frames_to_yuv420p(frames, scratch)
        torch.cuda.synchronize()
        return
    for name, frames in (("1024x1024", square), ("1920x1080", wide)):
        px = frames.shape[0] * frames.shape[1] * frames.shape[2]
        slots = render.frames_to_mjpeg(frames, scratch, QUALITY)
        render.frames_to_yuv420p(frames, scratch)
        torch.cuda.synchronize()
        head = slots[:, :8].cpu().numpy().view("<u4")
        assert (head[:, 1] == 0).all()
        enc_ms = statistics.median(graph_time_ms(lambda: render.frames_to_mjpeg(frames, scratch, QUALITY), 48) for _ in range(5))
        yuv_ms = statistics.median(graph_time_ms(lambda: render.frames_to_yuv420p(frames, scratch), 48) for _ in range(5))
        out_bytes = int(head[:, 0].sum())
        floor_bytes = px * 3 + 2 * px * 3 + out_bytes  # frames read, coefficients written and read, streams written
        result["encode"][name] = {"encode_us_per_batch": enc_ms * 1e3, "yuv420p_us_per_batch": yuv_ms * 1e3,
                                  "mean_stream_bytes": out_bytes / frames.shape[0], "bytes_per_pixel": out_bytes / px,
                                  "traffic_floor_bytes": floor_bytes, "floor_us_at_6.3TBps": floor_bytes / 6.3e12 * 1e6}
        print(name, json.dumps(result["encode"][name]), flush=True)
    sizes = []
    for u8 in batches:
        sizes += render.frames_to_mjpeg(u8, scratch, QUALITY)[:, :4].cpu().numpy().view("<u4").reshape(-1).tolist()
    result["mean_stream_bytes_32_frames"] = sum(sizes) / len(sizes)

    def delivered(pix_fmt):
        gc.collect()
        torch.cuda.synchronize()
        t = time.perf_counter()
        written = render.render_shard(g, lat, noise, 0, n / 30.0, batch, size, None, None, 1.0, [], {}, False, "slow", None, pipe_pix_fmt=pix_fmt)
        torch.cuda.synchronize()
        assert written == n
        return n / (time.perf_counter() - t)

    formats = ("rgb24", "yuv420p", f"mjpeg:{QUALITY}")
    for fmt in formats:  # pins the rings of every frame shape once
        delivered(fmt)
        delivered(fmt)
    rates = {fmt: [] for fmt in formats}
    for k in range(args.alternations):
        order = formats[k % 3:] + formats[: k % 3]
        for fmt in order:
            delivered(fmt)  # (the first render after a change of format re-makes the staging rings: not the figure)
            rates[fmt].append(delivered(fmt))
        print(f"alternation {k}: " + " | ".join(f"{fmt} {rates[fmt][-1]:.0f}/s" for fmt in formats), flush=True)
    result["frames_per_render"] = n
    result["frames_per_s"] = {fmt: spread(v) for fmt, v in rates.items()}
    print(json.dumps(result))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
