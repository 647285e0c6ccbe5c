"""Side measurement of the device latent loops (``ar.loop_sections``, maua_keyframe_blend_f32) on one MI355X — the figures of
profiles/latent_loops.md.

    python tools/bench_latent_loops.py [--rounds 7] [--host-sections 3] [--out FILE.json]

Two shapes on a 12 x 18 x 512 selection: "sections" = 30 sections of 300 frames, each a closed spline through 4 entries (5 keys; 9000
frames x 9216 floats, 332 MB), and "long" = one closed spline through all 12 entries (13 keys) over 1000 frames.  Per shape, warm:
1. host    — the host path (``ar.spline_loops`` on numpy input, one call per section: the only way to build the sequence before the
             device path existed); ``--host-sections`` calls are timed and scaled to the section count, every section being the same work;
2. device  — ``ar.loop_sections`` end to end (tables + one launch), host clock round a device synchronise;
3. kernel  — maua_keyframe_blend_f32 alone on prebuilt tables, HIP events round 20 launches, with the GB/s it writes;
4. torch   — the same sequence composed from torch ops on the device: ``(W @ keys)[rows]`` per section, then ``cat``.
2 and 4 alternate per round in one process; medians and the spread (min .. max) are printed.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import maua_stylegan2_amd.audioreactive as ar  # noqa: E402
from maua_stylegan2_amd import _lib  # noqa: E402
from maua_stylegan2_amd.audioreactive import latent  # noqa: E402

torch.set_grad_enabled(False)
SHAPES = {"sections": dict(frames=[300] * 30, key_starts=[s % 12 for s in range(30)], n_keys=4),
          "long": dict(frames=[1000], key_starts=[0], n_keys=12)}


def wall(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def spread(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def measure(name, spec, sel, dev, rounds, host_sections):
    frames, key_starts, n_keys = spec["frames"], spec["key_starts"], spec["n_keys"]
    n_frames, feats, m = sum(frames), sel[0].numel(), n_keys + 1
    sel_d = sel.to(dev)
    # 1. host path, per section
    timed = min(host_sections, len(frames))
    t0 = time.perf_counter()
    for s in range(timed):
        ar.spline_loops(ar.wrapping_slice(sel, key_starts[s], n_keys).numpy(), frames[s], 1)
    host = (time.perf_counter() - t0) / timed * len(frames)

    def device():
        return ar.loop_sections(sel_d, frames, key_starts, n_keys, 1)

    # 4. torch composition on the device (weights and index lists uploaded once, outside the timing)
    w_d = {p: torch.from_numpy(latent.spline_weights(m, p).astype(np.float32)).to(dev) for p in set(frames)}
    rows_d = {p: (torch.arange(p, device=dev) % p) for p in set(frames)}
    keys_d = [torch.cat([i, i[:1]]).to(dev) for i in (ar.wrapping_slice(sel, k, n_keys, return_indices=True) for k in key_starts)]
    flat = sel_d.reshape(len(sel), -1)

    def composed():
        return torch.cat([(w_d[p] @ flat[k])[rows_d[p]] for p, k in zip(frames, keys_d)]).reshape((n_frames,) + tuple(sel.shape[1:]))

    _, got = wall(device, dev)
    _, ref = wall(composed, dev)
    diff = float((got - ref).abs().max())
    times = {"device": [], "torch": []}
    for _ in range(rounds):
        times["device"].append(wall(device, dev)[0])
        times["torch"].append(wall(composed, dev)[0])
    # 3. the kernel alone
    bank = flat.contiguous()
    idx = torch.stack(keys_d).int().contiguous()
    weights = torch.cat([w_d[p] for p in frames]).contiguous()
    row, sec = latent.loop_frame_tables(frames, frames, device=dev)
    out = torch.empty((n_frames, feats), device=dev)
    lib, stream = _lib.load(), _lib.stream_ptr(dev)

    def launch():
        _lib.check(lib.maua_keyframe_blend_f32(bank.data_ptr(), len(sel), feats, idx.data_ptr(), weights.data_ptr(), row.data_ptr(),
                                               sec.data_ptr(), out.data_ptr(), n_frames, len(frames), len(weights), m, stream),
                   "maua_keyframe_blend_f32")

    launch()
    torch.cuda.synchronize(dev)
    assert torch.equal(out.view_as(got), got)
    kernel = []
    for _ in range(rounds):
        start, stop = _lib.HipEvent(), _lib.HipEvent()
        start.record()
        for _ in range(20):
            launch()
        stop.record()
        torch.cuda.synchronize(dev)
        kernel.append(start.elapsed_ms(stop) / 20 * 1e-3)
    written = 4 * n_frames * feats
    res = {"frames": n_frames, "keys": m, "sections": len(frames), "bytes_written": written, "host_s": host, "host_sections_timed": timed,
           "device_s": spread(times["device"]), "torch_s": spread(times["torch"]), "kernel_s": spread(kernel),
           "kernel_GB_per_s": written / spread(kernel)["median"] / 1e9, "max_abs_diff_device_vs_torch": diff}
    print(f"{name}: {n_frames} frames x {feats} floats, {m} keys, {len(frames)} sections, {written / 1e6:.0f} MB written\n"
          f"  host path        {host:9.3f} s  ({timed} of {len(frames)} sections timed)\n"
          f"  loop_sections    {res['device_s']['median'] * 1e3:9.3f} ms  ({res['device_s']['min'] * 1e3:.3f} .. {res['device_s']['max'] * 1e3:.3f})\n"
          f"  torch on device  {res['torch_s']['median'] * 1e3:9.3f} ms  ({res['torch_s']['min'] * 1e3:.3f} .. {res['torch_s']['max'] * 1e3:.3f})\n"
          f"  kernel alone     {res['kernel_s']['median'] * 1e3:9.3f} ms  ({res['kernel_s']['min'] * 1e3:.3f} .. {res['kernel_s']['max'] * 1e3:.3f})"
          f"  {res['kernel_GB_per_s']:.0f} GB/s written\n"
          f"  max |loop_sections - torch| = {diff:.3g}", flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-sections", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_latent_loops.py needs an MI355X: there is no CPU path to time")
    dev = torch.device("cuda:0")
    _lib.load()
    sel = torch.from_numpy(np.random.default_rng(0).standard_normal((12, 18, 512)).astype(np.float32))
    result = {"device": _lib.device_info()["name"]}
    for name, spec in SHAPES.items():
        result[name] = measure(name, spec, sel, dev, args.rounds, args.host_sections)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
