#!/usr/bin/env python3
"""Timing of probabilistic YIN on the MI355X (the figures of profiles/pyin.md):

    python tools/bench_pyin.py [--seconds 240] [--reps 5] [--torch-frames 2000] [--out pyin_bench.json]

  * maua_pyin_candidates_f32 alone and maua_pyin_viterbi_f64 alone, by device events around single launches after warm-up launches
    (minimum / median / maximum), on the intermediates of ar.raw_pyin's defaults (lags 10 .. 340, 602 bins, width 50) on bench_pitch's clip;
  * the decoder's recursion written as torch ops on the device (a per-frame loop of unfold / max in float64, the forward pass only),
    on the first --torch-frames frames, against the kernel on the same frames;
  * ar.pitch(method="pyin") against ar.pitch() end to end (margin=None as well), alternating in one warm process, host clock around a
    device synchronise.
Needs a GPU: there is no fallback."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maua_stylegan2_amd.audioreactive as ar  # noqa: E402
from bench_pitch import SR, clip  # noqa: E402
from maua_stylegan2_amd import _lib  # noqa: E402


def event_times(launch, warm=3, reps=10):
    for _ in range(warm):
        launch()
    torch.cuda.synchronize()
    start, stop = _lib.HipEvent(), _lib.HipEvent()
    out = []
    for _ in range(reps):
        start.record()
        launch()
        stop.record()
        torch.cuda.synchronize()
        out.append(start.elapsed_ms(stop))
    return {"min": min(out), "median": statistics.median(out), "max": max(out)}


def torch_forward(lov, lou, width, log_tri, log_norm, log_init, log_stay, log_switch):
    """The decoder's forward pass as torch ops, one frame at a time (float64 on the device): final delta and the back pointers."""
    T, P = lov.shape
    W = width
    lov, lou = lov.double(), lou.double()
    delta = torch.cat([lov[0] + log_init, (lou[0] + log_init).expand(P)])
    pad = torch.full((2, P + 2 * W), -math.inf, dtype=torch.float64, device=lov.device)
    tri = log_tri.flip(0)
    j = torch.arange(P, device=lov.device)
    back = torch.zeros(T, 2 * P, dtype=torch.int16, device=lov.device)
    back[0] = torch.arange(2 * P, device=lov.device)
    for t in range(1, T):
        pad[0, W:W + P] = delta[:P] - log_norm
        pad[1, W:W + P] = delta[P:] - log_norm
        best, k = (pad.unfold(1, 2 * W + 1, 1) + tri).max(dim=2)
        idx = j - W + k
        a, b = best[0] + log_stay, best[1] + log_switch
        sw = b > a
        back[t, :P] = torch.where(sw, P + idx[1], idx[0]).to(torch.int16)
        voiced = lov[t] + torch.where(sw, b, a)
        a, b = best[0] + log_switch, best[1] + log_stay
        sw = b > a
        back[t, P:] = torch.where(sw, P + idx[1], idx[0]).to(torch.int16)
        delta = torch.cat([voiced, lou[t] + torch.where(sw, b, a)])
    return delta, back


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-frames", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pyin: no GPU visible")
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    audio = clip(a.seconds)
    s = ar.signal._pyin_stages(audio, SR)
    T, P, W = s["states"].numel(), s["n_bins"], s["width"]
    stream = _lib.stream_ptr(dev)
    # the host tables again (as ar.raw_pyin builds them) for the direct calls
    import numpy as np
    import scipy.stats

    n_thr = 100
    cum = torch.from_numpy(np.concatenate([[0.0], np.cumsum(np.diff(scipy.stats.beta.cdf(np.arange(n_thr + 1) / n_thr, 2, 18)))]).astype(np.float32)).to(dev)
    edge = torch.from_numpy((SR / (65.0 * 2.0 ** ((np.arange(P + 1) - 0.5) / 120))).astype(np.float32)).to(dev)
    d = np.arange(-W, W + 1)
    tri_w = (W + 1 - np.abs(d)).astype(np.float64)
    log_tri = torch.from_numpy(np.log(tri_w)).to(dev)
    log_norm = torch.from_numpy(np.log(np.array([tri_w[(d + i >= 0) & (d + i <= P - 1)].sum() for i in range(P)]))).to(dev)
    consts = (-math.log(2 * P), math.log(0.99), math.log(0.01))
    obs, period, vp = torch.empty_like(s["obs"]), torch.empty_like(s["period"]), torch.empty_like(s["voiced_prob"])
    delta, back, states = torch.empty_like(s["delta_last"]), torch.empty_like(s["backptr"]), torch.empty_like(s["states"])

    def candidates():
        _lib.check(lib.maua_pyin_candidates_f32(s["cmndf"].data_ptr(), T, s["tau_min"], s["tau_max"], cum.data_ptr(), n_thr, 0.01, edge.data_ptr(), P,
                                                obs.data_ptr(), period.data_ptr(), vp.data_ptr(), stream), "maua_pyin_candidates_f32")

    def viterbi(frames=T):
        _lib.check(lib.maua_pyin_viterbi_f64(s["logobs_voiced"].data_ptr(), s["logobs_unvoiced"].data_ptr(), frames, P, W, log_tri.data_ptr(),
                                             log_norm.data_ptr(), *consts, delta.data_ptr(), back.data_ptr(), states.data_ptr(), stream),
                   "maua_pyin_viterbi_f64")

    result = {"clip_seconds": a.seconds, "sr": SR, "n_frames": T, "n_bins": P, "width": W, "lags": [s["tau_min"], s["tau_max"]],
              "voiced_fraction": float(s["voiced_flag"].float().mean()),
              "candidates_ms": event_times(candidates), "viterbi_ms": event_times(viterbi)}
    assert torch.equal(obs, s["obs"]) and torch.equal(states, s["states"])
    result["viterbi_us_per_frame"] = 1e3 * result["viterbi_ms"]["median"] / T

    n = min(a.torch_frames, T)
    result["torch_frames"] = n
    result["viterbi_ms_torch_frames"] = event_times(lambda: viterbi(n))
    kernel_delta = delta.clone()
    lov, lou = s["logobs_voiced"][:n], s["logobs_unvoiced"][:n]
    times = []
    for rep in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t_delta, t_back = torch_forward(lov, lou, W, log_tri, log_norm, *consts)
        torch.cuda.synchronize()
        if rep:
            times.append(1e3 * (time.perf_counter() - t0))
    result["torch_forward_ms"] = times
    # (torch.max names no tie rule: where two candidates tie, its back pointer may differ from the kernel's first maximum)
    result["torch_delta_equals_kernel"] = bool(torch.equal(t_delta, kernel_delta))
    result["torch_backptr_differing"] = int((t_back != back[:n]).sum())

    video_frames = int(a.seconds * 30)
    calls = {"pitch_yin": lambda: ar.pitch(audio, SR, video_frames, device="cuda"),
             "pitch_pyin": lambda: ar.pitch(audio, SR, video_frames, device="cuda", method="pyin"),
             "pitch_yin_margin_none": lambda: ar.pitch(audio, SR, video_frames, margin=None, device="cuda"),
             "pitch_pyin_margin_none": lambda: ar.pitch(audio, SR, video_frames, margin=None, device="cuda", method="pyin")}
    timings = {name: [] for name in calls}
    for rep in range(a.reps + 1):  # the first round warms every shape and is not counted
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                timings[name].append(1e3 * (time.perf_counter() - t0))
    for name, ts in timings.items():
        result[f"{name}_ms"] = ts
        result[f"{name}_ms_median"] = statistics.median(ts)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
