#!/usr/bin/env python3
"""Timing of the predominant local pulse on the MI355X (the figures of profiles/pulse.md):

    python tools/bench_pulse.py [--seconds 240] [--reps 5] [--out pulse_bench.json]

  * maua_tempogram_peak_f32 with tgram NULL and non-NULL, and maua_pulse_synth_f32, by device events around 20 back-to-back launches after
    warm-up launches (per launch: minimum / median / maximum of 10 timings), on the detrended onset envelope of a click-and-tone clip with ar.raw_plp's defaults
    (window 384, 271 tempi);
  * the same computation as torch ops on the device, by the same events: unfold -> complex matmul -> |.|^2 -> argmax / angle, and
    cos of [frames, window] arguments -> index_add overlap-add (numerator and denominator) -> divide;
  * ar.beat_phase end to end against ar.onsets, alternating in one warm process, host clock around a device synchronise.
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import maua_stylegan2_amd.audioreactive as ar  # noqa: E402
from maua_stylegan2_amd import _lib  # noqa: E402
from maua_stylegan2_amd.audioreactive import beat  # noqa: E402

SR = 22050


def clip(seconds, bpm=120.0, seed=0):
    """Noise bursts on the beat over a quiet tone that changes every two seconds."""
    rng = np.random.default_rng(seed)
    n = int(seconds * SR)
    t = np.arange(n) / SR
    y = 0.1 * np.sin(2 * np.pi * (220.0 * 2.0 ** ((np.floor(t / 2) % 5) / 12)) * t)
    for at in (np.arange(0.25, seconds - 0.1, 60.0 / bpm) * SR).astype(int):
        y[at: at + 220] += 0.5 * rng.standard_normal(220) * np.exp(-np.arange(220) / 60.0)
    return y.astype(np.float32)


def event_times(launch, warm=3, reps=10, inner=20):
    """Milliseconds per launch: ``reps`` timings of ``inner`` back-to-back launches between two device events, after ``warm`` launches."""
    for _ in range(warm):
        launch()
    torch.cuda.synchronize()
    start, stop = _lib.HipEvent(), _lib.HipEvent()
    out = []
    for _ in range(reps):
        start.record()
        for _ in range(inner):
            launch()
        stop.record()
        torch.cuda.synchronize()
        out.append(start.elapsed_ms(stop) / inner)
    return {"min": min(out), "median": statistics.median(out), "max": max(out)}


def torch_peak(env, table_c, win):
    """Entry A as torch ops: the [N, W] Hankel matrix (materialised by the matmul), the [N, B] complex tempogram, argmax."""
    x = torch.nn.functional.pad(env, (win // 2, win - 1 - win // 2)).unfold(0, win, 1)
    f = x.to(torch.complex64) @ table_c
    s = f.real * f.real + f.imag * f.imag
    best, at = s.max(dim=1)
    return at, torch.angle(f.gather(1, at[:, None])[:, 0]), best


def torch_synth(bins, phase, window, omega, win):
    """Entry B as torch ops: every frame's windowed sinusoid [N, W], overlap-added with index_add."""
    n = bins.numel()
    k = torch.arange(win, device=bins.device)
    valid = bins >= 0
    arg = omega[bins.clamp(min=0).long()][:, None] * k[None, :].float() + phase[:, None]
    kern = torch.where(valid[:, None], window[None, :] * torch.cos(arg), torch.zeros((), device=bins.device))
    at = (torch.arange(n, device=bins.device)[:, None] - win // 2 + k[None, :]).reshape(-1) + win
    num = torch.zeros(n + 2 * win, device=bins.device).index_add_(0, at, kern.reshape(-1))[win: win + n]
    den = torch.zeros(n + 2 * win, device=bins.device).index_add_(0, at, window[None, :].expand(n, win).reshape(-1))[win: win + n]
    return (num / den).clamp(min=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pulse: no GPU visible")
    audio = clip(a.seconds)
    s = beat._plp_stages(audio, SR, want_tgram=True)
    env, table, window, omega = s["env"], s["table"], s["window"], s["omega"]
    n, (n_tempi, win, _) = env.numel(), table.shape
    result = {"clip_seconds": a.seconds, "sr": SR, "n_frames": n, "win": win, "n_tempi": n_tempi,
              "beats_found": int(beat.pick_beats(s["pulse"], s["fr"]).numel()), "pulse_max": float(s["pulse"].max())}
    # direct calls into preallocated outputs: the time between the events is the kernel's, not the allocator's
    lib, stream = _lib.load(), _lib.stream_ptr(env.device)
    bins, phase, power = torch.empty_like(s["bin"]), torch.empty_like(s["phase"]), torch.empty_like(s["power"])
    tgram, curve = torch.empty_like(s["tgram"]), torch.empty_like(s["pulse"])

    def peak(tg=None):
        _lib.check(lib.maua_tempogram_peak_f32(env.data_ptr(), n, table.data_ptr(), win, n_tempi, None, bins.data_ptr(), phase.data_ptr(),
                                               power.data_ptr(), _lib.ptr(tg), stream), "maua_tempogram_peak_f32")

    def synth():
        _lib.check(lib.maua_pulse_synth_f32(s["bin"].data_ptr(), s["phase"].data_ptr(), n, window.data_ptr(), win, omega.data_ptr(), n_tempi,
                                            curve.data_ptr(), stream), "maua_pulse_synth_f32")

    result["peak_ms"] = event_times(peak)
    result["peak_tgram_ms"] = event_times(lambda: peak(tgram))
    result["synth_ms"] = event_times(synth)
    assert torch.equal(bins, s["bin"]) and torch.equal(tgram, s["tgram"]) and torch.equal(curve, s["pulse"])
    flops = 4.0 * n * n_tempi * win  # two fused multiply-adds per (frame, tempo, tap)
    result["peak_tflops"] = flops / (1e-3 * result["peak_ms"]["median"]) / 1e12

    table_c = torch.complex(table[:, :, 0], table[:, :, 1]).t().contiguous()
    result["torch_peak_ms"] = event_times(lambda: torch_peak(env, table_c, win))
    result["torch_synth_ms"] = event_times(lambda: torch_synth(s["bin"], s["phase"], window, omega, win))
    t_bin, t_phase, t_best = torch_peak(env, table_c, win)
    has = s["bin"] >= 0
    result["torch_bins_differing"] = int((t_bin[has] != s["bin"][has]).sum())
    result["torch_pulse_max_abs_diff"] = float((torch_synth(s["bin"], s["phase"], window, omega, win) - s["pulse"]).abs().max())
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    torch_peak(env, table_c, win)
    result["torch_peak_extra_mib"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    torch.cuda.reset_peak_memory_stats()
    beat.tempogram_peak(env, table)
    result["peak_extra_mib"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20

    video_frames = int(a.seconds * 30)
    calls = {"onsets": lambda: ar.onsets(audio, SR, video_frames, device="cuda"),
             "beat_phase": lambda: ar.beat_phase(audio, SR, video_frames, device="cuda"),
             "onsets_margin_none": lambda: ar.onsets(audio, SR, video_frames, margin=None, device="cuda"),
             "pulse": lambda: ar.pulse(audio, SR, video_frames, device="cuda")}
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
