#!/usr/bin/env python3
"""Timing of the recursive-filter entries and of the features on them on the MI355X (the figures of profiles/iir.md):

    python tools/bench_iir.py [--seconds 240] [--reps 10] [--out profiles/iir_bench.json]

Every step runs in a child process of its own under its own time limit; the first step that fails or runs out of time ends the run (what
was measured until then is still written).  Steps:
  kernel  maua_sosfilt_f64 alone (float in, float out; the four launches of a call between device events, minimum / median / maximum after
          warm-up) for F in {1, 4, 8} band-passes of 12 sections over one shared clip of --seconds of noise, over a sweep of chunk lengths
          and the default; the F = 1 result is compared with scipy's at every chunk length;
  scipy   scipy.signal.sosfilt on the host for the same clip and the same 12 sections (one filter; host clock, best of 3);
  rms     ar.rms() after ar.set_filter("device") against ar.rms() as it is by default — the parent commit's path — alternating in
          one warm process, host clock around a device synchronise;
  bands   ar.bands (four bands) against ar.onsets, the same way;
  follow  maua_env_follow_f32 alone on [43 200, 8] (24 minutes at 30 fps), device events.
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR = 22050
STEPS = {"kernel": 300, "scipy": 180, "rms": 240, "bands": 240, "follow": 60}  # step -> its time limit in seconds
CHUNKS = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 0)


def clip(seconds):
    import numpy as np

    return (0.25 * np.random.default_rng(0).standard_normal(int(seconds * SR))).astype(np.float32)


def bank(n_filters):
    import numpy as np
    import scipy.signal

    if n_filters == 1:
        return scipy.signal.butter(12, [20, 8000], "bp", fs=SR, output="sos")[None]
    edges = np.geomspace(20, 8000, n_filters + 1)
    return np.stack([scipy.signal.butter(12, [lo, hi], "bp", fs=SR, output="sos") for lo, hi in zip(edges[:-1], edges[1:])])


def summary(ms):
    return {"min": min(ms), "median": statistics.median(ms), "max": max(ms)}


def event_times(launch, warm=3, reps=10):
    import torch

    from maua_stylegan2_amd import _lib

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
    return summary(out)


def host_times(fn, warm=1, reps=5):
    import torch

    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return summary(out)


def step_kernel(a):
    import numpy as np
    import scipy.signal
    import torch

    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    dev = torch.device("cuda:0")
    x_host = clip(a.seconds)
    n = len(x_host)
    x = torch.from_numpy(x_host).to(dev)
    theirs = scipy.signal.sosfilt(bank(1)[0], x_host.astype(np.float64))
    res = {"n": n, "default_chunk": int(lib.maua_sosfilt_default_chunk(n)), "sweep": {}}
    for F in (1, 4, 8):
        sos = torch.from_numpy(bank(F)).to(dev)
        y = torch.empty((F, n), dtype=torch.float32, device=dev)
        rows = {}
        for chunk in CHUNKS:
            ws = torch.empty(int(lib.maua_sosfilt_ws_doubles(F, 12, n, chunk)), dtype=torch.float64, device=dev)

            def launch():
                _lib.check(lib.maua_sosfilt_f64(sos.data_ptr(), F, 12, x.data_ptr(), None, 1, n, chunk, None, None, y.data_ptr(), None,
                                                ws.data_ptr(), _lib.stream_ptr(dev)), "maua_sosfilt_f64")

            row = event_times(launch, reps=a.reps)
            if F == 1:
                row["max_abs_diff_vs_scipy_over_max"] = float(np.max(np.abs(y[0].cpu().numpy() - theirs)) / np.max(np.abs(theirs)))
            rows[str(chunk) if chunk else "default"] = row
            print(f"F={F} chunk={chunk or 'default'}: {row}", flush=True)
        res["sweep"][f"F{F}"] = rows
    return res


def step_scipy(a):
    import numpy as np
    import scipy.signal

    x = clip(a.seconds).astype(np.float64)
    sos = bank(1)[0]
    out = []
    for _ in range(3):
        t0 = time.perf_counter()
        scipy.signal.sosfilt(sos, x)
        out.append(1e3 * (time.perf_counter() - t0))
    return {"sosfilt_ms": summary(out), "n": len(x)}


def step_rms(a):
    import maua_stylegan2_amd.audioreactive as ar

    x = clip(a.seconds)
    n_frames = int(a.seconds * 30)
    res = {"n_frames": n_frames}
    for _ in range(2):  # alternating: the second round is the one reported first, both are kept
        for name in ("host", "device"):
            ar.set_filter(name)
            res.setdefault(f"rms_{name}_ms", []).append(host_times(lambda: ar.rms(x, SR, n_frames), reps=3))
    ar.set_filter("host")
    print(res, flush=True)
    return res


def step_bands(a):
    import maua_stylegan2_amd.audioreactive as ar

    x = clip(a.seconds)
    n_frames = int(a.seconds * 30)
    res = {"n_frames": n_frames}
    for _ in range(2):
        res.setdefault("bands_ms", []).append(host_times(lambda: ar.bands(x, SR, n_frames), reps=3))
        res.setdefault("onsets_ms", []).append(host_times(lambda: ar.onsets(x, SR, n_frames), reps=3))
    print(res, flush=True)
    return res


def step_follow(a):
    import torch

    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    dev = torch.device("cuda:0")
    T, C = 43200, 8
    x = torch.rand((T, C), device=dev)
    y = torch.empty_like(x)

    def launch():
        _lib.check(lib.maua_env_follow_f32(x.data_ptr(), None, y.data_ptr(), T, C, 1.0, 0.1175, _lib.stream_ptr(dev)), "maua_env_follow_f32")

    return {"frames": T, "cols": C, "env_follow_ms": event_times(launch, reps=a.reps)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iir_bench.json"))
    ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process and print its JSON (what the parent starts)")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(globals()[f"step_{a.step}"](a)), flush=True)
        return 0
    res = {"clip_seconds": a.seconds, "sr": SR}
    rc = 0
    for step, limit in STEPS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--seconds", str(a.seconds), "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            res[step] = {"error": f"no result within {limit} s"}
            rc = 1
            break
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            res[step] = {"error": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}
            rc = 1
            break
        res[step] = json.loads(lines[-1][len("RESULT "):])
        print(f"{step}: {json.dumps(res[step])}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh)
    print(json.dumps(res))
    return rc


if __name__ == "__main__":
    sys.exit(main())
