"""Device time of the bar-pointer decode (maua_bar_viterbi_f64 through ar.bar_viterbi) on a 5-minute envelope, beside
maua_hmm_viterbi_f64 over the same number of frames — the yardstick for one barrier per frame (profiles/bars.md).

    python tools/bench_bars.py [--out profiles/bars_bench.json] [--frames 12920] [--reps 7]

Device events round each call, sorted times of ``reps`` calls after two warm-up calls."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import bar_ref  # noqa: E402
import hmm_ref  # noqa: E402
import maua_stylegan2_amd.audioreactive as ar  # noqa: E402
from maua_stylegan2_amd import _lib  # noqa: E402


def timed(fn, reps):
    fn(), fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        start, stop = _lib.HipEvent(), _lib.HipEvent()
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        out.append(start.elapsed_ms(stop))
    return sorted(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=12920)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    T = args.frames
    interval, width, log_change = ar.bar_model(bar_ref.FR)
    seconds = T / bar_ref.FR + 1
    a, d, _ = bar_ref.accented_envelope(np.arange(0.5, seconds - 0.5, 0.5), 4, seconds)
    logobs = torch.from_numpy(bar_ref.observations(a, d)[:T]).to(dev)
    result = dict(frames=T, tempi=len(interval), reps=args.reps, ms={})

    def report(name, ms):
        result["ms"][name] = ms
        print(f"{name}: median {ms[len(ms) // 2]:.3f} ms ({ms[0]:.3f} .. {ms[-1]:.3f}), {1e3 * ms[len(ms) // 2] / T:.3f} us a frame")

    for beats in ((3, 4), (4,), (8,)):
        report(f"bar_viterbi beats_per_bar={beats}", timed(lambda: ar.bar_viterbi(logobs, interval, width, log_change, beats), args.reps))
    for S in (128, 25):
        lo, lt, li = (torch.from_numpy(x).to(dev) for x in hmm_ref.viterbi_operands(dict(S=S, T=T, kind="random", seed=1)))
        report(f"hmm_viterbi S={S}", timed(lambda: ar.viterbi(lo, lt, li), args.reps))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
