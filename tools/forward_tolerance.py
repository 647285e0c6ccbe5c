#!/usr/bin/env python
"""G of the whole-forward bound (tests/forward_ref.py): how much more the Winograd forms round than the direct fp32 form, measured on the CPU.

For every layer of the generators of forward_ref.CASES whose conv_mode is a Winograd form (2, 3, 4, 5, 6), on the seeded operands of
conv_ref.case_operands at the layer's spatial shape, in units of u M (conv_ref.ratio_of: max |form - fp64| / (u M)):

    emulated      conv_ref.emulate_f32(mode): the transforms, the packed-weight formulas, one float32 accumulator per frequency
    sequential    the DIRECT form with one float32 accumulator per output over (tap, channel), term after term (this file)
    once_rounded  conv_ref._direct_conv: the float32 product x * s, the convolution summed in float64, ONE rounding of the result

    G_all_cases[mode]    = max over the layers of  emulated / sequential      <- floored at 1; recorded, used by nothing
    G_once_rounded[mode] = max over the layers of  emulated / once_rounded    <- recorded, used by nothing
    G_by_orientation[o]  = the same (<- what the bound uses) over the layers of the cases of orientation o (square, wide = 2:1 maps, tall = 1:2) alone: a case's bound takes
                           the largest entry of its own orientation, so that the layer shapes of the non-square generators (the 16 x 32
                           map of the 2-D Winograd kernels among them) do not widen the bounds of forwards that never run them

Why the first.  The bound is 4 G E with E measured from a float32 CPU forward, whose convolutions accumulate in float32: E contains the
accumulation rounding of a direct form already, and G has to add only what the transforms amplify.  conv_ref._direct_conv contains no
accumulation rounding at all (0.4 .. 1.1 u M whatever the channel count), so the ratio to it (36 for mode 5) counts the accumulation a
second time: bounds built on it are 0.4e-3 .. 1.7e-3 on the image — no tighter than the 1e-3 they are meant to replace — and put 10 % of
a uint8 frame within reach of the next level.  Both are written to the JSON.

The emulations walk the input channels in Python, so ``cin`` is cut to at most --cin (default 32) and ``cout`` to at most --cout (default
64) at the SAME spatial shape: the transforms act on the spatial axes; the channel count only lengthens the accumulation, which numerator
and denominator share.  No GPU, nothing from a kernel under test.

    python tools/forward_tolerance.py --write      # prints the table and rewrites tests/golden/forward_tolerance.json
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import conv_ref  # noqa: E402
import forward_ref  # noqa: E402

_F = np.float32


def sequential_direct_f32(x, s, d, w, up):
    """The direct convolution (``up``: the transposed one, stride 2, [B, O, 2H+1, 2W+1]) with one float32 accumulator per output, the
    terms added one after the other over (channel, tap), every product and every sum rounded to float32; then the gain wscale * d."""
    x, s, d, g = (t.numpy().astype(_F) for t in (x, s, d, w[0]))
    b, c, h, wd = x.shape
    xs = (x * s[:, :, None, None]).astype(_F)
    gain = (_F(1.0 / np.sqrt(c * 9)) * d).astype(_F)[:, :, None, None]
    taps = [(ky, kx) for ky in range(3) for kx in range(3)]
    if not up:
        xp = np.pad(xs, ((0, 0), (0, 0), (1, 1), (1, 1)))
        acc = conv_ref._chain([g[None, :, ch, ky, kx, None, None] for ch in range(c) for ky, kx in taps],
                              [xp[:, None, ch, ky:ky + h, kx:kx + wd] for ch in range(c) for ky, kx in taps])
        return (acc * gain).astype(_F)
    y = np.zeros((b, g.shape[0], 2 * h + 1, 2 * wd + 1), _F)
    for ch in range(c):
        for ky, kx in taps:  # y[2 i + ky, 2 j + kx] += x[i, j] w[ky, kx]
            view = y[:, :, ky:ky + 2 * h:2, kx:kx + 2 * wd:2]
            view += (g[None, :, ch, ky, kx, None, None] * xs[:, None, ch]).astype(_F)
    return (y * gain).astype(_F)


def layer_ratios(mode, cin, cout, h, w):
    """(emulated, sequential, once_rounded) in units of u M."""
    _, x, s, d, wt = conv_ref.case_operands(mode, cin, cout, h, w, 1)
    s = s[:, :cin].contiguous()
    up = mode in (4, 6)
    emulated = conv_ref.ratio_of(mode, x, s, d, wt)
    sequential = conv_ref.ratio_of(mode, x, s, d, wt, got=sequential_direct_f32(x, s, d, wt, up))
    once = conv_ref.ratio_of(mode, x, s, d, wt, got=conv_ref._direct_conv(x, s, d, wt, up).numpy())
    return emulated, sequential, once


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cin", type=int, default=32)
    ap.add_argument("--cout", type=int, default=64)
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()
    shapes, orients = {}, {}
    for case in forward_ref.CASES:
        with forward_ref.switched(case):
            g = forward_ref.case_skeleton(case)
            for tag, layer, _, (h, w) in forward_ref.layer_shapes(g, case.orient):
                mode = layer.conv.conv_mode(h, w)
                if mode >= 2:
                    c = layer.conv
                    orient = "" if case.orient == "square" else case.orient + " "
                    key = (mode, min(c.in_channel, args.cin), min(c.out_channel, args.cout), h, w)
                    shapes.setdefault(key, []).append(f"{orient}{case.size}/cm{case.cm} {tag} {c.in_channel}->{c.out_channel}")
                    orients.setdefault(key, set()).add(case.orient)
    gain, once_rounded, rows = {"0": 1.0, "1": 1.0}, {"0": 1.0, "1": 1.0}, []
    by_orient = {o: {"0": 1.0, "1": 1.0} for o in forward_ref.ORIENTATIONS}
    for (mode, cin, cout, h, w), where in sorted(shapes.items()):
        emulated, sequential, once = layer_ratios(mode, cin, cout, h, w)
        rows.append(dict(mode=mode, cin=cin, cout=cout, h=h, w=w, emulated=round(emulated, 3), sequential=round(sequential, 3), once_rounded=round(once, 3),
                         layers=sorted(set(where))))
        gain[str(mode)] = max(gain.get(str(mode), 1.0), emulated / sequential)
        for o in orients[(mode, cin, cout, h, w)]:
            by_orient[o][str(mode)] = max(by_orient[o].get(str(mode), 1.0), emulated / sequential)
        once_rounded[str(mode)] = max(once_rounded.get(str(mode), 1.0), emulated / once)
        print(f"mode {mode}  {cin:3d} -> {cout:3d} @ {h:4d} x {w:4d}   emulated {emulated:6.2f}   sequential direct {sequential:5.2f}   once-rounded direct {once:5.2f} u M"
              f"   ratios {emulated / sequential:5.2f} / {emulated / once:5.2f}   {', '.join(sorted(set(where))[:3])}")
    ceil2 = lambda table: {k: round(float(np.ceil(v * 100) / 100), 2) for k, v in sorted(table.items())}  # noqa: E731
    gain, once_rounded = ceil2(gain), ceil2(once_rounded)
    by_orient = {o: ceil2(table) for o, table in by_orient.items()}
    print("G per mode (emulated / sequential fp32 direct form):", gain, " G =", max(gain.values()))
    for o, table in by_orient.items():
        print(f"  over the {o} cases' layers:", table, " G =", max(table.values()))
    print("recorded only, emulated / once-rounded direct form (conv_ref._direct_conv):", once_rounded)
    if args.write:
        out = dict(command=f"python tools/forward_tolerance.py --cin {args.cin} --cout {args.cout} --write",
                   note="units of u M; cin and cout cut at the layer's own spatial shape; G_all_cases = emulated fp32 rounding of the mode / rounding of the "
                        "direct form accumulated term after term in fp32, same operands, floored at 1, over the layers of every case (recorded, used by nothing); G_by_orientation = the same over the "
                        "layers of the square / wide (2:1) / tall (1:2) cases alone — the whole-forward bound of a case uses the largest "
                        "entry of its orientation; G_once_rounded = the ratio to conv_ref._direct_conv (fp64 sum rounded once), used by nothing",
                   G_all_cases=gain, G_by_orientation=by_orient, G_once_rounded=once_rounded, layers=rows)
        with open(forward_ref.TOLERANCE_JSON, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print("wrote", forward_ref.TOLERANCE_JSON)


if __name__ == "__main__":
    main()
