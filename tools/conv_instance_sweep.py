#!/usr/bin/env python
"""Which instances of modconv_mfma_kernel<BM, BN, WM, MODE, MULTI, FAST, MAXP> (csrc/modconv.hip) can a call reach, and by which
smallest shape?  -> tests/golden/conv_instances.json, the table tests/test_conv_instances_gpu.py and tests/test_conv_instances_host.py
are parametrised over.

    python tools/conv_instance_sweep.py            # on the CPU: walk the grid, record one row per distinct instance
    python tools/conv_instance_sweep.py --ratios   # on the CPU: measure the rounding amplification of modes 2 / 3 / 4 into the same file

The sweep asks the library's plan (maua_modconv_plan_instance: the host function maua_modconv3x3_f32 itself dispatches through, called
without a launch, so nothing here re-implements it) for modes 0 .. 4 over a grid of small shapes (aligned and ragged channel counts,
maps from one pixel to a few tile widths, widths odd, 2 mod 4 and just over 32 / 64 / 128, batches 1, 2, 3, 5, 8) and keeps the
cheapest shape (batch * cin * cout * h * w) per name.  A shape the plan refuses (MAUA_EINVAL) is counted; any other code ends the sweep.
Regenerating must reproduce the committed table byte for byte: a difference means make_plan() has changed what some shape runs.
That the table holds EVERY instance a call can reach, not only those of this grid, is tests/test_conv_instances_host.py's enumeration.

--ratios: for every row of modes 2, 3 and 4 (and the extra shapes of the GPU test's edge variants), on the seeded operands the GPU test
feeds (conv_ref.case_operands), a float32 numpy emulation of the transforms exactly as the kernel writes them (tests/conv_ref.py) is
compared with the fp64 direct convolution; the largest
|emulation - fp64| / (u M) per mode, u = 2^-24, M = the convolution of the absolute values, goes into "rounding_ratio".  The GPU
test's bound for those modes is four times that ratio: it comes from the transforms' arithmetic, not from the kernel under test."""
import argparse
import itertools
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
OUT = os.path.join(REPO, "tests", "golden", "conv_instances.json")

CHANNELS = [3, 4, 8, 12, 18, 24, 32, 40, 64, 68, 72, 128, 136, 200]
HEIGHTS = [1, 2, 3, 4, 5, 8, 9, 16, 20, 33, 40, 72]
WIDTHS = [1, 2, 3, 4, 5, 6, 8, 9, 12, 16, 20, 33, 34, 36, 65, 66, 68, 129, 130, 132]
BATCHES = [1, 2, 3, 5, 8]
MAX_COST = 1 << 26  # batch * cin * cout * h * w of a shape: every instance is reachable with few channels (the table's rows are launched by the GPU test)


def out_hw(mode, h, w):
    return (2 * h + 1, 2 * w + 1) if mode in (1, 4) else (h, w)


def grid():
    for mode in range(5):
        for cin, cout, h, w, b in itertools.product(CHANNELS, CHANNELS, HEIGHTS, WIDTHS, BATCHES):
            if (mode in (2, 4) and w % 2) or (mode == 3 and w % 4):
                continue
            if b * cin * cout * h * w > MAX_COST:
                continue
            yield mode, cin, cout, h, w, b


def sweep(out=None):
    import ctypes

    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    buf = ctypes.create_string_buffer(128)
    best, refused = {}, {}
    for mode, cin, cout, h, w, b in grid():
        rc = lib.maua_modconv_plan_instance(b, cin, cout, h, w, mode, buf, 128)
        if rc == -22:  # a shape the plan refuses (documented: no patch of that map fits a tile); recorded, not an error
            refused.setdefault(mode, []).append((cin, cout, h, w, b))
            continue
        if rc != 0:
            sys.exit(f"rc {rc} at mode {mode} cin {cin} cout {cout} h {h} w {w} batch {b}")
        name = buf.value.decode()
        cost = b * cin * cout * h * w
        if name not in best or cost < best[name][0]:
            n = lib.maua_modconv_ws_floats(b, cin, cout, h, w, mode)
            oh, ow = out_hw(mode, h, w)
            best[name] = (cost, dict(name=name, mode=mode, cin=cin, cout=cout, h=h, w=w, batch=b, ws_floats=int(n), split_k=n > 0,
                                     splits=int(n // (b * cout * oh * ow)) if n else 1))
    rows = [best[k][1] for k in sorted(best, key=lambda q: (best[q][1]["mode"], q))]
    # (the string is part of the committed table, which this sweep must reproduce byte for byte)
    doc = {"generated_by": "tools/conv_instance_sweep.py (GPU sweep; --ratios on the CPU)", "instances": rows,
           "refused_einval": {str(m): len(v) for m, v in sorted(refused.items())},
           "refused_examples": {str(m): v[:4] for m, v in sorted(refused.items())}}
    if os.path.exists(OUT):
        old = json.load(open(OUT))
        if "rounding_ratio" in old:
            doc["rounding_ratio"] = old["rounding_ratio"]
    dump(doc, out)
    print(f"{len(rows)} instances -> {out or OUT}")
    for r in rows:
        print(r)


def dump(doc, path=None):
    path = path or OUT
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("{\n")
        keys = list(doc)
        for i, k in enumerate(keys):
            end = ",\n" if i + 1 < len(keys) else "\n"
            if k == "instances":
                f.write(' "instances": [\n' + ",\n".join("  " + json.dumps(r) for r in doc[k]) + "\n ]" + end)
            else:
                f.write(f" {json.dumps(k)}: {json.dumps(doc[k])}" + end)
        f.write("}\n")


def ratios():
    import conv_ref
    import test_conv_instances_gpu as t

    doc = json.load(open(OUT))
    shapes = {(r["mode"], r["cin"], r["cout"], r["h"], r["w"], r["batch"]) for r in doc["instances"]} | set(t.extra_shapes())
    worst = {}
    for mode, cin, cout, h, w, b in sorted(shapes):
        if mode not in (2, 3, 4):
            continue
        r = conv_ref.rounding_ratio(mode, cin, cout, h, w, b)  # (the operands the GPU test feeds: conv_ref.case_operands)
        print(mode, cin, cout, h, w, b, f"{r:.2f}  (9 cin + 8 = {9 * cin + 8})", flush=True)
        worst[str(mode)] = max(worst.get(str(mode), 0.0), r)
    doc["rounding_ratio"] = {k: round(v, 2) for k, v in sorted(worst.items())}
    dump(doc, OUT)
    print(doc["rounding_ratio"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the sweep's table here instead of tests/golden/conv_instances.json")
    ap.add_argument("--ratios", action="store_true", help="CPU: measure the rounding ratios of modes 2, 3, 4 into the table")
    args = ap.parse_args()
    ratios() if args.ratios else sweep(args.out)
