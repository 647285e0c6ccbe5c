#!/usr/bin/env python
"""Which instances of modconv_mfma_kernel<BM, BN, WM, MODE, MULTI, FAST, MAXP> (csrc/modconv_kernel.h, instantiated by csrc/modconv_m0.hip .. modconv_m4.hip) can a call reach, and by which
smallest shape?  -> tests/golden/conv_instances.json, the table tests/test_conv_instances_gpu.py and tests/test_conv_instances_host.py
are parametrised over.

    python tools/conv_instance_sweep.py            # on the CPU: walk the grid, record one row per distinct instance
    python tools/conv_instance_sweep.py --ratios   # on the CPU: measure the rounding amplification of modes 2 / 3 / 4 into the same file
    python tools/conv_instance_sweep.py --dedicated  # on the CPU: the table of the dedicated kernels (modes 5 .. 8) -> conv_dedicated_instances.json

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
test's bound for those modes is four times that ratio: it comes from the transforms' arithmetic, not from the kernel under test.

--dedicated: modes 5 .. 8 (csrc/modconv_w2d.hip, modconv_up2d.hip, modconv_sbf16.hip) have no plan function, so their rows are LISTED below,
each with the reason for its shape and the instance name a reading of the launchers expects; tests/test_conv_dedicated_gpu.py asserts
the name on every launch.  Per row the rounding ratio R of modes 5 / 6 is measured on the operands the GPU test feeds (the pre-scaled ones
for the s == NULL instances) and the workspace size is asked of the library."""
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


OUT_DEDICATED = os.path.join(REPO, "tests", "golden", "conv_dedicated_instances.json")
W2D, W2DW, UP2D = "modconv_w2d_kernel<%s, %s>", "modconv_w2dw_kernel<%s>", "modconv_up2d_kernel<%d, %d, %s, %d>"
# (entry, mode, cin, cout, h, w, batch, pre, name, why this shape)
DEDICATED = [
    # ---- mode 5 through maua_modconv3x3_f32.  64-channel m-tiles x 8 rows x 32 columns; K chunks of 4 channels
    ("modconv3x3", 5, 4, 64, 8, 32, 1, False, W2D % ("4, 2, 2", "false"), "the minimum: one tile, one K chunk"),
    ("modconv3x3", 5, 12, 128, 16, 64, 3, False, W2D % ("4, 2, 2", "false"), "2 x 2 x 2 tiles (x, y, channels), 3 images, 3 K chunks"),
    ("modconv3x3", 5, 4, 64, 8, 32, 1, True, W2D % ("4, 2, 2", "true"), "the minimum, pre-scaled input"),
    # 32 channels, h % 16 != 0: the 8-row tile of the general kernel
    ("modconv3x3", 5, 4, 32, 8, 32, 1, False, W2D % ("2, 2, 3", "false"), "the minimum: h % 16 != 0 keeps the general kernel"),
    ("modconv3x3", 5, 20, 32, 24, 64, 2, False, W2D % ("2, 2, 3", "false"), "2 x 3 tiles, 2 images, 5 K chunks; h % 16 != 0"),
    ("modconv3x3", 5, 4, 32, 8, 32, 1, True, W2D % ("2, 2, 3", "true"), "the minimum, pre-scaled input"),
    # 32 channels, h % 16 == 0: the wave-complete kernel on 16-row tiles
    ("modconv3x3", 5, 4, 32, 16, 32, 1, False, W2DW % "false", "the minimum: one 16-row tile"),
    ("modconv3x3", 5, 20, 32, 32, 96, 2, False, W2DW % "false", "3 x 2 tiles, 2 images, 5 K chunks"),
    ("modconv3x3", 5, 4, 32, 16, 32, 1, True, W2DW % "true", "the minimum, pre-scaled input"),
    # ---- mode 6 through maua_modconv3x3_f32.  32-channel m-tiles x 8 x 32 positions; K chunks of 8 channels where cin % 8 == 0, else 4
    ("modconv3x3", 6, 4, 32, 8, 32, 1, False, UP2D % (4, 0, "false", 32), "the minimum: cin % 8 != 0"),
    ("modconv3x3", 6, 12, 64, 16, 64, 2, False, UP2D % (4, 0, "false", 32), "2 x 2 x 2 tiles, 2 images, 3 K chunks of 4"),
    ("modconv3x3", 6, 4, 32, 8, 32, 1, True, UP2D % (4, 0, "true", 32), "the minimum, pre-scaled input"),
    ("modconv3x3", 6, 8, 32, 8, 32, 1, False, UP2D % (8, 0, "false", 32), "the minimum: one K chunk of 8"),
    ("modconv3x3", 6, 24, 96, 24, 96, 3, False, UP2D % (8, 0, "false", 32), "3 x 3 x 3 tiles, 3 images, 3 K chunks of 8"),
    ("modconv3x3", 6, 8, 32, 8, 32, 1, True, UP2D % (8, 0, "true", 32), "the minimum, pre-scaled input"),
    # ---- maua_upconv_blur_f32: 60-column x tiles, vertical segments of tiles (H / 8 + 1 tiles in all)
    ("upconv_blur", 6, 8, 32, 8, 32, 1, False, UP2D % (8, 2, "false", 32), "the minimum: one segment"),
    ("upconv_blur", 6, 8, 32, 32, 32, 3, False, UP2D % (8, 2, "false", 32), "5 y tiles in several segments, the last one shorter; two x tiles; 3 images"),
    ("upconv_blur", 6, 24, 64, 16, 96, 2, False, UP2D % (8, 2, "false", 32), "four x tiles, two channel tiles, 3 K chunks, 2 images"),
    ("upconv_blur", 6, 8, 32, 8, 32, 1, True, UP2D % (8, 2, "true", 32), "the minimum, pre-scaled input"),
    # ---- maua_upconv_blur_lowres_f32(up = 6): 16 x 16-position tiles, K split over workgroups
    ("upconv_blur_lowres", 6, 8, 32, 16, 16, 1, False, UP2D % (8, 0, "false", 16), "the minimum: one slab"),
    ("upconv_blur_lowres", 6, 72, 32, 16, 16, 2, False, UP2D % (8, 0, "false", 16), "nine chunks in two splits of 5 + 4"),
    ("upconv_blur_lowres", 6, 136, 64, 16, 16, 2, False, UP2D % (8, 0, "false", 16), "seventeen chunks in four splits, the last of 2"),
    # ---- modes 7 / 8 (side measurements)
    ("modconv3x3", 7, 16, 128, 8, 32, 1, False, "modconv_sbf16_kernel<-1>", "the minimum"),
    ("modconv3x3", 7, 48, 128, 16, 64, 2, False, "modconv_sbf16_kernel<-1>", "2 x 2 tiles, 2 images, 3 K chunks: the fused tail with per-image noise"),
    ("modconv3x3", 8, 16, 32, 8, 32, 1, False, "modconv_sbf16_up_kernel", "the minimum"),
    ("modconv3x3", 8, 32, 64, 16, 64, 2, False, "modconv_sbf16_up_kernel", "2 x 2 x 2 tiles, 2 images"),
]


def dedicated(out=None):
    import conv_ref
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    rows = []
    for entry, mode, cin, cout, h, w, b, pre, name, why in DEDICATED:
        if entry == "upconv_blur":
            n = lib.maua_upconv_blur_ws_floats(b, cin, cout, h, w)
        elif entry == "upconv_blur_lowres":
            n = lib.maua_lowres_ws_floats(b, cin, cout, h, w, 6)
        else:
            n = lib.maua_modconv_ws_floats(b, cin, cout, h, w, mode)
        r = round(conv_ref.rounding_ratio(mode, cin, cout, h, w, b, pre=pre), 2) if mode in (5, 6) else None
        rows.append(dict(entry=entry, mode=mode, cin=cin, cout=cout, h=h, w=w, batch=b, pre=pre, name=name, ws_floats=int(n), R=r, why=why))
        print(rows[-1], flush=True)
    dump({"generated_by": "tools/conv_instance_sweep.py --dedicated (CPU)", "instances": rows}, out or OUT_DEDICATED)
    print(f"{len(rows)} rows -> {out or OUT_DEDICATED}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the sweep's table here instead of tests/golden/conv_instances.json")
    ap.add_argument("--ratios", action="store_true", help="CPU: measure the rounding ratios of modes 2, 3, 4 into the table")
    ap.add_argument("--dedicated", action="store_true", help="CPU: write the table of the dedicated kernels (modes 5 .. 8)")
    args = ap.parse_args()
    if args.dedicated:
        dedicated(args.out)
    else:
        ratios() if args.ratios else sweep(args.out)
