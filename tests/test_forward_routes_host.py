"""Host side of the whole-forward matrix (tests/forward_ref.py, tests/test_forward_matrix_gpu.py), no GPU: the restated dispatch rules
against the layer table of DESIGN.md, the coverage of the case list (every path, every reachable mode, both sides of the style fold), and
the arithmetic of the per-element bound and of the uint8 ambiguity cap on the CPU references alone."""
import pytest
import torch

import forward_ref as fr

torch.set_grad_enabled(False)


@pytest.fixture(scope="module", autouse=True)
def _lib_is_built(built_lib):
    return built_lib


# The layer table of DESIGN.md ("Whole-forward route table"), written out by hand: (conv_mode, path, input pre-scaled, posts for its
# consumer, ToRGB of the resolution, who writes the uint8 frame, kernel family).  The 4^2 .. 32^2 block runs the low-resolution entries
# (conv1 as y = T s on the constant); convs.4's tail is the first producer that posts (its consumer, convs.5, is the first 2-D Winograd
# layer), every layer up to the one before the last follows; 128- to 512-channel plain layers leave partial ToRGB sums, the 64- and
# 32-channel ones fold ToRGB into their epilogue, and the last of them writes the frame; up-sampling layers from 256-wide inputs are fused.
_LOW_BLOCK = {
    "conv1": (0, "const", False, False, "partial", None, "const"),
    "convs.0": (1, "lowres", False, False, None, None, "mfma"),
    "convs.1": (2, "lowres", False, False, "partial", None, "mfma"),
    "convs.2": (1, "lowres", False, False, None, None, "mfma"),
    "convs.3": (2, "lowres", False, False, "partial", None, "mfma"),
    "convs.4": (1, "lowres", False, True, None, None, "up2d"),
}
_PARTIAL = (5, "rgb_partial", True, True, "partial", None, "w2d")
_TORGB = (5, "torgb", True, True, "folded", None, "w2d")
_PAIR = (6, "pair", True, True, None, None, "up2d")
_FUSED = (6, "fused", True, True, None, None, "up2d")
_LAST = (5, "torgb", True, False, "folded", "layer", "w2d")
TABLE_1024_CM2 = dict(_LOW_BLOCK, **{
    "convs.5": _PARTIAL, "convs.6": _PAIR, "convs.7": _PARTIAL, "convs.8": _PAIR, "convs.9": _PARTIAL, "convs.10": _PAIR,
    "convs.11": _PARTIAL, "convs.12": _FUSED, "convs.13": _TORGB, "convs.14": _FUSED, "convs.15": _LAST})
TABLE_512_CM1 = dict(_LOW_BLOCK, **{
    "convs.5": _PARTIAL, "convs.6": _PAIR, "convs.7": _PARTIAL, "convs.8": _PAIR, "convs.9": _PARTIAL, "convs.10": _PAIR,
    "convs.11": _TORGB, "convs.12": _FUSED, "convs.13": _LAST})


@pytest.mark.parametrize("size,cm,batch,table", [(1024, 2, 8, TABLE_1024_CM2), (512, 1, 1, TABLE_512_CM1)])
def test_expected_route_is_the_documented_layer_table(size, cm, batch, table):
    got = fr.expected_route(fr.skeleton(size, cm), batch, dict(frames_u8=True))
    assert list(got) == list(table)
    assert {tag: r for tag, r in got.items()} == {tag: fr.Route(*row) for tag, row in table.items()}


def _all_routes():
    return {case.name: fr.case_route(case) for case in fr.CASES}


def test_cases_reach_every_path_with_both_sides_of_the_style_fold():
    """Every path name; every path that can post with ``posted`` true and false; every consumer kind that accepts a pre-scaled input
    (the plain 2-D Winograd layer through "plain", "rgb_partial" and "torgb", the F(2,2)^2 layer through "pair" and "fused") with
    ``prescaled`` true and false; every ToRGB outcome; both writers of the uint8 frame."""
    seen_path, seen_post, seen_pre, seen_rgb, seen_u8 = set(), set(), set(), set(), set()
    for name, route in _all_routes().items():
        for tag, r in route.items():
            seen_path.add(r.path)
            seen_post.add((r.path, "up" if tag != "conv1" and int(tag.split(".")[1]) % 2 == 0 else "plain", r.posted))
            seen_pre.add((r.path, r.prescaled))
            seen_rgb.add(r.rgb)
            seen_u8.add(r.u8)
    assert seen_path == set(fr.PATHS)
    for path, kind in (("torgb", "plain"), ("rgb_partial", "plain"), ("lowres", "up"), ("pair", "up"), ("fused", "up")):
        assert (path, kind, True) in seen_post and (path, kind, False) in seen_post, (path, sorted(seen_post))
    # the paths that never post, on any layer
    assert not any(posted for path, _, posted in seen_post if path in ("const", "plain")) and ("lowres", "plain", True) not in seen_post
    for path in ("plain", "rgb_partial", "torgb", "pair", "fused"):
        assert (path, True) in seen_pre and (path, False) in seen_pre, (path, sorted(seen_pre))
    # ... and the ones without an instance for a pre-scaled input
    assert ("const", True) not in seen_pre and ("lowres", True) not in seen_pre
    assert seen_rgb == {"folded", "partial", "separate", None} and seen_u8 == {"layer", "pass", None}


def test_cases_reach_every_reachable_mode():
    reachable = fr.reachable_modes()
    taken = {}
    for name, route in _all_routes().items():
        for tag, r in route.items():
            taken.setdefault(r.mode, name)
    print("reachable:", {m: where[0] for m, where in sorted(reachable.items())}, " taken:", dict(sorted(taken.items())))
    # modes 3, 7 and 8 are not reachable at the thresholds in force (3: every shape it accepts goes to mode 5 first; 7 / 8: off by default)
    assert set(reachable) == {0, 1, 2, 4, 5, 6}
    assert set(reachable) - set(taken) == set(fr.MODES_NOT_IN_CASES)
    # mode 4 lives in one layer of one generator: the reason the 1024^2 case exists
    assert reachable[4] == [(1024, 1, "convs.14")] and taken[4] == "1024-cm1-b1"
    # conv_mode takes no batch: what reachable_modes reports holds at batch 1 and 8 alike
    for size, cm in ((64, 2), (512, 1)):
        g = fr.skeleton(size, cm)
        for batch in (1, 8):
            assert [r.mode for r in fr.expected_route(g, batch).values()] == [layer.conv.conv_mode(h, h) for _, layer, _, h in fr.layer_shapes(g)]


def test_switch_cases_change_the_route_they_are_about():
    """Each switch case differs from the default route of its generator where the switch acts, and nowhere it does not."""
    routes = _all_routes()
    base = routes["truncation"]  # (the default route of the 128^2 generator with the lowered fused-blur width)
    assert [r.path for r in base.values()].count("fused") == 1 and base["convs.8"].path == "fused"
    for same in ("noise-shared", "noise-buffer", "noise-mix", "no-upconv-winograd", "blur-asym", "bend-lowres-up"):
        assert routes[same] == base, same  # (bend-lowres-up: convs.2 posts to nobody, and an up-sampling layer has no ToRGB to lose)
    assert not any(r.posted or r.prescaled for r in routes["acts"].values())
    assert routes["acts"] == routes["no-style-fold"]
    assert all(r.rgb in (None, "separate") for r in routes["no-rgb-fusion"].values())
    assert routes["no-lowres-fusion"]["conv1"].path == "plain" and routes["no-lowres-fusion"]["convs.4"].path == "pair"
    assert routes["no-lowres-up2d"]["convs.4"].family == "mfma" and base["convs.4"].family == "up2d"
    assert routes["latent-input"]["conv1"].path == "lowres" and routes["bend-const"]["conv1"].path == "lowres"
    assert routes["blur-nonsep"]["convs.8"].path == "pair"
    assert [r.rgb for r in routes["min-rgb-above"].values()] == [None] * len(base)
    # a bend: its layer's producer does not post, its own ToRGB is a separate pass, the neighbours keep their paths
    for name, tag, before in (("bend-pair", "convs.6", "convs.5"), ("bend-rgb-partial", "convs.7", "convs.6"), ("bend-fused", "convs.8", "convs.7"),
                              ("bend-last", "convs.9", "convs.8"), ("bend-lowres", "convs.1", "convs.0")):
        r = routes[name]
        assert not r[tag].posted, name
        if r[tag].rgb is not None:
            assert r[tag].rgb == "separate" and r[tag].path == "plain", name
        assert r[before] == base[before], name
    assert routes["bend-torgb"]["convs.11"].path == "plain" and routes["u8-torgb"]["convs.11"].path == "torgb"


def test_a_flipped_blur_tap_shows():
    """The asymmetric-taps case is only worth its name if a transposed tap matrix would be seen: the fp64 reference with the taps of every
    Blur transposed differs from the true one by far more than the bound of the image and of the fused layer's map."""
    case = fr.CASE_BY_NAME["blur-asym"]
    ref, bnd, inp = fr.reference(case), fr.bounds(case), fr.inputs(case)
    sd = dict(inp["sd"])
    for key in sd:
        if key.endswith("conv.blur.kernel"):
            sd[key] = sd[key].t().contiguous()
    b = case.batch
    flipped = fr.walk_as(torch.float64, sd, inp["latents"][:b], fr.frames(inp["noise"], 0, b))
    fused = 9  # convs.8 = activation map 9
    assert fr.case_route(case)["convs.8"].path == "fused"
    assert float((flipped["raw"][fused] - ref["raw"][fused]).abs().max()) > 100 * bnd["raw"][fused]
    assert float((flipped["image"] - ref["image"]).abs().max()) > 100 * bnd["image"]


@pytest.mark.parametrize("case", fr.CASES, ids=lambda c: c.name)
def test_fp32_forward_is_inside_its_own_bounds(case):
    """The bound's arithmetic on the CPU alone: the float32 forward the bound is built from lies inside it (trivially: 4 G >= 1) and the
    layout of reference and bounds agrees.  Prints how the image bound compares with the 1e-3 of tests/test_generator_gpu.py."""
    ref, rnd, bnd = fr.reference(case), fr.rounding(case), fr.bounds(case)
    assert len(ref["acts"]) == len(bnd["acts"]) == 2 * (len(ref["images"]) - 1) + 1
    for key in ("raw", "acts"):
        for a64, a32, b in zip(ref[key], rnd[key], bnd[key]):
            assert a64.dtype == torch.float64 and a32.dtype == torch.float32 and b > 0
            assert float((a32.double() - a64).abs().max()) <= b
    if ref["image"] is None:
        assert case.min_rgb_size > case.size and bnd["image"] is None
        return
    assert float((rnd["image"].double() - ref["image"]).abs().max()) <= bnd["image"]
    print(f"[{case.name}] image bound {bnd['image']:.2e} = {fr.OLD_IMAGE_TOL / bnd['image']:.1f} x tighter than {fr.OLD_IMAGE_TOL}; "
          f"E per map {min(bnd['E']):.1e} .. {max(bnd['E']):.1e}")


@pytest.mark.parametrize("case", [c for c in fr.CASES if c.u8 is not None], ids=lambda c: c.name)
def test_uint8_ambiguity_cap(case):
    """From the fp64 reference alone: fewer than 5 % of the frame's values lie within (image bound) x 127.5 of a boundary between two
    levels, where the frame comparison of the GPU test allows one level instead of none.

    Measured with G = 2.47: image bounds 2.6e-5 .. 3.7e-5, ambiguous share 0.65 % .. 0.92 % on two hosts (about 2 x bound x 127.5 of the
    unclamped values, whatever the seed; the fp32 CPU forward behind the bound rounds a little differently from host to host).  With the ratio to conv_ref._direct_conv (36.32, recorded in the JSON and used by nothing) it would be
    9.5 % .. 11.6 %: a cap no seed could meet."""
    ref, bnd = fr.reference(case), fr.bounds(case)
    levels, ambiguous = fr.frames_u8_reference(ref["image"], bnd["image"])
    share = float(ambiguous.float().mean())
    clamped = float(((levels == 0) | (levels == 255)).float().mean())
    print(f"[{case.name}] image bound {bnd['image']:.2e}: ambiguous share {100 * share:.2f} %, on the clamp {100 * clamped:.2f} %")
    assert clamped < 0.25, clamped  # (most of the frame lies inside the grey range, where a level can be wrong: seeding.unsaturated_rgb_gain)
    assert share < 0.05, share
