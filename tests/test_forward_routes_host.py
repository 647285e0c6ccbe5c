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


# The same generator behind the layer-0 bend of a 1920 (maps 2:1) and of a 1080 render (1:2), DESIGN.md "Non-square forwards": a bent
# constant goes through the convolution (conv1 on the low-resolution entry of the generic kernel).  2:1: the 16 x 32 map is the smallest the
# 2-D Winograd kernel takes, so the pre-scaled chain starts one resolution earlier — convs.2 (8 x 16, polyphase) is the first producer that
# posts, convs.4 has no low-resolution entry left — and so does the fused up-sampling layer (128 x 256 is 256 wide).  1:2: 32 x 16 is too
# narrow for either Winograd-2-D kernel, convs.3 stays on F(2,3) and convs.4 runs the polyphase kernel + blur tail (the low-resolution
# entries end at 16 columns ... and 16 rows), posting from the tail; the fused layer needs 256 columns, one resolution later than 2:1.
_BENT_CONV1 = (0, "lowres", False, False, "partial", None, "mfma")
_LOWRES_UP = (1, "lowres", False, False, None, None, "mfma")
_LOWRES_PLAIN = (2, "lowres", False, False, "partial", None, "mfma")
TABLE_1024_CM2_1920 = {
    "conv1": _BENT_CONV1, "convs.0": _LOWRES_UP, "convs.1": _LOWRES_PLAIN, "convs.2": (1, "lowres", False, True, None, None, "mfma"),
    "convs.3": _PARTIAL, "convs.4": _PAIR, "convs.5": _PARTIAL, "convs.6": _PAIR, "convs.7": _PARTIAL, "convs.8": _PAIR, "convs.9": _PARTIAL,
    "convs.10": _FUSED, "convs.11": _PARTIAL, "convs.12": _FUSED, "convs.13": _TORGB, "convs.14": _FUSED, "convs.15": _LAST}
TABLE_1024_CM2_1080 = {
    "conv1": _BENT_CONV1, "convs.0": _LOWRES_UP, "convs.1": _LOWRES_PLAIN, "convs.2": _LOWRES_UP, "convs.3": _LOWRES_PLAIN,
    "convs.4": (1, "pair", False, True, None, None, "mfma"),
    "convs.5": _PARTIAL, "convs.6": _PAIR, "convs.7": _PARTIAL, "convs.8": _PAIR, "convs.9": _PARTIAL, "convs.10": _PAIR,
    "convs.11": _PARTIAL, "convs.12": _FUSED, "convs.13": _TORGB, "convs.14": _FUSED, "convs.15": _LAST}


@pytest.mark.parametrize("size,cm,batch,table", [(1024, 2, 8, TABLE_1024_CM2), (512, 1, 1, TABLE_512_CM1)])
def test_expected_route_is_the_documented_layer_table(size, cm, batch, table):
    got = fr.expected_route(fr.skeleton(size, cm), batch, dict(frames_u8=True))
    assert list(got) == list(table)
    assert {tag: r for tag, r in got.items()} == {tag: fr.Route(*row) for tag, row in table.items()}


@pytest.mark.parametrize("orient,table", [("wide", TABLE_1024_CM2_1920), ("tall", TABLE_1024_CM2_1080)])
def test_expected_route_is_the_documented_non_square_layer_table(orient, table):
    g = fr.skeleton(1024, 2, output_size=fr.OUTPUT_SIZE[orient])
    got = fr.expected_route(g, 8, dict(frames_u8=True, orient=orient, bends=(0,)))
    assert list(got) == list(table)
    assert got == {tag: fr.Route(*row) for tag, row in table.items()}
    # the orientation is what the generator's own noise buffers say
    shapes = [(h * (1 if layer.conv.upsample is False else 2), w * (1 if layer.conv.upsample is False else 2))
              for _, layer, _, (h, w) in fr.layer_shapes(g, orient)]
    assert shapes == [tuple(getattr(g.noises, f"noise_{i}").shape[-2:]) for i in range(g.num_layers)]


def test_image_bound_exceptions_are_square_cases_from_before():
    assert all(fr.CASE_BY_NAME[name].orient == "square" and not fr.CASE_BY_NAME[name].unsaturated for name in fr.IMAGE_BOUND_EXCEPTIONS)
    assert all(fr.OLD_IMAGE_TOL / 10 < ceiling <= fr.OLD_IMAGE_TOL / 5 for ceiling in fr.IMAGE_BOUND_EXCEPTIONS.values())


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
            assert [r.mode for r in fr.expected_route(g, batch).values()] == [layer.conv.conv_mode(h, w) for _, layer, _, (h, w) in fr.layer_shapes(g)]
    # the non-square generators return the same set of modes (from other layers: see the next test)
    for orient in ("wide", "tall"):
        assert set(fr.reachable_modes(orient)) == set(reachable), orient
        assert fr.reachable_modes(orient)[4] == [(1024, 1, "convs.14")]


# What the issue behind the non-square cases claims of them, layer by layer: (case, layer, input shape, Route fields that matter there).
_NON_SQUARE_CLAIMS = [
    ("wide-64-cm2-b3", "conv1", (4, 8), dict(mode=0, path="lowres", family="mfma")),
    ("wide-64-cm2-b3", "convs.2", (8, 16), dict(mode=1, path="lowres", posted=True, family="mfma")),
    ("wide-64-cm2-b3", "convs.3", (16, 32), dict(mode=5, path="rgb_partial", prescaled=True, posted=True)),
    ("wide-64-cm2-b3", "convs.4", (16, 32), dict(mode=6, path="pair", prescaled=True)),
    ("tall-64-cm2-b1", "conv1", (8, 4), dict(mode=0, path="lowres", family="mfma")),
    ("tall-64-cm2-b1", "convs.3", (32, 16), dict(mode=2, path="lowres", prescaled=False)),
    ("tall-64-cm2-b1", "convs.4", (32, 16), dict(mode=1, path="pair", posted=True)),
    ("tall-64-cm2-b8", "convs.4", (32, 16), dict(mode=1, path="pair", posted=True)),
    ("wide-256-cm1-b2", "convs.10", (128, 256), dict(mode=6, path="fused", prescaled=True, posted=True)),
    ("wide-256-cm1-b2", "convs.11", (256, 512), dict(mode=5, path="torgb", rgb="folded", u8="layer")),
    ("wide-256-cm1-b2-tap", "convs.11", (256, 512), dict(mode=5, path="torgb", rgb="folded", u8="layer")),
    ("tall-256-cm1-b2", "convs.10", (256, 128), dict(mode=6, path="pair", prescaled=True, posted=True)),
    ("tall-256-cm1-b2", "convs.11", (512, 256), dict(mode=5, path="torgb", rgb="folded", u8="layer")),
    ("tall-256-cm1-b2-tap", "convs.11", (512, 256), dict(mode=5, path="torgb", rgb="folded", u8="layer")),
    ("wide-64-cm2-b2", "convs.2", (8, 16), dict(mode=1, path="lowres", posted=True)),
    ("wide-1024-cm1-b1", "convs.14", (512, 1024), dict(mode=4, path="pair", family="mfma")),
    ("wide-1024-cm1-b1", "convs.15", (1024, 2048), dict(mode=0, path="torgb", rgb="folded", family="mfma")),
]


def test_non_square_cases_reach_what_no_square_generator_does():
    """reachable_routes over sizes 8 .. 1024 x cm 1, 2 x batch 1, 8 x the three orientations: every (mode, path, prescaled, posted, rgb,
    family) that a non-square generator takes and no square one does is taken by a non-square case; and the layers the cases were chosen
    for run where they were said to."""
    from maua_stylegan2_amd import _lib

    found = fr.reachable_routes()
    only_non_square = (set(found["wide"]) | set(found["tall"])) - set(found["square"])
    cases = [c for c in fr.CASES if c.orient != "square"]
    assert not set(fr.CASES_LEFT_OUT) & set(fr.CASE_BY_NAME)
    taken = {}
    for case in cases:
        for tag, r in fr.case_route(case).items():
            taken.setdefault(fr.route_key(r), (case.name, tag))
    print("only non-square:", {k: (found["wide"].get(k) or found["tall"].get(k))[0] for k in sorted(only_non_square, key=str)})
    assert only_non_square and only_non_square <= set(taken), only_non_square - set(taken)
    # a posting polyphase layer (mode 1: low-resolution entry on 2:1 maps, pair on 1:2 maps) is such a route: no square generator has one
    assert (1, "lowres", False, True, None, "mfma") in only_non_square and (1, "pair", False, True, None, "mfma") in only_non_square
    for name, tag, hw, want in _NON_SQUARE_CLAIMS:
        case = fr.CASE_BY_NAME[name]
        shapes = {t: s for t, _, _, s in fr.layer_shapes(fr.case_skeleton(case), case.orient)}
        got = fr.case_route(case)[tag]
        assert shapes[tag] == hw and all(getattr(got, k) == v for k, v in want.items()), (name, tag, shapes[tag], got)
    # the posting pair of the portrait generator splits K at batch 1 and not at batch 8; the wide cases' conv1 instances are the 4 x 8 / 8 x 4 ones
    lib = _lib.load()
    assert lib.maua_modconv_ws_floats(1, 512, 512, 32, 16, 1) > 0 and lib.maua_modconv_ws_floats(8, 512, 512, 32, 16, 1) == 0
    assert _lib.planned_modconv_instance(3, 512, 512, 4, 8, 0) == (0, "modconv_mfma_kernel<128, 128, 2, 0, true, true, 1>")
    assert _lib.planned_modconv_instance(1, 512, 512, 8, 4, 0) == (0, "modconv_mfma_kernel<128, 128, 2, 0, true, true, 2>")
    # no square case stands in for them: the routes above differ from the square generator's at the same layer
    square = fr.case_route(fr.CASE_BY_NAME["64-cm2-b3"])
    for name in ("wide-64-cm2-b3", "tall-64-cm2-b1"):
        route = fr.case_route(fr.CASE_BY_NAME[name])
        assert [t for t in route if route[t] != square[t]] and route["convs.4"] != square["convs.4"], name


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


@pytest.mark.parametrize("name", ["wide-64-cm2-b3", "tall-64-cm2-b1"])
def test_a_transposed_noise_map_or_constant_shows(name):
    """What a non-square forward can get wrong and a square one cannot see as a wrong shape: (a) one layer's noise map read with rows and
    columns exchanged (the 4 x 8 / 8 x 4 map of conv1: the same floats, indexed x * h + y), (b) the constant padded on the other axis
    (= the transposed constant padded on the right one).  The fp64 forward with either defect differs from the true one, on conv1's map
    and on the image, by far more than their bounds."""
    case = fr.CASE_BY_NAME[name]
    ref, bnd, inp = fr.reference(case), fr.bounds(case), fr.inputs(case)
    b = case.batch
    noise = fr.frames(inp["noise"], 0, b)
    bends = fr.bend_callables(case)

    def run(noise=noise, bends=bends):
        return fr.walk_as(torch.float64, inp["sd"], inp["latents"][:b], noise, bends=bends)

    same = run()
    assert torch.equal(same["image"], ref["image"])
    swapped = list(noise)
    swapped[0] = noise[0].transpose(-1, -2).contiguous().view(noise[0].shape)
    other_axis = dict(bends)
    other_axis[0] = lambda x: bends[0](x.transpose(-1, -2))
    for what, bad in (("noise map of conv1 transposed", run(noise=swapped)), ("constant padded on the other axis", run(bends=other_axis))):
        d_map, d_img = float((bad["raw"][0] - ref["raw"][0]).abs().max()), float((bad["image"] - ref["image"]).abs().max())
        print(f"[{name}] {what}: conv1 map off by {d_map:.2e} (bound {bnd['raw'][0]:.1e}), image by {d_img:.2e} (bound {bnd['image']:.1e})")
        assert d_map > 100 * bnd["raw"][0] and d_img > 100 * bnd["image"], what


@pytest.mark.parametrize("case", fr.CASES, ids=lambda c: c.name)
def test_fp32_forward_is_inside_its_own_bounds(case):
    """The bound's arithmetic on the CPU alone: the float32 forward the bound is built from lies inside it (trivially: 4 G >= 1) and the
    layout of reference and bounds agrees.  The image bound is 10 x under the 1e-3 of tests/test_generator_gpu.py, whatever G
    tools/forward_tolerance.py measures — but for the square cases of forward_ref.IMAGE_BOUND_EXCEPTIONS, which have a ceiling of their own."""
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
    assert bnd["image"] <= fr.IMAGE_BOUND_EXCEPTIONS.get(case.name, fr.OLD_IMAGE_TOL / 10), (case.name, bnd["image"])


@pytest.mark.parametrize("case", [c for c in fr.CASES if c.u8 is not None], ids=lambda c: c.name)
def test_uint8_ambiguity_cap(case):
    """From the fp64 reference alone: fewer than 5 % of the frame's values lie within (image bound) x 127.5 of a boundary between two
    levels, where the frame comparison of the GPU test allows one level instead of none.

    Measured with G = 2.47: image bounds 2.6e-5 .. 3.7e-5, ambiguous share 0.65 % .. 0.92 % on two hosts (about 2 x bound x 127.5 of the
    unclamped values, whatever the seed; the fp32 CPU forward behind the bound rounds a little differently from host to host).  With the ratio to conv_ref._direct_conv (36.32, recorded in the JSON and used by nothing) it would be
    9.5 % .. 11.6 %: a cap no seed could meet.  The non-square cases (G = 4.68 on 2:1 maps, 3.15 on 1:2 maps) run with
    seeding.unsaturated_rgb_gain as it is."""
    ref, bnd = fr.reference(case), fr.bounds(case)
    levels, ambiguous = fr.frames_u8_reference(ref["image"], bnd["image"])
    share = float(ambiguous.float().mean())
    clamped = float(((levels == 0) | (levels == 255)).float().mean())
    print(f"[{case.name}] image bound {bnd['image']:.2e}: ambiguous share {100 * share:.2f} %, on the clamp {100 * clamped:.2f} %")
    assert clamped < 0.25, clamped  # (most of the frame lies inside the grey range, where a level can be wrong: seeding.unsaturated_rgb_gain)
    assert share < 0.05, share
