"""CPU: the lens's definition (tests/lens_ref.py) on known answers, the float32 emulation against it, the plan rule, the wrong variants the
GPU case list must catch, ar.Lens / the --lens flag, and the plumbing that carries a lens into generate() without touching a pinned
signature."""
import argparse
import inspect
import math
import os

import numpy as np
import pytest
import torch

import lens_ref as lr

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------------ the definition
def test_a_unit_impulse_blurs_to_the_outer_product_of_the_taps():
    taps = np.array([[0.4, 0.2, 0.1]])
    x = np.zeros((1, 1, 9, 11))
    x[0, 0, 4, 5] = 1
    full = np.concatenate([taps[0, :0:-1], taps[0]])
    want = np.zeros((9, 11))
    want[2:7, 3:8] = np.outer(full, full)
    assert np.allclose(lr.blur(x, taps), want, atol=1e-15)
    # per-frame taps: frame 0 the delta, frame 1 the kernel
    both = lr.blur(np.concatenate([x, x]), np.array([[1, 0, 0], taps[0]]))
    assert np.array_equal(both[0], x[0]) and np.allclose(both[1, 0], want, atol=1e-15)


def test_a_constant_plane_is_a_fixed_point_of_the_replicate_edge_blur():
    for radius in (1, 7, 64):
        taps = lr.gaussian_taps([radius / 3.0], radius)
        total = float(taps[0, 0].astype(F64) + 2 * taps[0, 1:].astype(F64).sum())
        assert abs(total - 1) < (radius + 1) * 2.0 ** -24  # (the cast's rounding)
        x = np.full((1, 1, 5, 6), 0.75)
        assert np.allclose(lr.blur(x, taps), 0.75 * total * total, rtol=1e-14)
        # zero-padded edges (the wrong variant) lose light at the border
        assert lr.blur(x, taps, edge="zero")[0, 0, 0, 0] < 0.75 - 0.01


def test_an_impulse_in_a_corner_shows_the_replicate_rule():
    taps = np.array([[0.5, 0.25]])
    x = np.zeros((1, 1, 3, 4))
    x[0, 0, 0, 0] = 1
    # along a row: y[0] = 0.5 x[0] + 0.25 (x[clamp(-1)] + x[1]) = 0.75, y[1] = 0.25; the same down the column
    want = np.zeros((3, 4))
    want[:2, :2] = np.outer([0.75, 0.25], [0.75, 0.25])
    assert np.array_equal(lr.blur(x, taps)[0, 0], want)
    assert lr.blur(x, taps, edge="zero")[0, 0, 0, 0] == 0.25
    # every tap clamped: a radius of the plane's width on a 1 x 1 plane returns the pixel times the taps' sum
    assert lr.blur(np.full((1, 1, 1, 1), 3.0), np.array([[0.5, 0.125, 0.125]]))[0, 0, 0, 0] == 3.0 * 1.0 * 1.0


def _grey(v):
    return np.full((1, 3, 1, 1), 2 * v - 1, F64)


def test_the_knee_formula_on_hand_values():
    rows = lr.make_row(threshold=0.5, knee=0.1)[None]
    th, kn = float(rows[0, lr.THRESHOLD]), float(rows[0, lr.KNEE])
    assert lr.highlight(_grey(0.3), rows).max() == 0  # below threshold - knee
    assert lr.highlight(_grey(th - kn), rows).max() < 1e-30
    far = lr.highlight(_grey(0.9), rows)[0, :, 0, 0]
    assert np.allclose(far, 0.9 * (0.9 - th) / 0.9, rtol=1e-12)  # far above: v (m - threshold) / m
    # inside the knee: s = (m - th + knee)^2 / (4 knee + 1e-5)
    mid = lr.highlight(_grey(th), rows)[0, 0, 0, 0]
    assert np.isclose(mid, th * (kn * kn / (4 * kn + 1e-5)) / th, rtol=1e-12) and mid > 0
    # the hue is kept: hl_c = v_c q with one q for the pixel
    x = (2 * np.array([0.9, 0.45, 0.0]) - 1).reshape(1, 3, 1, 1)
    hl = lr.highlight(x, rows)[0, :, 0, 0]
    assert np.allclose(hl, np.array([0.9, 0.45, 0.0]) * (0.4 / 0.9), rtol=1e-12)
    # knee 0: a hard threshold; threshold 1: nothing glows without a knee; NaN pixels are black; out-of-range pixels are clamped
    hard = lr.make_row(threshold=0.5, knee=0)[None]
    assert lr.highlight(_grey(0.5), hard).max() == 0 and np.isclose(lr.highlight(_grey(0.75), hard).max(), 0.25)
    assert lr.highlight(_grey(1.0), lr.make_row(threshold=1, knee=0)[None]).max() == 0
    assert lr.highlight(np.full((1, 3, 1, 1), np.nan), rows).max() == 0
    assert np.array_equal(lr.highlight(_grey(4.0), rows), lr.highlight(_grey(1.0), rows))
    # the wrong variant: the knee ignored
    assert lr.highlight(_grey(th), rows, knee=False).max() == 0


def test_box_reduction_of_a_5_by_7_plane_shows_the_edge_block_counts():
    hl = np.arange(35, dtype=F64).reshape(1, 1, 5, 7)
    two = lr.box_reduce(hl, 2)
    assert two.shape == (1, 1, 3, 4)
    assert two[0, 0, 0, 0] == (0 + 1 + 7 + 8) / 4 and two[0, 0, 0, 3] == (6 + 13) / 2  # a column block of one pixel's width
    assert two[0, 0, 2, 0] == (28 + 29) / 2 and two[0, 0, 2, 3] == 34  # the bottom row block; the corner block of one pixel
    four = lr.box_reduce(hl, 4)
    assert four.shape == (1, 1, 2, 2)
    assert four[0, 0, 0, 0] == hl[0, 0, :4, :4].mean() and four[0, 0, 0, 1] == hl[0, 0, :4, 4:].mean()
    assert four[0, 0, 1, 0] == hl[0, 0, 4:, :4].mean() and four[0, 0, 1, 1] == hl[0, 0, 4:, 4:].mean()
    assert np.array_equal(lr.box_reduce(hl, 1), hl)
    assert lr.box_reduce(hl, 8).shape == (1, 1, 1, 1) and lr.box_reduce(hl, 8)[0, 0, 0, 0] == 17


def test_the_bilinear_up_sample_of_a_ramp_is_a_ramp_away_from_the_clamp():
    d, bh, bw = 4, 3, 5
    small = np.broadcast_to(np.arange(bw, dtype=F64), (1, 3, bh, bw)).copy()
    up = lr.upsample(small, bh * d, bw * d, d)
    px = np.arange(bw * d)
    want = (px + 0.5) / d - 0.5  # the cell centre of reduced cell i is at pixel (i + 0.5) d - 0.5
    inside = (want >= 0) & (want <= bw - 1)
    assert inside.sum() == bw * d - d and np.allclose(up[0, 0, 5, inside], want[inside], atol=1e-14)
    assert (up[0, 0, :, :2] == 0).all() and (up[0, 0, :, -2:] == bw - 1).all()  # clamped
    # without the half-pixel shift (the wrong variant) the ramp is displaced by (d - 1) / (2 d) of a cell
    wrong = lr.upsample(small, bh * d, bw * d, d, half_pixel=False)
    assert np.allclose(wrong[0, 0, 5, 4:12] - up[0, 0, 5, 4:12], 0.5 - 0.5 / d)
    # a 1 x 1 map: every sample clamped
    assert (lr.upsample(np.full((1, 3, 1, 1), 0.3), 7, 9, 8) == 0.3).all()


def test_the_vignette_is_one_at_the_centre_and_one_minus_strength_at_the_corner():
    f = lr.vignette_factor(64, 48, 0.6, 0.0, 1.0)
    r_centre = math.hypot(0.5 / 32, 0.5 / 24) / math.sqrt(2)
    assert abs(f[32, 24] - (1 - 0.6 * r_centre ** 2 * (3 - 2 * r_centre))) < 1e-12 and f[32, 24] > 0.999
    r_corner = math.hypot(1 - 0.5 / 32, 1 - 0.5 / 24) / math.sqrt(2)  # the corner PIXEL's centre; the corner itself has r = 1
    assert abs(f[0, 0] - (1 - 0.6 * r_corner ** 2 * (3 - 2 * r_corner))) < 1e-12 and abs(f[0, 0] - 0.4) < 0.01
    big = lr.vignette_factor(4096, 4096, 0.6, 0.0, 1.0)
    assert abs(big[0, 0] - 0.4) < 1e-5 and abs(big[2048, 2048] - 1) < 1e-6
    assert np.array_equal(f, f[::-1]) and np.array_equal(f, f[:, ::-1])
    # inside the inner radius nothing changes; it acts in display range: black stays black
    f = lr.vignette_factor(64, 64, 0.5, 0.5, 1.0)
    assert (f[24:40, 24:40] == 1).all()
    rows = lr.make_row(vignette=0.5, inner=0.0, outer=1.0)[None]
    assert (lr.apply(np.full((1, 3, 8, 8), -1.0), rows) == -1).all()


def test_apply_composes_the_terms_and_keeps_identity_frames_bits():
    x = lr.image(3, 6, 8, seed=1)
    x.reshape(-1).view(np.uint32)[:3] = (0x7FC12345, 0xFFC00001, 0x7F800001)
    rows = np.stack([lr.make_row(), lr.make_row(bloom_rgb=(1, 0.5, 0.25), sharpen=0.5), lr.make_row(sharpen=-1)])
    soft = lr.image(3, 6, 8, seed=2)
    bloom = np.abs(lr.image(3, 3, 4, seed=3))
    y = lr.apply(x, rows, bloom, 2, soft, F32)
    assert np.array_equal(y[0].view(np.uint32), x[0].view(np.uint32))
    up = lr.upsample(bloom, 6, 8, 2)
    want = x[1].astype(F64) + 0.5 * (x[1].astype(F64) - soft[1]) + 2 * np.array([1, 0.5, 0.25])[:, None, None] * up[1]
    assert np.allclose(y[1], want, atol=1e-5)
    assert np.allclose(y[2], soft[2], atol=1e-6)  # sharpen -1 is the blur itself
    # the wrong variant: the bloom without its factor 2
    assert np.allclose(lr.apply(x, rows, bloom, 2, soft, bloom_factor=1)[1], want - np.array([1, 0.5, 0.25])[:, None, None] * up[1], atol=1e-12)


# ------------------------------------------------------------------------------------------------------------------ the plan rule
def test_the_plan_rule():
    import maua_stylegan2_amd.audioreactive as ar

    assert [lr.plan_reduction(s) for s in (0, 6, 6.01, 12, 12.5, 24, 24.1, 48, 100)] == [1, 1, 2, 2, 4, 4, 8, 8, 8]
    for size, h, d, radius in ((0.02, 256, 1, 16), (0.02, 1024, 4, 16), (0.01, 1024, 2, 16), (0.03, 1024, 8, 12), (0.1, 1024, 8, 39), (0, 1024, 1, 0),
                               (0.16, 1024, 8, 62)):
        lens = ar.Lens(bloom=1, bloom_size=size, sharpen=0.5, sharpen_radius=1.5)
        got = lens.plan(h, h)
        want = lr.plan(size, h, 1.5)
        assert got[:2] == (d, radius) == want[:2] and got[3] == want[3] == 5
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[4], want[4]) and got[2].dtype == F32 and got[2].shape == (1, radius + 1)
        for taps in (got[2], got[4]):
            assert abs(float(taps[0, 0].astype(F64) + 2 * taps[0, 1:].astype(F64).sum()) - 1) < 1e-6 and (np.diff(taps[0]) <= 0).all()
    # per-frame sizes share d and the radius of the widest; sigma 0 is the delta
    lens = ar.Lens(bloom=1, bloom_size=[0, 0.01, 0.03], sharpen=0.3, sharpen_radius=[0, 1, 2])
    d, rb, bt, rs, st = lens.plan(512, 512)
    assert (d, rb, rs) == (4, 12, 6) and bt.shape == (3, 13) and st.shape == (3, 7)
    assert list(bt[0]) == [1] + [0] * 12 and list(st[0]) == [1] + [0] * 6
    sigma = 0.01 * 512 / 4
    g = np.exp(-np.arange(13.0) ** 2 / (2 * sigma * sigma))
    assert np.array_equal(bt[1], (g / (g[0] + 2 * g[1:].sum())).astype(F32))
    # refusals, with the reason
    with pytest.raises(ValueError, match=r"radius is 77 taps.*serves 64"):
        ar.Lens(bloom=1, bloom_size=0.2).plan(1024, 1024)
    ar.Lens(bloom=1, bloom_size=0.2).plan(256, 256)  # (the same fraction on a small checkpoint is fine)
    with pytest.raises(ValueError, match="sharpen_radius of 8.5 px"):
        ar.Lens(sharpen=1, sharpen_radius=8.5)
    assert ar.Lens(sharpen=1, sharpen_radius=8).plan(64, 64)[3] == 24
    with pytest.raises(ValueError):
        lr.plan(0.2, 1024, 1)


def test_a_block_of_a_table_plans_as_the_whole_table_does():
    """The maxima of the plan rule are the whole job's (``plan_max``): with a modulated bloom_size or sharpen_radius a slice, and a rank's
    block under a process group, derive the reduction, the radii and the taps of a frame that the one-rank job derives."""
    import maua_stylegan2_amd.audioreactive as ar

    n, h = 10, 1024
    size, sigma = np.linspace(0.002, 0.02, n), np.linspace(0.5, 3.0, n)
    lens = ar.Lens(bloom=0.5, bloom_size=size, sharpen=0.3, sharpen_radius=sigma)
    assert lens.plan_max == (0.02, 3.0)
    d, rb, bt, rs, st = lens.plan(h, h)
    assert (d, rb, rs) == (4, 16, 9)
    # what the first half would plan on its own: another reduction and other radii
    alone = ar.Lens(bloom=0.5, bloom_size=size[:5], sharpen=0.3, sharpen_radius=sigma[:5]).plan(h, h)
    assert (alone[0], alone[1], alone[3]) == (2, 16, 5) and alone[0] != d and alone[3] != rs
    for lo, hi in ((0, 5), (5, 10), (3, 4)):
        part = lens.slice(lo, hi)
        assert part.plan_max == lens.plan_max
        pd, prb, pbt, prs, pst = part.plan(h, h)
        assert (pd, prb, prs) == (d, rb, rs) and np.array_equal(pbt, bt[lo:hi]) and np.array_equal(pst, st[lo:hi])
        assert part.slice(0, hi - lo).plan_max == lens.plan_max and lr.plan(size, h, sigma)[:2] == (pd, prb)
    # from_tables: a plan_max below the table's own maxima, or beyond the sharpen's limit, is refused
    for bad in ((0.01, 3.0), (0.02, 2.0), (0.02, 9.0), (float("nan"), 3.0)):
        with pytest.raises(ValueError, match="plan_max"):
            ar.Lens.from_tables(lens.table, lens.bloom_size, lens.sharpen_sigma, bad)
    # only rows that HAVE a bloom (a sharpen) count: a lens without one plans d = 1, radius 0, whatever its sizes say
    vig = ar.Lens(vignette=0.3, bloom_size=0.2, sharpen_radius=4.0)
    assert vig.plan_max == (0.0, 0.0) and vig.plan(h, h)[:2] == (1, 0) and vig.plan(h, h)[3] == 0 and list(vig.plan(h, h)[2][0]) == [1]
    mixed = ar.Lens(bloom=[0, 1, 0], bloom_size=[0.2, 0.01, 0.2], sharpen=[0, 0, 1], sharpen_radius=[6, 6, 1])
    assert mixed.plan_max == (0.01, 1.0) and (mixed.plan(h, h)[0], mixed.plan(h, h)[1], mixed.plan(h, h)[3]) == (2, 16, 3)


# ------------------------------------------------------------------------------------------------------------------ wrong variants
def _gpu_like_case(seed=5):
    """The operands of test_lens_gpu.py's whole-chain case (test_the_chain_as_lens_frames_launches_it)."""
    import maua_stylegan2_amd.audioreactive as ar

    b, h, w = 3, 37, 50
    x = lr.image(b, h, w, seed)
    lens = ar.Lens(b, bloom=[0.8, 0.5, 1.0], bloom_size=0.25, bloom_threshold=0.5, bloom_knee=0.15, bloom_tint=(1, 0.8, 0.6), sharpen=[0.5, 0, -0.5],
                   sharpen_radius=1.0)
    d, rb, bt, rs, st = lens.plan(h, w)
    return x, np.array(lens.table), d, bt, st


def test_the_case_list_tells_the_wrong_variants_from_the_definition():
    """Zero-padded edges, an up-sample without the half-pixel shift, the knee ignored, the bloom without its factor 2: each differs from
    the float32 emulation of the definition by far more than the emulation differs from float64 (which is what the GPU tests allow)."""
    x, rows, d, bt, st = _gpu_like_case()
    assert d == 2 and bt.shape[1] - 1 == 14
    want = lr.lens(x, rows, d, bt, st, F32)
    allowed, own = lr.chain_allowance(x, rows, d, bt, st)  # what the GPU test allows the device on this case
    assert 4 * own <= allowed < 1e-5
    for wrong in (dict(edge="zero"), dict(half_pixel=False), dict(knee=False), dict(bloom_factor=1)):
        diff = np.abs(lr.lens(x, rows, d, bt, st, F32, **wrong).astype(F64) - want)
        assert diff.max() > 1000 * allowed, (wrong, diff.max(), allowed)
        assert (diff > allowed).mean() > 0.01, (wrong, (diff > allowed).mean())
    # the blur's own case list: zero-padded edges on every plane and radius >= 1 (real operands, the wide frame)
    for case in lr.blur_cases():
        if case["radius"] == 0:
            continue
        xb, taps = lr.blur_operands(case, "real")
        t = taps[:, :case["radius"] + 1]
        allow, _, ceiling = lr.blur_allowance(xb, t)
        assert allow <= ceiling
        assert np.abs(lr.blur(xb, t, F32, edge="zero").astype(F64) - lr.blur(xb, t, F32))[1].max() > 100 * allow, case


def test_the_float32_emulation_stays_inside_the_stated_ceiling():
    for case in lr.blur_cases():
        x, taps = lr.blur_operands(case, "real")
        allow, own, ceiling = lr.blur_allowance(x, taps[:, :case["radius"] + 1])
        assert own <= 0.25 * ceiling and allow <= ceiling, (case, own, ceiling)
        xd, td = lr.blur_operands(case, "dyadic")
        td = td[:, :case["radius"] + 1]
        assert np.array_equal(lr.blur(xd, td, F32).astype(F64), lr.blur(xd, td, F64)), case  # exact: any order gives these bits


def test_the_blur_case_list_covers_what_the_issue_names():
    cases = lr.blur_cases()
    planes = {c["shape"][2:] for c in cases}
    assert planes == {(1, 1), (3, 5), (17, 33), (63, 65), (64, 64), (65, 63)} and lr.TILE == 64
    for h, w in planes:
        assert {c["radius"] for c in cases if c["shape"][2:] == (h, w)} == {0, 1, min(w, 64), 64}
    assert any(c["stride"] > c["radius"] + 1 for c in cases) and any(c["stride"] == c["radius"] + 1 for c in cases)
    assert all(c["shape"][0] == 2 for c in cases)
    x, taps = lr.blur_operands(cases[5], "real")
    r = cases[5]["radius"]
    assert list(taps[0, :r + 1]) == [1] + [0] * r and taps[1, 1] > 0 and (taps[:, r + 1:] == F32(1e30)).all()


# ------------------------------------------------------------------------------------------------------------------ ar.Lens
def test_lens_rows_and_validation():
    import maua_stylegan2_amd.audioreactive as ar

    assert ar.LENS_ROW == lr.ROW == 16 and ar.Lens is ar.lens.Lens
    lens = ar.Lens()
    assert lens.n_rows == 1 and lens.is_identity and not lens.has_bloom and not lens.has_sharpen and len(lens) == 1
    assert np.array_equal(lens.table[0], lr.make_row(0.7, 0.1, (0, 0, 0), 0, 0, 0.5, 1.0))
    lens = ar.Lens(bloom=0.8, bloom_tint=(1, 0.5, 0.25), bloom_threshold=0.6, bloom_knee=0.2, sharpen=-0.3, vignette=0.4, vignette_inner=0.2, vignette_outer=1.1)
    assert np.array_equal(lens.table[0], lr.make_row(0.6, 0.2, (0.8, 0.4, 0.2), -0.3, 0.4, 0.2, 1.1)) and not lens.is_identity
    assert (lens.table[:, 9:] == 0).all()
    # per-frame sequences: numpy, torch, [n, 1], tints [n, 3]
    kick = np.array([0.0, 1.0, 0.0, 0.5])
    lens = ar.Lens(bloom=kick, vignette=torch.tensor([0.0, 0.0, 0.0, 0.2]).reshape(4, 1), bloom_tint=np.tile([1.0, 0.5, 0.0], (4, 1)))
    assert lens.n_rows == 4 and list(lens.identity) == [True, False, True, False] and lens.has_bloom and not lens.has_sharpen
    assert np.array_equal(lens.table[1, 2:5], F32([1, 0.5, 0])) and lr.is_identity(lens.table).tolist() == lens.identity.tolist()
    assert ar.Lens(5, bloom=1).n_rows == 1 and ar.Lens(4, bloom=kick).n_rows == 4
    assert ar.Lens(bloom=0, sharpen=0, vignette=0, bloom_size=0.5).is_identity
    for bad, match in ((dict(bloom=-1), "bloom must not be negative"), (dict(bloom_knee=-0.1), "knee"), (dict(bloom_threshold=1.5), r"\[0, 1\]"),
                       (dict(bloom_threshold=-0.1), r"\[0, 1\]"), (dict(bloom_size=-0.1), "negative"), (dict(sharpen_radius=-1), "negative"),
                       (dict(vignette_inner=1.0, vignette_outer=1.0), "greater"), (dict(vignette_inner=0.9, vignette_outer=0.3), "greater"),
                       (dict(bloom=float("nan")), "non-finite"), (dict(vignette=[0.1, float("inf")]), "non-finite"),
                       (dict(bloom=kick, sharpen=np.zeros(3)), "4|3"), (dict(n_frames=5, bloom=kick), "n_frames says 5"),
                       (dict(bloom_tint=(1, 1)), "triple"), (dict(bloom_tint=0.5), "triple"), (dict(bloom=np.zeros((2, 2))), "scalar"),
                       (dict(n_frames=0), "positive"), (dict(bloom=1e39), "overflow")):
        with pytest.raises(ValueError, match=match):
            ar.Lens(**bad)


def test_lens_slice_from_tables_and_operands():
    import maua_stylegan2_amd.audioreactive as ar

    lens = ar.Lens(bloom=np.linspace(0, 1, 6), bloom_size=np.linspace(0.01, 0.06, 6), sharpen_radius=np.linspace(0, 2.5, 6), sharpen=0.2)
    part = lens.slice(2, 5)
    assert part.n_rows == 3 and np.array_equal(part.table, lens.table[2:5]) and np.array_equal(part.bloom_size, lens.bloom_size[2:5])
    assert np.array_equal(part.sharpen_sigma, lens.sharpen_sigma[2:5])
    one = ar.Lens(bloom=1)
    assert one.slice(3, 9) is one
    for lo, hi in ((-1, 2), (2, 7), (3, 3), (4, 2)):
        with pytest.raises(ValueError):
            lens.slice(lo, hi)
    again = ar.Lens.from_tables(lens.table, lens.bloom_size, lens.sharpen_sigma)
    assert np.array_equal(again.table, lens.table) and again.plan(100, 80)[:2] == lens.plan(100, 80)[:2]
    for bad in ((lens.table[:, :15], lens.bloom_size, lens.sharpen_sigma), (lens.table, lens.bloom_size[:5], lens.sharpen_sigma),
                (lens.table, -lens.bloom_size, lens.sharpen_sigma), (-lens.table, lens.bloom_size, lens.sharpen_sigma),
                (lens.table, lens.bloom_size, lens.sharpen_sigma + 8)):
        with pytest.raises(ValueError):
            ar.Lens.from_tables(*bad)
    rows, d, rb, bt, rs, st = lens.operands("cpu", 90, 80)
    assert (d, rb, rs) == (1, 17, 8) and rows.dtype == bt.dtype == st.dtype == torch.float32
    assert rows.shape == (6, 16) and bt.shape == (6, 18) and st.shape == (6, 9) and lens.operands("cpu", 90, 80)[0] is rows
    assert np.array_equal(bt.numpy(), lr.plan(lens.bloom_size, 90, lens.sharpen_sigma)[2])


def test_the_lens_flag_parses_and_resolves(built_lib):
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import generate_audiovisual as gav

    assert [f for f, _ in gav.LENS_FLAGS] == ["--lens"] and len(gav.CLI_FLAGS) == 29 and len(gav.GRADE_FLAGS) == 3
    base = ["--ckpt", "c.pt", "--audio_file", "a.wav"]
    assert gav.build_parser().parse_args(base).lens_spec is None and gav._lens_of(gav.build_parser().parse_args(base)) is None
    args = gav.build_parser().parse_args(base + ["--lens", "bloom=0.8,bloom_size=0.03,bloom_threshold=0.6,sharpen=0.4,vignette=0.3"])
    lens = gav._lens_of(args)
    want = ar.Lens(bloom=0.8, bloom_size=0.03, bloom_threshold=0.6, sharpen=0.4, vignette=0.3)
    assert isinstance(lens, ar.Lens) and np.array_equal(lens.table, want.table) and np.array_equal(lens.bloom_size, want.bloom_size)
    assert ar.lens.parse_spec("bloom_tint=1:0.8:0.6, bloom=1") == dict(bloom_tint=[1, 0.8, 0.6], bloom=1)
    for bad in ("", "bloom", "glare=1", "bloom=1,bloom=2", "bloom=x", "bloom=1:2", "bloom_tint=1"):
        with pytest.raises(ValueError, match="--lens"):
            ar.lens.parse_spec(bad)
    # args.lens: an ar.Lens, a callable evaluated on the namespace, a string; next to --lens it is refused
    plugin = ar.Lens(vignette=0.2)
    assert gav._lens_of(argparse.Namespace(lens=plugin)) is plugin
    assert gav._lens_of(argparse.Namespace(lens=lambda a: ar.Lens(a.n_frames, bloom=np.ones(a.n_frames)), n_frames=4)).n_rows == 4
    assert gav._lens_of(argparse.Namespace(lens="vignette=0.2")).table[0, 6] == F32(0.2)
    assert gav._lens_of(argparse.Namespace(lens=lambda a: None)) is None
    with pytest.raises(ValueError, match="cannot be combined"):
        gav._lens_of(argparse.Namespace(lens=plugin, lens_spec="bloom=1"))
    for bad in (3, lambda a: 3):
        with pytest.raises(TypeError, match="ar.Lens"):
            gav._lens_of(argparse.Namespace(lens=bad))


def test_broadcast_lens_hands_every_rank_its_block(monkeypatch, built_lib):
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import generate_audiovisual as gav

    lens = ar.Lens(bloom=np.linspace(0, 1, 10), bloom_size=np.linspace(0.01, 0.05, 10), sharpen=0.2, sharpen_radius=np.linspace(0.5, 2, 10))
    wire = {}

    def broadcast_object(obj):
        if obj is not None:
            wire["sent"] = obj
        return wire["sent"]

    monkeypatch.setattr(gav.sharding, "broadcast_object", broadcast_object)
    monkeypatch.setattr(gav.sharding, "rank_world", lambda: (0, 2))
    first = gav._broadcast_lens(lens, 0, 5)
    monkeypatch.setattr(gav.sharding, "rank_world", lambda: (1, 2))
    second = gav._broadcast_lens(None, 5, 10)
    for part, (lo, hi) in ((first, (0, 5)), (second, (5, 10))):
        assert np.array_equal(part.table, lens.table[lo:hi]) and np.array_equal(part.bloom_size, lens.bloom_size[lo:hi])
        assert np.array_equal(part.sharpen_sigma, lens.sharpen_sigma[lo:hi])
        # the blocks have different maxima of their own; both plan as the whole table does
        assert part.plan_max == lens.plan_max == (0.05, 2.0) and part.plan(1024, 1024)[:2] == lens.plan(1024, 1024)[:2]
        assert np.array_equal(part.plan(1024, 1024)[2], lens.plan(1024, 1024)[2][lo:hi]) and np.array_equal(part.plan(1024, 1024)[4], lens.plan(1024, 1024)[4][lo:hi])
    assert ar.Lens.from_tables(lens.table[:5], lens.bloom_size[:5], lens.sharpen_sigma[:5]).plan(1024, 1024)[1] != lens.plan(1024, 1024)[1]
    assert gav._broadcast_lens(None, 10, 10).n_rows == 1  # a rank without frames: never applied
    with pytest.raises(RuntimeError, match="10 rows"):
        gav._broadcast_lens(None, 8, 12)
    one = ar.Lens(vignette=0.3)
    monkeypatch.setattr(gav.sharding, "rank_world", lambda: (0, 2))
    assert np.array_equal(gav._broadcast_lens(one, 0, 5).table, one.table)
    monkeypatch.setattr(gav.sharding, "rank_world", lambda: (1, 2))
    assert np.array_equal(gav._broadcast_lens(None, 5, 10).table, one.table)


def test_pinned_signatures_and_the_new_surface(built_lib):
    from ctypes import c_int, c_void_p

    from maua_stylegan2_amd import _lib
    from maua_stylegan2_amd import generate_audiovisual as gav
    from maua_stylegan2_amd import render

    sig = inspect.signature(gav.generate)
    assert list(sig.parameters)[-1] == "args" and len(sig.parameters) == 31 and not {"lens", "lens_spec"} & set(sig.parameters)
    graded, lensed = inspect.signature(render.render_graded).parameters, inspect.signature(render.render_lensed).parameters
    assert list(lensed) == list(graded) + ["lens"] and lensed["lens"].default is None and lensed["grade"].default is None
    body = inspect.signature(render.render_frames).parameters
    assert list(body)[-3:] == ["grade", "lens", "feedback"] and body["lens"].default is None
    for fn in (render.render, render.render_shard, render.render_folded, render.render_delivered, render.render_graded, gav._scatter_from_rank0):
        assert "lens" not in inspect.signature(fn).parameters
    assert list(inspect.signature(render.lens_frames).parameters) == ["images", "lens_ops", "first", "count", "scratch"]
    P, I = c_void_p, c_int
    pinned = {
        "maua_lens_extract_f32": [P, P, I, I, I, I, P, I, P],
        "maua_lens_blur_f32": [P, P, I, I, I, I, I, P, I, P],
        "maua_lens_blur_plan": [I, I, I, P, P],
        "maua_lens_apply_f32": [P, P, I, I, I, P, I, P, I, I, I, P, P],
    }
    for name, argtypes in pinned.items():
        assert _lib._SIGNATURES[name] == (c_int, argtypes), name
    assert set(pinned) <= set(_lib.exported_symbols()) and _lib.ABI_VERSION == 8
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "maua_hip.h")).read()
    for name in pinned:
        assert f"int {name}(" in header


def test_the_blur_plan_answers_without_a_device(built_lib):
    """maua_lens_blur_plan is host code: the LDS of a workgroup at every radius and plane height stays within 64 KiB, so that two fit a
    CU's 160 KiB; the instance follows w % 4 and the source's alignment."""
    import ctypes

    from maua_stylegan2_amd import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    fn = lib.maua_lens_blur_plan
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2
    plan = (ctypes.c_int * 6)()
    worst = 0
    for h in (1, 3, 63, 64, 65, 1024):
        for radius in range(65):
            assert fn(h, 64, radius, 4096, plan) == 0
            assert list(plan)[:3] == [1, 64, 64] and plan[5] == 1 and plan[3] == -(-h // 64)
            r4 = (radius + 3) // 4 * 4
            assert plan[4] == 4 * (68 + 16 * (65 + 2 * r4) + 64 * ((min(h, 64) + 3) // 4 * 4 + 2 * radius))
            worst = max(worst, plan[4])
    assert worst == 61776 <= 64 * 1024
    assert fn(64, 64, 3, 4100, plan) == 0 and plan[0] == 0  # a skewed source
    assert fn(64, 63, 3, 4096, plan) == 0 and plan[0] == 0 and plan[3] == 1  # w % 4 != 0
    assert fn(65, 65, 3, 4096, plan) == 0 and plan[3] == 4
    for bad in ((0, 4, 1), (4, 0, 1), (4, 4, -1), (4, 4, 65)):
        assert fn(*bad, 4096, plan) == -22
    assert fn(4, 4, 1, 4096, None) == -22


def test_the_glow_example_builds_a_valid_lens(monkeypatch, built_lib):
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd.audioreactive.examples import default, glow

    n = 12
    kick = torch.tensor([0, 1.0, 0.2, 0, 0, 0.7, 0, 0, 1.5, 0, 0, 0])

    def fake_initialize(args):
        args.lo_onsets = kick[:, None, None]
        return args

    monkeypatch.setattr(default, "initialize", fake_initialize)
    monkeypatch.setattr(ar, "rms", lambda audio, sr, n_frames, **kw: torch.linspace(0, 1.2, n_frames))
    args = glow.initialize(argparse.Namespace(audio=None, sr=8000, n_frames=n))
    lens = args.lens
    assert isinstance(lens, ar.Lens) and lens.n_rows == n and lens.has_bloom and lens.has_sharpen == (glow.SHARPEN != 0)
    assert np.allclose(lens.table[:, 2], glow.BLOOM * np.clip(kick.numpy(), 0, 1)) and np.allclose(lens.table[1, 2:5], glow.BLOOM * np.array(glow.BLOOM_TINT))
    assert lens.table[0, 6] == F32(glow.VIGNETTE[0]) and np.isclose(lens.table[-1, 6], glow.VIGNETTE[1]) and (np.diff(lens.table[:, 6]) <= 0).all()
    assert lens.plan(1024, 1024)[:2] == (8, 10) and lens.plan(256, 256)[:2] == (2, 10)
