"""CPU: the colour grade's definition (tests/grade_ref.py) on known answers, the float32 emulation against it, the wrong variants the GPU
case list must catch, ar.Grade / .cube files, and the plumbing that carries a grade into generate() without touching a pinned signature."""
import argparse
import inspect

import numpy as np
import pytest
import torch

import grade_ref as gr

F32 = np.float32


def _px(rgb):
    """One pixel (r, g, b in [0, 1]) as the image x = 2 v - 1, [1, 3, 1, 1]."""
    return (2 * np.asarray(rgb, np.float64) - 1).astype(F32).reshape(1, 3, 1, 1)


def _out(y):
    """y [1, 3, 1, 1] -> (r, g, b) in [0, 1]."""
    return (np.asarray(y, np.float64).reshape(3) + 1) / 2


def _row(**kw):
    return gr.make_row(**kw).astype(F32)[None]


# ------------------------------------------------------------------------------------------------------------------ the definition
def test_cdl_on_hand_values():
    # 0.5, 0.25, 0.75 are exact in float32, and so is every product below
    y = _out(gr.grade(_px([0.5, 0.25, 0.75]), _row(slope=[1.5, 2.0, 0.5], offset=[0.125, -0.25, 0.0], power=[2.0, 1.0, 0.5])))
    np.testing.assert_allclose(y, [(0.5 * 1.5 + 0.125) ** 2, 0.25 * 2 - 0.25, np.sqrt(0.375)], rtol=0, atol=1e-15)
    # slope / offset are clamped before the power (CDL v1.2): 0.75 * 2 = 1.5 -> 1; a negative result -> 0, and 0 stays 0 under any power
    y = _out(gr.grade(_px([0.75, 0.25, 0.0]), _row(slope=[2.0, 1.0, 1.0], offset=[0.0, -0.5, 0.0], power=[3.0, 0.3, 0.4])))
    np.testing.assert_array_equal(y, [1.0, 0.0, 0.0])
    # the input is clamped first; a NaN becomes 0 (x = -1)
    x = np.array([3.0, -7.0, np.nan], F32).reshape(1, 3, 1, 1)
    np.testing.assert_array_equal(_out(gr.grade(x, _row(slope=0.5))), [0.5, 0.0, 0.0])


def test_row_helpers_on_known_answers():
    assert gr.exposure_slope(1) == 2.0 and gr.exposure_slope(-2) == 0.25 and gr.exposure_slope(0) == 1.0
    np.testing.assert_allclose(_out(gr.grade(_px([0.125, 0.25, 0.375]), _row(exposure=1))), [0.25, 0.5, 0.75], atol=1e-15)  # +1 stop doubles
    for c in (0.5, 1.7):  # contrast leaves the pivot fixed, and scales distances from it
        s, o = gr.contrast_slope_offset(c, 0.25)
        assert s * 0.25 + o == 0.25 and abs((s * 0.5 + o) - (0.25 + c * 0.25)) < 1e-15
    np.testing.assert_allclose(_out(gr.grade(_px([0.25, 0.5, 0.75]), _row(contrast=1.5, pivot=0.5))), [0.125, 0.5, 0.875], atol=1e-7)
    assert gr.gamma_power(2.0) == 0.5
    np.testing.assert_allclose(_out(gr.grade(_px([0.25, 0.25, 0.25]), _row(gamma=2.0))), [0.5] * 3, atol=1e-15)
    np.testing.assert_allclose(_out(gr.grade(_px([0.5, 0.5, 0.5]), _row(white_balance=[1.5, 1.0, 0.5]))), [0.75, 0.5, 0.25], atol=1e-15)
    # saturation 0: Rec. 709 luma on all three channels
    rgb = np.array([0.75, 0.25, 0.5])
    luma = 0.2126 * 0.75 + 0.7152 * 0.25 + 0.0722 * 0.5
    np.testing.assert_allclose(_out(gr.grade(_px(rgb), _row(saturation=0))), [luma] * 3, atol=2e-7)
    np.testing.assert_array_equal(gr.saturation_matrix(1.0), np.eye(3))
    np.testing.assert_allclose(gr.saturation_matrix(0.0), [[0.2126, 0.7152, 0.0722]] * 3)
    np.testing.assert_allclose(gr.saturation_matrix(0.3).sum(axis=1), 1.0)  # greys stay grey
    # hue: 0 is the identity exactly; 90 and 180 degrees are the SVG closed form (cos, sin) = (0, 1) and (-1, 0)
    np.testing.assert_array_equal(gr.hue_matrix(0), np.eye(3))
    a0 = np.array([[0.213, 0.715, 0.072]] * 3)
    a1 = np.array([[0.787, -0.715, -0.072], [-0.213, 0.285, -0.072], [-0.213, -0.715, 0.928]])
    a2 = np.array([[-0.213, -0.715, 0.928], [0.143, 0.140, -0.283], [-0.787, 0.715, 0.072]])
    np.testing.assert_allclose(gr.hue_matrix(90), a0 + a2, atol=1e-15)
    np.testing.assert_allclose(gr.hue_matrix(180), a0 - a1, atol=1e-15)
    np.testing.assert_allclose(gr.hue_matrix(360), np.eye(3), atol=1e-12)
    np.testing.assert_allclose(gr.hue_matrix(77) @ [1, 1, 1], [1, 1, 1], atol=1e-12)  # luma-preserving on greys
    # an explicit matrix and bias; the matrix is row-major out_c = sum_k M[c][k] t_k
    m = [[0, 1, 0], [0, 0, 1], [0.5, 0, 0]]
    np.testing.assert_allclose(_out(gr.grade(_px([0.5, 0.25, 0.75]), _row(matrix=m, bias=[0.0, 0.125, 0.0]))), [0.25, 0.875, 0.25], atol=1e-15)
    # composition: hue . saturation . user — the user matrix is applied first
    user = np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1.0]])
    row = gr.make_row(hue=40, saturation=0.6, matrix=user)
    np.testing.assert_allclose(row[gr.MATRIX:gr.MATRIX + 9].reshape(3, 3), gr.hue_matrix(40) @ gr.saturation_matrix(0.6) @ user, atol=1e-15)
    assert gr.is_identity(gr.make_row().astype(F32)[None], has_lut=False)[0]


def test_identity_rule():
    x = gr.case_image(2, 3, 5, 0, seed=3)
    rows = np.stack([gr.identity_row(), gr.identity_row()]).astype(F32)
    lut = gr.sample_lut(3)
    y = gr.grade(x, rows, None, F32)
    assert np.array_equal(y.view(np.uint32), x.view(np.uint32))  # bit for bit, NaN included
    rows[:, gr.MIX] = 1
    assert gr.is_identity(rows, has_lut=False).all() and not gr.is_identity(rows, has_lut=True).any()  # with a LUT and a weight the frame is graded
    rows[:, gr.MIX] = 0
    assert gr.is_identity(rows, has_lut=True).all() and np.array_equal(gr.grade(x, rows, lut, F32).view(np.uint32), x.view(np.uint32))
    # why the rule exists: the neutral arithmetic is not the identity in float32
    neutral = rows.copy()
    neutral[:, gr.OFFSET] = F32(1e-30)
    finite = np.isfinite(x) & (np.abs(x) <= 1)
    assert (gr.grade(x, neutral, None, F32)[finite] != x[finite]).any()
    for col in range(gr.MIX):
        off = rows.copy()
        off[1, col] += F32(0.25)
        assert list(gr.is_identity(off, has_lut=False)) == [True, False]


def test_tetra_known_answers():
    rng = np.random.default_rng(1)
    for n in (2, 3, 17):
        lut = gr.sample_lut(n, seed=5)
        g = np.linspace(0, 1, n)
        # exact at the lattice points
        idx = rng.integers(0, n, (50, 3))
        pts = np.stack([g[idx[:, 0]], g[idx[:, 1]], g[idx[:, 2]]], axis=-1)
        np.testing.assert_allclose(gr.tetra(lut, pts), lut[idx[:, 2], idx[:, 1], idx[:, 0]].astype(np.float64), atol=1e-14)
        # an affine function is reproduced to rounding
        b, gg, r = np.meshgrid(g, g, g, indexing="ij")
        affine = np.stack([0.1 + 0.5 * r + 0.2 * gg + 0.1 * b, 0.9 - 0.3 * r - 0.2 * b, 0.2 * gg + 0.6 * b], axis=-1)
        m = rng.uniform(0, 1, (200, 3))
        want = np.stack([0.1 + 0.5 * m[:, 0] + 0.2 * m[:, 1] + 0.1 * m[:, 2], 0.9 - 0.3 * m[:, 0] - 0.2 * m[:, 2], 0.2 * m[:, 1] + 0.6 * m[:, 2]], axis=-1)
        np.testing.assert_allclose(gr.tetra(affine, m), want, atol=1e-13)
        # the independently written barycentric walk, ties and faces included
        m[:20, 1] = m[:20, 0]
        m[20:40, 2] = m[20:40, 1]
        m[40:50] = m[40:50, :1]
        np.testing.assert_allclose(gr.tetra(lut, m), gr.barycentric(lut, m), atol=1e-13)
        # the edge m = 1 reads no index beyond n - 1 and returns the last lattice point
        top = []
        edge = np.array([[1.0, 1.0, 1.0], [1.0, 0.3, 0.0], [0.2, 1.0, 1.0]])
        got = gr.tetra(lut, edge, max_index=top)
        assert top == [n - 1]
        np.testing.assert_allclose(got[0], lut[-1, -1, -1].astype(np.float64), atol=1e-14)
        assert gr.tetra(lut, edge.astype(F32), F32).dtype == F32
    # n = 2: one cell, the six tetrahedra around its main diagonal
    lut = gr.sample_lut(2)
    m = np.array([[0.9, 0.5, 0.1], [0.9, 0.1, 0.5], [0.5, 0.1, 0.9], [0.1, 0.5, 0.9], [0.1, 0.9, 0.5], [0.5, 0.9, 0.1]])
    _, code, w = gr.tetra_setup(m, 2)
    assert list(code) == [0, 1, 2, 3, 4, 5] and np.allclose(w.sum(axis=1), 1) and (w >= 0).all()
    np.testing.assert_allclose(gr.tetra(lut, m), gr.barycentric(lut, m), atol=1e-14)


def test_float32_emulation_stays_within_its_bound():
    """power == 1: every operation is one float32 rounding of values in [0, 1] scaled by the row, so the emulation is within a few hundred
    eps of the definition on the bit-for-bit cases (3e-5: 512 eps); the power cases must leave room under the ceiling."""
    for case in gr.gpu_cases()[::5]:
        x, rows, lut = gr.build_case(case)
        y32, y64 = gr.grade(x, rows, lut, F32), gr.grade(x, rows, lut, np.float64)
        ok = np.isfinite(y64)
        assert np.array_equal(np.isfinite(y32), ok) and np.max(np.abs(y32[ok] - y64[ok])) < 512 * gr.EPS32, case
    for case in gr.power_cases():
        allow, err = gr.allowance(*gr.build_case(case, power=True))
        assert 64 * gr.EPS32 <= allow <= gr.CEILING and err < gr.CEILING / 4, (case, allow, err)


def test_the_gpu_cases_tell_wrong_definitions_apart():
    """Each deliberately wrong variant differs from the definition on the GPU case list by far more than anything the device test allows."""

    def worst(cases, power, **wrong):
        out = 0.0
        for case in cases:
            x, rows, lut = gr.build_case(case, power=power)
            if "sat_weights" in wrong:  # the wrong row helper: the same user-level grade with BT.601 luma weights
                rows_wrong = rows.copy()
                rows_wrong[:] = gr.make_row(saturation=0.4, hue=20).astype(F32)
                rows = rows_wrong.copy()
                rows_wrong[:] = gr.make_row(saturation=0.4, hue=20, sat_weights=gr.BT601).astype(F32)
                a, b = gr.grade(x, rows, lut, F32), gr.grade(x, rows_wrong, lut, F32)
            else:
                a, b = gr.grade(x, rows, lut, F32), gr.grade(x, rows, lut, F32, **wrong)
            ok = np.isfinite(a) & np.isfinite(b)
            out = max(out, float(np.max(np.abs(a[ok] - b[ok]), initial=0)))
        return out

    with_lut = [c for c in gr.gpu_cases() if c["n_lut"] and c["mix"]]
    assert worst(with_lut, False, variant="trilinear") > 1e-2
    assert worst(gr.gpu_cases(), False, variant="transposed") > 1e-2
    assert worst(gr.power_cases(), True, variant="power_first") > 1e-2
    assert worst(gr.gpu_cases(), False, sat_weights=gr.BT601) > 1e-2
    # every shape carries at least one LUT case of every mix, both row kinds and both strides
    cases = gr.gpu_cases()
    assert {c["shape"] for c in cases} == set(gr.SHAPES) and {c["n_lut"] for c in cases} == set(gr.LUT_SIZES)
    assert {c["mix"] for c in cases} == {0.0, 0.5, 1.0} and {c["stride"] for c in cases} == {24, 32} and {c["kind"] for c in cases} == {"graded", "mixed"}


def test_quantiser_twin_is_the_8_bit_twin():
    import deep_ref

    x = gr.case_image(2, 5, 7, 0, seed=9)
    assert np.array_equal(gr.quant8(x), np.ascontiguousarray(deep_ref.quant8(x).transpose(0, 2, 3, 1)))


# ------------------------------------------------------------------------------------------------------------------ ar.Grade
def test_grade_row_layout_column_by_column():
    import maua_stylegan2_amd.audioreactive as ar

    g = ar.Grade(exposure=1, contrast=2, pivot=0.25, slope=[1, 2, 3], offset=[0.1, 0.2, 0.3], power=[1, 2, 4], gamma=2, white_balance=[1, 0.5, 0.25],
                 saturation=0.5, hue=30, matrix=[[1, 2, 3], [4, 5, 6], [7, 8, 9]], bias=[-1, 0, 1], lut_mix=0.75)
    t = g.table
    assert t.shape == (1, 24) and t.dtype == np.float32 and g.n_rows == len(g) == 1 and ar.GRADE_ROW == 24
    want = gr.make_row(exposure=1, contrast=2, pivot=0.25, slope=[1, 2, 3], offset=[0.1, 0.2, 0.3], power=[1, 2, 4], gamma=2, white_balance=[1, 0.5, 0.25],
                       saturation=0.5, hue=30, matrix=[[1, 2, 3], [4, 5, 6], [7, 8, 9]], bias=[-1, 0, 1], lut_mix=0.75)
    np.testing.assert_allclose(t[0], want.astype(F32), rtol=1e-6, atol=0)
    np.testing.assert_allclose(t[0, 0:3], np.array([1, 2 * 0.5, 3 * 0.25]) * 2 * 2, rtol=1e-7)                       # slope
    np.testing.assert_allclose(t[0, 3:6], np.array([0.1, 0.2, 0.3]) * 2 + 0.25 * (1 - 2), rtol=1e-6)                 # offset
    np.testing.assert_allclose(t[0, 6:9], [0.5, 1, 2], rtol=1e-7)                                                    # power / gamma
    np.testing.assert_allclose(t[0, 9:18].reshape(3, 3), gr.hue_matrix(30) @ gr.saturation_matrix(0.5) @ np.arange(1, 10).reshape(3, 3), rtol=1e-6)
    assert list(t[0, 18:21]) == [-1, 0, 1] and t[0, 21] == 0.75 and list(t[0, 22:]) == [0, 0]
    np.testing.assert_allclose(ar.hue_matrix(30), gr.hue_matrix(30), atol=1e-15)
    np.testing.assert_allclose(ar.saturation_matrix(0.5), gr.saturation_matrix(0.5), atol=1e-15)


def test_grade_broadcasting_identity_and_slice():
    import maua_stylegan2_amd.audioreactive as ar

    assert ar.Grade().is_identity and ar.Grade(7).n_rows == 1 and ar.Grade(hue=0, saturation=1, exposure=0, gamma=1).is_identity
    lut = ar.lut_from_function(lambda rgb: rgb ** 2, 5)
    assert not ar.Grade(lut=lut).is_identity and ar.Grade(lut=lut, lut_mix=0).is_identity and ar.Grade(lut=lut).lut_n == 5
    flash = torch.tensor([0.0, 1.0, 0.0, 0.5])
    g = ar.Grade(exposure=flash, saturation=np.array([1.0, 1.0, 1.0, 1.0]), slope=[1, 1, 1])
    assert g.n_rows == 4 and list(g.identity) == [True, False, True, False] and not g.is_identity
    np.testing.assert_allclose(g.table[:, 0], [1, 2, 1, 2 ** 0.5], rtol=1e-7)
    assert np.array_equal(g.table[0, :21], gr.identity_row().astype(F32)[:21])  # a neutral frame's row is THE identity row, bit for bit
    per_channel = ar.Grade(4, offset=np.arange(12.0).reshape(4, 3) / 100, hue=torch.arange(4.0)[:, None])
    assert per_channel.n_rows == 4 and np.allclose(per_channel.table[:, 3:6], np.arange(12).reshape(4, 3) / 100)
    mats = np.stack([np.eye(3) * k for k in (1, 2)])
    assert ar.Grade(matrix=mats).n_rows == 2 and list(ar.Grade(matrix=mats).identity) == [True, False]
    s = g.slice(1, 3)
    assert s.n_rows == 2 and np.array_equal(s.table, g.table[1:3]) and list(s.identity) == [False, True]
    one = ar.Grade(exposure=0.5)
    assert one.slice(3, 9) is one
    with pytest.raises(ValueError, match="slice"):
        g.slice(2, 5)
    with pytest.raises(ValueError, match="slice"):
        g.slice(2, 2)
    rows = g.rows("cpu")
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (4, 24) and rows is g.rows("cpu") and np.array_equal(rows.numpy(), g.table)
    padded = ar.Grade(lut=lut).lut_table("cpu")
    assert tuple(padded.shape) == (125, 4) and np.array_equal(padded.numpy(), gr.pad_lut(lut)) and ar.Grade().lut_table("cpu") is None
    with_lut = one.with_lut(lut, 0.25)
    assert with_lut.lut_n == 5 and with_lut.table[0, 21] == 0.25 and np.array_equal(with_lut.table[0, :21], one.table[0, :21])
    again = ar.Grade.from_table(g.table, lut)
    assert np.array_equal(again.table, g.table) and not again.identity.any()  # (lut_mix is 1 on every row: with a LUT nothing is neutral)


def test_grade_refusals():
    import maua_stylegan2_amd.audioreactive as ar

    for kw, match in [(dict(exposure=float("nan")), "non-finite"), (dict(slope=[1, float("inf"), 1]), "non-finite"), (dict(power=0), "greater than 0"),
                      (dict(power=[1, -1, 1]), "greater than 0"), (dict(gamma=0), "greater than 0"), (dict(lut_mix=1.5), r"\[0, 1\]"),
                      (dict(lut_mix=-0.1), r"\[0, 1\]"), (dict(exposure=np.zeros(4), hue=np.zeros(5)), "entries"),
                      (dict(exposure=[0.0, 0.0, 0.0]), "entries"), (dict(slope=np.ones((4, 2))), "shape"), (dict(matrix=np.eye(4)), "matrix"),
                      (dict(exposure=np.zeros((2, 2, 2))), "dimensions"), (dict(lut=np.zeros((3, 3, 3))), "LUT"), (dict(lut=np.zeros((1, 1, 1, 3))), "LUT"),
                      (dict(lut=np.zeros((66, 66, 66, 3), np.float32)), "LUT"), (dict(lut=np.full((2, 2, 2, 3), np.nan)), "non-finite"),
                      (dict(exposure=200), "overflow")]:
        with pytest.raises(ValueError, match=match):
            ar.Grade(4, **kw)
    with pytest.raises(ValueError, match="n_frames"):
        ar.Grade(0)
    with pytest.raises(ValueError, match="LUT already"):
        ar.Grade(lut=np.zeros((2, 2, 2, 3))).with_lut(np.zeros((2, 2, 2, 3)))
    for table, match in [(np.zeros((2, 23)), "24"), (np.full((1, 24), np.nan), "non-finite"), (np.zeros((1, 24)), "power")]:
        with pytest.raises(ValueError, match=match):
            ar.Grade.from_table(table)
    with pytest.raises(ValueError, match="n must be"):
        ar.lut_from_function(lambda rgb: rgb, 1)
    with pytest.raises(ValueError, match="returned shape"):
        ar.lut_from_function(lambda rgb: rgb[..., :2], 3)


def test_cube_files(tmp_path):
    import maua_stylegan2_amd.audioreactive as ar

    table = gr.sample_lut(5, seed=2)
    path = tmp_path / "look.cube"
    ar.save_cube(path, table, title='a "look"')
    text = path.read_text()
    assert text.startswith("TITLE") and "LUT_3D_SIZE 5" in text and len(text.splitlines()) == 4 + 125
    back = ar.load_cube(path)
    assert back.dtype == np.float32 and np.array_equal(back, table)  # 9 significant digits round-trip float32
    # red is the fastest index of the file, and of the table's last lattice axis
    first_rows = np.array([[float(v) for v in line.split()] for line in text.splitlines()[4:7]], F32)
    assert np.array_equal(first_rows, table[0, 0, :3])
    path.write_text("# a comment\n\nTITLE \"x\"\n  # indented comment\nLUT_3D_SIZE 2\nDOMAIN_MIN 0 0 0\nDOMAIN_MAX 1.0 1.0 1.0\n" +
                    "\n".join(f"{r} {g} {b}" for b in (0, 1) for g in (0, 1) for r in (0, 1)) + "\n")
    ident = ar.load_cube(path)
    assert ident.shape == (2, 2, 2, 3) and list(ident[0, 0, 1]) == [1, 0, 0] and list(ident[1, 0, 0]) == [0, 0, 1]
    assert ar.Grade(lut=str(path)).lut_n == 2  # a path is loaded
    identity = ar.lut_from_function(lambda rgb: rgb, 2)
    assert np.array_equal(identity, ident)
    body = "\n".join("0 0 0" for _ in range(8))
    for content, match in [("LUT_1D_SIZE 4\n0 0 0\n", "1-D"), (f"LUT_3D_SIZE 2\nDOMAIN_MAX 2 2 2\n{body}\n", "domain"),
                           (f"LUT_3D_SIZE 2\nDOMAIN_MIN -1 0 0\n{body}\n", "domain"), (f"LUT_3D_SIZE 2\n{body}\n0 0 0\n", "entries"),
                           (f"{body}\n", "no LUT_3D_SIZE"), (f"LUT_3D_SIZE 2\nLUT_MAGIC 1\n{body}\n", "unknown keyword"),
                           ("LUT_3D_SIZE 2\n0 0\n", "three"), ("LUT_3D_SIZE 2\n0 0 nan\n", "finite"), ("LUT_3D_SIZE 1\n0 0 0\n", "LUT_3D_SIZE"),
                           ("LUT_3D_SIZE 99\n", "LUT_3D_SIZE")]:
        path.write_text(content)
        with pytest.raises(ValueError, match=match):
            ar.load_cube(path)


# ------------------------------------------------------------------------------------------------------------------ plumbing
def test_pinned_signatures_and_the_new_surface(built_lib):
    from maua_stylegan2_amd import generate_audiovisual as gav
    from maua_stylegan2_amd import render

    sig = inspect.signature(gav.generate)
    assert list(sig.parameters)[:3] == ["ckpt", "audio_file", "initialize"] and list(sig.parameters)[-1] == "args" and len(sig.parameters) == 31
    assert not {"grade", "grade_lut", "grade_spec"} & set(sig.parameters)
    delivered = list(inspect.signature(render.render_delivered).parameters)
    graded = inspect.signature(render.render_graded).parameters
    assert list(graded) == delivered + ["grade"] and graded["grade"].default is None
    for fn in (render.render, render.render_shard, render.render_folded, render.render_delivered, gav._scatter_from_rank0):
        assert "grade" not in inspect.signature(fn).parameters
    assert list(inspect.signature(render.grade_frames).parameters) == ["images", "grade_rows", "lut", "scratch", "out"]
    assert list(inspect.signature(gav._scatter_from_rank0).parameters) == ["latents", "noise", "truncation", "bends", "rewrites", "n_frames", "subframes"]
    from maua_stylegan2_amd import _lib

    assert {"maua_grade_f32", "maua_grade_to_u8"} <= set(_lib.exported_symbols()) and _lib.ABI_VERSION == 8


def test_grade_flags_parse_and_resolve(tmp_path, built_lib):
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import generate_audiovisual as gav

    assert [f for f, _ in gav.GRADE_FLAGS] == ["--grade_lut", "--grade_lut_mix", "--grade"]
    assert len(gav.CLI_FLAGS) == 29 and [f for f, _ in gav.DELIVERY_FLAGS] == ["--deliver_size", "--deliver_filter", "--deliver_fit"]
    base = ["--ckpt", "c.pt", "--audio_file", "a.wav"]
    args = gav.build_parser().parse_args(base)
    assert (args.grade_lut, args.grade_lut_mix, args.grade_spec) == (None, 1.0, None) and gav._grade_of(args) is None
    cube = tmp_path / "k.cube"
    ar.save_cube(cube, gr.sample_lut(3))
    args = gav.build_parser().parse_args(base + ["--grade", "exposure=0.3,saturation=1.2,gamma=0.9,hue=15", "--grade_lut", str(cube), "--grade_lut_mix", "0.5"])
    g = gav._grade_of(args)
    want = gr.make_row(exposure=0.3, saturation=1.2, gamma=0.9, hue=15, lut_mix=0.5).astype(F32)
    assert g.n_rows == 1 and g.lut_n == 3 and np.allclose(g.table[0], want, rtol=1e-6, atol=1e-7)
    assert gav._grade_of(gav.build_parser().parse_args(base + ["--grade_lut", str(cube)])).table[0, 21] == 1.0
    ns = argparse.Namespace
    mine = ar.Grade(exposure=[0.0, 1.0])
    assert gav._grade_of(ns(grade=mine)) is mine and gav._grade_of(ns()) is None
    assert gav._grade_of(ns(grade=lambda a: ar.Grade(hue=a.turn), turn=90)).table[0, 9] == F32(gr.hue_matrix(90)[0, 0])
    assert gav._grade_of(ns(grade="slope=1.1:1:0.9")).table[0, 2] == F32(0.9)
    attached = gav._grade_of(ns(grade=mine, grade_lut=str(cube), grade_lut_mix=0.25))
    assert attached.n_rows == 2 and attached.lut_n == 3 and list(attached.table[:, 21]) == [0.25, 0.25] and mine.lut is None
    with pytest.raises(ValueError, match="cannot be combined"):
        gav._grade_of(ns(grade=mine, grade_spec="hue=3"))
    with pytest.raises(ValueError, match="LUT of its own"):
        gav._grade_of(ns(grade=attached, grade_lut=str(cube)))
    with pytest.raises(TypeError, match="ar.Grade"):
        gav._grade_of(ns(grade=3))
    with pytest.raises(TypeError, match="must return"):
        gav._grade_of(ns(grade=lambda a: "no"))


def test_grade_string_errors():
    from maua_stylegan2_amd.audioreactive import grade as g

    assert g.parse_spec(" exposure = 0.5 , bias=0.1:0:-0.1,") == {"exposure": 0.5, "bias": [0.1, 0.0, -0.1]}
    for text, match in [("brightness=1", "not key=value"), ("exposure", "not key=value"), ("exposure=bright", "not a number"), ("hue=1:2:3", "one number"),
                        ("slope=1:2", "one number or three"), ("hue=1,hue=2", "twice"), ("", "no parameter"), ("lut=x.cube", "not key=value")]:
        with pytest.raises(ValueError, match=match):
            g.parse_spec(text)
    import maua_stylegan2_amd.audioreactive as ar

    with pytest.raises(ValueError, match="greater than 0"):
        ar.Grade(**g.parse_spec("gamma=-2"))


def test_render_graded_refuses_a_table_of_the_wrong_length_without_a_device():
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render

    with pytest.raises(ValueError, match="5 rows.*one per rendered frame \\(7\\)"):
        render.GradeOperands(ar.Grade(exposure=np.zeros(5)), 7, 2, torch.device("cpu"))
    with pytest.raises(TypeError, match="Grade"):
        render.GradeOperands("exposure=1", 7, 2, torch.device("cpu"))
    ops = render.GradeOperands(ar.Grade(exposure=1), 7, 4, torch.device("cpu"))
    rows, lut, per_frame = ops.rows, ops.lut, ops.per_frame
    assert tuple(rows.shape) == (4, 24) and rows.is_contiguous() and lut is None and not per_frame and bool((rows[:, 0] == 2).all())
    ops = render.GradeOperands(ar.Grade(exposure=np.zeros(7)), 7, 4, torch.device("cpu"))
    assert tuple(ops.rows.shape) == (7, 24) and ops.per_frame
