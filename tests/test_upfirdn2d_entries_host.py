"""CPU: what the case list of tests/upfirdn_cases.py reaches, asked of the library and not restated.  maua_upfirdn2d_plan_instance is the
plan maua_upfirdn2d_f32 dispatches through (csrc/upfirdn2d.hip plan_upfirdn2d_f32), called without a launch: it names the instance of a
geometry and its workgroups per plane.  Whether an output height is a whole number of tiles is asked the same way — one more output row
opens a new tile row exactly when the last one was full — so no tile size is written down here.  tests/test_upfirdn2d_entries_gpu.py
launches every case."""
import ctypes

import numpy as np
import pytest

from upfirdn_cases import CASES, EDGE_WIDTHS, EXACT_WIDTHS, INSTANCES, TILED
from upfirdn_ref import reference_and_bound, upfirdn_out_shape, upfirdn_ref

EINVAL = -22


@pytest.fixture(scope="module")
def plan(built_lib):
    from maua_stylegan2_amd import _lib

    def ask(case):
        rc, name, tiles_x, tiles_y = _lib.planned_upfirdn2d_instance(*case)
        assert rc == 0, (case, rc)
        return name, tiles_x, tiles_y

    return ask


def one_more(case, axis):
    """The same geometry with one more output row (axis 0) or column (axis 1): the trailing pad grows by the down factor."""
    c = list(case)
    c[13 if axis == 0 else 11] += c[9 if axis == 0 else 8]
    assert np.array(upfirdn_out_shape(c))[1 + axis] == upfirdn_out_shape(case)[1 + axis] + 1
    return tuple(c)


def test_case_list_is_well_formed():
    assert len(set(CASES.values())) == len(CASES) >= 49
    for name, case in CASES.items():
        assert len(case) == 14 and min(upfirdn_out_shape(case)) >= 1, name
    assert sum(int(np.prod(upfirdn_out_shape(c))) for c in CASES.values()) < 1_500_000  # (the suite stays quick)


def test_the_list_reaches_all_16_instances(plan):
    reached = {plan(case)[0] for case in CASES.values()}
    assert reached == set(INSTANCES) and len(INSTANCES) == 16


@pytest.mark.parametrize("inst", TILED)
def test_every_tiled_instance_sees_its_edges(plan, inst):
    mine = {name: case for name, case in CASES.items() if plan(case)[0] == inst}
    two_rows_last_partial = full_rows = two_planes_odd = per_axis_pads = two_cols_last_partial = False
    for name, case in mine.items():
        _, tiles_x, tiles_y = plan(case)
        major, out_h, out_w, _ = upfirdn_out_shape(case)
        taller = plan(one_more(case, 0))
        assert taller[0] == inst and taller[2] in (tiles_y, tiles_y + 1)
        last_row_full = taller[2] == tiles_y + 1
        two_rows_last_partial |= tiles_y >= 2 and not last_row_full
        full_rows |= last_row_full
        two_planes_odd |= major >= 2 and (case[1] * case[2]) % 4 != 0 and (out_h * out_w) % 4 != 0
        per_axis_pads |= case[10] != case[12]
        wider = plan(one_more(case, 1))
        two_cols_last_partial |= tiles_x >= 2 and wider[0] == inst and wider[1] == tiles_x
    assert two_rows_last_partial, f"{inst}: no case with two tile rows and a partial last one"
    assert full_rows, f"{inst}: no case whose height is a whole number of tiles"
    assert two_planes_odd, f"{inst}: no case with major >= 2 and planes that are no multiple of 4 floats"
    assert per_axis_pads, f"{inst}: no case with pad_x0 != pad_y0"
    family, wx = inst.split(".wx")
    family = "tile" if family.startswith("tile") else family
    widths = {upfirdn_out_shape(case)[2] for case in mine.values()}
    if wx == "4":
        assert two_cols_last_partial, f"{inst}: no case with two tile columns and a partial last one"
    else:  # one tile column by construction: the instance's last lane must be in use
        assert all(plan(case)[1] == 1 for case in mine.values())
        assert EXACT_WIDTHS[family][0 if wx == "1" else 1] in widths, (inst, sorted(widths))


@pytest.mark.parametrize("family", ["tile2", "tile3", "tile4", "up2", "down2"])
def test_output_widths_sit_on_both_sides_of_every_dispatch_edge(plan, family):
    """64 | 65 and 128 | 129 outputs (128 | 129 and 256 | 257 for up2) must land on wx1 | wx2 and wx2 | wx4, for every tap count of the
    tile kernel."""
    edges = EDGE_WIDTHS[family.rstrip("234") if family.startswith("tile") else family]
    seen = {}
    for case in CASES.values():
        inst = plan(case)[0]
        if inst.startswith(family + "."):
            seen.setdefault(upfirdn_out_shape(case)[2], set()).add(inst[-1])
    for width, wx in zip(edges, "1224"):
        assert seen.get(width) == {wx}, (family, width, seen.get(width))


def test_plan_entry_refuses_what_the_call_refuses(built_lib):
    """Every refusal of maua_upfirdn2d_f32 that does not depend on a pointer (tests/test_abi.py, tests/test_upfirdn2d_entries_gpu.py:
    REFUSED is shared) and the entry's own: a null or too short buffer.  major == 0 is no refusal: nothing is launched."""
    from maua_stylegan2_amd import _lib
    from upfirdn_cases import REFUSED

    lib = _lib.load()
    for why, case in REFUSED.items():
        assert _lib.planned_upfirdn2d_instance(*case) == (EINVAL, None, 0, 0), why
        assert lib.maua_upfirdn2d_f32(None, None, None, *case, None) == EINVAL, why
        fake = ctypes.c_void_p(256)  # never dereferenced: the call is refused before any launch
        assert lib.maua_upfirdn2d_f32(fake, fake, fake, *case, None) == EINVAL, why
    good = CASES["tile4_two_tile_rows_w64"]
    assert _lib.planned_upfirdn2d_instance(*good) == (0, "tile4.wx1", 1, 2)
    assert _lib.planned_upfirdn2d_instance(0, *good[1:]) == (0, "none", 0, 0)
    buf = ctypes.create_string_buffer(64)
    assert lib.maua_upfirdn2d_plan_instance(*good, None, 64) == EINVAL
    assert lib.maua_upfirdn2d_plan_instance(*good, buf, 0) == EINVAL and lib.maua_upfirdn2d_plan_instance(*good, buf, -1) == EINVAL
    text = b"tile4.wx1 1x2"
    assert lib.maua_upfirdn2d_plan_instance(*good, buf, len(text)) == EINVAL      # no room for the terminator
    assert lib.maua_upfirdn2d_plan_instance(*good, buf, len(text) + 1) == 0 and buf.value == text
    # the grid limit of the tiled kernels (one workgroup per tile) and the 2 GiB plane that sends a tiled geometry to the gather
    assert _lib.planned_upfirdn2d_instance(1 << 30, 1, 1, 1, 4, 4, 1, 1, 1, 1, 3, 3, 3, 3) == (0, "tile4.wx1", 1, 1)
    assert _lib.planned_upfirdn2d_instance((1 << 30) + 1, 200, 1, 1, 4, 4, 1, 1, 1, 1, 3, 3, 3, 3)[0] == EINVAL
    assert _lib.planned_upfirdn2d_instance(1, 23171, 23171, 1, 4, 4, 1, 1, 1, 1, 2, 1, 2, 1)[1] == "generic"
    assert _lib.planned_upfirdn2d_instance(1, 23170, 23170, 1, 4, 4, 1, 1, 1, 1, 2, 1, 2, 1)[1] == "tile4.wx4"


LOOP_CASES = ["tile3_crop_both_axes", "up2_taps_3x4_square_pads", "generic_minor_2_blur", "generic_minor_3_up2", "down2_4x4", "up2_8x8",
              "generic_up3", "generic_up2_down2"]


def test_reference_agrees_with_the_oracle_loops():
    """upfirdn_ref against the scalar float64 loops of oracle/ops_oracle.py (one factor and one pad pair for both axes, so the cases are
    those of the list with such a geometry): a crop, a rectangular tap matrix, minor > 1, up 2, down 2, up 3, both factors."""
    from oracle.ops_oracle import upfirdn2d_loops

    kinds = set()
    for name in LOOP_CASES:
        case = CASES[name]
        major, in_h, in_w, minor, kh, kw, up_x, up_y, down_x, down_y, px0, px1, py0, py1 = case
        assert up_x == up_y and down_x == down_y and (px0, px1) == (py0, py1), name
        kinds |= {kind for kind, here in (("crop", min(px0, px1) < 0), ("rect", kh != kw), ("minor", minor > 1)) if here}
        r = np.random.default_rng(len(name))
        x, k = r.standard_normal((major, in_h, in_w, minor)), r.standard_normal((kh, kw))
        got = upfirdn_ref(x, k, *case[6:])
        want = upfirdn2d_loops(x.transpose(0, 3, 1, 2), k, up_x, down_x, (px0, px1)).transpose(0, 2, 3, 1)
        assert got.shape == want.shape == upfirdn_out_shape(case), name
        assert float(np.abs(got - want).max()) <= 1e-13 * max(1.0, float(np.abs(want).max())), name  # two summation orders in float64
    assert kinds == {"crop", "rect", "minor"} and len(LOOP_CASES) >= 5


def test_integer_operands_make_every_sum_exact():
    """x in -8 .. 8 and k in -4 .. 4: sum |k||x| < 2^24 for every output of every case, so every product and every partial sum is an
    integer that fp32 holds exactly, in any order, and the GPU test may demand equality with the float64 reference."""
    from upfirdn_cases import integer_operands

    for name, case in CASES.items():
        x, k = integer_operands(case)
        assert x.dtype == k.dtype == np.float32 and np.array_equal(x, np.rint(x)) and np.array_equal(k, np.rint(k))
        assert float(np.abs(x).max()) <= 8 and float(np.abs(k).max()) <= 4
        mag = upfirdn_ref(np.abs(x.astype(np.float64)), np.abs(k.astype(np.float64)), *case[6:])
        assert float(mag.max()) < 2.0 ** 24, name
        want, bound = reference_and_bound(x, k, case[6:])
        assert np.array_equal(want, np.rint(want)) and bound.shape == want.shape == upfirdn_out_shape(case)
