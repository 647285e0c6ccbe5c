"""CPU: the instance table of the generic convolution kernel (tests/golden/conv_instances.json, written by tools/conv_instance_sweep.py)
against what the library answers without a GPU.  maua_modconv_plan_instance is the plan maua_modconv3x3_f32 dispatches through, called
without a launch: every row's name is what the plan gives for its shape, an enumeration of the plan over a range that saturates it
(the comment at make_plan, csrc/modconv.hip, says why) reaches the table's 58 names and no other, and a change of make_plan() that
moves a recorded shape to another split-K layout shows up as a different maua_modconv_ws_floats.  The GPU test
(tests/test_conv_instances_gpu.py) launches the rows and asserts the same names on what really ran."""
import ctypes
import json
import os
import re

import pytest

TABLE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_instances.json")))
ROWS = TABLE["instances"]
NAME = re.compile(r"modconv_mfma_kernel<(32|64|128), (64|128|256), (1|2), ([0-4]), (true|false), (true|false), ([123])>")


@pytest.fixture(scope="module")
def lib(built_lib):
    from maua_stylegan2_amd import _lib

    return _lib.load()


def test_rows_are_distinct_well_formed_and_obey_the_argument_rules():
    names = [r["name"] for r in ROWS]
    assert len(set(names)) == len(names) == 58
    for r in ROWS:
        m = NAME.fullmatch(r["name"])
        assert m, r["name"]
        assert int(m[4]) == r["mode"]
        assert min(r["cin"], r["cout"], r["h"], r["w"], r["batch"]) >= 1
        if r["mode"] in (2, 4):
            assert r["w"] % 2 == 0, r  # maua_modconv3x3_f32: up == 2 / 4 need an even width
        if r["mode"] == 3:
            assert r["w"] % 4 == 0, r  # up == 3: W % 4 == 0
        oh, ow = (2 * r["h"] + 1, 2 * r["w"] + 1) if r["mode"] in (1, 4) else (r["h"], r["w"])
        assert r["split_k"] == (r["ws_floats"] > 0)
        assert r["ws_floats"] == (r["splits"] * r["batch"] * r["cout"] * oh * ow if r["split_k"] else 0)
    # every (mode, FAST) and every (mode, MULTI) combination the kernel has is in the table (mode 4 runs on flat runs: one image per tile)
    seen = {(r["mode"], NAME.fullmatch(r["name"])[5], NAME.fullmatch(r["name"])[6]) for r in ROWS}
    for mode in range(4):
        assert {(mode, a, b) for a in ("true", "false") for b in ("true", "false")} <= seen
    assert {(4, "false", "true"), (4, "false", "false")} <= seen and (4, "true", "true") not in seen


@pytest.mark.parametrize("row", ROWS, ids=lambda r: re.sub(r"[^0-9a-z]+", "_", r["name"][20:-1]))
def test_workspace_size_of_every_row_is_the_recorded_one(lib, row):
    assert lib.maua_modconv_ws_floats(row["batch"], row["cin"], row["cout"], row["h"], row["w"], row["mode"]) == row["ws_floats"]


def plan(lib, batch, cin, cout, h, w, mode):
    from maua_stylegan2_amd import _lib

    return _lib.planned_modconv_instance(batch, cin, cout, h, w, mode)


@pytest.mark.parametrize("row", ROWS, ids=lambda r: re.sub(r"[^0-9a-z]+", "_", r["name"][20:-1]))
def test_plan_gives_the_recorded_name_of_every_row(lib, row):
    assert plan(lib, row["batch"], row["cin"], row["cout"], row["h"], row["w"], row["mode"]) == (0, row["name"])


ENUM_COUT = (8, 32, 40, 64, 72, 96, 128)
ENUM_CIN = (3, 8)
ENUM_H = tuple(range(1, 140)) + (255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2048, 4096)
ENUM_W = tuple(range(1, 300)) + (511, 512, 513, 514, 516, 1023, 1024, 1025, 1026, 1028, 2048, 4096)


def test_enumerated_plan_reaches_exactly_the_table(lib):
    """Every name the plan can answer is a row of the table (so every compiled instance is tested on the GPU) and every row is reached.
    The plan refuses some of these shapes (MAUA_EINVAL: no tile of modes 3 / 4 holds the patch); it never answers MAUA_ENOSYS, i.e. it
    never asks for an instance the library does not hold."""
    buf = ctypes.create_string_buffer(128)
    fn = lib.maua_modconv_plan_instance
    seen, codes = set(), set()
    for mode in range(5):
        widths = [w for w in ENUM_W if not ((mode in (2, 4) and w % 2) or (mode == 3 and w % 4))]
        for cout in ENUM_COUT:
            for cin in ENUM_CIN:
                for h in ENUM_H:
                    for w in widths:
                        rc = fn(1, cin, cout, h, w, mode, buf, 128)
                        if rc == 0:
                            seen.add(buf.value)
                        else:
                            codes.add(rc)
    assert codes <= {-22}, codes
    assert {n.decode() for n in seen} == {r["name"] for r in ROWS}


def test_plan_does_not_depend_on_batch(lib):
    shapes = [(r["cin"], r["cout"], r["h"], r["w"], r["mode"]) for r in ROWS[::7]]
    shapes += [(512, 512, 4, 4, 0), (512, 512, 4, 4, 1), (512, 512, 8, 8, 2), (64, 32, 16, 16, 3), (64, 64, 16, 66, 4), (3, 3, 1, 4, 3)]
    for cin, cout, h, w, mode in shapes:
        first = plan(lib, 1, cin, cout, h, w, mode)
        assert first[0] in (0, -22)
        assert plan(lib, 3, cin, cout, h, w, mode) == first and plan(lib, 8, cin, cout, h, w, mode) == first, (cin, cout, h, w, mode)


def test_plan_entry_refuses_what_the_call_refuses(lib):
    """Width rules, the 2^31 element limit, modes outside 0 .. 4 and bad arguments: MAUA_EINVAL, as maua_modconv3x3_f32 (tests/test_abi.py)."""
    assert plan(lib, 1, 64, 64, 64, 63, 2)[0] == -22 and plan(lib, 1, 64, 64, 64, 66, 3)[0] == -22 and plan(lib, 1, 64, 64, 64, 63, 4)[0] == -22
    assert plan(lib, 1, 64, 64, 4, 4, 4)[0] == -22                                   # grid too small for flat pair runs
    assert plan(lib, 1, 8, 8, 1 << 14, 1 << 14, 0)[0] == -22 and plan(lib, 1, 7, 8, 1 << 14, 1 << 14, 0)[0] == 0
    assert plan(lib, 1, 64, 64, 64, 64, 5)[0] == -22 and plan(lib, 1, 64, 64, 64, 64, -1)[0] == -22 and plan(lib, 0, 64, 64, 64, 64, 0)[0] == -22
    assert lib.maua_modconv_plan_instance(1, 64, 64, 64, 64, 0, None, 128) == -22


def test_rounding_ratios_are_recorded_and_sane():
    """Measured on the CPU (tools/conv_instance_sweep.py --ratios); an F(2,3) / F(2,2) transform amplifies rounding by a few units, F(4,3)
    by a few tens — a ratio outside 1 .. 200 means the emulation or the table is broken, not the arithmetic."""
    rr = TABLE["rounding_ratio"]
    assert set(rr) == {"2", "3", "4"}
    assert all(1.0 <= v <= 200.0 for v in rr.values()), rr
    assert rr["3"] > rr["2"]


def test_emulations_agree_with_fp64_on_one_shape_per_mode():
    """The float32 emulations behind the ratios compute the convolution (a wrong transform would be off by O(1), i.e. ratio ~ 1e7)."""
    import conv_ref

    for mode, shape in ((2, (5, 7, 3, 6, 2)), (3, (5, 7, 3, 8, 2)), (4, (5, 7, 3, 6, 2))):
        assert conv_ref.rounding_ratio(mode, *shape) <= TABLE["rounding_ratio"][str(mode)] * 4
