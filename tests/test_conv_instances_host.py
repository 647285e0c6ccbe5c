"""CPU: the instance table of the generic convolution kernel (tests/golden/conv_instances.json, written by tools/conv_instance_sweep.py)
against what the library answers without a GPU.  A change of make_plan() that moves a recorded shape to another split-K layout shows up
here as a different maua_modconv_ws_floats; the GPU test (tests/test_conv_instances_gpu.py) asserts the instance names themselves."""
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
