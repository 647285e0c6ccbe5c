"""Static check of the generated gfx950 code of csrc/resample.hip (no GPU needed: hipcc cross-compiles), from the kernels' metadata alone:
the four fused instances (sample type x store path) and the four two-pass kernels keep everything in registers — no spill, no scratch —
and declare no static LDS: the fused kernel's LDS is all dynamic, sized per launch by the planner, whose every answer stays within the 64
KB a launch may ask for without an attribute (maua_resample_plan's ``lds`` field, swept here over the geometries that matter)."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("resample_fused_kernel", "resample_h_kernel", "resample_v_kernel")
N_KERNELS = 4 + 2 + 2
LDS_LIMIT = 64 * 1024


@pytest.fixture(scope="module")
def resample_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    dst = str(tmp_path_factory.mktemp("isa") / "resample.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{REPO}/include",
                    f"{REPO}/maua_stylegan2_amd/csrc/resample.hip", "-o", dst], check=True, capture_output=True)
    return open(dst).read()


def _metadata(asm, key):
    names = re.findall(r"^\s+\.name:\s+(\S+)", asm, flags=re.M)
    values = [int(v) for v in re.findall(rf"\.{key}:\s+(\d+)", asm)]
    assert names and len(names) == len(values), (len(names), len(values))
    return dict(zip(names, values))


def test_resample_kernels_do_not_spill_use_no_scratch_and_no_static_lds(resample_asm):
    vgpr, sgpr = _metadata(resample_asm, "vgpr_count"), _metadata(resample_asm, "sgpr_count")
    assert len(vgpr) == N_KERNELS, sorted(vgpr)
    assert all(any(k in name for k in KERNELS) for name in vgpr), sorted(vgpr)
    for kernel in KERNELS:
        assert any(kernel in name for name in vgpr), kernel
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
        found = _metadata(resample_asm, key)
        assert len(found) == N_KERNELS, (key, sorted(found))
        assert all(v == 0 for v in found.values()), (key, {n: v for n, v in found.items() if v})
    assert max(vgpr.values()) <= 128, vgpr  # two workgroups of 256 threads per SIMD pair at least: the kernel lives on occupancy
    for name in sorted(vgpr):
        print(f"{name}: vgpr {vgpr[name]}, sgpr {sgpr[name]}")


def test_planned_dynamic_lds_stays_within_the_default_limit(built_lib):
    """Every fused plan's ``lds`` is at most 64 KB and holds the tables plus ``rows`` rows of 64 pixels (a tile of 64, 32 or 16 rows); a
    geometry that would need more is planned as two-pass, never as a larger allocation."""
    from maua_stylegan2_amd import _lib

    seen = set()
    for sz in (1, 2):
        for ksx in (0, 1, 3, 7, 21, 63, 64):
            for ksy in (0, 1, 3, 7, 21, 41, 63, 64):
                for in_h, dst_h in ((3, 16400), (1024, 1080), (1024, 512), (1024, 103), (2000, 20), (64, 64)):
                    if (ksy == 0) != (in_h == dst_h):
                        continue
                    in_w = dst_w = 70
                    rc, name, fields = _lib.planned_resample(sz, 1, in_h, in_w, dst_h, dst_w, 0, 0, dst_w, dst_h, ksx, ksy)
                    assert rc == 0, (sz, ksx, ksy, in_h, dst_h, rc)
                    seen.add(name.split(".")[0])
                    if name.startswith("fused"):
                        stride = lambda k: max(k, 1) | 1  # noqa: E731
                        th = int(fields["tile"].split("x")[1])
                        assert th in (64, 32, 16)
                        tables = 4 * (64 * stride(ksx) + 128 + th * stride(ksy) + 2 * th)
                        assert int(fields["lds"]) == tables + int(fields["rows"]) * 64 * 3 * sz <= LDS_LIMIT, (name, fields)
                        assert int(fields["rows"]) >= max(ksy, 1)  # one output row's taps always fit: the tile loop can make progress
    assert seen == {"fused", "twopass"}
