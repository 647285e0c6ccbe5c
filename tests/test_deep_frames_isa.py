"""Static check of the generated gfx950 code of csrc/deep_frames.hip (no GPU needed: hipcc cross-compiles), from the kernels' metadata
alone: every kernel of the file — the two quantisers, the 16-bit resize, and the twelve planar instances (three subsamplings x vector /
scalar path x packed / fp32 input), whose strips of up to 2 x 8 pixels x 3 colours live in fully unrolled register arrays — keeps
everything in registers: no spill, no scratch."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("frames_to_u16_kernel", "frames_to_u16_scalar_kernel", "crop_resize_u16_kernel", "rgb48_to_yuv_p10_kernel", "frames_to_yuv_p10_kernel")
N_KERNELS = 3 + 2 * 3 * 2


@pytest.fixture(scope="module")
def deep_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    dst = str(tmp_path_factory.mktemp("isa") / "deep_frames.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{REPO}/include",
                    f"{REPO}/maua_stylegan2_amd/csrc/deep_frames.hip", "-o", dst], check=True, capture_output=True)
    return open(dst).read()


def _metadata(asm, key):
    names = re.findall(r"^\s+\.name:\s+(\S+)", asm, flags=re.M)
    values = [int(v) for v in re.findall(rf"\.{key}:\s+(\d+)", asm)]
    assert names and len(names) == len(values), (len(names), len(values))
    return dict(zip(names, values))


def test_deep_frame_kernels_do_not_spill_and_use_no_scratch(deep_asm):
    vgpr, sgpr = _metadata(deep_asm, "vgpr_count"), _metadata(deep_asm, "sgpr_count")
    assert len(vgpr) == N_KERNELS, sorted(vgpr)
    assert all(any(k in name for k in KERNELS) for name in vgpr), sorted(vgpr)
    for kernel in KERNELS:
        assert any(kernel in name for name in vgpr), kernel
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
        found = _metadata(deep_asm, key)
        assert len(found) == N_KERNELS, (key, sorted(found))
        assert all(v == 0 for v in found.values()), (key, {n: v for n, v in found.items() if v})
    for name in sorted(vgpr):
        print(f"{name}: vgpr {vgpr[name]}, sgpr {sgpr[name]}")
