"""Static check of the generated gfx950 code of csrc/grade.hip (no GPU needed: hipcc cross-compiles), from the kernels' metadata alone:
the eight instances of the grade kernel (output type x vector / scalar path x with / without a LUT) keep everything in registers — no
spill, no scratch —, use no LDS (the row lives in SGPRs, the LUT is gathered), and stay at the occupancy a streaming kernel lives on."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
N_KERNELS = 8


@pytest.fixture(scope="module")
def grade_asm(tmp_path_factory):
    dst = str(tmp_path_factory.mktemp("isa") / "grade.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{REPO}/include",
                    f"{REPO}/maua_stylegan2_amd/csrc/grade.hip", "-o", dst], check=True, capture_output=True)
    return open(dst).read()


def _metadata(asm, key):
    names = re.findall(r"^\s+\.name:\s+(\S+)", asm, flags=re.M)
    values = [int(v) for v in re.findall(rf"\.{key}:\s+(\d+)", asm)]
    assert names and len(names) == len(values), (len(names), len(values))
    return dict(zip(names, values))


def test_grade_kernels_do_not_spill_and_use_no_scratch_or_lds(grade_asm):
    vgpr, sgpr = _metadata(grade_asm, "vgpr_count"), _metadata(grade_asm, "sgpr_count")
    assert len(vgpr) == N_KERNELS and all("grade_kernel" in name for name in vgpr), sorted(vgpr)
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
        found = _metadata(grade_asm, key)
        assert len(found) == N_KERNELS and all(v == 0 for v in found.values()), (key, {n: v for n, v in found.items() if v})
    # grade_kernel<U8, VEC, LUT>: the mangled name carries the three booleans as Lb0E / Lb1E
    flags = {name: tuple(int(b) for b in re.findall(r"Lb([01])E", name)[:3]) for name in vgpr}
    assert sorted(flags.values()) == sorted((u, v, l) for u in (0, 1) for v in (0, 1) for l in (0, 1))
    for name, (_, vec, lut) in flags.items():
        # without a LUT 8 waves per SIMD fit (64 VGPRs); with one, the 16 vertices in flight of a lane's 4 pixels cost registers: 4 waves
        assert vgpr[name] <= (128 if vec and lut else 64), (name, vgpr[name])
    for name in sorted(vgpr):
        print(f"{name}: vgpr {vgpr[name]}, sgpr {sgpr[name]}")
