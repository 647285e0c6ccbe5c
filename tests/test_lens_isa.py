"""Static check of the generated gfx950 code of csrc/lens.hip (no GPU needed: hipcc cross-compiles), from the kernels' metadata alone:
the twelve instances — blur (vector / scalar staging), extract (d = 1, 2, 4, 8 x vector / scalar), apply (vector / scalar) — keep
everything in registers: no spill, no scratch.  Only the blur uses LDS, and all of it is dynamic: maua_lens_blur_plan states the bytes per
workgroup (tests/test_lens_host.py holds it to 64 KiB at every radius); here the static part is shown to be nothing on top of that."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
N_KERNELS = 12
LDS_LIMIT = 64 * 1024


@pytest.fixture(scope="module")
def lens_asm(tmp_path_factory):
    dst = str(tmp_path_factory.mktemp("isa") / "lens.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{REPO}/include",
                    f"{REPO}/maua_stylegan2_amd/csrc/lens.hip", "-o", dst], check=True, capture_output=True)
    return open(dst).read()


def _metadata(asm, key):
    names = re.findall(r"^\s+\.name:\s+(\S+)", asm, flags=re.M)
    values = [int(v) for v in re.findall(rf"\.{key}:\s+(\d+)", asm)]
    assert names and len(names) == len(values), (len(names), len(values))
    return dict(zip(names, values))


def test_lens_kernels_do_not_spill_and_use_no_scratch(lens_asm):
    vgpr, sgpr = _metadata(lens_asm, "vgpr_count"), _metadata(lens_asm, "sgpr_count")
    assert len(vgpr) == N_KERNELS, sorted(vgpr)
    kinds = {k: [n for n in vgpr if k in n] for k in ("lens_blur_kernel", "lens_extract_kernel", "lens_apply_kernel")}
    assert [len(v) for v in kinds.values()] == [2, 8, 2]
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        found = _metadata(lens_asm, key)
        assert len(found) == N_KERNELS and all(v == 0 for v in found.values()), (key, {n: v for n, v in found.items() if v})
    # extract<D, VEC>: the mangled name carries Li<D>E and Lb<VEC>E
    flags = sorted((int(re.search(r"Li(\d)E", n).group(1)), int(re.search(r"Lb([01])E", n).group(1))) for n in kinds["lens_extract_kernel"])
    assert flags == [(d, v) for d in (1, 2, 4, 8) for v in (0, 1)]
    for name in vgpr:
        # the streaming kernels and the blur stay at 8 waves a SIMD (64 VGPRs) except the vector apply, whose 4 pixels x 3 channels x
        # (image, result, four bloom vertices in flight) cost registers: 4 waves
        assert vgpr[name] <= (128 if "lens_apply_kernel" in name else 64), (name, vgpr[name])
    for name in sorted(vgpr):
        print(f"{name}: vgpr {vgpr[name]}, sgpr {sgpr[name]}")


def test_the_blurs_lds_is_the_dynamic_allocation_the_plan_reports(lens_asm, built_lib):
    """No kernel has static LDS, so a blur workgroup's LDS is what the launcher asks for: the bytes maua_lens_blur_plan (host code, the
    launcher's own formula) reports, within the limit at every radius and plane height, so that two workgroups fit a CU."""
    import ctypes

    lds = _metadata(lens_asm, "group_segment_fixed_size")
    assert len(lds) == N_KERNELS and all(v == 0 for v in lds.values()), {n: v for n, v in lds.items() if v}
    fn = ctypes.CDLL(built_lib).maua_lens_blur_plan
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2
    plan = (ctypes.c_int * 6)()
    worst = 0
    for h in (1, 17, 63, 64, 65, 4096):
        for radius in range(65):
            assert fn(h, 256, radius, 4096, plan) == 0
            worst = max(worst, plan[4])
    assert 0 < worst <= LDS_LIMIT
    # no inline assembly anywhere in the file
    src = open(f"{REPO}/maua_stylegan2_amd/csrc/lens.hip").read()
    assert "asm" not in re.sub(r"//.*", "", src)
