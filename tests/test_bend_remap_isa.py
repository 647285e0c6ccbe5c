"""Static checks of the generated gfx950 code of the coordinate-remap bend kernel (csrc/bend_remap.hip; no GPU needed: hipcc
cross-compiles).  The kernel is a gather of four taps and one store per element with its coordinate state held in registers over a chunk
of channels: a spill or a scratch array would add memory traffic nothing accounts for.  Code-object metadata only."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNEL = "bend_remap_kernel"


@pytest.fixture(scope="module")
def remap_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    dst = str(tmp_path_factory.mktemp("isa") / "bend_remap.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{REPO}/include",
                    f"{REPO}/maua_stylegan2_amd/csrc/bend_remap.hip", "-o", dst], check=True, capture_output=True)
    return open(dst).read()


def _metadata(asm, key):
    names = re.findall(r"^\s+\.name:\s+(\S+)", asm, flags=re.M)
    kernels = [n for n in names if n.startswith("_Z")]  # (argument names are listed under .name too)
    values = [int(v) for v in re.findall(rf"^\s+\.{key}:\s+(\d+)", asm, flags=re.M)]
    assert kernels and len(kernels) == len(values), (kernels, values)
    return dict(zip(kernels, values))


def test_remap_kernel_does_not_spill_and_uses_no_scratch(remap_asm):
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        found = _metadata(remap_asm, key)
        assert found and all(KERNEL in n for n in found), sorted(found)  # every kernel of the file is a remap kernel
        assert all(v == 0 for v in found.values()), (key, found)


def test_remap_kernel_needs_no_lds_and_keeps_full_occupancy(remap_asm):
    assert all(v == 0 for v in _metadata(remap_asm, "group_segment_fixed_size").values())
    vgprs = _metadata(remap_asm, "vgpr_count")
    assert all(v <= 128 for v in vgprs.values()), vgprs  # 128 registers: 4 waves per SIMD still, enough to hide a gather's latency


def test_kernel_names_stay_apart_from_the_point_and_morph_kernels(remap_asm):
    names = _metadata(remap_asm, "vgpr_count")
    assert not any("bend_point_kernel" in n or "bend_morph_kernel" in n for n in names)  # tests/test_bend_ops_isa.py counts those
