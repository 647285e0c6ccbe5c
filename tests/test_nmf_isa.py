"""Static check of the generated gfx950 code of the factorisation kernels (csrc/nmf.hip; no GPU needed: hipcc cross-compiles), from the
kernels' metadata alone: every instance keeps its K accumulators, its H column and the W row in registers — no spill, no scratch."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("nmf_h_kernel", "nmf_w_kernel", "nmf_div_kernel")
INSTANCES = 4  # K tiles 4 / 8 / 16 / 32 of every kernel


@pytest.fixture(scope="module")
def nmf_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    dst = str(tmp_path_factory.mktemp("isa") / "nmf.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{REPO}/include",
                    f"{REPO}/maua_stylegan2_amd/csrc/nmf.hip", "-o", dst], check=True, capture_output=True)
    return open(dst).read()


def _metadata(asm, key):
    names = re.findall(r"^\s+\.name:\s+(\S+)", asm, flags=re.M)
    values = [int(v) for v in re.findall(rf"\.{key}:\s+(\d+)", asm)]
    assert names and len(names) == len(values), (len(names), len(values))
    return {n: v for n, v in zip(names, values) if any(k in n for k in KERNELS)}


def test_nmf_kernels_do_not_spill_and_use_no_scratch(nmf_asm):
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        found = _metadata(nmf_asm, key)
        assert len(found) == INSTANCES * len(KERNELS), sorted(found)
        assert all(v == 0 for v in found.values()), (key, found)
    vgpr, sgpr, lds = (_metadata(nmf_asm, k) for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size"))
    for name in sorted(vgpr):
        print(f"{name}: vgpr {vgpr[name]}, sgpr {sgpr[name]}, static LDS {lds[name]} bytes")
