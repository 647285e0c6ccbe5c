"""Static checks of the generated gfx950 code of the bend kernels (csrc/bend_ops.hip; no GPU needed: hipcc cross-compiles).  Both kernels
move one read and one write of HBM per element and nothing else: a spill or a scratch array would add memory traffic nothing accounts for,
and the aligned instances must move 16 bytes per lane."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("bend_point_kernel", "bend_morph_kernel")


@pytest.fixture(scope="module")
def bend_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    dst = str(tmp_path_factory.mktemp("isa") / "bend_ops.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{REPO}/include",
                    f"{REPO}/maua_stylegan2_amd/csrc/bend_ops.hip", "-o", dst], check=True, capture_output=True)
    return open(dst).read()


def _metadata(asm, key):
    names = re.findall(r"^\s+\.name:\s+(\S+)", asm, flags=re.M)
    values = [int(v) for v in re.findall(rf"\.{key}:\s+(\d+)", asm)]
    assert names and len(names) == len(values), (len(names), len(values))
    return {n: v for n, v in zip(names, values) if any(k in n for k in KERNELS)}


def _body(asm, mangled):
    """Instructions of one kernel: from its label to its s_endpgm."""
    start = asm.index(f"\n{mangled}:")
    return asm[start: asm.index("s_endpgm", start)]


def test_bend_kernels_do_not_spill_and_use_no_scratch(bend_asm):
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        found = _metadata(bend_asm, key)
        for kernel in KERNELS:  # the aligned (16 bytes per lane) and the element-wise instance of each
            assert sum(kernel in n for n in found) == 2, (kernel, sorted(found))
        assert all(v == 0 for v in found.values()), (key, found)
    assert "scratch_" not in bend_asm


def test_morph_kernel_keeps_its_tile_in_48_kib_of_lds(bend_asm):
    lds = {n: v for n, v in _metadata(bend_asm, "group_segment_fixed_size").items()}
    assert all(v == (48 * 1024 if "bend_morph_kernel" in n else 0) for n, v in lds.items()), lds  # 3 workgroups per CU


def test_aligned_instances_move_16_bytes_per_lane(bend_asm):
    names = [n for n in _metadata(bend_asm, "private_segment_fixed_size")]
    for kernel in KERNELS:
        vec = [n for n in names if kernel in n and "ILb1E" in n]  # template <bool VEC = true>
        assert len(vec) == 1, names
        body = _body(bend_asm, vec[0])
        assert re.search(r"^\s+global_load_dwordx4\s", body, flags=re.M), f"{kernel}: no 16-byte global load"
        assert re.search(r"^\s+global_store_dwordx4\s", body, flags=re.M), f"{kernel}: no 16-byte global store"
        assert not re.search(r"^\s+global_store_(dword|dwordx2|dwordx3)\s", body, flags=re.M), f"{kernel}: narrow global stores"
    morph = _body(bend_asm, [n for n in names if "bend_morph_kernel" in n and "ILb1E" in n][0])
    assert re.search(r"^\s+ds_read_b128\s", morph, flags=re.M) and re.search(r"^\s+ds_write_b128\s", morph, flags=re.M)
