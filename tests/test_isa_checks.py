"""Static checks of the generated gfx950 code of the two hot convolution kernels (no GPU needed: hipcc cross-compiles).

Why they exist: in round 3 a prologue change made the compiler treat a buffer resource descriptor as divergent; every LDS-DMA
instruction of the K loop was then wrapped in a waterfall loop (v_readfirstlane x4 + compare + s_and_saveexec), +25 % VALU per K step
and -6 % on the whole plain-layer family, with every parity test still green.  Nothing but the ISA shows that."""
import json
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SOURCES = ("modconv_w2d", "modconv_up2d")
STREAMING = ("upfirdn2d",)  # HBM-bound kernels: no LDS-DMA, but a spill or a scratch array there is HBM traffic the roofline does not count
# the generic convolution kernel, one unit per mode: which instances the product build holds, and that the FAST ones do not spill
GENERIC = ("modconv_m0", "modconv_m1", "modconv_m2", "modconv_m3", "modconv_m4")
SIDE = ("modconv_sbf16",)  # the split-bf16 side measurement: only which kernels the product build holds


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa")

    def build(name):
        dst = str(out / f"{name}.s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{REPO}/include",
                        f"{REPO}/maua_stylegan2_amd/csrc/{name}.hip", "-o", dst], check=True, capture_output=True)
        return name, open(dst).read()

    with ThreadPoolExecutor(len(SOURCES + STREAMING + GENERIC + SIDE)) as pool:
        return dict(pool.map(build, SOURCES + STREAMING + GENERIC + SIDE))


@pytest.mark.parametrize("name", SOURCES)
def test_lds_dma_loads_are_not_waterfalled(device_asm, name):
    lines = device_asm[name].split("\n")
    dma = [i for i, line in enumerate(lines) if "buffer_load" in line and " lds" in line]
    assert dma, "the kernels stage their operands with buffer_load ... lds"
    for i in dma:
        before = " ".join(lines[max(0, i - 10):i])
        assert not ("v_readfirstlane" in before and "s_and_saveexec" in before), (
            f"{name}.hip: the LDS-DMA load at asm line {i} sits in a waterfall loop — its buffer descriptor is no longer uniform "
            "(keep __builtin_amdgcn_make_buffer_rsrc ahead of thread-dependent prologue loops)")


# The persistent fused kernel (modconv_up2d_kernel<8, 2>, round 5) walks several tiles per workgroup: workgroup constants of its per-tile
# prologue (LDS destinations of the operand DMA, a few uniform conditions) survive a K loop that uses every register, as SGPR -> vector-lane
# copies made once per workgroup and a handful of dwords of scratch re-read once per TILE (~40 us).  That is tolerated for this one instance —
# bounded here, and only OUTSIDE the K loop (test_fused_kernel_spills_stay_outside_the_k_loop); every other hot kernel stays at zero.
FUSED = "modconv_up2d_kernelILi8ELi2E"
FUSED_LIMITS = {"vgpr": 8, "sgpr": 40, "scratch": 40}


def _per_kernel(asm, key):
    """{kernel symbol: value} of a .amdhsa metadata key listed once per kernel (in the order of the .name entries)."""
    names = re.findall(r"^\s+\.name:\s+(\S+)", asm, flags=re.M)
    values = [int(v) for v in re.findall(rf"\.{key}:\s+(\d+)", asm)]
    assert names and len(names) == len(values), (len(names), len(values))
    return dict(zip(names, values))


@pytest.mark.parametrize("name", SOURCES + STREAMING)
def test_hot_kernels_do_not_spill(device_asm, name):
    vg, sg = _per_kernel(device_asm[name], "vgpr_spill_count"), _per_kernel(device_asm[name], "sgpr_spill_count")
    for kernel in vg:
        if FUSED in kernel:
            assert vg[kernel] <= FUSED_LIMITS["vgpr"] and sg[kernel] <= FUSED_LIMITS["sgpr"], (kernel, vg[kernel], sg[kernel])
        elif name in STREAMING:
            # the FIR kernels hold 16 taps + row offsets in SGPRs: their 32-row instances park up to 44 of them in vector lanes (v_writelane /
            # v_readlane, no memory); what must not happen in an HBM-bound kernel is a spill to MEMORY
            assert vg[kernel] == 0 and sg[kernel] <= 48, (kernel, vg[kernel], sg[kernel])
        else:
            assert vg[kernel] == 0 and sg[kernel] == 0, (kernel, vg[kernel], sg[kernel])


@pytest.mark.parametrize("name", SOURCES + STREAMING)
def test_hot_kernels_use_no_scratch_memory(device_asm, name):
    """A dynamically indexed register array (e.g. `cond ? acc[1] : acc[0]` on vectors) is lowered to a scratch buffer without counting
    as a spill: the first build of the wave-complete 32-channel kernel carried 112 bytes of it in its epilogue."""
    sizes = _per_kernel(device_asm[name], "private_segment_fixed_size")
    for kernel, size in sizes.items():
        assert size <= (FUSED_LIMITS["scratch"] if FUSED in kernel else 0), (kernel, size)


def test_generic_conv_kernel_compiled_set_is_the_instance_table(device_asm):
    """csrc/modconv_m0.hip .. modconv_m4.hip instantiate modconv_mfma_kernel (csrc/modconv_kernel.h), each from the table of its mode
    (MAUA_CONV_ROWS); together, and each in exactly one unit, the product build must hold exactly the 58 instances of
    tests/golden/conv_instances.json — the ones the plan can reach (tests/test_conv_instances_host.py enumerates it) and the GPU test launches — so no kernel is compiled that no call runs, and none is tested that is not compiled.  The FAST instances
    (channel counts in whole K chunks and weight tiles: every layer of a real generator) keep everything in registers; the ragged-channel
    instances carry 12 .. 196 bytes of scratch for their masked loads and are not held to that."""
    table = json.load(open(os.path.join(REPO, "tests", "golden", "conv_instances.json")))["instances"]
    mangled = re.compile(r"modconv_mfma_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])ELi(\d+)EE")

    def demangled(symbol):
        bm, bn, wm, mode, multi, fast, maxp = mangled.search(symbol).groups()
        return f"modconv_mfma_kernel<{bm}, {bn}, {wm}, {mode}, {('false', 'true')[int(multi)]}, {('false', 'true')[int(fast)]}, {maxp}>"

    spills, scratch, symbols = {}, {}, []
    for unit in GENERIC:
        unit_spills = _per_kernel(device_asm[unit], "vgpr_spill_count")
        symbols += [k for k in unit_spills if "modconv_mfma_kernel" in k]
        spills.update(unit_spills)
        scratch.update(_per_kernel(device_asm[unit], "private_segment_fixed_size"))
    assert len(set(symbols)) == len(symbols), "an instance is compiled in two units"
    assert sorted(demangled(k) for k in symbols) == sorted(r["name"] for r in table) and len(symbols) == 58
    fast = [k for k in symbols if mangled.search(k).group(6) == "1"]
    assert len(fast) == 29
    for k in fast:
        assert spills[k] == 0 and scratch[k] == 0, (demangled(k), spills[k], scratch[k])


def test_dedicated_conv_kernels_compiled_set_is_the_dedicated_table(device_asm):
    """csrc/modconv_w2d.hip, modconv_up2d.hip and modconv_sbf16.hip: the product build must hold exactly the conv kernel instances named in
    tests/golden/conv_dedicated_instances.json (6 + 7 + 2, each launched by tests/test_conv_dedicated_gpu.py under that name) plus the
    helper kernels listed here — no kernel is compiled that no case runs, and none is tested that is not compiled."""
    table = json.load(open(os.path.join(REPO, "tests", "golden", "conv_dedicated_instances.json")))["instances"]
    helpers = {"modconv_w2d": {"pack_weight_wino2d_kernel"},
               "modconv_up2d": {"up2d_seam_kernel", "up2d_edge_kernel", "pack_weight_up2d_kernel"},
               "modconv_sbf16": {"export_last_column_kernel", "pack_weight_sbf16_kernel", "pack_edge_taps_kernel"}}
    flag = ("false", "true")

    def demangled(symbol):
        if m := re.search(r"\d+modconv_w2d_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])EE", symbol):
            return f"modconv_w2d_kernel<{m[1]}, {m[2]}, {m[3]}, {flag[int(m[4])]}>"
        if m := re.search(r"\d+modconv_w2dw_kernelILb([01])EE", symbol):
            return f"modconv_w2dw_kernel<{flag[int(m[1])]}>"
        if m := re.search(r"\d+modconv_up2d_kernelILi(\d+)ELi(\d+)ELb([01])ELi(\d+)EE", symbol):
            return f"modconv_up2d_kernel<{m[1]}, {m[2]}, {flag[int(m[3])]}, {m[4]}>"
        if m := re.search(r"\d+modconv_sbf16_kernelILi(n?)(\d+)EE", symbol):
            return f"modconv_sbf16_kernel<{'-' if m[1] else ''}{m[2]}>"
        if re.search(r"\d+modconv_sbf16_up_kernelE", symbol):
            return "modconv_sbf16_up_kernel"
        m = re.match(r"_ZN12_GLOBAL__N_1\d+([a-z0-9_]+?)E", symbol)
        assert m, symbol
        return m[1]

    compiled = {}
    for source in SOURCES + SIDE:
        names = [demangled(k) for k in re.findall(r"^\s+\.name:\s+(_Z\S+)", device_asm[source], flags=re.M)]
        assert len(set(names)) == len(names), names
        assert helpers[source] <= set(names), (source, names)
        compiled[source] = set(names) - helpers[source]
    assert [len(compiled[k]) for k in SOURCES + SIDE] == [6, 7, 2], compiled
    assert set().union(*compiled.values()) == {r["name"] for r in table}


def test_fused_kernel_spills_stay_outside_the_k_loop(device_asm):
    """The K loop of the persistent fused kernel must be as clean as the plain kernel's: no scratch access, no SGPR <-> lane copy, no
    waterfall — its (bounded) spills belong to the per-tile prologue / epilogue."""
    body = _kernel_body(device_asm["modconv_up2d"], FUSED)
    first, last = _main_loop(body)
    loop = body[first:last + 1]
    assert sum("v_mfma" in line for line in loop) == 100, "two K groups of 50 matrix instructions per step"
    bad = [line.strip() for line in loop if re.search(r"scratch_|v_readlane|v_writelane|v_readfirstlane", line)]
    assert not bad, bad[:5]
    # one exec-masked region is legitimate: the right-edge tile column zeroes image column W of its operand rows after the DMA (a uniform
    # branch no other tile takes); a waterfall loop would show as several
    assert sum("s_and_saveexec" in line for line in loop) <= 1


def _kernel_body(asm, mangled_fragment):
    lines = asm.split("\n")
    start = next(i for i, line in enumerate(lines) if line.startswith("_Z") and mangled_fragment in line.split(":")[0])
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    return lines[start + 1:end]


def _main_loop(body):
    """(first, last) line index of the backward-branch loop that holds the most matrix instructions."""
    labels = {m.group(1): i for i, line in enumerate(body) if (m := re.match(r"^(\.LBB\d+_\d+):", line))}
    loops = []
    for i, line in enumerate(body):
        m = re.search(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", line)
        if m and labels.get(m.group(1), len(body)) < i:
            loops.append((labels[m.group(1)], i))
    return max(loops, key=lambda ab: sum("v_mfma" in line for line in body[ab[0]:ab[1]]))


def test_wave_complete_kernel_k_step_composition(device_asm):
    """modconv_w2dw_kernel: one K step = 48 matrix instructions (4 y-frequencies x 6 x-frequencies x 2 m-tiles) around <= 72 VALU
    instructions (the four window transforms: fp32 VALU and fp32 matrix instructions share the datapath, every extra one is matrix time
    lost), 16 window + 24 weight + 1 style LDS reads, ONE barrier, and no full vmcnt drain except the one in front of that barrier."""
    body = _kernel_body(device_asm["modconv_w2d"], "modconv_w2dw_kernel")
    lo, hi = _main_loop(body)
    ops = [line.split()[0] for line in body[lo:hi + 1] if line.strip() and not line.strip().startswith((".", ";")) and not line.strip().endswith(":")]
    assert sum(op.startswith("v_mfma") for op in ops) == 48
    valu = sum(op.startswith("v_") and not op.startswith("v_mfma") for op in ops)
    assert valu <= 72, valu
    assert sum(op.startswith("ds_read") for op in ops) == 41
    assert sum(op == "s_barrier" for op in ops) == 1
    drains = [i for i, line in enumerate(body[lo:hi + 1]) if "s_waitcnt" in line and "vmcnt(0)" in line]
    barrier = next(i for i, line in enumerate(body[lo:hi + 1]) if "s_barrier" in line)
    assert drains and all(0 < barrier - d < 12 for d in drains), (drains, barrier)


@pytest.mark.parametrize("name", SOURCES + STREAMING)
def test_wide_buffer_stores_carry_their_own_wait_states(device_asm, name):
    """Round 6 finding (csrc/conv_device.h buffer_store_b128_sgpr_offset; profiles/r06_store_hazard.md): a MUBUF store of more than 64
    bits whose soffset is an SGPR is hazard-free in the compiler's model, which then lets the next instructions overwrite the data
    registers — on the MI355X the stored row carried the NEXT row's last dword in a quarter of the lanes.  Every buffer store of 3 or 4
    dwords in the hot kernels therefore sits in an inline-assembly blob with `s_nop` right behind it (global_store_* has no soffset and
    is covered by the compiler's own rule)."""
    lines = [line.strip() for line in device_asm[name].split("\n")]
    wide = [i for i, line in enumerate(lines) if re.match(r"buffer_store_(dwordx[34]|format_xyzw?)\b", line)]
    for i in wide:
        assert lines[i + 1].startswith("s_nop"), f"{name}.hip: `{lines[i]}` (asm line {i}) is not followed by its wait states"
    if name == "modconv_w2d":
        assert wide, "the 2-D Winograd kernels store their feature rows with buffer_store_dwordx4"


def test_prescaled_instances_drop_the_style_multiplies(device_asm):
    """The style fold (include/maua_hip.h): kernel instances for a map that arrives multiplied by the layer's styles run the K step
    without the style multiplies — 4 of 16 transform instructions per window of the 2-D Winograd kernels (16 of 64 per K step of the
    wave-complete kernel), 9 of 23 VALU per K group of the F(2,2)^2 transposed kernel — and without the style's LDS read."""
    def k_step(source, fragment):
        body = _kernel_body(device_asm[source], fragment)
        lo, hi = _main_loop(body)
        ops = [line.split()[0] for line in body[lo:hi + 1] if line.strip() and not line.strip().startswith((".", ";")) and not line.strip().endswith(":")]
        return (sum(op.startswith("v_mfma") for op in ops), sum(op.startswith("v_") and not op.startswith("v_mfma") for op in ops),
                sum(op.startswith("ds_read") for op in ops))

    mf0, valu0, lds0 = k_step("modconv_w2d", "modconv_w2dw_kernelILb0")
    mf1, valu1, lds1 = k_step("modconv_w2d", "modconv_w2dw_kernelILb1")
    assert mf0 == mf1 == 48 and valu0 - valu1 >= 16 and lds0 - lds1 == 1, (valu0, valu1, lds0, lds1)
    mf0, valu0, lds0 = k_step("modconv_w2d", "modconv_w2d_kernelILi4ELi2ELi2ELb0")
    mf1, valu1, lds1 = k_step("modconv_w2d", "modconv_w2d_kernelILi4ELi2ELi2ELb1")
    assert mf0 == mf1 and valu0 - valu1 >= 8 and lds0 - lds1 == 1, (valu0, valu1, lds0, lds1)  # two windows per wave and K step
    mf0, valu0, lds0 = k_step("modconv_up2d", "modconv_up2d_kernelILi8ELi0ELb0")
    mf1, valu1, lds1 = k_step("modconv_up2d", "modconv_up2d_kernelILi8ELi0ELb1")
    # two K groups per step; the 18 scalar multiplies were packed by the compiler (v_pk_mul_f32): 39 -> 30 VALU per 100 matrix instructions
    assert mf0 == mf1 == 100 and valu0 - valu1 >= 8 and valu1 <= 32 and lds0 - lds1 == 2, (valu0, valu1, lds0, lds1)
