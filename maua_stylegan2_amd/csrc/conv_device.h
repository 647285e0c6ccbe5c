// Device primitives that the convolution kernels share (modconv*.hip, upfirdn2d.hip): vector types, compile-time loops, single-instruction
// LDS reads with explicit waits, raw buffer descriptors and the LDS-DMA load.  Like epilogue.h everything is __forceinline__ and works on
// values and references: no pointer to a local array leaves a helper (that is how scratch appears, tests/test_isa_checks.py).
#pragma once
#include "common.h"

#include <type_traits>

#if defined(__HIP_DEVICE_COMPILE__)
#define MAUA_DEVICE_PASS 1
#endif

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef f32x4 f32x4u __attribute__((aligned(4)));  // 4-byte aligned forms for loads / stores at odd columns
typedef f32x2 f32x2u __attribute__((aligned(4)));

template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// LDS reads of the main loops are issued as single `ds_read_b64` instructions through inline assembly: left to itself the
// compiler pairs neighbouring 8-byte reads into ds_read2_b64 / ds_read2st64_b64, which are serviced in 16-lane groups on a
// 32-bank modulus at half the bytes per clock (MI355X_MICROARCH.md, LDS table) — measured 30 % of the LDS-active cycles of the
// 2-D Winograd kernel as bank conflicts for a layout that is conflict-free under ds_read_b64's rule (32-lane groups, 64 banks).  The
// compiler does not count inline-assembly LDS operations, so the waits are explicit as well; a wait "produces" the values it
// guards (tied operands), which keeps their consumers behind it.
template <int OFF>
__device__ __forceinline__ f32x2 lds_read64(unsigned addr) {
    f32x2 v;
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}
__device__ __forceinline__ float lds_read32(unsigned addr) {
    float v;
    asm volatile("ds_read_b32 %0, %1" : "=v"(v) : "v"(addr));
    return v;
}
template <int N>
__device__ __forceinline__ void lds_wait(f32x2& a) {
    asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a) : "n"(N));
}
template <int N>
__device__ __forceinline__ void lds_wait(f32x2& a, f32x2& b) {
    asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N));
}

// ---- raw buffer descriptors (stride 0, DATA_FORMAT = 32) and the offset that lies beyond every one of them: a raw buffer load from
// kOutOfRange returns 0 and a store to it is dropped, which is how the kernels get their zero padding without exec masks.
// `bytes`: the range that is checked; 2^31 - 1 unless the kernel must not touch memory behind its operand (the launchers keep every real
// offset below it: fits_raw_descriptor, common.h).
constexpr unsigned kOutOfRange = 0x80000000u;
#ifdef MAUA_DEVICE_PASS
typedef __amdgpu_buffer_rsrc_t buffer_rsrc_t;
#else
struct [[maybe_unused]] buffer_rsrc_t {};  // (the host pass only parses the kernels; their descriptors may go unused there)
#endif
template <typename T>
__device__ __forceinline__ buffer_rsrc_t raw_buffer(const T* base, int bytes = 0x7fffffff) {
#ifdef MAUA_DEVICE_PASS
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(base), 0, bytes, 0x00020000);
#else
    (void)base, (void)bytes;
    return {};
#endif
}

// 16 bytes per lane from rsrc[voffset + soffset] straight into LDS (MUBUF `buffer_load ... lds`): lane l's bytes land at dst + 16 l, dst
// and soffset are wave-uniform.  (The builtin wants its size as a literal: the one 4-byte user, modconv.hip, spells it out.)
__device__ __forceinline__ void lds_dma16(buffer_rsrc_t rsrc, void* dst, int voffset, int soffset) {
#ifdef MAUA_DEVICE_PASS
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)dst, 16, voffset, soffset, 0, 0);
#else
    (void)rsrc, (void)dst, (void)voffset, (void)soffset;
#endif
}

// 16-byte MUBUF store whose channel offset is a SCALAR (soffset SGPR), followed by its own wait states.  Round 6 finding, measured on the
// MI355X (tools/dbg/w2dw_val.py: every thread's value correct in its register, the fourth dword of the stored row not): the compiler
// treats a buffer store of more than 64 bits as hazard-free when its soffset is a register (LLVM GCNHazardRecognizer::createsVALUHazard:
// "this hazard only exists if the instruction is not using a register in the soffset field") and lets the very next instructions
// overwrite the data registers — it had emitted `buffer_store_dwordx4 v[190:193], .., s67 offen` followed at once by four v_mov into
// v190..v193 for the next row, and on gfx950 the row-0 store then carried the NEXT row's last dword in a quarter of its lanes.  With an
// immediate soffset it keeps 2 wait states (and those builds were right).  The store therefore goes out as one inline-assembly blob
// with `s_nop` behind it: no instruction the compiler schedules can reach the data registers earlier than 4 wait states after the issue.
__device__ __forceinline__ void buffer_store_b128_sgpr_offset(u32x4 data, const float* base, unsigned voffset_bytes, unsigned soffset_bytes) {
#ifdef MAUA_DEVICE_PASS
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    const uint64_t a = (uint64_t)(uintptr_t)base;
    // the descriptor of raw_buffer(base) from scalars: the inline assembly wants it in SGPRs
    i32x4 rsrc = i32x4{__builtin_amdgcn_readfirstlane((int)(unsigned)a), __builtin_amdgcn_readfirstlane((int)(unsigned)(a >> 32) & 0xffff), 0x7fffffff, 0x00020000};
    asm volatile("buffer_store_dwordx4 %0, %1, %2, %3 offen\n\ts_nop 3" ::"v"(data), "v"(voffset_bytes), "s"(rsrc), "s"(soffset_bytes) : "memory");
#else
    (void)data, (void)base, (void)voffset_bytes, (void)soffset_bytes;
#endif
}
