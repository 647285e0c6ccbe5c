// Device functions of the counter-based noise definition (include/maua_hip.h, "counter-based noise"): Philox4x32-10 (Salmon et al., SC'11),
// the 24-bit open-interval uniform and Box-Muller.  Shared by csrc/noise.hip (maua_randn_frames_f32) and csrc/noise_synth.hip (the NULL-bank
// term of maua_noise_synth_f32), so that both produce the same bits for the same (seed, frame, slot, element).
#pragma once
#include "common.h"

namespace maua_philox {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

typedef __attribute__((address_space(1))) float global_float;
typedef float vec4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) vec4f global_vec4f;

struct U4 {
    uint32_t x, y, z, w;
};

__device__ __forceinline__ U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(PHILOX_M0, c.x), lo0 = PHILOX_M0 * c.x;
        const uint32_t hi1 = __umulhi(PHILOX_M1, c.z), lo1 = PHILOX_M1 * c.z;
        c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    return c;
}

// u = ((x >> 9) + 0.5) * 2^-23: 24 significant bits, exact in fp32, inside (0, 1)
__device__ __forceinline__ float unit_open(uint32_t x) { return ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f; }

// (r cos 2 pi u1, r sin 2 pi u1), r = sqrt(-2 ln u0).  sincospif takes the angle in half turns: 2 u1 is exact, no rounded 2 pi u1.
__device__ __forceinline__ void box_muller(uint32_t x0, uint32_t x1, float& a, float& b) {
    const float r = sqrtf(-2.0f * logf(unit_open(x0)));
    float sn, cs;
    sincospif(2.0f * unit_open(x1), &sn, &cs);
    a = r * cs;
    b = r * sn;
}

// elements 4 i .. 4 i + 3 of the map of (key, absolute frame, slot)
__device__ __forceinline__ float4 randn_quad(uint32_t i, uint32_t frame, uint32_t slot, uint32_t key0, uint32_t key1) {
    const U4 x = philox4x32_10(U4{i, frame, slot, 0u}, key0, key1);
    float4 z;
    box_muller(x.x, x.y, z.x, z.y);
    box_muller(x.z, x.w, z.z, z.w);
    return z;
}

}  // namespace maua_philox
