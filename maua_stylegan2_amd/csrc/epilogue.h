// Device pieces that several convolution kernels' epilogues share (the tail's operands themselves: TailArgs / RgbArgs in common.h).
// Everything here is __forceinline__ and works on register arrays taken by reference: no pointer to a local array leaves a helper
// (that is how scratch appears, tests/test_isa_checks.py).  The arithmetic order of every expression is part of the contract —
// tests assert bit-equality between the kernels that use these pieces.
#pragma once
#include "common.h"

// ---- split-K slab sum.  THE association of every reducer (reduce_tail_kernel, reduce_blur_tail_kernel, reduce_tail_rgbpart_kernel store
// the same bits for the same slabs): per group of four slabs v += (a0 + a1) + (a2 + a3), then singles.  N elements per thread advance
// together, eight slabs of every element in flight; load(q, sp) = element q of slab sp.
template <int N, typename Load>
__device__ __forceinline__ void slab_sum(float (&v)[N], int splits, Load&& load) {
    int sp = 0;
    for (; sp + 8 <= splits; sp += 8) {
        float a[N][8];
#pragma unroll
        for (int q = 0; q < N; ++q)
#pragma unroll
            for (int k = 0; k < 8; ++k) a[q][k] = load(q, sp + k);
#pragma unroll
        for (int q = 0; q < N; ++q) {
            v[q] += (a[q][0] + a[q][1]) + (a[q][2] + a[q][3]);
            v[q] += (a[q][4] + a[q][5]) + (a[q][6] + a[q][7]);
        }
    }
    for (; sp + 4 <= splits; sp += 4) {
        float a[N][4];
#pragma unroll
        for (int q = 0; q < N; ++q)
#pragma unroll
            for (int k = 0; k < 4; ++k) a[q][k] = load(q, sp + k);
#pragma unroll
        for (int q = 0; q < N; ++q) v[q] += (a[q][0] + a[q][1]) + (a[q][2] + a[q][3]);
    }
    for (; sp < splits; ++sp) {
        float a[N];
#pragma unroll
        for (int q = 0; q < N; ++q) a[q] = load(q, sp);
#pragma unroll
        for (int q = 0; q < N; ++q) v[q] += a[q];
    }
}

// ---- uint8 frames (render.py:40-43): clamp(-1, 1), (x + 1) * 127.5, truncating cast
__device__ __forceinline__ uint32_t rgb8_quant(float v) { return (uint32_t)((fminf(fmaxf(v, -1.f), 1.f) + 1.f) * 127.5f); }
__device__ __forceinline__ uint32_t pack_rgb8(float r, float g, float b) {  // R | G << 8 | B << 16
    uint32_t pix = 0u;
    pix |= rgb8_quant(r) << 0, pix |= rgb8_quant(g) << 8, pix |= rgb8_quant(b) << 16;
    return pix;
}
// four packed pixels = 12 bytes at a 12-byte multiple of a 4-byte aligned frame: three dword stores
__device__ __forceinline__ void store_rgb8x4(uint8_t* dst, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3) {
    uint32_t* fw = reinterpret_cast<uint32_t*>(dst);
    fw[0] = p0 | (p1 << 24);
    fw[1] = (p1 >> 8) | (p2 << 16);
    fw[2] = (p2 >> 16) | (p3 << 8);
}

// ---- 2x FIR-upsampled skip image of the fused ToRGB, for the four pixels (oy, ox .. ox + 3), ox a multiple of 4:
// upfirdn2d(skip, k4, up=2, pad=(2,1)) at (oy, x) has two live source rows / columns, iy0 = floor((oy-1)/2), iy0+1 with taps k4[3]/k4[1]
// for even oy and k4[2]/k4[0] for odd (models/stylegan2.py:34-52, op/upfirdn2d.py:159-200).  All 24 source values of the 4 output pixels
// (2 live rows x 4 live columns x 3 channels) are fetched unconditionally from clamped addresses, in flight together; positions outside
// the skip image are masked through their tap weight wy / wx (per-pixel conditional loads serialise ~48 dependent L2 round trips behind
// each other: measured 0.5 ms of the 1024^2 layer).  Output column x = ox + px reads source columns (x-1)>>1 and +1: px 0 -> k 0,1;
// 1, 2 -> k 1,2; 3 -> k 2,3 of k = (ox>>1) - 1 + {0..3}, with taps k4[.][3], k4[.][1] for even x and k4[.][2], k4[.][0] for odd x.
// The kernels fetch sv [colour][live row][k], wy [live row], wx [k] themselves (their load_skip), where the round trip hides — before their
// last combine pass; as a shared function next to skip_quad_add the loads changed the register allocation of the 64-channel K loop.
template <typename Quad>
__device__ __forceinline__ void skip_quad_add(const float* k4, int oy, const float (&sv)[3][2][4], const float (&wy)[2],
                                              const float (&wx)[4], Quad (&outc)[3]) {  // Quad: the caller's float ext_vector_type(4)
    const int ty_ = (oy & 1) ? 2 : 3;
    float kt[2][4];  // the two live tap rows
#pragma unroll
    for (int qy = 0; qy < 2; ++qy)
#pragma unroll
        for (int t4 = 0; t4 < 4; ++t4) kt[qy][t4] = k4[(ty_ - 2 * qy) * 4 + t4] * wy[qy];
#pragma unroll
    for (int px = 0; px < 4; ++px) {
        const int k0 = (px + 1) >> 1;              // first live source column of this pixel
        const int t0 = (px & 1) ? 2 : 3;           // its tap; the second live column uses tap t0 - 2
#pragma unroll
        for (int qy = 0; qy < 2; ++qy) {
            const float w0 = kt[qy][t0] * wx[k0], w1 = kt[qy][t0 - 2] * wx[k0 + 1];
#pragma unroll
            for (int c = 0; c < 3; ++c) outc[c][px] = fmaf(w0, sv[c][qy][k0], fmaf(w1, sv[c][qy][k0 + 1], outc[c][px]));
        }
    }
}
