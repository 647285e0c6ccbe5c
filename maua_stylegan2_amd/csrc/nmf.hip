// Spectrogram factorisation for gfx950: non-negative matrix factorisation under the generalised Kullback-Leibler divergence by
// multiplicative updates (Lee & Seung, NIPS 2000) — the device side of audioreactive.decompose (nmf / decompose / components).  The
// definition of a step, the layouts and the exact-behaviour promises are the comment of maua_nmf_kl_f32 in include/maua_hip.h and
// DESIGN.md 4.17; tests/nmf_ref.py restates them in float64.
//
// V [F, T] is read twice per iteration, W.H and V / (W.H) are never stored: every element of P is one K-long fmaf chain
// p = fmaf(W[f, k], H[k, t], p), k ascending from p = 0, in registers, in BOTH kernels and in the divergence (nmf_p below).
//   * H step, nmf_h_kernel: a workgroup of eight waves owns 64 columns, one column per lane, so a row of V is one coalesced 256-byte
//     load per wave.  The lane keeps its H column and K accumulators in registers; W[f, :] is wave-uniform and arrives by scalar loads.
//     The eight waves take the eight shares of the f range and combine through LDS as (((s0 + s1) + s2) + ...) + s7.  The column sums of
//     W (the denominators) are summed by the whole workgroup before the main loop: thread (part, k) over f = part, part + 512 / KP, ...,
//     the parts then added in ascending order.
//   * W step, nmf_w_kernel: a workgroup owns FR rows (2 up to K = 16, 1 above) and walks all of T, lanes striding over t; the K loads of
//     H[:, t] are shared by the rows of the tile and the row sums of H (the denominators) are accumulated in the same pass.  Partial
//     sums are reduced across the lanes by an xor butterfly (both partners add the same two numbers, so every lane ends with the same
//     bits), then across the four waves through LDS in ascending order.
// K is a compile-time tile KP in {4, 8, 16, 32}; components k >= K are zeros in registers and are never loaded or stored.  Lanes
// beyond T and rows beyond F are masked: they load nothing and store nothing.  No atomics, no workspace, no reduction across
// workgroups: the result is a function of the arguments alone, bit for bit.
#include <math.h>

#include "common.h"

namespace {

constexpr int NMF_H_WAVES = 8;  // waves of an H-step / divergence workgroup: shares of the f range

template <int KP>
__device__ __forceinline__ float nmf_p(const float (&wk)[KP], const float (&hk)[KP], float eps) {
    float p = 0.f;
#pragma unroll
    for (int k = 0; k < KP; ++k) p = fmaf(wk[k], hk[k], p);
    return fmaxf(p, eps);
}

// W[f, 0 .. K) of a wave-uniform row f into registers, zeros behind K.  The row arrives by scalar loads; `in_vgprs` then moves it to
// vector registers (the empty asm pins the register class), where a row of 32 beside the loop's other scalars would leave the scalar file.
template <int KP>
__device__ __forceinline__ void nmf_load_w_row(const float* wr, int K, float (&wk)[KP], bool in_vgprs) {
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        wk[k] = k < K ? wr[k] : 0.f;
        if (in_vgprs) asm volatile("" : "+v"(wk[k]));
    }
}

// H[0 .. K, t] into registers, zeros behind K and for a masked lane.
template <int KP>
__device__ __forceinline__ void nmf_load_h_col(const float* h, int64_t T, int K, int t, bool live, float (&hk)[KP]) {
#pragma unroll
    for (int k = 0; k < KP; ++k) hk[k] = (live && k < K) ? h[(size_t)k * T + t] : 0.f;
}

template <int KP>
__global__ __launch_bounds__(64 * NMF_H_WAVES) void nmf_h_kernel(const float* __restrict__ v, const float* __restrict__ w, float* __restrict__ h, int F, int T,
                                                    int K, float eps) {
    constexpr int NP = 64 * NMF_H_WAVES / KP;
    __shared__ float part[NMF_H_WAVES - 1][KP][64];
    __shared__ float colsum[64 * NMF_H_WAVES];  // [NP][KP]
    __shared__ float den[KP];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = blockIdx.x * 64 + lane;
    const bool live = t < T;

    {
        const int k = tid % KP, pt = tid / KP;
        float s = 0.f;
        if (k < K)
            for (int f = pt; f < F; f += NP) s += w[(size_t)f * K + k];
        colsum[tid] = s;
    }
    __syncthreads();
    if (tid < KP) {
        float s = 0.f;
        for (int pt = 0; pt < NP; ++pt) s += colsum[pt * KP + tid];
        den[tid] = fmaxf(s, eps);
    }

    float hk[KP], acc[KP];
    nmf_load_h_col<KP>(h, T, K, t, live, hk);
#pragma unroll
    for (int k = 0; k < KP; ++k) acc[k] = 0.f;
    const int share = (F + NMF_H_WAVES - 1) / NMF_H_WAVES;
    const int f0 = wave * share < F ? wave * share : F;
    const int f1 = f0 + share < F ? f0 + share : F;
    for (int f = f0; f < f1; ++f) {
        float wk[KP];
        nmf_load_w_row<KP>(w + (size_t)f * K, K, wk, KP > 16);
        const float vv = live ? v[(size_t)f * T + t] : 0.f;
        const float r = vv / nmf_p<KP>(wk, hk, eps);
#pragma unroll
        for (int k = 0; k < KP; ++k) acc[k] = fmaf(wk[k], r, acc[k]);
    }
    if (wave > 0) {
#pragma unroll
        for (int k = 0; k < KP; ++k) part[wave - 1][k][lane] = acc[k];
    }
    __syncthreads();
    if (wave == 0 && live) {
#pragma unroll
        for (int k = 0; k < KP; ++k)
            if (k < K) {
                float num = acc[k];
#pragma unroll
                for (int s = 0; s < NMF_H_WAVES - 1; ++s) num += part[s][k][lane];
                h[(size_t)k * T + t] = (hk[k] * num) / den[k];
            }
    }
}

template <int KP, int FR>
__global__ __launch_bounds__(256) void nmf_w_kernel(const float* __restrict__ v, float* __restrict__ w, const float* __restrict__ h, int F, int T,
                                                    int K, float eps) {
    constexpr int NV = (FR + 1) * KP;  // FR rows of numerators, then the row sums of H
    __shared__ float red[4][NV];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int f_base = blockIdx.x * FR;

    float wk[FR][KP];
#pragma unroll
    for (int r = 0; r < FR; ++r) {
        const int f = f_base + r < F ? f_base + r : F - 1;  // (a row beyond F is computed on row F - 1 and never stored)
        nmf_load_w_row<KP>(w + (size_t)f * K, K, wk[r], true);
    }
    float acc[FR][KP], hs[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        hs[k] = 0.f;
#pragma unroll
        for (int r = 0; r < FR; ++r) acc[r][k] = 0.f;
    }
    for (int t = tid; t < T; t += 256) {
        float hk[KP];
        int64_t stride = T;  // (opaque per trip: the K row offsets k T are scalar arithmetic inside the loop, not 2 K scalars held across it)
        asm volatile("" : "+s"(stride));
        nmf_load_h_col<KP>(h, stride, K, t, true, hk);
#pragma unroll
        for (int k = 0; k < KP; ++k) hs[k] += hk[k];
#pragma unroll
        for (int r = 0; r < FR; ++r) {
            const int f = f_base + r;
            const float vv = f < F ? v[(size_t)f * T + t] : 0.f;
            const float q = vv / nmf_p<KP>(wk[r], hk, eps);
#pragma unroll
            for (int k = 0; k < KP; ++k) acc[r][k] = fmaf(q, hk[k], acc[r][k]);
        }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float x = i < FR * KP ? acc[i / KP][i % KP] : hs[i % KP];  // (wave_sum of wave.h, spelled out: the call reschedules this kernel)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
        if (lane == 0) red[wave][i] = x;
    }
    __syncthreads();
    if (tid < FR * KP) {
        const int r = tid / KP, k = tid % KP, f = f_base + r;
        if (f < F && k < K) {
            const float num = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
            const float sum = ((red[0][FR * KP + k] + red[1][FR * KP + k]) + red[2][FR * KP + k]) + red[3][FR * KP + k];
            float* dst = w + (size_t)f * K + k;
            *dst = (*dst * num) / fmaxf(sum, eps);
        }
    }
}

// d_cols[t] = sum_f (V log(V / P) - V + P) in double, P the fp32 value of the updates; the H kernel's geometry.
template <int KP>
__global__ __launch_bounds__(64 * NMF_H_WAVES) void nmf_div_kernel(const float* __restrict__ v, const float* __restrict__ w, const float* __restrict__ h, int F,
                                                      int T, int K, float eps, double* __restrict__ d_cols) {
    __shared__ double part[NMF_H_WAVES - 1][64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = blockIdx.x * 64 + lane;
    const bool live = t < T;
    float hk[KP];
    nmf_load_h_col<KP>(h, T, K, t, live, hk);
    const int share = (F + NMF_H_WAVES - 1) / NMF_H_WAVES;
    const int f0 = wave * share < F ? wave * share : F;
    const int f1 = f0 + share < F ? f0 + share : F;
    double d = 0.0;
    for (int f = f0; f < f1; ++f) {
        float wk[KP];
        nmf_load_w_row<KP>(w + (size_t)f * K, K, wk, KP > 16);
        const double vv = live ? (double)v[(size_t)f * T + t] : 0.0;
        const double p = (double)nmf_p<KP>(wk, hk, eps);
        d += vv > 0.0 ? vv * log(vv / p) - vv + p : p - vv;  // 0 log 0 = 0 (a NaN compares false and stays a NaN)
    }
    if (wave > 0) part[wave - 1][lane] = d;
    __syncthreads();
    if (wave == 0 && live) {
#pragma unroll
        for (int s = 0; s < NMF_H_WAVES - 1; ++s) d += part[s][lane];
        d_cols[t] = d;
    }
}

inline bool nmf_shape_ok(int F, int T, int K, float eps) {
    return F >= 1 && T >= 1 && K >= 1 && K <= MAUA_NMF_MAX_K && (int64_t)F * T < (1LL << 31) && isfinite(eps) && eps > 0.f;
}

template <int KP>
int nmf_iterate(const float* v, float* w, float* h, int F, int T, int K, int n_iter, int update_w, int update_h, float eps, hipStream_t st) {
    constexpr int FR = KP <= 16 ? 2 : 1;
    for (int it = 0; it < n_iter; ++it) {
        if (update_h) {
            hipLaunchKernelGGL(nmf_h_kernel<KP>, dim3((unsigned)ceil_div(T, 64)), dim3(64 * NMF_H_WAVES), 0, st, v, (const float*)w, h, F, T, K, eps);
            MAUA_LAUNCH_CHECK();
        }
        if (update_w) {
            hipLaunchKernelGGL((nmf_w_kernel<KP, FR>), dim3((unsigned)ceil_div(F, FR)), dim3(256), 0, st, v, w, (const float*)h, F, T, K, eps);
            MAUA_LAUNCH_CHECK();
        }
    }
    return 0;
}

}  // namespace

extern "C" int maua_nmf_kl_f32(const float* v, float* w, float* h, int F, int T, int K, int n_iter, int update_w, int update_h, float eps,
                               void* stream) {
    if (!v || !w || !h || !nmf_shape_ok(F, T, K, eps) || n_iter < 0 || (!update_w && !update_h)) return MAUA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (K <= 4) return nmf_iterate<4>(v, w, h, F, T, K, n_iter, update_w, update_h, eps, st);
    if (K <= 8) return nmf_iterate<8>(v, w, h, F, T, K, n_iter, update_w, update_h, eps, st);
    if (K <= 16) return nmf_iterate<16>(v, w, h, F, T, K, n_iter, update_w, update_h, eps, st);
    return nmf_iterate<32>(v, w, h, F, T, K, n_iter, update_w, update_h, eps, st);
}

extern "C" int maua_nmf_kl_div_f32(const float* v, const float* w, const float* h, int F, int T, int K, float eps, double* d_cols, void* stream) {
    if (!v || !w || !h || !d_cols || !nmf_shape_ok(F, T, K, eps)) return MAUA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)ceil_div(T, 64)), block(64 * NMF_H_WAVES);
    if (K <= 4)
        hipLaunchKernelGGL(nmf_div_kernel<4>, grid, block, 0, st, v, w, h, F, T, K, eps, d_cols);
    else if (K <= 8)
        hipLaunchKernelGGL(nmf_div_kernel<8>, grid, block, 0, st, v, w, h, F, T, K, eps, d_cols);
    else if (K <= 16)
        hipLaunchKernelGGL(nmf_div_kernel<16>, grid, block, 0, st, v, w, h, F, T, K, eps, d_cols);
    else
        hipLaunchKernelGGL(nmf_div_kernel<32>, grid, block, 0, st, v, w, h, F, T, K, eps, d_cols);
    MAUA_LAUNCH_CHECK();
    return 0;
}
