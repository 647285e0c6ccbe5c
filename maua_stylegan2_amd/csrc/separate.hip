// Source separation for gfx950: from a factorisation V ~ W.H (csrc/nmf.hip) to per-source masked complex spectra — the device side of
// audioreactive.separate.  The definition of an element, the layouts and the exact-behaviour promises are the comment of
// maua_nmf_separate_f32 in include/maua_hip.h and DESIGN.md 4.18; tests/separate_ref.py restates them in float64.
//
// The launch is bound by memory: an element reads re and im and writes 2 n_out numbers, (2 + 2 n_out) * 4 bytes, against 2 K FMAs.
//   * Lanes run along t: a wave's loads of re / im, its H column and every store are one coalesced 256-byte access.  A workgroup of four
//     waves owns 64 columns and SEP_ROWS rows; wave w takes the rows f_base + w, f_base + w + 4, ...  A lane keeps its H column in
//     registers across those rows; the workgroup's rows of W are staged in LDS once and read back as broadcasts (one address a wave).
//   * The host sorts the components by group (stable: k stays ascending inside a group) and hands over, in the kernel arguments, the
//     order, the group of every position, a bit mask of the positions that end a group and a bit mask of the empty groups.  The kernel
//     loads W and H in that order, so that one fully unrolled walk over the positions computes every P_g as a chain in registers: no
//     dynamically indexed register array, no scratch, no table in device memory (nothing to upload: the call can be captured).
//   * Two walks per element: the first sums D over ALL groups, the second recomputes each q_g (the same instructions, the same bits)
//     and stores the groups of the window.  The second K FMAs are free next to the memory traffic, and nothing per group is kept.
// K is a compile-time tile KP in {4, 8, 16, 32}; positions >= K hold zeros and end no group.  Lanes beyond T and rows beyond F load
// nothing (but the staging, clamped to row F - 1) and store nothing.  No atomics: the result is a function of the arguments alone,
// bit for bit.
#include <math.h>

#include "common.h"

// P * P and the sum over the groups are two roundings each by definition: nothing here may be fused but the explicit fmaf chain.
#pragma clang fp contract(off)

namespace {

constexpr int SEP_WAVES = 4;
constexpr int SEP_ROWS = 64;  // rows of a workgroup: 16 a wave, the H column is loaded once for all of them

struct SepTable {
    uint8_t order[MAUA_NMF_MAX_K];  // position i -> component k, sorted by (group, k); 0 behind K
    uint32_t gid[MAUA_NMF_MAX_K / 4];  // position i -> group[order[i]], byte i % 4 of word i / 4
    uint32_t ends;                  // bit i: position i is the last of its group
    uint32_t empty;                 // bit g: no component names group g
};

template <int KP>
__global__ __launch_bounds__(64 * SEP_WAVES) void separate_kernel(const float* __restrict__ re, const float* __restrict__ im, const float* __restrict__ w,
                                                                  const float* __restrict__ h, SepTable tab, int F, int T, int K, int G, int square,
                                                                  int g0, int n_out, int t_blocks, float* __restrict__ out_re,
                                                                  float* __restrict__ out_im) {
    __shared__ float wt[SEP_ROWS][KP];  // the workgroup's rows of W in the sorted order, zeros behind K
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = (int)(blockIdx.x % (unsigned)t_blocks) * 64 + lane;
    const int f_base = (int)(blockIdx.x / (unsigned)t_blocks) * SEP_ROWS;
    {
        const int f = f_base + lane < F ? f_base + lane : F - 1;  // (a row beyond F is staged from row F - 1 and never used)
        const float* wr = w + (size_t)f * K;
#pragma unroll
        for (int i = 0; i < KP; ++i)
            if (i % SEP_WAVES == wave) wt[lane][i] = i < K ? wr[tab.order[i]] : 0.f;
    }
    __syncthreads();
    if (t >= T) return;  // (no barrier below)

    float hk[KP];
#pragma unroll
    for (int i = 0; i < KP; ++i) hk[i] = i < K ? h[(size_t)tab.order[i] * T + t] : 0.f;
    const float equal = 1.0f / (float)G;
    const int64_t plane = (int64_t)F * T;
    const int f_end = f_base + SEP_ROWS < F ? f_base + SEP_ROWS : F;

    // the next row's re / im are requested before this row's arithmetic and stores: a wave always has a load in flight
    float next_r = 0.f, next_i = 0.f;
    if (f_base + wave < f_end) next_r = re[(f_base + wave) * T + t], next_i = im[(f_base + wave) * T + t];
    for (int f = f_base + wave; f < f_end; f += SEP_WAVES) {
        float wk[KP];
#pragma unroll
        for (int i = 0; i < KP; ++i) wk[i] = wt[f - f_base][i];  // one address for the whole wave: a broadcast read
        const int at = f * T + t;  // < 2^31 (checked by the entry)
        const float xr = next_r, xi = next_i;
        if (f + SEP_WAVES < f_end) next_r = re[at + SEP_WAVES * T], next_i = im[at + SEP_WAVES * T];
        // (opaque per trip: the tests of the group ends and of the window and the stems' offsets g * plane are scalar arithmetic inside
        // the loop, not some 8 K scalars held across it)
        int64_t step = plane;
        uint32_t ends = tab.ends;
        int first = g0;
        asm volatile("" : "+s"(step), "+s"(ends), "+s"(first));
        uint32_t gid[(KP + 3) / 4];
#pragma unroll
        for (int j = 0; j < (KP + 3) / 4; ++j) {
            gid[j] = tab.gid[j];
            asm volatile("" : "+s"(gid[j]));
        }

        float D = 0.f, P = 0.f;
#pragma unroll
        for (int i = 0; i < KP; ++i) {
            P = fmaf(wk[i], hk[i], P);
            if ((ends >> i) & 1u) {
                D += square ? P * P : P;
                P = 0.f;
            }
        }
        const bool positive = D > 0.f;
        P = 0.f;
#pragma unroll
        for (int i = 0; i < KP; ++i) {
            P = fmaf(wk[i], hk[i], P);
            if ((ends >> i) & 1u) {
                const int g = (int)((gid[i / 4] >> (8 * (i % 4))) & 0xffu) - first;
                if (g >= 0 && g < n_out) {
                    const float q = square ? P * P : P;
                    const float m = positive ? q / D : equal;
                    out_re[(int64_t)g * step + at] = m * xr;
                    out_im[(int64_t)g * step + at] = m * xi;
                }
                P = 0.f;
            }
        }
        if ((tab.empty >> g0) & ((n_out < 32 ? 1u << n_out : 0u) - 1u)) {
            const float m = positive ? 0.f / D : equal;  // q_g = 0
            for (int g = 0; g < n_out; ++g)
                if ((tab.empty >> (g0 + g)) & 1u) {
                    out_re[(int64_t)g * step + at] = m * xr;
                    out_im[(int64_t)g * step + at] = m * xi;
                }
        }
    }
}

}  // namespace

extern "C" int maua_nmf_separate_f32(const float* re, const float* im, const float* w, const float* h, const int32_t* group, int F, int T, int K,
                                     int G, int power, int g0, int n_out, float* out_re, float* out_im, void* stream) {
    if (!re || !im || !w || !h || !group || !out_re || !out_im) return MAUA_EINVAL;
    if (F < 1 || T < 1 || K < 1 || K > MAUA_NMF_MAX_K || G < 1 || G > MAUA_SEPARATE_MAX_GROUPS || (int64_t)F * T >= (1LL << 31)) return MAUA_EINVAL;
    if ((power != 1 && power != 2) || g0 < 0 || n_out < 1 || n_out > G || g0 > G - n_out) return MAUA_EINVAL;
    for (int k = 0; k < K; ++k)
        if (group[k] < 0 || group[k] >= G) return MAUA_EINVAL;

    SepTable tab = {};
    int n = 0;
    for (int g = 0; g < G; ++g) {
        const int first = n;
        for (int k = 0; k < K; ++k)
            if (group[k] == g) {
                tab.order[n] = (uint8_t)k;
                tab.gid[n / 4] |= (uint32_t)g << (8 * (n % 4));
                ++n;
            }
        if (n > first)
            tab.ends |= 1u << (n - 1);
        else
            tab.empty |= 1u << g;
    }

    hipStream_t st = (hipStream_t)stream;
    const int t_blocks = ceil_div(T, 64);
    const dim3 grid((unsigned)((int64_t)t_blocks * ceil_div(F, SEP_ROWS))), block(64 * SEP_WAVES);  // < 2^31 / 64 + F + T workgroups, in x
    const int square = power == 2;
    if (K <= 4)
        hipLaunchKernelGGL(separate_kernel<4>, grid, block, 0, st, re, im, w, h, tab, F, T, K, G, square, g0, n_out, t_blocks, out_re, out_im);
    else if (K <= 8)
        hipLaunchKernelGGL(separate_kernel<8>, grid, block, 0, st, re, im, w, h, tab, F, T, K, G, square, g0, n_out, t_blocks, out_re, out_im);
    else if (K <= 16)
        hipLaunchKernelGGL(separate_kernel<16>, grid, block, 0, st, re, im, w, h, tab, F, T, K, G, square, g0, n_out, t_blocks, out_re, out_im);
    else
        hipLaunchKernelGGL(separate_kernel<32>, grid, block, 0, st, re, im, w, h, tab, F, T, K, G, square, g0, n_out, t_blocks, out_re, out_im);
    MAUA_LAUNCH_CHECK();
    return 0;
}
