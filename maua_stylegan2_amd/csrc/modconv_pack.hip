// Weight packs of the generic 3x3 modulated convolution kernel (modconv_kernel.h; the layouts' reasons: the head of modconv.hip):
// tap-major repack for modes 0 / 1, and the pre-transformed packs of the Winograd modes 2, 3 and 4.
#include "modconv_plan.h"

namespace {

// wp[tap][i][o_pad] = w[o][i][tap], wsq[o][i] = sum_tap w^2.
__global__ __launch_bounds__(256) void pack_weight_kernel(const float* __restrict__ w, float* __restrict__ wp,
                                                          float* __restrict__ wsq, int cout, int cout_pad, int cin,
                                                          int ktaps) {
    const int64_t total = (int64_t)cout_pad * cin;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int o = (int)(idx % cout_pad);
        const int i = (int)(idx / cout_pad);
        float ss = 0.f;
        for (int tp = 0; tp < ktaps; ++tp) {
            const float v = (o < cout) ? w[((size_t)o * cin + i) * ktaps + tp] : 0.f;
            if (wp) wp[((size_t)tp * cin + i) * cout_pad + o] = v;
            ss = fmaf(v, v, ss);
        }
        if (wsq && o < cout) wsq[(size_t)o * cin + i] = ss;
    }
}

// Destination column -> source channel of the Winograd weight packs (modes 2 and 3; the column layout: at wino_cout_pad, modconv_plan.h)
__device__ inline int wino_src_channel(int od, int cout) {
    return cout > 32 ? (od & ~63) + ((od & 1) << 5) + ((od & 63) >> 1) : od;
}

// Winograd F(2,3) weight transform along kx, tap-major repack: wq[(ky*4 + xi)][i][o_pad],
//   xi 0: g0   1: (g0+g1+g2)/2   2: (g0-g1+g2)/2   3: g2        (g = W[o][i][ky][0..2])
__global__ __launch_bounds__(256) void pack_weight_wino_kernel(const float* __restrict__ w, float* __restrict__ wq, int cout,
                                                               int cout_pad, int cin) {
    const int64_t total = (int64_t)cout_pad * cin;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int od = (int)(idx % cout_pad);  // destination column
        const int o = wino_src_channel(od, cout);
        const int i = (int)(idx / cout_pad);
        for (int ky = 0; ky < 3; ++ky) {
            float g0 = 0.f, g1 = 0.f, g2 = 0.f;
            if (o < cout) {
                const float* gp = w + (((size_t)o * cin + i) * 3 + ky) * 3;
                g0 = gp[0], g1 = gp[1], g2 = gp[2];
            }
            const float u[4] = {g0, 0.5f * (g0 + g1 + g2), 0.5f * (g0 - g1 + g2), g2};
            for (int xi = 0; xi < 4; ++xi) wq[((size_t)(ky * 4 + xi) * cin + i) * cout_pad + od] = u[xi];
        }
    }
}

// Winograd F(4,3) weight transform along kx (G g, interpolation points 0, +-1, +-2, inf): wq[(ky*6 + xi)][i][o_pad],
//   xi 0: g0/4   1: -(g0+g1+g2)/6   2: -(g0-g1+g2)/6   3: (g0+2g1+4g2)/24   4: (g0-2g1+4g2)/24   5: g2
__global__ __launch_bounds__(256) void pack_weight_wino43_kernel(const float* __restrict__ w, float* __restrict__ wq,
                                                                 int cout, int cout_pad, int cin) {
    const int64_t total = (int64_t)cout_pad * cin;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int od = (int)(idx % cout_pad);  // destination column
        const int o = wino_src_channel(od, cout);
        const int i = (int)(idx / cout_pad);
        for (int ky = 0; ky < 3; ++ky) {
            float g0 = 0.f, g1 = 0.f, g2 = 0.f;
            if (o < cout) {
                const float* gp = w + (((size_t)o * cin + i) * 3 + ky) * 3;
                g0 = gp[0], g1 = gp[1], g2 = gp[2];
            }
            const float u[6] = {g0 * 0.25f,
                                -(g0 + g1 + g2) * (1.f / 6.f),
                                -(g0 - g1 + g2) * (1.f / 6.f),
                                (g0 + 2.f * g1 + 4.f * g2) * (1.f / 24.f),
                                (g0 - 2.f * g1 + 4.f * g2) * (1.f / 24.f),
                                g2};
            // (padded columns hold +0.0, not the -0.0 that the negated sums of zeros would give)
            for (int xi = 0; xi < 6; ++xi) wq[((size_t)(ky * 6 + xi) * cin + i) * cout_pad + od] = o < cout ? u[xi] : 0.f;
        }
    }
}

// Transposed conv, F(2,2) on the even x-phase: wq[(ky*4 + j)][i][o_pad],  j 0: g2   1: g0 + g2   2: g0   3: g1
__global__ __launch_bounds__(256) void pack_weight_upwino_kernel(const float* __restrict__ w, float* __restrict__ wq,
                                                                 int cout, int cout_pad, int cin) {
    const int64_t total = (int64_t)cout_pad * cin;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int o = (int)(idx % cout_pad);
        const int i = (int)(idx / cout_pad);
        for (int ky = 0; ky < 3; ++ky) {
            float g0 = 0.f, g1 = 0.f, g2 = 0.f;
            if (o < cout) {
                const float* gp = w + (((size_t)o * cin + i) * 3 + ky) * 3;
                g0 = gp[0], g1 = gp[1], g2 = gp[2];
            }
            const float u[4] = {g2, g0 + g2, g0, g1};
            for (int j = 0; j < 4; ++j) wq[((size_t)(ky * 4 + j) * cin + i) * cout_pad + o] = u[j];
        }
    }
}

}  // namespace

extern "C" int maua_pack_weight_f32(const float* w, float* wp, float* wsq, int cout, int cin, int ktaps, void* stream) {
    if (!w || cout <= 0 || cin <= 0 || ktaps <= 0) return MAUA_EINVAL;
    const int cout_pad = pad32(cout);
    hipLaunchKernelGGL(pack_weight_kernel, dim3(pack_grid((int64_t)cout_pad * cin)), dim3(256), 0, (hipStream_t)stream, w, wp, wsq, cout,
                       cout_pad, cin, ktaps);
    MAUA_LAUNCH_CHECK();
    return 0;
}

extern "C" int maua_pack_weight_wino_f32(const float* w, float* wq, int cout, int cin, void* stream) {
    if (!w || !wq || cout <= 0 || cin <= 0) return MAUA_EINVAL;
    const int cout_pad = wino_cout_pad(cout);
    hipLaunchKernelGGL(pack_weight_wino_kernel, dim3(pack_grid((int64_t)cout_pad * cin)), dim3(256), 0, (hipStream_t)stream, w, wq, cout, cout_pad, cin);
    MAUA_LAUNCH_CHECK();
    return 0;
}

extern "C" int maua_pack_weight_upwino_f32(const float* w, float* wq, int cout, int cin, void* stream) {
    if (!w || !wq || cout <= 0 || cin <= 0) return MAUA_EINVAL;
    const int cout_pad = pad32(cout);
    hipLaunchKernelGGL(pack_weight_upwino_kernel, dim3(pack_grid((int64_t)cout_pad * cin)), dim3(256), 0, (hipStream_t)stream, w, wq, cout, cout_pad, cin);
    MAUA_LAUNCH_CHECK();
    return 0;
}

extern "C" int maua_pack_weight_wino43_f32(const float* w, float* wq, int cout, int cin, void* stream) {
    if (!w || !wq || cout <= 0 || cin <= 0) return MAUA_EINVAL;
    const int cout_pad = wino_cout_pad(cout);
    hipLaunchKernelGGL(pack_weight_wino43_kernel, dim3(pack_grid((int64_t)cout_pad * cin)), dim3(256), 0, (hipStream_t)stream, w, wq, cout, cout_pad, cin);
    MAUA_LAUNCH_CHECK();
    return 0;
}
