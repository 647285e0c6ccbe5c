// Point and morphological network bends (Broad, Leymarie, Grierson 2020: ablate, invert, scalar multiply, binary threshold, erode,
// dilate) on a subset of a feature map's channels — maua_bend_point_f32 / maua_bend_morph_f32 of include/maua_hip.h.  Both move
// one read and one write of HBM per element (the point kernel at the device's copy rate, the morphological one bound by its row pass:
// profiles/bend_ops.md), 16 bytes per lane where the planes allow it (w, resp. h * w, a multiple
// of 4 and 16-byte aligned pointers; element by element otherwise).  Per-frame parameters are read on the device through the frame
// source like the warp's inverse maps (csrc/signal.hip), so one captured launch serves every replay.
//
// maua_bend_pad_f32: the padding bend (torch.nn.functional.pad in its four modes, plus a static noise plane) that turns the 4 x 4 constant
// into the 4 x 8 one of a 2:1 render.  A pure gather: one thread per 4 consecutive output elements, source indices computed per element.
#include "common.h"

namespace {

__device__ __forceinline__ int param_row(int rows, const maua_frame_source_t* src, int b) {
    return rows == 1 ? 0 : (src ? src->frame0 + b : b);
}

__device__ __forceinline__ float point_op(int op, float v, float p) {
    switch (op) {
        case 0: return 0.f;
        case 1: return 1.f - v;
        case 2: return v * p;
        default: return v > p ? 1.f : 0.f;
    }
}

// grid (ceil(hw / (4 blockDim)), channels, batch); a thread owns 4 consecutive elements of one plane.
template <bool VEC>
__global__ __launch_bounds__(256) void bend_point_kernel(const float* x, float* y /* may be x */, int channels, int64_t hw,
                                                         int op, const float* __restrict__ param, int param_rows,
                                                         const uint8_t* __restrict__ chan_mask,
                                                         const maua_frame_source_t* __restrict__ src) {
    const int b = blockIdx.z, c = blockIdx.y;
    const bool selected = !chan_mask || chan_mask[c];
    if (!selected && x == y) return;  // in place: an unselected plane is already where it belongs
    const int64_t e = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (e >= hw) return;
    const float p = param ? param[param_row(param_rows, src, b)] : 0.f;
    const size_t at = ((size_t)b * channels + c) * (size_t)hw + (size_t)e;
    if (VEC) {
        float4 v = *reinterpret_cast<const float4*>(x + at);
        if (selected) v = make_float4(point_op(op, v.x, p), point_op(op, v.y, p), point_op(op, v.z, p), point_op(op, v.w, p));
        *reinterpret_cast<float4*>(y + at) = v;
    } else {
        const int n = hw - e < 4 ? (int)(hw - e) : 4;
        for (int i = 0; i < n; ++i) {
            const float v = x[at + i];
            y[at + i] = selected ? point_op(op, v, p) : v;
        }
    }
}

// Erode / dilate.  Erosion is computed as -dilate(-x) (what -max_pool2d(-x) does), so the tile holds the running MAXIMUM either way:
// window positions outside the map hold -inf, and a NaN wins every comparison it takes part in (max_pool2d's rule).
constexpr int MORPH_TH = 32, MORPH_TW = 64, MORPH_HALO = MAUA_BEND_MAX_RADIUS;
constexpr int MORPH_ROWS = MORPH_TH + 2 * MORPH_HALO;   // 64 tile rows
constexpr int MORPH_IN_STRIDE = 128;                    // floats per input tile row: 16 + 64 + 16 used; a multiple of 64 dwords keeps the
                                                        // 16-lane groups of ds_read_b128 on distinct banks (16 lanes = one tile row)
static_assert(MORPH_HALO % 4 == 0 && MORPH_TW + 2 * MORPH_HALO <= MORPH_IN_STRIDE, "tile layout");

__device__ __forceinline__ float nan_max(float acc, float v) { return (v > acc || v != v) ? v : acc; }

__device__ __forceinline__ float4 nan_max4(float4 a, float4 v) {
    return make_float4(nan_max(a.x, v.x), nan_max(a.y, v.y), nan_max(a.z, v.z), nan_max(a.w, v.w));
}

// grid (tiles_x * tiles_y, channels, batch), 256 threads; a workgroup owns a 32 x 64 output tile of one plane:
//   1. the tile and a halo of r rows / round_up(r, 4) columns go to LDS (sign-flipped for erosion, -inf outside the map);
//   2. maximum along rows: a thread owns 4 consecutive columns of a tile row, one ds_read_b128 per 4 columns of the window;
//   3. maximum along columns of the row maxima, 4 columns per thread again, stored as one 16-byte vector.
template <bool VEC>
__global__ __launch_bounds__(256) void bend_morph_kernel(const float* __restrict__ x, float* __restrict__ y, int channels, int h, int w,
                                                         int tiles_x, int op, const int32_t* __restrict__ radius, int radius_rows,
                                                         const uint8_t* __restrict__ chan_mask,
                                                         const maua_frame_source_t* __restrict__ src) {
    __shared__ float4 tile[MORPH_ROWS * MORPH_IN_STRIDE / 4];  // input, origin (y0 - 16, x0 - 16)
    __shared__ float4 rowmax[MORPH_ROWS * MORPH_TW / 4];       // row maxima, origin (y0 - 16, x0)
    const int b = blockIdx.z, c = blockIdx.y, tid = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * MORPH_TH, x0 = tx * MORPH_TW;
    const int rows_out = min(MORPH_TH, h - y0), cols_out = min(MORPH_TW, w - x0);
    const int f4_out = (cols_out + 3) >> 2;  // 4-column groups of this tile that hold output
    int r = radius[param_row(radius_rows, src, b)];
    r = min(max(r, 0), MAUA_BEND_MAX_RADIUS);
    const bool selected = !chan_mask || chan_mask[c];
    const float* xp = x + ((size_t)b * channels + c) * (size_t)h * w;
    float* yp = y + ((size_t)b * channels + c) * (size_t)h * w;
    const float sgn = op == 0 ? -1.f : 1.f;
    const float lowest = -__builtin_inff();

    // four columns gx .. gx + 3 of map row gy (the row is inside the map; VEC: the group is entirely inside or outside)
    auto load4 = [&](int gy, int gx) -> float4 {
        const int64_t at = (int64_t)gy * w + gx;  // gx may be negative in the element-wise form: every access below is guarded
        if (VEC) return *reinterpret_cast<const float4*>(xp + at);
        float4 v;
        v.x = gx >= 0 && gx < w ? xp[at] : lowest * sgn;
        v.y = gx + 1 >= 0 && gx + 1 < w ? xp[at + 1] : lowest * sgn;
        v.z = gx + 2 >= 0 && gx + 2 < w ? xp[at + 2] : lowest * sgn;
        v.w = gx + 3 >= 0 && gx + 3 < w ? xp[at + 3] : lowest * sgn;
        return v;
    };
    auto store4 = [&](int gy, int gx, float4 v) {
        const int64_t at = (int64_t)gy * w + gx;  // gx >= 0: only output columns are stored
        if (VEC) {
            *reinterpret_cast<float4*>(yp + at) = v;
            return;
        }
        if (gx < w) yp[at] = v.x;
        if (gx + 1 < w) yp[at + 1] = v.y;
        if (gx + 2 < w) yp[at + 2] = v.z;
        if (gx + 3 < w) yp[at + 3] = v.w;
    };

    if (!selected || r == 0) {  // copied through
        for (int i = tid; i < rows_out * (MORPH_TW / 4); i += 256) {
            const int row = i >> 4, f4 = i & 15;
            if (f4 < f4_out) store4(y0 + row, x0 + 4 * f4, load4(y0 + row, x0 + 4 * f4));
        }
        return;
    }

    const int q = (r + 3) >> 2;                 // halo in 4-column groups
    const int in_f4 = f4_out + 2 * q;           // groups per loaded row, from tile column 16 - 4 q
    const int in_rows = rows_out + 2 * r;       // loaded rows, from tile row 16 - r
    for (int i = tid; i < in_rows * in_f4; i += 256) {
        const int lr = i / in_f4, lf = i - lr * in_f4;
        const int trow = MORPH_HALO - r + lr, tf4 = MORPH_HALO / 4 - q + lf;
        const int gy = y0 - MORPH_HALO + trow, gx = x0 - MORPH_HALO + 4 * tf4;
        float4 v = make_float4(lowest, lowest, lowest, lowest);
        if (gy >= 0 && gy < h && gx + 3 >= 0 && gx < w) {
            v = load4(gy, gx);
            v = make_float4(v.x * sgn, v.y * sgn, v.z * sgn, v.w * sgn);
        }
        tile[trow * (MORPH_IN_STRIDE / 4) + tf4] = v;
    }
    __syncthreads();

    for (int i = tid; i < in_rows * (MORPH_TW / 4); i += 256) {
        const int lr = i >> 4, f4 = i & 15;
        if (f4 >= f4_out) continue;
        const int trow = MORPH_HALO - r + lr;
        const float4* in = tile + trow * (MORPH_IN_STRIDE / 4) + MORPH_HALO / 4 + f4;
        float acc[4] = {lowest, lowest, lowest, lowest};
        for (int k = -q; k <= q; ++k) {
            const float4 v4 = in[k];
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int d = 4 * k + e - j;  // column of v[e] relative to output column j
                    if (d >= -r && d <= r) acc[j] = nan_max(acc[j], v[e]);
                }
        }
        rowmax[trow * (MORPH_TW / 4) + f4] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
    __syncthreads();

    for (int i = tid; i < rows_out * (MORPH_TW / 4); i += 256) {
        const int row = i >> 4, f4 = i & 15;
        if (f4 >= f4_out) continue;
        const float4* in = rowmax + (MORPH_HALO + row) * (MORPH_TW / 4) + f4;
        float4 acc = make_float4(lowest, lowest, lowest, lowest);
        for (int dy = -r; dy <= r; ++dy) acc = nan_max4(acc, in[dy * (MORPH_TW / 4)]);
        store4(y0 + row, x0 + 4 * f4, make_float4(acc.x * sgn, acc.y * sgn, acc.z * sgn, acc.w * sgn));
    }
}

bool aligned16(const void* a, const void* b) { return (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

// Source index along an axis of length n for the padded position i (relative to the source: -pad_before .. n - 1 + pad_after), by the
// rules of torch.nn.functional.pad; -1: the constant fill.  The entry guarantees pad < n (reflect) and pad <= n (circular), so one fold
// or one wrap lands inside [0, n).
__device__ __forceinline__ int pad_source(int mode, int i, int n) {
    if (i >= 0 && i < n) return i;
    switch (mode) {
        case 0: return -1;
        case 1: return i < 0 ? 0 : n - 1;
        case 2: return i < 0 ? -i : 2 * (n - 1) - i;
        default: return i < 0 ? i + n : i - n;
    }
}

// grid (ceil(planes * quads / blockDim)); a thread owns 4 consecutive elements (a quad) of one padded plane of oh x ow elements, `quads`
// = ceil(oh ow / 4) of them per plane.  VEC (ow % 4 == 0, y and noise 16-byte aligned): the quad lies in one row and leaves as one 16-byte
// store; otherwise element by element, across row ends.  The noise is added with one fp32 add, nothing else is computed on a value.
template <bool VEC>
__global__ __launch_bounds__(256) void bend_pad_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t planes, int channels,
                                                       int h, int w, int oh, int ow, int pad_l, int pad_t, int mode, float value,
                                                       const float* __restrict__ noise, int noise_channels, int quads) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= planes * quads) return;
    const int64_t plane = q / quads;  // b * channels + c
    const int e = (int)(q - plane * quads) * 4;
    const int ohw = oh * ow;
    const float* xp = x + (size_t)plane * ((size_t)h * w);
    float* yp = y + (size_t)plane * (size_t)ohw;
    const float* np = !noise ? nullptr : noise + (noise_channels == 1 ? (size_t)0 : (size_t)(plane % channels) * (size_t)ohw);
    int i = e / ow, j = e - i * ow;
    const int n = ohw - e < 4 ? ohw - e : 4;  // (VEC: always 4)
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = 0.f;
        if (k < n) {
            const int sy = pad_source(mode, i - pad_t, h), sx = pad_source(mode, j - pad_l, w);
            v[k] = sy < 0 || sx < 0 ? value : xp[(size_t)sy * w + sx];
            if (++j == ow) j = 0, ++i;
        }
    }
    if (VEC) {
        float4 out = make_float4(v[0], v[1], v[2], v[3]);
        if (np) {
            const float4 z = *reinterpret_cast<const float4*>(np + e);
            out = make_float4(out.x + z.x, out.y + z.y, out.z + z.z, out.w + z.w);
        }
        *reinterpret_cast<float4*>(yp + e) = out;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) yp[e + k] = np ? v[k] + np[e + k] : v[k];
    }
}

}  // namespace

extern "C" int maua_bend_point_f32(const float* x, float* y, int batch, int channels, int64_t hw, int op, const float* param,
                                   int param_rows, const uint8_t* chan_mask, const maua_frame_source_t* src, void* stream) {
    if (!x || !y || batch <= 0 || batch > 64 || channels <= 0 || channels > 65535 || hw <= 0 || hw >= (int64_t)1 << 29) return MAUA_EINVAL;
    if (op < 0 || op > 3 || (op >= 2 && !param)) return MAUA_EINVAL;
    if (param && (param_rows <= 0 || (!src && param_rows != 1 && param_rows != batch))) return MAUA_EINVAL;
    const bool vec = hw % 4 == 0 && aligned16(x, y);
    const int64_t quads = (hw + 3) / 4;
    const int threads = quads <= 64 ? 64 : 256;
    const dim3 grid((unsigned)ceil_div64(quads, threads), channels, batch);
    if (vec)
        hipLaunchKernelGGL(bend_point_kernel<true>, grid, dim3(threads), 0, (hipStream_t)stream, x, y, channels, hw, op, param,
                           param_rows, chan_mask, src);
    else
        hipLaunchKernelGGL(bend_point_kernel<false>, grid, dim3(threads), 0, (hipStream_t)stream, x, y, channels, hw, op, param,
                           param_rows, chan_mask, src);
    MAUA_LAUNCH_CHECK();
    return 0;
}

extern "C" int maua_bend_morph_f32(const float* x, float* y, int batch, int channels, int h, int w, int op, const int32_t* radius,
                                   int radius_rows, const uint8_t* chan_mask, const maua_frame_source_t* src, void* stream) {
    if (!x || !y || x == y || !radius || batch <= 0 || batch > 64 || channels <= 0 || channels > 65535 || h <= 0 || w <= 0)
        return MAUA_EINVAL;
    if ((int64_t)h * w >= (int64_t)1 << 29 || op < 0 || op > 1) return MAUA_EINVAL;
    if (radius_rows <= 0 || (!src && radius_rows != 1 && radius_rows != batch)) return MAUA_EINVAL;
    const int tiles_x = ceil_div(w, MORPH_TW), tiles_y = ceil_div(h, MORPH_TH);
    const dim3 grid((unsigned)((int64_t)tiles_x * tiles_y), channels, batch);
    if (w % 4 == 0 && aligned16(x, y))
        hipLaunchKernelGGL(bend_morph_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, y, channels, h, w, tiles_x, op, radius,
                           radius_rows, chan_mask, src);
    else
        hipLaunchKernelGGL(bend_morph_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, y, channels, h, w, tiles_x, op, radius,
                           radius_rows, chan_mask, src);
    MAUA_LAUNCH_CHECK();
    return 0;
}

extern "C" int maua_bend_pad_f32(const float* x, float* y, int batch, int channels, int h, int w, int pad_l, int pad_r, int pad_t, int pad_b,
                                 int mode, float value, const float* noise, int noise_channels, void* stream) {
    if (!x || !y || x == y || batch <= 0 || batch > 64 || channels <= 0 || channels > 65535 || h <= 0 || w <= 0) return MAUA_EINVAL;
    if (pad_l < 0 || pad_r < 0 || pad_t < 0 || pad_b < 0 || mode < 0 || mode > 3) return MAUA_EINVAL;
    if (mode == 2 && (pad_l >= w || pad_r >= w || pad_t >= h || pad_b >= h)) return MAUA_EINVAL;
    if (mode == 3 && (pad_l > w || pad_r > w || pad_t > h || pad_b > h)) return MAUA_EINVAL;
    if (noise && noise_channels != 1 && noise_channels != channels) return MAUA_EINVAL;
    const int64_t oh = (int64_t)h + pad_t + pad_b, ow = (int64_t)w + pad_l + pad_r;
    if ((int64_t)h * w >= (int64_t)1 << 29 || oh >= (int64_t)1 << 29 || ow >= (int64_t)1 << 29 || oh * ow >= (int64_t)1 << 29) return MAUA_EINVAL;
    const int64_t planes = (int64_t)batch * channels;
    const int quads = (int)((oh * ow + 3) / 4);
    const int threads = planes * quads <= 64 ? 64 : 256;
    const int64_t blocks = ceil_div64(planes * quads, threads);
    if (blocks > 0x7fffffff) return MAUA_EINVAL;
    const dim3 grid((unsigned)blocks);
    if (ow % 4 == 0 && aligned16(y, noise))
        hipLaunchKernelGGL(bend_pad_kernel<true>, grid, dim3(threads), 0, (hipStream_t)stream, x, y, planes, channels, h, w, (int)oh, (int)ow,
                           pad_l, pad_t, mode, value, noise, noise_channels, quads);
    else
        hipLaunchKernelGGL(bend_pad_kernel<false>, grid, dim3(threads), 0, (hipStream_t)stream, x, y, planes, channels, h, w, (int)oh, (int)ow,
                           pad_l, pad_t, mode, value, noise, noise_channels, quads);
    MAUA_LAUNCH_CHECK();
    return 0;
}
