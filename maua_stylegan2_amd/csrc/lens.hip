// Lens effects on the generator's fp32 image (render.py lens_frames; audioreactive/lens.py builds the per-frame rows and taps): bloom, sharpen
// / soften and vignette, in front of the grade and of every quantiser.  Three entries, one launch each (include/maua_hip.h states the
// arithmetic):
//   maua_lens_extract_f32  [B,3,H,W] -> [B,3,ceil(H/d),ceil(W/d)]: the soft-knee highlight of every pixel, averaged over d x d blocks
//   maua_lens_blur_f32     [B,P,H,W] -> [B,P,H,W]: a separable symmetric FIR of radius <= 64 with replicated edges, the half-kernel a
//                          per-frame row (the bloom's Gaussian on the reduced map, the sharpen's on the image)
//   maua_lens_apply_f32    y = x + sharpen (x - soft) + 2 bloom_rgb up(bloom), then the vignette; in place is legal
//
// Blur: one workgroup of 256 lanes computes a 64 x 64 output tile.  Its input rows (the tile's rows and `radius` above and below, row
// indices clamped: replicated edges cost nothing extra) pass through LDS in chunks of 16 rows of 64 + 2 * R4 columns (R4 = radius rounded
// up to 4, column indices clamped while staging; row stride odd, so the 4 rows x 16 column groups of a wave's horizontal pass hit 64
// different banks).  The horizontal pass gives every lane 4 neighbouring outputs of one row: per tap it reads ONE new value either side and
// shifts its two windows in registers (2 LDS reads + 1 tap broadcast per 4 multiply-adds), and writes the intermediate [rows + 2 R][64]
// to LDS with one 16-byte store.  The vertical pass gives a lane one column and 4 neighbouring rows with the same sliding windows: a wave
// reads 64 consecutive floats of one intermediate row per access (conflict free) and stores 64 consecutive floats.  The frame is
// blockIdx.z, so the taps' address is uniform: they are read once per workgroup into LDS.  LDS is dynamic, (68 + 16 (65 + 2 R4) +
// 64 (min(64, h) up to 4 + 2 R)) floats: 17.5 KiB at radius 0, 32 KiB at 18, 60.3 KiB at 64 (<= 64 KiB: two workgroups a CU at worst,
// four at the bloom's usual radii); maua_lens_blur_plan reports it.  No second launch: at radius 64 the horizontal pass runs over 3x the
// tile's rows, which is what a scratch plane would save.  The accumulation order is the lanes' (centre, then k = 1 .. R, pairs summed
// first) and multiply-adds may be fused: the header leaves both open.  Vector instance: w % 4 == 0 and src 16-byte aligned: the halo is
// staged with 16-byte loads (a group of 4 columns is then wholly inside or wholly outside the row).  Stores are one float per lane.
// Not free, and not measured on its own: the vector staging writes a group's four floats to LDS as four scalar stores at a lane stride of 4
// floats (the odd row stride rules out a 16-byte store), a 4-way bank conflict per store; it is paid once per staged value, against 2 R + 1
// reads of it, so it weighs most at the sharpen's small radii.
//
// Extract and apply stream like grade.hip: the frame is blockIdx.y, its row of 16 floats is read with scalar loads, a lane takes 4
// consecutive pixels of a row (16-byte accesses when w % 4 == 0 and the pointers allow, else one pixel at a time through the same code
// with scalar accesses).  In extract a lane owns whole output cells: a span of max(4, d) columns and d rows.
#include "common.h"

namespace {
constexpr int GRID_CAP = 1024;  // workgroups per frame (x) of the streaming kernels
constexpr int TW = 64, TH = 64, CH = 16, RMAX = 64, TAP_PAD = 68;
constexpr int64_t MAX_TILES = 0xffffff;  // x 256 lanes < 2^32

enum { LR_THRESHOLD = 0, LR_KNEE = 1, LR_BLOOM = 2, LR_SHARPEN = 5, LR_VIGNETTE = 6, LR_INNER = 7, LR_OUTER = 8, LR_ROW = 16 };

__host__ __device__ inline int round4(int r) { return (r + 3) & ~3; }
inline int blur_mid_rows(int h, int radius) { return round4(h < TH ? h : TH) + 2 * radius; }
inline int blur_lds_bytes(int h, int radius) { return (TAP_PAD + CH * ((TW + 2 * round4(radius)) | 1) + blur_mid_rows(h, radius) * TW) * 4; }

// one tap further out: the windows move one element apart, a[j] += t * (l[j] + r[j])
__device__ __forceinline__ void slide(float (&a)[4], float (&l)[4], float (&r)[4], float t, float left, float right) {
    l[3] = l[2], l[2] = l[1], l[1] = l[0], l[0] = left;
    r[0] = r[1], r[1] = r[2], r[2] = r[3], r[3] = right;
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] += t * (l[j] + r[j]);
}

template <bool VEC>
__global__ __launch_bounds__(256) void lens_blur_kernel(const float* __restrict__ src, float* __restrict__ dst, int planes, int h, int w, int radius,
                                                        const float* __restrict__ taps, int tap_stride, int tiles_x) {
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x;
    const int R = radius, R4 = round4(R), SW = TW + 2 * R4, SWP = SW | 1;
    float* tap_s = lds;
    float* in_s = lds + TAP_PAD;
    float* mid = in_s + CH * SWP;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * TW, y0 = ty * TH;
    const int rows_out = min(TH, h - y0), MR = rows_out + 2 * R;
    const int64_t plane = ((int64_t)blockIdx.z * planes + blockIdx.y) * ((int64_t)h * w);
    const float* in = src + plane;
    if (tid <= R) tap_s[tid] = taps[(int64_t)blockIdx.z * tap_stride + tid];

    for (int r0 = 0; r0 < MR; r0 += CH) {
        const int n_rows = min(CH, MR - r0);
        if constexpr (VEC) {
            const int G = SW >> 2;
            for (int idx = tid; idx < n_rows * G; idx += 256) {
                const int i = idx / G, g = idx - i * G;
                const int gy = min(max(y0 - R + r0 + i, 0), h - 1), gx = x0 - R4 + 4 * g;
                const float* row = in + (int64_t)gy * w;
                float4 v;
                if (gx < 0) v.x = v.y = v.z = v.w = row[0];
                else if (gx >= w) v.x = v.y = v.z = v.w = row[w - 1];
                else v = *reinterpret_cast<const float4*>(row + gx);
                float* s = in_s + i * SWP + 4 * g;
                s[0] = v.x, s[1] = v.y, s[2] = v.z, s[3] = v.w;
            }
        } else {
            for (int idx = tid; idx < n_rows * SW; idx += 256) {
                const int i = idx / SW, j = idx - i * SW;
                const int gy = min(max(y0 - R + r0 + i, 0), h - 1), gx = min(max(x0 - R4 + j, 0), w - 1);
                in_s[i * SWP + j] = in[(int64_t)gy * w + gx];
            }
        }
        __syncthreads();
        {
            const int i = tid >> 4, c = tid & 15;
            if (i < n_rows) {
                const float* s = in_s + i * SWP + R4 + 4 * c;  // s[-R] .. s[3 + R] are columns R4 - R + 4 c .. of the staged row: inside it
                float a[4], l[4], r[4];
                const float t0 = tap_s[0];
#pragma unroll
                for (int j = 0; j < 4; ++j) l[j] = r[j] = s[j], a[j] = t0 * s[j];
#pragma unroll 4
                for (int k = 1; k <= R; ++k) slide(a, l, r, tap_s[k], s[-k], s[3 + k]);
                *reinterpret_cast<float4*>(mid + (r0 + i) * TW + 4 * c) = make_float4(a[0], a[1], a[2], a[3]);
            }
        }
        __syncthreads();
    }

    const int x = tid & 63, gx = x0 + x;
    float* out = dst + plane + (int64_t)y0 * w + gx;
    for (int oy = (tid >> 6) * 4; oy < rows_out; oy += 16) {
        const float* m = mid + (oy + R) * TW + x;  // m[(j - R) * TW] .. m[(j + R) * TW], j < 4: rows oy .. oy + 3 + 2 R < round4(rows_out) + 2 R
        float a[4], u[4], d[4];
        const float t0 = tap_s[0];
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = d[j] = m[j * TW], a[j] = t0 * u[j];
#pragma unroll 4
        for (int k = 1; k <= R; ++k) slide(a, u, d, tap_s[k], m[-k * TW], m[(3 + k) * TW]);
        if (gx < w) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (oy + j < rows_out) out[(int64_t)(oy + j) * w] = a[j];
        }
    }
}

bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

bool pow2_to_8(int d) { return d == 1 || d == 2 || d == 4 || d == 8; }

int blur_check(int batch, int planes, int h, int w, int radius, int tap_stride) {
    if (batch < 0 || planes <= 0 || h <= 0 || w <= 0 || radius < 0 || radius > RMAX || tap_stride < radius + 1) return MAUA_EINVAL;
    return 0;
}
}  // namespace

extern "C" int maua_lens_blur_plan(int h, int w, int radius, const float* src, int* plan) {
    if (blur_check(1, 1, h, w, radius, radius + 1) || !plan) return MAUA_EINVAL;
    plan[0] = (w % 4 == 0 && (((uintptr_t)src) & 15) == 0) ? 1 : 0;
    plan[1] = TW, plan[2] = TH;
    const int64_t tiles = ceil_div64(w, TW) * ceil_div64(h, TH);
    plan[3] = tiles > 0x7fffffffll ? 0x7fffffff : (int)tiles;
    plan[4] = blur_lds_bytes(h, radius);
    plan[5] = 1;
    return 0;
}

extern "C" int maua_lens_blur_f32(const float* src, float* dst, int batch, int planes, int h, int w, int radius, const float* taps,
                                  int tap_stride, void* stream) {
    if (blur_check(batch, planes, h, w, radius, tap_stride)) return MAUA_EINVAL;
    if (batch == 0) return 0;
    if (!src || !dst || !taps) return MAUA_EINVAL;
    const int64_t plane = (int64_t)h * w;
    const int tiles_x = ceil_div(w, TW);
    const int64_t tiles = (int64_t)tiles_x * ceil_div(h, TH);
    // the grid's y and z; the plane's 32-bit offsets; a launch holds fewer than 2^32 lanes in x (a thin plane has few pixels and many tiles)
    if (batch > 65535 || planes > 65535 || plane > 0x7fffff00ll || tiles > MAX_TILES) return MAUA_ENOSYS;
    const size_t bytes = (size_t)batch * planes * plane * 4;
    if (overlap(src, bytes, dst, bytes)) return MAUA_EINVAL;
    const dim3 grid((unsigned)tiles, (unsigned)planes, (unsigned)batch);
    const size_t lds = (size_t)blur_lds_bytes(h, radius);
    hipStream_t st = (hipStream_t)stream;
    if (w % 4 == 0 && (((uintptr_t)src) & 15) == 0)
        hipLaunchKernelGGL((lens_blur_kernel<true>), grid, dim3(256), lds, st, src, dst, planes, h, w, radius, taps, tap_stride, tiles_x);
    else
        hipLaunchKernelGGL((lens_blur_kernel<false>), grid, dim3(256), lds, st, src, dst, planes, h, w, radius, taps, tap_stride, tiles_x);
    MAUA_LAUNCH_CHECK();
    return 0;
}

// ---- extract and apply: every operation rounded on its own (hipcc contracts a * b + c by default)
#pragma clang fp contract(off)

namespace {
__device__ __forceinline__ float clamp01(float a) { return fminf(fmaxf(a, 0.f), 1.f); }

struct Knee {
    float threshold, knee, two_knee, denom;
};

// x (the image's values) -> hl, both [3]
__device__ __forceinline__ void highlight(const Knee& k, const float (&x)[3], float (&hl)[3]) {
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = clamp01(x[c] * 0.5f + 0.5f);
    const float m = fmaxf(fmaxf(v[0], v[1]), v[2]);
    const float over = m - k.threshold;
    float s = fminf(fmaxf(over + k.knee, 0.f), k.two_knee);
    s = (s * s) / k.denom;
    const float q = fmaxf(s, over) / fmaxf(m, 1e-5f);
#pragma unroll
    for (int c = 0; c < 3; ++c) hl[c] = v[c] * q;
}

// An item is a span of SP = max(4, D) columns and D rows: SP / D whole output cells.  VEC: w % 4 == 0 and img 16-byte aligned.
template <int D, bool VEC>
__global__ __launch_bounds__(256) void lens_extract_kernel(const float* __restrict__ img, float* __restrict__ out, int h, int w, int oh, int ow,
                                                           uint32_t items, uint32_t spans, const float* __restrict__ rows, int row_stride) {
    constexpr int SP = D > 4 ? D : 4, CELLS = SP / D;
    const int64_t b = blockIdx.y;
    const float* row = rows + b * row_stride;
    Knee k;
    k.threshold = row[LR_THRESHOLD], k.knee = row[LR_KNEE];
    k.two_knee = 2.f * k.knee, k.denom = 4.f * k.knee + 1e-5f;
    const int64_t plane = (int64_t)h * w, oplane = (int64_t)oh * ow;
    const float* frame = img + b * 3 * plane;
    float* oframe = out + b * 3 * oplane;
    for (uint32_t it = blockIdx.x * 256u + threadIdx.x; it < items; it += gridDim.x * 256u) {
        const int oy = it / spans, ix = it - oy * spans, xs = ix * SP;
        float acc[CELLS][3];
#pragma unroll
        for (int e = 0; e < CELLS; ++e) acc[e][0] = acc[e][1] = acc[e][2] = 0.f;
#pragma unroll
        for (int r = 0; r < D; ++r) {
            const int y = oy * D + r;
            if (y >= h) break;
            const float* p = frame + (int64_t)y * w + xs;
#pragma unroll
            for (int q = 0; q < SP / 4; ++q) {
                const int x = xs + 4 * q;
                float px[4][3];
                if constexpr (VEC) {
                    if (x >= w) break;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float4 v = *reinterpret_cast<const float4*>(p + c * plane + 4 * q);
                        px[0][c] = v.x, px[1][c] = v.y, px[2][c] = v.z, px[3][c] = v.w;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int c = 0; c < 3; ++c) px[j][c] = x + j < w ? p[c * plane + 4 * q + j] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (x + j < w) {
                        float hl[3];
                        highlight(k, px[j], hl);
#pragma unroll
                        for (int c = 0; c < 3; ++c) acc[(4 * q + j) / D][c] = acc[(4 * q + j) / D][c] + hl[c];
                    }
                }
            }
        }
        const int ch = min(D, h - oy * D);
#pragma unroll
        for (int e = 0; e < CELLS; ++e) {
            const int ox = ix * CELLS + e;
            if (ox < ow) {
                const float count = (float)(ch * min(D, w - ox * D));
#pragma unroll
                for (int c = 0; c < 3; ++c) oframe[c * oplane + (int64_t)oy * ow + ox] = acc[e][c] / count;
            }
        }
    }
}

struct LensRow {
    float bloom[3], sharpen, vignette, inner, outer;
    bool identity;
};

__device__ __forceinline__ LensRow load_row(const float* __restrict__ row) {
    LensRow r;
#pragma unroll
    for (int c = 0; c < 3; ++c) r.bloom[c] = row[LR_BLOOM + c];
    r.sharpen = row[LR_SHARPEN], r.vignette = row[LR_VIGNETTE], r.inner = row[LR_INNER], r.outer = row[LR_OUTER];
    r.identity = r.bloom[0] == 0.f && r.bloom[1] == 0.f && r.bloom[2] == 0.f && r.sharpen == 0.f && r.vignette == 0.f;
    return r;
}

// VEC: w % 4 == 0, img, out and soft 16-byte aligned: an item is 4 consecutive pixels of a row.  !VEC: an item is one pixel.  img and out may
// be the same buffer: a lane reads its own pixels before it writes them, and nobody else's.
template <bool VEC>
__global__ __launch_bounds__(256) void lens_apply_kernel(const float* img, float* out, int h, int w, uint32_t items, uint32_t per_row,
                                                         const float* __restrict__ rows, int row_stride, const float* __restrict__ bloom, int bh, int bw,
                                                         int d, const float* soft) {
    constexpr int N = VEC ? 4 : 1;
    const int64_t b = blockIdx.y;
    const LensRow r = load_row(rows + b * row_stride);
    const int64_t plane = (int64_t)h * w, bplane = (int64_t)bh * bw;
    const float* frame = img + b * 3 * plane;
    const float* sframe = soft ? soft + b * 3 * plane : nullptr;
    const float* bframe = bloom ? bloom + b * 3 * bplane : nullptr;
    float* oframe = out + b * 3 * plane;
    const float fd = (float)d, half_w = (float)w * 0.5f, half_h = (float)h * 0.5f;
    for (uint32_t it = blockIdx.x * 256u + threadIdx.x; it < items; it += gridDim.x * 256u) {
        const int py = it / per_row, px0 = (it - py * per_row) * N;
        const int64_t p = (int64_t)py * w + px0;
        float x[N][3], y[N][3];
        if constexpr (VEC) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float4 q = *reinterpret_cast<const float4*>(frame + c * plane + p);
                x[0][c] = q.x, x[1][c] = q.y, x[2][c] = q.z, x[3][c] = q.w;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) x[0][c] = frame[c * plane + p];
        }
#pragma unroll
        for (int k = 0; k < N; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) y[k][c] = x[k][c];
        if (!r.identity) {  // (uniform; an identity frame keeps its bits, NaN payloads included)
            if (sframe) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float s[N];
                    if constexpr (VEC) {
                        const float4 q = *reinterpret_cast<const float4*>(sframe + c * plane + p);
                        s[0] = q.x, s[1] = q.y, s[2] = q.z, s[3] = q.w;
                    } else {
                        s[0] = sframe[c * plane + p];
                    }
#pragma unroll
                    for (int k = 0; k < N; ++k) y[k][c] = y[k][c] + r.sharpen * (x[k][c] - s[k]);
                }
            }
            if (bframe) {
                const float v = fminf(fmaxf(((float)py + 0.5f) / fd - 0.5f, 0.f), (float)(bh - 1));
                const int v0 = (int)v, v1 = min(v0 + 1, bh - 1);
                const float fy = v - (float)v0;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const float u = fminf(fmaxf(((float)(px0 + k) + 0.5f) / fd - 0.5f, 0.f), (float)(bw - 1));
                    const int u0 = (int)u, u1 = min(u0 + 1, bw - 1);
                    const float fx = u - (float)u0;
                    const float w00 = (1.f - fx) * (1.f - fy), w01 = fx * (1.f - fy), w10 = (1.f - fx) * fy, w11 = fx * fy;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float* g = bframe + c * bplane;
                        const float up = ((w00 * g[(int64_t)v0 * bw + u0] + w01 * g[(int64_t)v0 * bw + u1]) + w10 * g[(int64_t)v1 * bw + u0]) +
                                         w11 * g[(int64_t)v1 * bw + u1];
                        y[k][c] = y[k][c] + (2.f * r.bloom[c]) * up;
                    }
                }
            }
            if (r.vignette != 0.f) {  // (uniform)
                const float dy = (((float)py + 0.5f) - half_h) / half_h;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const float dx = (((float)(px0 + k) + 0.5f) - half_w) / half_w;
                    const float rad = sqrtf(dx * dx + dy * dy) * 0.70710678118654752f;
                    const float t = clamp01((rad - r.inner) / (r.outer - r.inner));
                    const float f = 1.f - r.vignette * ((t * t) * (3.f - 2.f * t));
#pragma unroll
                    for (int c = 0; c < 3; ++c) y[k][c] = (y[k][c] + 1.f) * f - 1.f;
                }
            }
        }
        if constexpr (VEC) {
#pragma unroll
            for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(oframe + c * plane + p) = make_float4(y[0][c], y[1][c], y[2][c], y[3][c]);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) oframe[c * plane + p] = y[0][c];
        }
    }
}

dim3 stream_grid(int64_t items, int batch) {
    const int64_t blocks = ceil_div64(items, 256);
    return dim3((unsigned)(blocks < GRID_CAP ? blocks : GRID_CAP), (unsigned)batch);
}

template <int D>
void launch_extract(bool vec, dim3 grid, hipStream_t st, const float* img, float* out, int h, int w, int oh, int ow, uint32_t items, uint32_t spans,
                    const float* rows, int row_stride) {
    if (vec) hipLaunchKernelGGL((lens_extract_kernel<D, true>), grid, dim3(256), 0, st, img, out, h, w, oh, ow, items, spans, rows, row_stride);
    else hipLaunchKernelGGL((lens_extract_kernel<D, false>), grid, dim3(256), 0, st, img, out, h, w, oh, ow, items, spans, rows, row_stride);
}
}  // namespace

extern "C" int maua_lens_extract_f32(const float* img, float* out, int batch, int h, int w, int d, const float* rows, int row_stride,
                                     void* stream) {
    if (h <= 0 || w <= 0 || batch < 0 || !pow2_to_8(d) || row_stride < LR_ROW) return MAUA_EINVAL;
    if (batch == 0) return 0;
    if (!img || !out || !rows) return MAUA_EINVAL;
    const int64_t plane = (int64_t)h * w;
    if (batch > 65535 || plane > 0x7fffff00ll) return MAUA_ENOSYS;  // the grid's y; the 32-bit item index
    const int oh = ceil_div(h, d), ow = ceil_div(w, d);
    if (overlap(img, (size_t)batch * 3 * plane * 4, out, (size_t)batch * 3 * oh * ow * 4)) return MAUA_EINVAL;
    const int sp = d > 4 ? d : 4;
    const int64_t spans = ceil_div(w, sp), items = spans * oh;
    const bool vec = w % 4 == 0 && (((uintptr_t)img) & 15) == 0;
    const dim3 grid = stream_grid(items, batch);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n = (uint32_t)items, s = (uint32_t)spans;
    if (d == 1) launch_extract<1>(vec, grid, st, img, out, h, w, oh, ow, n, s, rows, row_stride);
    else if (d == 2) launch_extract<2>(vec, grid, st, img, out, h, w, oh, ow, n, s, rows, row_stride);
    else if (d == 4) launch_extract<4>(vec, grid, st, img, out, h, w, oh, ow, n, s, rows, row_stride);
    else launch_extract<8>(vec, grid, st, img, out, h, w, oh, ow, n, s, rows, row_stride);
    MAUA_LAUNCH_CHECK();
    return 0;
}

extern "C" int maua_lens_apply_f32(const float* img, float* out, int batch, int h, int w, const float* rows, int row_stride, const float* bloom,
                                   int bh, int bw, int d, const float* soft, void* stream) {
    if (h <= 0 || w <= 0 || batch < 0 || row_stride < LR_ROW) return MAUA_EINVAL;
    if (bloom && (bh <= 0 || bw <= 0 || !pow2_to_8(d))) return MAUA_EINVAL;
    if (batch == 0) return 0;
    if (!img || !out || !rows) return MAUA_EINVAL;
    const int64_t plane = (int64_t)h * w;
    if (batch > 65535 || plane > 0x7fffff00ll || (bloom && (int64_t)bh * bw > 0x7fffff00ll)) return MAUA_ENOSYS;
    const size_t bytes = (size_t)batch * 3 * plane * 4;
    if (out != img && overlap(img, bytes, out, bytes)) return MAUA_EINVAL;  // overlapping, and not the whole image in place
    if (soft && overlap(soft, bytes, out, bytes)) return MAUA_EINVAL;
    if (bloom && overlap(bloom, (size_t)batch * 3 * bh * bw * 4, out, bytes)) return MAUA_EINVAL;
    const bool vec = w % 4 == 0 && ((((uintptr_t)img) | ((uintptr_t)out) | ((uintptr_t)soft)) & 15) == 0;
    const int64_t per_row = vec ? w / 4 : w, items = per_row * h;
    const dim3 grid = stream_grid(items, batch);
    hipStream_t st = (hipStream_t)stream;
    if (!bloom) bh = bw = d = 1;
    if (vec) hipLaunchKernelGGL((lens_apply_kernel<true>), grid, dim3(256), 0, st, img, out, h, w, (uint32_t)items, (uint32_t)per_row, rows, row_stride, bloom, bh, bw, d, soft);
    else hipLaunchKernelGGL((lens_apply_kernel<false>), grid, dim3(256), 0, st, img, out, h, w, (uint32_t)items, (uint32_t)per_row, rows, row_stride, bloom, bh, bw, d, soft);
    MAUA_LAUNCH_CHECK();
    return 0;
}
