// Colour grading of the generator's fp32 image (render.py grade_frames; audioreactive/grade.py builds the per-frame rows): ASC CDL slope /
// offset / power, a 3 x 3 matrix with bias and a 3-D LUT, in front of every quantiser.  Two entries, one kernel:
//   maua_grade_f32    [B,3,H,W] fp32 -> [B,3,H,W] fp32 (in place is legal)
//   maua_grade_to_u8  [B,3,H,W] fp32 -> [B,H,W,3] uint8 = maua_frames_to_u8 applied to the first, the graded value kept in registers
//
// Per frame one row of 24 floats (GR_* below), per pixel in fp32, every operation correctly rounded and none contracted (the pragma
// below: hipcc contracts a * b + c by default, and __fmul_rn / __fadd_rn are plain operators to it):
//   v = clamp01(x * 0.5 + 0.5)                      clamp01(a) = fminf(fmaxf(a, 0), 1): a NaN becomes 0
//   t = clamp01(v * slope + offset);  t = power == 1 ? t : powf(t, power)
//   m_c = clamp01(((M[c][0] t_0 + M[c][1] t_1) + M[c][2] t_2) + bias_c)
//   lut != NULL and lut_mix != 0:  l = tetra(lut, m);  m_c = clamp01(m_c + lut_mix * (l_c - m_c))
//   y = m * 2 - 1
// A frame whose row is the identity (slope 1, offset 0, power 1, M = I, bias 0, and no LUT or lut_mix 0) is copied (fp32) or quantised
// as it is (uint8): 2 * fl(0.5 x + 0.5) - 1 is not x in fp32.  The test is uniform over the frame's workgroups.
//
// tetra: p = m * (N - 1), i = min((int)p, N - 2), f = p - i per axis; the comparison chain of tetra_setup orders the fractions
// hi >= mid >= lo with the lattice steps of their axes, the vertices are c000, c000 + step(hi), that + step(mid), c111 and
//   l = ((1 - hi) v0 + (hi - mid) v1) + (mid - lo) v2) + lo v3
// m is clamped before the table is indexed, so every index is inside the table whatever the row and the pixel hold.
//
// The kernel streams: 12 bytes in and 12 or 3 out per pixel.  A lane takes 4 consecutive pixels of the three planes (three 16-byte loads;
// three 16-byte stores or three dwords of packed uint8) when plane % 4 == 0 and the pointers allow; otherwise one pixel per lane with
// scalar accesses.  The frame is blockIdx.y, so the row's address is uniform: it is read once per workgroup with scalar loads and lives in
// SGPRs.  The LUT is gathered from global memory, one 16-byte load per vertex (entries padded to 4 floats), four vertices per pixel: a
// 33^3 table is 575 KB padded and stays in an XCD's 4 MiB L2; 65^3 (4.4 MB) is served by L2 and the Infinity Cache; neither fits the
// 160 KB of LDS, and neighbouring pixels hit neighbouring cells, so the gathers of a wave touch few cache lines.  All 16 vertex loads of a
// lane's 4 pixels are issued before the first is used.
#include "common.h"

#pragma clang fp contract(off)

namespace {
constexpr int GRID_CAP = 1024;  // workgroups per frame (x): 1024^2 pixels are 1024 workgroups of the vector path, one trip

enum { GR_SLOPE = 0, GR_OFFSET = 3, GR_POWER = 6, GR_MATRIX = 9, GR_BIAS = 18, GR_MIX = 21 };

struct Row {
    float slope[3], offset[3], power[3], m[9], bias[3], mix;
    bool identity;
};

// the frame's row; `row` is uniform over the workgroup (scalar loads)
template <bool LUT>
__device__ __forceinline__ Row load_row(const float* __restrict__ row) {
    Row r;
#pragma unroll
    for (int c = 0; c < 3; ++c) r.slope[c] = row[GR_SLOPE + c], r.offset[c] = row[GR_OFFSET + c], r.power[c] = row[GR_POWER + c], r.bias[c] = row[GR_BIAS + c];
#pragma unroll
    for (int k = 0; k < 9; ++k) r.m[k] = row[GR_MATRIX + k];
    r.mix = row[GR_MIX];
    bool id = !LUT || r.mix == 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) id = id && r.slope[c] == 1.f && r.offset[c] == 0.f && r.power[c] == 1.f && r.bias[c] == 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) id = id && r.m[k] == (k % 4 == 0 ? 1.f : 0.f);
    r.identity = id;
    return r;
}

__device__ __forceinline__ float clamp01(float a) { return fminf(fmaxf(a, 0.f), 1.f); }

// x (the image's values) -> m (after the matrix), both [3]
__device__ __forceinline__ void cdl_matrix(const Row& r, const float (&x)[3], float (&m)[3]) {
    float t[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = clamp01(x[c] * 0.5f + 0.5f);
        const float s = clamp01(v * r.slope[c] + r.offset[c]);
        t[c] = r.power[c] == 1.f ? s : powf(s, r.power[c]);  // (uniform branch)
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) m[c] = clamp01(((r.m[3 * c] * t[0] + r.m[3 * c + 1] * t[1]) + r.m[3 * c + 2] * t[2]) + r.bias[c]);
}

struct Tet {
    int idx[4];
    float w[4];
};

// m in [0, 1]^3 -> the four vertices (entry indices, red fastest) and weights of its tetrahedron in an n^3 lattice
__device__ __forceinline__ Tet tetra_setup(const float (&m)[3], int n, float nm1) {
    float f[3];
    int i[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float p = m[c] * nm1;
        i[c] = min((int)p, n - 2);
        f[c] = p - (float)i[c];
    }
    const int sr = 1, sg = n, sb = n * n;
    const float fr = f[0], fg = f[1], fb = f[2];
    float hi, mid, lo;
    int s1, s2;  // lattice step to the second vertex, and from the first to the third
    if (fr >= fg) {
        if (fg >= fb) hi = fr, mid = fg, lo = fb, s1 = sr, s2 = sr + sg;
        else if (fr >= fb) hi = fr, mid = fb, lo = fg, s1 = sr, s2 = sr + sb;
        else hi = fb, mid = fr, lo = fg, s1 = sb, s2 = sb + sr;
    } else {
        if (fb >= fg) hi = fb, mid = fg, lo = fr, s1 = sb, s2 = sb + sg;
        else if (fb >= fr) hi = fg, mid = fb, lo = fr, s1 = sg, s2 = sg + sb;
        else hi = fg, mid = fr, lo = fb, s1 = sg, s2 = sg + sr;
    }
    Tet t;
    t.idx[0] = (i[2] * n + i[1]) * n + i[0];
    t.idx[1] = t.idx[0] + s1;
    t.idx[2] = t.idx[0] + s2;
    t.idx[3] = t.idx[0] + sr + sg + sb;
    t.w[0] = 1.f - hi, t.w[1] = hi - mid, t.w[2] = mid - lo, t.w[3] = lo;
    return t;
}

__device__ __forceinline__ float tetra_sum(const Tet& t, float v0, float v1, float v2, float v3) {
    return ((t.w[0] * v0 + t.w[1] * v1) + t.w[2] * v2) + t.w[3] * v3;
}

// N pixels x[k][c] of a frame that is not the identity, graded in place
template <bool LUT, int N>
__device__ __forceinline__ void grade_pixels(const Row& r, const float4* __restrict__ lut, int lut_n, float (&x)[N][3]) {
    float m[N][3];
#pragma unroll
    for (int k = 0; k < N; ++k) cdl_matrix(r, x[k], m[k]);
    if (LUT && r.mix != 0.f) {  // (uniform)
        const float nm1 = (float)(lut_n - 1);
        Tet t[N];
        float4 v[N][4];
#pragma unroll
        for (int k = 0; k < N; ++k) t[k] = tetra_setup(m[k], lut_n, nm1);
#pragma unroll
        for (int k = 0; k < N; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[k][j] = lut[t[k].idx[j]];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const float l[3] = {tetra_sum(t[k], v[k][0].x, v[k][1].x, v[k][2].x, v[k][3].x), tetra_sum(t[k], v[k][0].y, v[k][1].y, v[k][2].y, v[k][3].y),
                                tetra_sum(t[k], v[k][0].z, v[k][1].z, v[k][2].z, v[k][3].z)};
#pragma unroll
            for (int c = 0; c < 3; ++c) m[k][c] = clamp01(m[k][c] + r.mix * (l[c] - m[k][c]));
        }
    }
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) x[k][c] = m[k][c] * 2.f - 1.f;
}

__device__ __forceinline__ uint32_t quant8(float x) {  // maua_frames_to_u8's (runtime.hip)
    const float v = fminf(fmaxf(x, -1.f), 1.f);
    return (uint32_t)((v + 1.f) * 127.5f);
}

// VEC: plane % 4 == 0, img 16-byte aligned, out 16-byte (fp32) / 4-byte (uint8) aligned: an item is 4 consecutive pixels.  !VEC: an item is
// one pixel.  img and out may be the same buffer (fp32): a lane reads its own pixels before it writes them, and nobody else's.
template <bool U8, bool VEC, bool LUT>
__global__ __launch_bounds__(256) void grade_kernel(const float* img, void* out_, int64_t plane, uint32_t items, const float* __restrict__ rows,
                                                    int row_stride, const float4* __restrict__ lut, int lut_n) {
    constexpr int N = VEC ? 4 : 1;
    const int64_t b = blockIdx.y;
    const Row r = load_row<LUT>(rows + b * row_stride);
    const float* frame = img + b * 3 * plane;
    for (uint32_t it = blockIdx.x * 256u + threadIdx.x; it < items; it += gridDim.x * 256u) {
        const int64_t p = (int64_t)it * N;
        float x[N][3];
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
        if (!r.identity) grade_pixels<LUT, N>(r, lut, lut_n, x);  // (uniform; an identity frame keeps its bits, NaN payloads included)
        if constexpr (U8) {
            uint8_t* o = static_cast<uint8_t*>(out_) + (b * plane + p) * 3;
            if constexpr (VEC) {
                uint32_t q[12];
#pragma unroll
                for (int k = 0; k < 12; ++k) q[k] = quant8(x[k / 3][k % 3]);
                uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
                for (int d = 0; d < 3; ++d) o32[d] = q[4 * d] | (q[4 * d + 1] << 8) | (q[4 * d + 2] << 16) | (q[4 * d + 3] << 24);
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c] = (uint8_t)quant8(x[0][c]);
            }
        } else {
            float* o = static_cast<float*>(out_) + b * 3 * plane + p;
            if constexpr (VEC) {
#pragma unroll
                for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(o + c * plane) = make_float4(x[0][c], x[1][c], x[2][c], x[3][c]);
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c * plane] = x[0][c];
            }
        }
    }
}

template <bool U8, bool VEC>
void launch(dim3 grid, hipStream_t st, const float* img, void* out, int64_t plane, uint32_t items, const float* rows, int row_stride,
            const float* lut, int lut_n) {
    const float4* table = reinterpret_cast<const float4*>(lut);
    if (lut) hipLaunchKernelGGL((grade_kernel<U8, VEC, true>), grid, dim3(256), 0, st, img, out, plane, items, rows, row_stride, table, lut_n);
    else hipLaunchKernelGGL((grade_kernel<U8, VEC, false>), grid, dim3(256), 0, st, img, out, plane, items, rows, row_stride, table, lut_n);
}

template <bool U8>
int grade(const float* img, void* out, int batch, int h, int w, const float* rows, int row_stride, const float* lut, int lut_n, void* stream) {
    if (h <= 0 || w <= 0 || batch < 0 || row_stride < 24) return MAUA_EINVAL;
    if (lut && (lut_n < 2 || lut_n > 65 || (((uintptr_t)lut) & 15))) return MAUA_EINVAL;
    if (batch == 0) return 0;
    if (!img || !out || !rows) return MAUA_EINVAL;
    const int64_t plane = (int64_t)h * w;
    if (batch > 65535 || plane > 0x7fffff00ll) return MAUA_ENOSYS;  // the grid's y; the 32-bit item index
    const uintptr_t a0 = (uintptr_t)img, a1 = a0 + (uintptr_t)batch * 3 * plane * 4;
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)batch * 3 * plane * (U8 ? 1 : 4);
    if (o0 < a1 && a0 < o1 && (U8 || o0 != a0)) return MAUA_EINVAL;  // overlapping, and not the whole image in place
    if (batch > 65535 || plane > 0x7fffff00ll) return MAUA_ENOSYS;   // the grid's y; the 32-bit item index
    const bool vec = plane % 4 == 0 && (a0 & 15) == 0 && (o0 & (U8 ? 3 : 15)) == 0;
    const int64_t items = vec ? plane / 4 : plane;
    const int64_t blocks = ceil_div64(items, 256);
    const dim3 grid((unsigned)(blocks < GRID_CAP ? blocks : GRID_CAP), (unsigned)batch);
    hipStream_t st = (hipStream_t)stream;
    if (vec) launch<U8, true>(grid, st, img, out, plane, (uint32_t)items, rows, row_stride, lut, lut_n);
    else launch<U8, false>(grid, st, img, out, plane, (uint32_t)items, rows, row_stride, lut, lut_n);
    MAUA_LAUNCH_CHECK();
    return 0;
}
}  // namespace

extern "C" int maua_grade_f32(const float* img, float* out, int batch, int h, int w, const float* rows, int row_stride, const float* lut,
                              int lut_n, void* stream) {
    return grade<false>(img, out, batch, h, w, rows, row_stride, lut, lut_n, stream);
}

extern "C" int maua_grade_to_u8(const float* img, uint8_t* out, int batch, int h, int w, const float* rows, int row_stride, const float* lut,
                                int lut_n, void* stream) {
    return grade<true>(img, out, batch, h, w, rows, row_stride, lut, lut_n, stream);
}
