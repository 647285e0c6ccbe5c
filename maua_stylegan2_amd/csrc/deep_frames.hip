// Deep frame delivery (render.py DEEP_PIX_FMTS): the generator's fp32 image leaves the device at 16 bits per sample (packed RGB, ffmpeg's
// rgb48le) or as planar 10-bit YUV (yuv420p10le / yuv422p10le / yuv444p10le) instead of through the 8-bit quantiser.  Four entries:
//   maua_frames_to_u16         [B,3,H,W] fp32 -> [B,H,W,3] uint16, the 16-bit master
//   maua_crop_resize_u16       the wide-output crop + bilinear up-scale on the master (16-bit sibling of maua_crop_resize_u8)
//   maua_rgb48_to_yuv_p10      the master -> planar 10-bit YUV
//   maua_frames_to_yuv_p10_f32 fp32 planes -> planar 10-bit YUV in one launch (= the third applied to the first, master in registers)
//
// Quantiser: the 8-bit one (runtime.hip) with the scale changed, q = (uint16)((fminf(fmaxf(x, -1), 1) + 1) * 32767.5), a truncating cast;
// the add and the multiply are two correctly rounded fp32 operations (__fadd_rn / __fmul_rn: never contracted).  NaN -> 0 (fmaxf returns
// its other operand), -inf -> 0, +inf -> 65535; 32767.5 and 65535 are exact in fp32, so 1 -> 65535.
//
// Matrix: ITU-R BT.709, limited range, 10 bits, in integers: the exact rational value of the real definition with Kr = 0.2126,
// Kg = 0.7152, Kb = 0.0722 (times 10000: 2126, 7152, 722), 876 = 940 - 64 luma codes, 896 = 960 - 64 chroma codes, 9278 = 10000 - 722 and
// 7874 = 10000 - 2126 (the 2 (1 - Kb) and 2 (1 - Kr) of the colour-difference scaling), rounded half up.  For a block of n pixels (1 for
// luma; for chroma 2 x 2 for 4:2:0, 2 x 1 for 4:2:2, 1 for 4:4:4 — the box sum, i.e. centre siting, as yuv420.hip) whose 16-bit codes sum
// to Sr, Sg, Sb:
//   L  = 2126 Sr + 7152 Sg + 722 Sb
//   Y  = 64 + (2 * 876 * L + D) / (2 D)                              D  = 10000 * 65535          (n = 1)
//   Cb = (2 * (512 Eb + 896 * (10000 Sb - L)) + Eb) / (2 Eb)         Eb = 2 * 9278 * 65535 * n
//   Cr = (2 * (512 Er + 896 * (10000 Sr - L)) + Er) / (2 Er)         Er = 2 * 7874 * 65535 * n
// Every numerator is positive and below 2^44: `/` is floor on unsigned 64-bit, by a compile-time constant (no division instruction).
//
// All four kernels are memory-bound and elementwise.  The two conversions give a thread a strip: ROWS rows (2 for 4:2:0, else 1) of
//   8 pixels of the packed master  = three 16-byte loads per row, one 16-byte luma store per row, 8- or 16-byte chroma stores;
//   4 pixels of the fp32 planes    = one 16-byte load per plane and row (six for 4:2:0), 8-byte luma stores, 4- or 8-byte chroma stores.
// The fp32 kernel moves 12 bytes in for 3 (4:2:0) to 6 (4:4:4) out per pixel, so its strip is chosen for the reads: with 4 pixels every
// load instruction of a wave covers one contiguous KiB of a plane row at the full 16 bytes per lane, and the 8-byte luma stores of a wave
// are one contiguous 512-byte run (8 to 16 bytes per lane is where global accesses stop gaining).  An 8-pixel strip would widen the stores
// to 16 bytes but leave every load instruction with a 32-byte lane stride, twice the instructions for the dominant traffic, and double the
// registers held across the loads.  Consecutive lanes own consecutive strips of a row (pair), so a wave touches one contiguous run of every
// row and plane.  Grid: y = frame, x = at most GRID_CAP workgroups walking the frame's strips with a grid-stride loop.
#include "common.h"

namespace {
constexpr int GRID_CAP = 1024;  // workgroups per frame (x); 8 frames of 1024^2 are 4096 workgroups of the fp32 4:2:0 kernel, one trip

__device__ __forceinline__ uint32_t quant16(float x) {
    const float v = fminf(fmaxf(x, -1.f), 1.f);
    return (uint32_t)__fmul_rn(__fadd_rn(v, 1.f), 32767.5f);  // truncating cast, as numpy astype(uint16) on [0, 65535]
}

constexpr uint64_t kD = 10000ull * 65535ull;
__device__ __forceinline__ uint32_t luma10(uint32_t r, uint32_t g, uint32_t b) {
    const uint64_t l = 2126u * r + 7152u * g + 722u * b;  // <= 10000 * 65535: fits 32 bits
    return 64u + (uint32_t)((2ull * 876ull * l + kD) / (2ull * kD));
}
// n: pixels of the block the sums were taken over
template <int n>
__device__ __forceinline__ void chroma10(uint32_t sr, uint32_t sg, uint32_t sb, uint32_t& cb, uint32_t& cr) {
    constexpr int64_t eb = 2ll * 9278ll * 65535ll * n, er = 2ll * 7874ll * 65535ll * n;
    const int64_t l = 2126ll * sr + 7152ll * sg + 722ll * sb;
    cb = (uint32_t)((uint64_t)(2ll * (512ll * eb + 896ll * (10000ll * sb - l)) + eb) / (uint64_t)(2ll * eb));
    cr = (uint32_t)((uint64_t)(2ll * (512ll * er + 896ll * (10000ll * sr - l)) + er) / (uint64_t)(2ll * er));
}

// geometry of a planar layout: rows and columns of luma per chroma sample
template <int SUB>
struct Sub {
    static constexpr int ROWS = SUB == 420 ? 2 : 1;
    static constexpr int CW = SUB == 444 ? 1 : 2;
};

// K (2, 4 or 8) 16-bit samples as one 4-, 8- or 16-byte store / sample by sample, the first `count` only
template <int K>
__device__ __forceinline__ void store_samples_vec(uint16_t* p, const uint32_t (&v)[K]) {
    static_assert(K == 2 || K == 4 || K == 8, "4-, 8- or 16-byte stores");
    if constexpr (K == 2) {
        *reinterpret_cast<uint32_t*>(p) = v[0] | (v[1] << 16);
    } else if constexpr (K == 4) {
        *reinterpret_cast<uint2*>(p) = make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
    } else {
        *reinterpret_cast<uint4*>(p) = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
    }
}
template <int K>
__device__ __forceinline__ void store_samples_scalar(uint16_t* p, const uint32_t (&v)[K], int count) {
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (k < count) p[k] = (uint16_t)v[k];
}

// The 16-bit codes c[row][pixel][colour] of a strip of N pixels -> its luma and chroma samples, stored at the strip's place in the frame.
// VEC: whole strips and aligned planes; !VEC: the first `npx` pixels of the strip only (npx a multiple of CW), sample by sample.
template <int SUB, int N, bool VEC>
__device__ __forceinline__ void convert_store_strip(const uint32_t (&c)[Sub<SUB>::ROWS][N][3], uint16_t* __restrict__ frame, int h, int w,
                                                    int rg, int x0, int npx) {
    constexpr int ROWS = Sub<SUB>::ROWS, CW = Sub<SUB>::CW, NC = N / CW;
    const int64_t plane = (int64_t)h * w;
    const int cw = w / CW;
    const int64_t cplane = (int64_t)(h / ROWS) * cw;
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        uint32_t y[N];
#pragma unroll
        for (int p = 0; p < N; ++p) y[p] = luma10(c[i][p][0], c[i][p][1], c[i][p][2]);
        uint16_t* dst = frame + (int64_t)(rg * ROWS + i) * w + x0;
        if constexpr (VEC) store_samples_vec<N>(dst, y);
        else store_samples_scalar<N>(dst, y, npx);
    }
    uint32_t cb[NC], cr[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        uint32_t sr = 0, sg = 0, sb = 0;
#pragma unroll
        for (int i = 0; i < ROWS; ++i)
#pragma unroll
            for (int p = j * CW; p < (j + 1) * CW; ++p) sr += c[i][p][0], sg += c[i][p][1], sb += c[i][p][2];
        chroma10<ROWS * CW>(sr, sg, sb, cb[j], cr[j]);
    }
    uint16_t* u = frame + plane + (int64_t)rg * cw + x0 / CW;
    uint16_t* v = u + cplane;
    if constexpr (VEC) {
        store_samples_vec<NC>(u, cb);
        store_samples_vec<NC>(v, cr);
    } else {
        store_samples_scalar<NC>(u, cb, npx / CW);
        store_samples_scalar<NC>(v, cr, npx / CW);
    }
}

// ---------------------------------------------------------------------------------------------------------------- (a) fp32 -> 16-bit master
// Each thread converts 4 consecutive pixels of one row: three 16-byte loads (one per colour plane) and three 8-byte stores (24 bytes).
__global__ __launch_bounds__(256) void frames_to_u16_kernel(const float* __restrict__ img, uint16_t* __restrict__ out, int64_t quads_per_frame,
                                                            int64_t plane, int64_t total) {
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int64_t b = q / quads_per_frame;
        const int64_t p = (q - b * quads_per_frame) * 4;
        const float* base = img + b * 3 * plane + p;
        const float4 r = *reinterpret_cast<const float4*>(base);
        const float4 g = *reinterpret_cast<const float4*>(base + plane);
        const float4 bl = *reinterpret_cast<const float4*>(base + 2 * plane);
        uint2* o = reinterpret_cast<uint2*>(out + (b * plane + p) * 3);
        o[0] = make_uint2(quant16(r.x) | (quant16(g.x) << 16), quant16(bl.x) | (quant16(r.y) << 16));
        o[1] = make_uint2(quant16(g.y) | (quant16(bl.y) << 16), quant16(r.z) | (quant16(g.z) << 16));
        o[2] = make_uint2(quant16(bl.z) | (quant16(r.w) << 16), quant16(g.w) | (quant16(bl.w) << 16));
    }
}

__global__ __launch_bounds__(256) void frames_to_u16_scalar_kernel(const float* __restrict__ img, uint16_t* __restrict__ out, int64_t plane,
                                                                   int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t c = i % 3;
        const int64_t p = (i / 3) % plane;
        const int64_t b = i / (3 * plane);
        out[i] = (uint16_t)quant16(img[(b * 3 + c) * plane + p]);
    }
}

// ---------------------------------------------------------------------------------------------------------------- (b) crop + resize, 16 bits
// maua_crop_resize_u8's arithmetic (runtime.hip: the 2-tap triangle at (dst + 0.5) * in / out - 0.5 evaluated in integers, taps clamped to
// the crop, coefficients rounded to 22 fractional bits) on 16-bit samples: 22 + 16 bits leave int32, so the products are 64 bits wide.  The
// horizontal pass is rounded half up to 16 bits, then the vertical pass runs on that; clamped to 0 .. 65535.  One thread per output pixel.
constexpr int RESIZE_BITS = 22;
struct ResizeTap {
    int a, b;    // source indices of the two taps (clamped)
    int k0, k1;  // fixed-point weights
};
__device__ __forceinline__ ResizeTap resize_tap(int o, int n_in, int n_out) {
    const long long num = (2ll * o + 1) * n_in - n_out, den = 2ll * n_out;
    long long i0 = num / den;
    if (num < 0 && i0 * den != num) --i0;  // floor division
    const double f = (double)(num - i0 * den) / (double)den;
    ResizeTap t;
    t.k1 = (int)floor(0.5 + f * (double)(1 << RESIZE_BITS));
    t.k0 = (int)floor(0.5 + (1.0 - f) * (double)(1 << RESIZE_BITS));
    t.a = min(max((int)i0, 0), n_in - 1);
    t.b = min(max((int)i0 + 1, 0), n_in - 1);
    return t;
}
__device__ __forceinline__ int64_t resize_mix(int k0, int64_t a, int k1, int64_t b) {
    constexpr int64_t HALF = 1ll << (RESIZE_BITS - 1);
    const int64_t v = (k0 * a + k1 * b + HALF) >> RESIZE_BITS;
    return v < 0 ? 0 : (v > 65535 ? 65535 : v);
}
__global__ __launch_bounds__(256) void crop_resize_u16_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out, int in_h, int in_w,
                                                              int x0, int y0, int cw, int ch, int out_w, int out_h, int64_t total) {
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int ox = (int)(idx % out_w);
        const int oy = (int)((idx / out_w) % out_h);
        const int64_t b = idx / ((int64_t)out_w * out_h);
        const ResizeTap tx = resize_tap(ox, cw, out_w), ty = resize_tap(oy, ch, out_h);
        const uint16_t* ra = in + ((b * in_h + y0 + ty.a) * in_w + x0) * 3;
        const uint16_t* rb = in + ((b * in_h + y0 + ty.b) * in_w + x0) * 3;
        uint16_t* o = out + idx * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int64_t ha = resize_mix(tx.k0, ra[tx.a * 3 + c], tx.k1, ra[tx.b * 3 + c]);
            const int64_t hb = resize_mix(tx.k0, rb[tx.a * 3 + c], tx.k1, rb[tx.b * 3 + c]);
            o[c] = (uint16_t)resize_mix(ty.k0, ha, ty.k1, hb);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- (c) master -> planar 10-bit
// VEC: w % 8 == 0 and 16-byte aligned buffers -> every strip is whole, every row segment starts on a multiple of 48 bytes and every store
// is naturally aligned (planes and frames start at multiples of 16 / 8 bytes: h is even for 4:2:0).  !VEC: any legal w, any alignment.
template <int SUB, bool VEC>
__global__ __launch_bounds__(256) void rgb48_to_yuv_p10_kernel(const uint16_t* __restrict__ rgb, uint16_t* __restrict__ out, int h, int w,
                                                               uint32_t strips_per_row, uint32_t strips_per_frame, int64_t frame_out) {
    constexpr int ROWS = Sub<SUB>::ROWS, N = 8;
    const int64_t b = blockIdx.y;
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < strips_per_frame; idx += gridDim.x * 256u) {
        const int rg = (int)(idx / strips_per_row);  // row group: a row pair for 4:2:0, a row otherwise
        const int x0 = (int)(idx - (uint32_t)rg * strips_per_row) * N;
        const int npx = VEC ? N : min(N, w - x0);
        uint32_t c[ROWS][N][3];
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const uint16_t* row = rgb + ((b * h + rg * ROWS + i) * w + x0) * 3;
            if constexpr (VEC) {
                uint32_t d[12];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const uint4 q = reinterpret_cast<const uint4*>(row)[k];
                    d[4 * k] = q.x, d[4 * k + 1] = q.y, d[4 * k + 2] = q.z, d[4 * k + 3] = q.w;
                }
#pragma unroll
                for (int k = 0; k < 3 * N; ++k) c[i][k / 3][k % 3] = (k & 1) ? d[k >> 1] >> 16 : d[k >> 1] & 0xffffu;
            } else {
#pragma unroll
                for (int k = 0; k < 3 * N; ++k) c[i][k / 3][k % 3] = k / 3 < npx ? row[k] : 0u;
            }
        }
        convert_store_strip<SUB, N, VEC>(c, out + b * frame_out, h, w, rg, x0, npx);
    }
}

// ---------------------------------------------------------------------------------------------------------------- (d) fp32 planes -> planar 10-bit
// VEC: w % 4 == 0, 16-byte aligned image, 8-byte aligned output -> float4 loads, naturally aligned 8- / 4-byte stores.  !VEC: the rest.
template <int SUB, bool VEC>
__global__ __launch_bounds__(256) void frames_to_yuv_p10_kernel(const float* __restrict__ img, uint16_t* __restrict__ out, int h, int w,
                                                                uint32_t strips_per_row, uint32_t strips_per_frame, int64_t frame_out) {
    constexpr int ROWS = Sub<SUB>::ROWS, N = 4;
    const int64_t b = blockIdx.y;
    const int64_t plane = (int64_t)h * w;
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < strips_per_frame; idx += gridDim.x * 256u) {
        const int rg = (int)(idx / strips_per_row);
        const int x0 = (int)(idx - (uint32_t)rg * strips_per_row) * N;
        const int npx = VEC ? N : min(N, w - x0);
        uint32_t c[ROWS][N][3];
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const float* row = img + b * 3 * plane + (int64_t)(rg * ROWS + i) * w + x0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if constexpr (VEC) {
                    const float4 q = *reinterpret_cast<const float4*>(row + k * plane);
                    c[i][0][k] = quant16(q.x), c[i][1][k] = quant16(q.y), c[i][2][k] = quant16(q.z), c[i][3][k] = quant16(q.w);
                } else {
#pragma unroll
                    for (int p = 0; p < N; ++p) c[i][p][k] = p < npx ? quant16(row[k * plane + p]) : 0u;
                }
            }
        }
        convert_store_strip<SUB, N, VEC>(c, out + b * frame_out, h, w, rg, x0, npx);
    }
}

// the argument checks the two planar entries share; 1: nothing to do (batch == 0)
int planar_args(const void* in, const void* out, int batch, int h, int w, int subsampling) {
    if (subsampling != 420 && subsampling != 422 && subsampling != 444) return MAUA_EINVAL;
    if (h <= 0 || w <= 0 || batch < 0) return MAUA_EINVAL;
    if ((subsampling != 444 && (w & 1)) || (subsampling == 420 && (h & 1))) return MAUA_EINVAL;
    if (batch == 0) return 1;
    if (!in || !out) return MAUA_EINVAL;
    return 0;
}

// grid and strip counts of a planar launch with strips of n pixels; MAUA_ENOSYS past the 32-bit strip index or the grid's y
template <int SUB>
int planar_grid(int batch, int h, int w, int n, dim3* grid, uint32_t* strips_per_row, uint32_t* strips_per_frame, int64_t* frame_out) {
    const int spr = ceil_div(w, n);
    const int64_t spf = (int64_t)(h / Sub<SUB>::ROWS) * spr;
    if (spf > 0x7fffff00ll || batch > 65535) return MAUA_ENOSYS;
    const int64_t blocks = ceil_div64(spf, 256);
    *grid = dim3((unsigned)(blocks < GRID_CAP ? blocks : GRID_CAP), (unsigned)batch);
    *strips_per_row = (uint32_t)spr;
    *strips_per_frame = (uint32_t)spf;
    *frame_out = (int64_t)h * w + 2 * (int64_t)(h / Sub<SUB>::ROWS) * (w / Sub<SUB>::CW);
    return 0;
}

template <int SUB>
int launch_rgb48(const uint16_t* rgb, uint16_t* out, int batch, int h, int w, hipStream_t st) {
    dim3 grid;
    uint32_t spr, spf;
    int64_t frame_out;
    if (int rc = planar_grid<SUB>(batch, h, w, 8, &grid, &spr, &spf, &frame_out)) return rc;
    if (w % 8 == 0 && ((((uintptr_t)rgb) | ((uintptr_t)out)) & 15) == 0) {
        hipLaunchKernelGGL((rgb48_to_yuv_p10_kernel<SUB, true>), grid, dim3(256), 0, st, rgb, out, h, w, spr, spf, frame_out);
    } else {
        hipLaunchKernelGGL((rgb48_to_yuv_p10_kernel<SUB, false>), grid, dim3(256), 0, st, rgb, out, h, w, spr, spf, frame_out);
    }
    MAUA_LAUNCH_CHECK();
    return 0;
}

template <int SUB>
int launch_f32(const float* img, uint16_t* out, int batch, int h, int w, hipStream_t st) {
    dim3 grid;
    uint32_t spr, spf;
    int64_t frame_out;
    if (int rc = planar_grid<SUB>(batch, h, w, 4, &grid, &spr, &spf, &frame_out)) return rc;
    if (w % 4 == 0 && (((uintptr_t)img) & 15) == 0 && (((uintptr_t)out) & 7) == 0) {
        hipLaunchKernelGGL((frames_to_yuv_p10_kernel<SUB, true>), grid, dim3(256), 0, st, img, out, h, w, spr, spf, frame_out);
    } else {
        hipLaunchKernelGGL((frames_to_yuv_p10_kernel<SUB, false>), grid, dim3(256), 0, st, img, out, h, w, spr, spf, frame_out);
    }
    MAUA_LAUNCH_CHECK();
    return 0;
}
}  // namespace

extern "C" int maua_frames_to_u16(const float* img, uint16_t* out, int batch, int h, int w, void* stream) {
    if (!img || !out || batch <= 0 || h <= 0 || w <= 0) return MAUA_EINVAL;
    const int64_t plane = (int64_t)h * w;
    hipStream_t st = (hipStream_t)stream;
    if (plane % 4 == 0 && (((uintptr_t)img) & 15) == 0 && (((uintptr_t)out) & 7) == 0) {
        const int64_t total = (int64_t)batch * plane / 4;
        hipLaunchKernelGGL(frames_to_u16_kernel, dim3(pack_grid(total)), dim3(256), 0, st, img, out, plane / 4, plane, total);
    } else {
        const int64_t total = (int64_t)batch * plane * 3;
        hipLaunchKernelGGL(frames_to_u16_scalar_kernel, dim3(pack_grid(total)), dim3(256), 0, st, img, out, plane, total);
    }
    MAUA_LAUNCH_CHECK();
    return 0;
}

extern "C" int maua_crop_resize_u16(const uint16_t* in, uint16_t* out, int batch, int in_h, int in_w, int x0, int y0, int crop_w, int crop_h,
                                    int out_w, int out_h, void* stream) {
    if (!in || !out || batch <= 0 || in_h <= 0 || in_w <= 0 || crop_w <= 0 || crop_h <= 0 || out_w <= 0 || out_h <= 0) return MAUA_EINVAL;
    if (x0 < 0 || y0 < 0 || x0 + crop_w > in_w || y0 + crop_h > in_h) return MAUA_EINVAL;
    if (out_w < crop_w || out_h < crop_h) return MAUA_ENOSYS;  // a down-scale widens the filter's support: not the 2-tap form
    const int64_t total = (int64_t)batch * out_w * out_h;
    const int64_t blocks = ceil_div64(total, 256);
    hipLaunchKernelGGL(crop_resize_u16_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, (hipStream_t)stream, in, out,
                       in_h, in_w, x0, y0, crop_w, crop_h, out_w, out_h, total);
    MAUA_LAUNCH_CHECK();
    return 0;
}

extern "C" int maua_rgb48_to_yuv_p10(const uint16_t* rgb, uint16_t* out, int batch, int h, int w, int subsampling, void* stream) {
    if (int rc = planar_args(rgb, out, batch, h, w, subsampling)) return rc < 0 ? rc : 0;
    hipStream_t st = (hipStream_t)stream;
    if (subsampling == 420) return launch_rgb48<420>(rgb, out, batch, h, w, st);
    if (subsampling == 422) return launch_rgb48<422>(rgb, out, batch, h, w, st);
    return launch_rgb48<444>(rgb, out, batch, h, w, st);
}

extern "C" int maua_frames_to_yuv_p10_f32(const float* img, uint16_t* out, int batch, int h, int w, int subsampling, void* stream) {
    if (int rc = planar_args(img, out, batch, h, w, subsampling)) return rc < 0 ? rc : 0;
    hipStream_t st = (hipStream_t)stream;
    if (subsampling == 420) return launch_f32<420>(img, out, batch, h, w, st);
    if (subsampling == 422) return launch_f32<422>(img, out, batch, h, w, st);
    return launch_f32<444>(img, out, batch, h, w, st);
}
