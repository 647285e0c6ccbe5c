// Packed RGB frames -> planar YUV 4:2:0 (I420), the pixel format the encoder wants (render.py FrameSink, pix_fmt yuv420p): the last
// per-frame pixel step behind maua_frames_to_u8 / maua_crop_resize_u8, so that a frame leaves the device at 1.5 bytes per pixel.
//
// ITU-R BT.601, limited range, in integers only (every term fits int32, every numerator is positive: `/` is floor):
//   Y  = 16 + (65481 R + 128553 G + 24966 B + 127500) / 255000                                  per pixel
//   Cb = (130560000 + 510000 -  37797 Sr -  74203 Sg + 112000 Sb) / 1020000                      per 2 x 2 block,
//   Cr = (130560000 + 510000 + 112000 Sr -  93786 Sg -  18214 Sb) / 1020000                      Sr, Sg, Sb = sums of its four pixels
// (131070000 below = 130560000 + 510000; the numerators are positive and below 2^31, so the divisions run unsigned)
// = the BT.601 matrix (0.299, 0.587, 0.114; 219 / 224 code values) scaled by 1000, rounded half up.  Chroma is the matrix applied to the
// box average of the 2 x 2 block, i.e. the chroma sample sits in the CENTRE of its four luma samples; the sink tags the stream
// smpte170m / tv range so that a player decodes with this matrix (render.py FrameSink).
//
// Memory-bound: 3 bytes read + 1.5 written per pixel.  A thread owns a strip of 2 rows x 8 pixels = one 24-byte segment of two rows in,
// 8 bytes of two luma rows and 4 bytes of each chroma row out; consecutive lanes own consecutive strips of a row pair, so a wave reads
// and writes one contiguous run of every row and plane it touches.
#include "common.h"

namespace {
constexpr int STRIP = 8;  // pixels per strip row

__device__ __forceinline__ int luma(int r, int g, int b) { return 16 + (int)((uint32_t)(65481 * r + 128553 * g + 24966 * b + 127500) / 255000u); }
__device__ __forceinline__ int chroma_b(int sr, int sg, int sb) { return (int)((uint32_t)(131070000 - 37797 * sr - 74203 * sg + 112000 * sb) / 1020000u); }
__device__ __forceinline__ int chroma_r(int sr, int sg, int sb) { return (int)((uint32_t)(131070000 + 112000 * sr - 93786 * sg - 18214 * sb) / 1020000u); }

// byte k (0 .. 23) of a 24-byte row segment held in three 8-byte words
__device__ __forceinline__ int seg_byte(const uint2 (&d)[3], int k) {
    const uint32_t word = (k & 4) ? d[k >> 3].y : d[k >> 3].x;
    return (int)((word >> ((k & 3) * 8)) & 0xffu);
}

// VEC: w % 8 == 0 and 8-byte aligned buffers -> every strip is whole, every row segment starts on a multiple of 24 bytes and every
// store below is naturally aligned (h is even, so the planes start at multiples of 8 / 4 bytes as well): 8-byte loads and stores.
// !VEC: any even w, any alignment (w * 3 % 4 != 0 leaves the rows off the dword grid, e.g. w = 6, 10): byte accesses, the last strip of
// a row checked against w pixel by pixel.
template <bool VEC>
__global__ __launch_bounds__(256) void rgb_to_yuv420p_kernel(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ out, int h, int w,
                                                             uint32_t strips_per_row, uint32_t strips_per_frame) {
    const int64_t plane = (int64_t)h * w;
    const int64_t frame_out = plane + plane / 2;
    const int half_w = w / 2;
    const int64_t b = blockIdx.y;  // grid: y = frame, x walks the frame's strips (32-bit index arithmetic)
    for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < strips_per_frame; idx += gridDim.x * 256u) {
        const int py = (int)(idx / strips_per_row);  // row pair
        const int x0 = (int)(idx - (uint32_t)py * strips_per_row) * STRIP;
        const uint8_t* row0 = rgb + ((b * h + 2 * py) * w + x0) * 3;
        const uint8_t* row1 = row0 + (int64_t)w * 3;
        uint8_t* y0 = out + b * frame_out + (int64_t)(2 * py) * w + x0;
        uint8_t* y1 = y0 + w;
        uint8_t* u = out + b * frame_out + plane + (int64_t)py * half_w + x0 / 2;
        uint8_t* v = u + plane / 4;
        if constexpr (VEC) {
            uint2 a[3], c[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                a[i] = reinterpret_cast<const uint2*>(row0)[i];
                c[i] = reinterpret_cast<const uint2*>(row1)[i];
            }
            uint32_t ya[2] = {0, 0}, yc[2] = {0, 0}, uu = 0, vv = 0;
#pragma unroll
            for (int j = 0; j < STRIP / 2; ++j) {  // 2 x 2 blocks of the strip
                int sr = 0, sg = 0, sb = 0;
#pragma unroll
                for (int i = 2 * j; i < 2 * j + 2; ++i) {
                    const int r0 = seg_byte(a, 3 * i), g0 = seg_byte(a, 3 * i + 1), b0 = seg_byte(a, 3 * i + 2);
                    const int r1 = seg_byte(c, 3 * i), g1 = seg_byte(c, 3 * i + 1), b1 = seg_byte(c, 3 * i + 2);
                    ya[i >> 2] |= (uint32_t)luma(r0, g0, b0) << ((i & 3) * 8);
                    yc[i >> 2] |= (uint32_t)luma(r1, g1, b1) << ((i & 3) * 8);
                    sr += r0 + r1, sg += g0 + g1, sb += b0 + b1;
                }
                uu |= (uint32_t)chroma_b(sr, sg, sb) << (j * 8);
                vv |= (uint32_t)chroma_r(sr, sg, sb) << (j * 8);
            }
            *reinterpret_cast<uint2*>(y0) = make_uint2(ya[0], ya[1]);
            *reinterpret_cast<uint2*>(y1) = make_uint2(yc[0], yc[1]);
            *reinterpret_cast<uint32_t*>(u) = uu;
            *reinterpret_cast<uint32_t*>(v) = vv;
        } else {
            const int blocks = min(STRIP, w - x0) / 2;  // w is even: whole 2 x 2 blocks only
            for (int j = 0; j < blocks; ++j) {
                int sr = 0, sg = 0, sb = 0;
#pragma unroll
                for (int i = 2 * j; i < 2 * j + 2; ++i) {
                    const int r0 = row0[3 * i], g0 = row0[3 * i + 1], b0 = row0[3 * i + 2];
                    const int r1 = row1[3 * i], g1 = row1[3 * i + 1], b1 = row1[3 * i + 2];
                    y0[i] = (uint8_t)luma(r0, g0, b0);
                    y1[i] = (uint8_t)luma(r1, g1, b1);
                    sr += r0 + r1, sg += g0 + g1, sb += b0 + b1;
                }
                u[j] = (uint8_t)chroma_b(sr, sg, sb);
                v[j] = (uint8_t)chroma_r(sr, sg, sb);
            }
        }
    }
}
}  // namespace

extern "C" int maua_rgb_to_yuv420p_u8(const uint8_t* rgb, uint8_t* out, int batch, int h, int w, void* stream) {
    if (h <= 0 || w <= 0 || (h & 1) || (w & 1) || batch < 0) return MAUA_EINVAL;
    if (batch == 0) return 0;
    if (!rgb || !out) return MAUA_EINVAL;
    const int strips_per_row = ceil_div(w, STRIP);
    const int64_t strips_per_frame = (int64_t)(h / 2) * strips_per_row;
    // (the strip index is 32 bits wide, the frame is the grid's y: a frame of more than 3e10 pixels or 65535 frames a launch are not served)
    if (strips_per_frame > 0x7fffff00ll || batch > 65535) return MAUA_ENOSYS;
    const int64_t blocks = ceil_div64(strips_per_frame, 256);
    const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536), (unsigned)batch);
    const bool vec = w % STRIP == 0 && ((((uintptr_t)rgb) | ((uintptr_t)out)) & 7) == 0;
    if (vec) {
        hipLaunchKernelGGL(rgb_to_yuv420p_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, rgb, out, h, w, (uint32_t)strips_per_row,
                           (uint32_t)strips_per_frame);
    } else {
        hipLaunchKernelGGL(rgb_to_yuv420p_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, rgb, out, h, w, (uint32_t)strips_per_row,
                           (uint32_t)strips_per_frame);
    }
    MAUA_LAUNCH_CHECK();
    return 0;
}
