// Non-affine network bends (mirror, kaleidoscope, swirl, ripple, flow-field displacement) on a subset of a feature map's channels —
// maua_bend_remap_f32 of include/maua_hip.h.  A coordinate remap with bilinear sampling: every output pixel names a source coordinate,
// the coordinate is folded into the map (reflect or clamp) and the four taps round it are blended.
//
// The source coordinate depends on (sample, oy, ox) only, never on the channel, so a thread owns ONE pixel of ONE sample and walks a
// chunk of REMAP_CHUNK channels with it: the trigonometry, the fold, the four tap offsets and the two weights are computed once and
// serve every channel of the chunk (per-channel trig would turn a memory-bound gather into a VALU-bound one).  What remains per channel
// is four gathered loads, three fused multiply-adds and one store, coalesced along x; no LDS.  The channel chunk is a grid axis; an
// unselected channel is a wave-uniform copy.  Per-frame parameter rows are read on the device through the frame source like the other
// bends' tables (csrc/bend_ops.hip), so one captured launch serves every replay.
#include "common.h"

namespace {

constexpr int REMAP_CHUNK = 16;  // channels a thread walks with one set of taps
constexpr float TWO_PI = 6.28318530717958648f;

__device__ __forceinline__ int param_row(int rows, const maua_frame_source_t* src, int b) {
    return rows == 1 ? 0 : (src ? src->frame0 + b : b);
}

__device__ __forceinline__ bool is_finite(float v) { return fabsf(v) < __builtin_inff(); }  // (false for a NaN)

// s folded into [0, n - 1]: border 0 reflects about the first and the last element (period 2 (n - 1)), border 1 clamps.  The closing
// clamp also maps what a huge parameter leaves behind (an infinity, a NaN: fmaxf returns its other operand) to a valid coordinate.
__device__ __forceinline__ float fold(float s, int n, int border) {
    const float last = (float)(n - 1);
    if (border == 0 && n > 1) {
        const float period = 2.f * last;
        s = fabsf(s);
        s -= period * floorf(s / period);
        if (s > last) s = period - s;
    }
    return fminf(fmaxf(s, 0.f), last);
}

// Integer taps i0, i1 = min(i0 + 1, n - 1) and the weight of i1 for a coordinate already inside [0, n - 1].
__device__ __forceinline__ void taps(float s, int n, int& i0, int& i1, float& wgt) {
    i0 = min(max((int)s, 0), n - 1);
    i1 = min(i0 + 1, n - 1);
    wgt = s - (float)i0;
}

__device__ __forceinline__ float lerp(float a, float b, float t) { return fmaf(t, b - a, a); }

// One plane [fh, fw] of the flow field at (u, v), bilinear.
__device__ __forceinline__ float field_plane(const float* __restrict__ f, int fw, int i0, int i1, int j0, int j1, float wu, float wv) {
    const float top = lerp(f[(size_t)j0 * fw + i0], f[(size_t)j0 * fw + i1], wu);
    const float bot = lerp(f[(size_t)j1 * fw + i0], f[(size_t)j1 * fw + i1], wu);
    return lerp(top, bot, wv);
}

// grid (ceil(hw / blockDim), ceil(channels / REMAP_CHUNK), batch); a thread owns one pixel of one sample over a chunk of channels.
__global__ __launch_bounds__(256) void bend_remap_kernel(const float* __restrict__ x, float* __restrict__ y, int channels, int h, int w,
                                                         int op, int border, const float* __restrict__ param, int param_rows,
                                                         const float* __restrict__ field, int field_frames, int field_h, int field_w,
                                                         const uint8_t* __restrict__ chan_mask,
                                                         const maua_frame_source_t* __restrict__ src) {
    const int b = blockIdx.z;
    const int c0 = blockIdx.y * REMAP_CHUNK, c1 = min(c0 + REMAP_CHUNK, channels);
    const int hw = h * w;
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= hw) return;
    const float* xp = x + ((size_t)b * channels + c0) * (size_t)hw + pix;
    float* yp = y + ((size_t)b * channels + c0) * (size_t)hw + pix;

    const float* p = param + (size_t)param_row(param_rows, src, b) * MAUA_BEND_REMAP_PARAMS;
    const float p0 = p[0], p1 = p[1], p2 = p[2];
    bool good = is_finite(p0) && is_finite(p1) && (op == 2 || op == 4 || is_finite(p2));
    if (op == 2 || op == 3) good = good && p1 > 0.f;
    if (!good) {  // uniform for the sample: it passes through
        for (int c = c0; c < c1; ++c, xp += hw, yp += hw) *yp = *xp;
        return;
    }

    const int oy = pix / w, ox = pix - oy * w;
    const float fx = (float)ox, fy = (float)oy;
    const float cx = 0.5f * (float)(w - 1), cy = 0.5f * (float)(h - 1);
    const float dx = fx - cx, dy = fy - cy;
    float sx = fx, sy = fy;
    switch (op) {
        case 0: {  // mirror across the line d . n = p2, n = (p0, p1): the side t < 0 shows the other side's reflection
            const float t = dx * p0 + dy * p1 - p2;
            if (t < 0.f) {
                sx = fx - 2.f * t * p0;
                sy = fy - 2.f * t * p1;
            }
            break;
        }
        case 1: {  // kaleidoscope: the angle folded into half a sector
            const float n = fminf(fmaxf(rintf(p0), 1.f), 64.f);
            const float ws = TWO_PI / n;
            const float r = sqrtf(dx * dx + dy * dy);
            float a = atan2f(dy, dx) - p1;
            a -= ws * floorf(a / ws);
            if (a > 0.5f * ws) a = ws - a;
            a += p1 + p2;
            float sn, cs;
            sincosf(a, &sn, &cs);
            sx = cx + r * cs;
            sy = cy + r * sn;
            break;
        }
        case 2: {  // swirl: a rotation that decays with the distance from the centre
            const float r = sqrtf(dx * dx + dy * dy);
            const float phi = p0 * expf(-r / p1);
            float sn, cs;
            sincosf(phi, &sn, &cs);
            sx = cx + (cs * dx - sn * dy);
            sy = cy + (sn * dx + cs * dy);
            break;
        }
        case 3: {  // ripple: a radial displacement that oscillates with the distance from the centre
            const float r = sqrtf(dx * dx + dy * dy);
            if (r > 0.f) {
                const float q = p0 * sinf(TWO_PI * (r / p1 - p2)) / r;
                sx = fx + q * dx;
                sy = fy + q * dy;
            }
            break;
        }
        default: {  // displace along a flow field, blended between two neighbouring frames of a looping bank
            const float ku = w > 1 ? (float)(field_w - 1) / (float)(w - 1) : 0.f;
            const float kv = h > 1 ? (float)(field_h - 1) / (float)(h - 1) : 0.f;
            const float u = fminf(fmaxf(fx * ku, 0.f), (float)(field_w - 1));
            const float v = fminf(fmaxf(fy * kv, 0.f), (float)(field_h - 1));
            int i0, i1, j0, j1;
            float wu, wv;
            taps(u, field_w, i0, i1, wu);
            taps(v, field_h, j0, j1, wv);
            const float t = floorf(p1), ft = p1 - t;
            const float frames = (float)field_frames;
            const float tw = fminf(fmaxf(t - frames * floorf(t / frames), 0.f), frames - 1.f);  // t mod F; the clamp serves a huge t
            const int t0 = min((int)tw, field_frames - 1), t1 = t0 + 1 == field_frames ? 0 : t0 + 1;
            const size_t plane = (size_t)field_h * field_w;
            const float* f0 = field + (size_t)t0 * 2 * plane;
            const float* f1 = field + (size_t)t1 * 2 * plane;
            const float ddx = lerp(field_plane(f0, field_w, i0, i1, j0, j1, wu, wv), field_plane(f1, field_w, i0, i1, j0, j1, wu, wv), ft);
            const float ddy = lerp(field_plane(f0 + plane, field_w, i0, i1, j0, j1, wu, wv),
                                   field_plane(f1 + plane, field_w, i0, i1, j0, j1, wu, wv), ft);
            sx = fx + p0 * ddx;
            sy = fy + p0 * ddy;
            break;
        }
    }

    int x0, x1, y0, y1;
    float wx, wy;
    taps(fold(sx, w, border), w, x0, x1, wx);
    taps(fold(sy, h, border), h, y0, y1, wy);
    const int o00 = y0 * w + x0 - pix, o01 = y0 * w + x1 - pix, o10 = y1 * w + x0 - pix, o11 = y1 * w + x1 - pix;  // relative to xp

#pragma unroll 4
    for (int c = c0; c < c1; ++c, xp += hw, yp += hw) {
        if (chan_mask && !chan_mask[c]) {  // wave-uniform
            *yp = *xp;
            continue;
        }
        const float v00 = xp[o00], v01 = xp[o01], v10 = xp[o10], v11 = xp[o11];
        float v = lerp(lerp(v00, v01, wx), lerp(v10, v11, wx), wy);
        // a convex combination stays inside the range of its taps; rounding may leave it by an ulp, so it is put back (comparisons, not
        // fminf / fmaxf: a NaN among the taps stays a NaN)
        const float lo = fminf(fminf(v00, v01), fminf(v10, v11)), hi = fmaxf(fmaxf(v00, v01), fmaxf(v10, v11));
        v = v < lo ? lo : v;
        v = v > hi ? hi : v;
        *yp = v;
    }
}

}  // namespace

extern "C" int maua_bend_remap_f32(const float* x, float* y, int batch, int channels, int h, int w, int op, int border,
                                   const float* param, int param_rows, const float* field, int field_frames, int field_h, int field_w,
                                   const uint8_t* chan_mask, const maua_frame_source_t* src, void* stream) {
    if (!x || !y || x == y || !param || batch <= 0 || batch > 64 || channels <= 0 || channels > 65535 || h <= 0 || w <= 0)
        return MAUA_EINVAL;
    if ((int64_t)h * w >= (int64_t)1 << 29 || op < 0 || op > 4 || border < 0 || border > 1) return MAUA_EINVAL;
    if (param_rows <= 0 || (!src && param_rows != 1 && param_rows != batch)) return MAUA_EINVAL;
    if (op == 4 && (!field || field_frames <= 0 || field_h <= 0 || field_w <= 0 || (int64_t)field_h * field_w >= (int64_t)1 << 29))
        return MAUA_EINVAL;
    const int hw = h * w;
    const int threads = hw <= 64 ? 64 : 256;
    const dim3 grid((unsigned)ceil_div(hw, threads), (unsigned)ceil_div(channels, REMAP_CHUNK), batch);
    hipLaunchKernelGGL(bend_remap_kernel, grid, dim3(threads), 0, (hipStream_t)stream, x, y, channels, h, w, op, border, param, param_rows,
                       field, field_frames, field_h, field_w, chan_mask, src);
    MAUA_LAUNCH_CHECK();
    return 0;
}
