// Frame feedback on the generator's fp32 image (render.py feedback_frames; audioreactive/feedback.py builds the per-frame rows): the
// previous OUTPUT frame is fed back under the new one — warped by an affine map, scaled by gain x tint, combined in unit space — so that
// highlights leave trails.  A recurrence over frames: frame i gathers from frame i - 1 of `out`, frame 0 from the persistent `state`, and
// the last frame leaves the new state behind.  include/maua_hip.h states the arithmetic; tests/feedback_ref.py restates it in numpy.
//
// Two kernels, both streaming like grade.hip and lens.hip's apply (a lane takes 4 consecutive pixels of a row with 16-byte accesses when
// w % 4 == 0 and the pointers allow, else one pixel through the same code; grid-stride over at most GRID_CAP workgroups of 256 lanes —
// 1024^2 pixels are 1024 workgroups of the vector instance, one trip, four waves on each SIMD of 256 CUs; no LDS, nothing indexed at run time
// but kernel arguments):
//   feedback_warp_kernel   ONE frame per launch (the gather needs the whole previous frame finished: launches on one stream are the only
//                          grid-wide barrier that costs nothing to capture).  The source coordinate and the four tap offsets are computed
//                          once per pixel and serve the three channels.  Reads 4 taps x 3 channels (neighbouring lanes' taps share cache
//                          lines: an affine map keeps them close) + cur, writes out — and `state` as well when it is the batch's last
//                          frame (a dual store: no copy launch).
//   feedback_still_kernel  a run of consecutive frames whose matrix is exactly the identity: the tap is the lane's own pixel, so the lane
//                          keeps its 4 pixels x 3 channels of state in registers and walks the run's frames: state (or the preceding
//                          frame) is read once, every frame of the run is read and written once.
// The frame's row travels BY VALUE in the kernel arguments (the entry reads `rows` on the host while it plans the launches — it needs the
// still flags there anyway), so a kernel reads nothing but images.  A captured launch keeps the values it was captured with.
//
// Rounding: the definition has no fused multiply-add anywhere, and every operation is rounded to fp32 on its own.  hipcc contracts
// a * b + c by default, and this toolchain's __fmul_rn / __fadd_rn are plain operators inside a header that is compiled with that default
// (after inlining they fuse like any other pair), so the file switches contraction off for every function in it with the pragma below and
// spells each operation as its own expression; a fused multiply-add, were one wanted, would be __builtin_fmaf.  The dyadic cases of
// tests/test_feedback_gpu.py hold the device to the emulation bit for bit, which is what would notice a fused pair.
#include "common.h"

#pragma clang fp contract(off)

namespace {
constexpr int GRID_CAP = 2048;   // workgroups of a launch
constexpr int STILL_MAX = 64;    // frames of one still launch (its rows are kernel arguments: 64 x 24 bytes); a longer run is split
constexpr float COORD_MAX = 1073741824.f;  // 2^30: a coordinate is clamped to +-2^30 before it becomes an integer (a NaN becomes -2^30)
int g_grid_cap = 0;  // maua_feedback_test_grid_cap

enum { FR_A = 0, FR_B = 1, FR_TX = 2, FR_C = 3, FR_D = 4, FR_TY = 5, FR_GAIN = 6, FR_TINT = 7, FR_DRY = 10, FR_LIMIT = 11, FR_STILL = 12, FR_ROW = 16 };
enum { MODE_ADD = 0, MODE_MAX = 1, MODE_SCREEN = 2, N_MODES = 3 };
enum { BORDER_ZERO = 0, BORDER_REPLICATE = 1, BORDER_MIRROR = 2, BORDER_WRAP = 3, N_BORDERS = 4 };

struct MixRow {   // what the combine needs of a row
    float g[3];   // gain * tint_c, rounded once (on the host, in fp32)
    float dry, limit;
    int neutral;  // gain == 0 and dry == 1: out = cur bit for bit
};
struct WarpRow {
    float a, b, tx, c, d, ty;
    MixRow m;
};
struct StillRun {
    int n;
    MixRow r[STILL_MAX];
};

__device__ __forceinline__ float clamp01(float a) { return fminf(fmaxf(a, 0.f), 1.f); }

__device__ __forceinline__ float mix(const MixRow& m, int mode, int c, float cur, float prev) {
    const float u_prev = 0.5f * prev + 0.5f;
    const float u_cur = 0.5f * cur + 0.5f;
    const float a = m.dry * u_cur, b = m.g[c] * u_prev;
    float u;
    if (mode == MODE_ADD) u = a + b;
    else if (mode == MODE_MAX) u = fmaxf(a, b);
    else u = 1.f - (1.f - clamp01(a)) * (1.f - clamp01(b));
    u = fminf(u, m.limit);
    return 2.f * u - 1.f;
}

// tap index i of an axis of n elements under the border rule -> an index inside the axis, or -1: outside (BORDER_ZERO: the tap is black)
__device__ __forceinline__ int fold_tap(int i, int n, int border) {
    if (border == BORDER_ZERO) return (i < 0 || i >= n) ? -1 : i;
    if (border == BORDER_REPLICATE) return min(max(i, 0), n - 1);
    if (border == BORDER_WRAP) {
        const int m = i % n;
        return m < 0 ? m + n : m;
    }
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m > n - 1 ? p - m : m;
}

struct Taps {
    int x0, x1, y0, y1;  // folded indices, -1: outside
    float fx, fy;
};

__device__ __forceinline__ Taps taps_of(const WarpRow& r, int px, int py, int h, int w, float cx, float cy, int border) {
    const float dx = (float)px - cx, dy = (float)py - cy;
    float sx = ((r.a * dx + r.b * dy) + r.tx) + cx;
    float sy = ((r.c * dx + r.d * dy) + r.ty) + cy;
    sx = fminf(fmaxf(sx, -COORD_MAX), COORD_MAX);
    sy = fminf(fmaxf(sy, -COORD_MAX), COORD_MAX);
    const float flx = floorf(sx), fly = floorf(sy);
    const int ix = (int)flx, iy = (int)fly;
    Taps t;
    t.fx = sx - flx, t.fy = sy - fly;
    t.x0 = fold_tap(ix, w, border), t.x1 = fold_tap(ix + 1, w, border);
    t.y0 = fold_tap(iy, h, border), t.y1 = fold_tap(iy + 1, h, border);
    return t;
}

__device__ __forceinline__ float tap(const float* plane, int y, int x, int w) {
    return (x < 0 || y < 0) ? -1.f : plane[(int64_t)y * w + x];  // every index that is not -1 is inside the plane (fold_tap)
}

__device__ __forceinline__ float bilinear(const float* plane, const Taps& t, int w) {
    const float v00 = tap(plane, t.y0, t.x0, w), v01 = tap(plane, t.y0, t.x1, w);
    const float v10 = tap(plane, t.y1, t.x0, w), v11 = tap(plane, t.y1, t.x1, w);
    const float top = v00 + t.fx * (v01 - v00);
    const float bottom = v10 + t.fx * (v11 - v10);
    return top + t.fy * (bottom - top);
}

// One frame.  cur: the frame's image; prev: the frame it gathers from (NULL: black); out: the result (may be cur: a lane reads its own
// pixels of cur before it writes them, and gathers from another frame); state: when not NULL the result is stored there as well.
// VEC: w % 4 == 0 and cur, out, state 16-byte aligned: an item is 4 consecutive pixels of a row.  !VEC: an item is one pixel.
template <bool VEC>
__global__ __launch_bounds__(256) void feedback_warp_kernel(const float* cur, float* out, const float* prev, float* state, int h, int w,
                                                            uint32_t items, uint32_t per_row, WarpRow r, int mode, int border) {
    constexpr int N = VEC ? 4 : 1;
    const int64_t plane = (int64_t)h * w;
    const float cx = (float)(w - 1) * 0.5f, cy = (float)(h - 1) * 0.5f;
    for (uint32_t it = blockIdx.x * 256u + threadIdx.x; it < items; it += gridDim.x * 256u) {
        const int py = it / per_row, px0 = (it - py * per_row) * N;
        const int64_t p = (int64_t)py * w + px0;
        float x[N][3], y[N][3];
        if constexpr (VEC) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float4 q = *reinterpret_cast<const float4*>(cur + c * plane + p);
                x[0][c] = q.x, x[1][c] = q.y, x[2][c] = q.z, x[3][c] = q.w;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) x[0][c] = cur[c * plane + p];
        }
        if (r.m.neutral) {  // (uniform; the frame keeps its bits, NaN payloads included)
#pragma unroll
            for (int k = 0; k < N; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) y[k][c] = x[k][c];
        } else {
#pragma unroll
            for (int k = 0; k < N; ++k) {
                if (prev) {
                    const Taps t = taps_of(r, px0 + k, py, h, w, cx, cy, border);
#pragma unroll
                    for (int c = 0; c < 3; ++c) y[k][c] = mix(r.m, mode, c, x[k][c], bilinear(prev + c * plane, t, w));
                } else {
#pragma unroll
                    for (int c = 0; c < 3; ++c) y[k][c] = mix(r.m, mode, c, x[k][c], -1.f);
                }
            }
        }
        if constexpr (VEC) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float4 q = make_float4(y[0][c], y[1][c], y[2][c], y[3][c]);
                *reinterpret_cast<float4*>(out + c * plane + p) = q;
                if (state) *reinterpret_cast<float4*>(state + c * plane + p) = q;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                out[c * plane + p] = y[0][c];
                if (state) state[c * plane + p] = y[0][c];
            }
        }
    }
}

// run.n consecutive still frames, cur / out their first ([n,3,h,w], frame stride 3 h w).  prev: what the first gathers from (NULL: black).
// The tap of a still frame is the pixel itself (fx = fy = 0: a + 0 (b - a) = a for finite a, b), so a lane carries its own pixels.
template <bool VEC>
__global__ __launch_bounds__(256) void feedback_still_kernel(const float* cur, float* out, const float* prev, float* state, int64_t plane,
                                                             uint32_t items, StillRun run, int mode) {
    constexpr int N = VEC ? 4 : 1;
    for (uint32_t it = blockIdx.x * 256u + threadIdx.x; it < items; it += gridDim.x * 256u) {
        const int64_t p = (int64_t)it * N;
        float s[N][3];
        if (prev) {
            if constexpr (VEC) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float4 q = *reinterpret_cast<const float4*>(prev + c * plane + p);
                    s[0][c] = q.x, s[1][c] = q.y, s[2][c] = q.z, s[3][c] = q.w;
                }
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) s[0][c] = prev[c * plane + p];
            }
        } else {
#pragma unroll
            for (int k = 0; k < N; ++k) s[k][0] = s[k][1] = s[k][2] = -1.f;
        }
        for (int f = 0; f < run.n; ++f) {  // (uniform: run is a kernel argument)
            const MixRow m = run.r[f];
            const float* frame = cur + (int64_t)f * 3 * plane;
            float* oframe = out + (int64_t)f * 3 * plane;
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
#pragma unroll
            for (int k = 0; k < N; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) s[k][c] = m.neutral ? x[k][c] : mix(m, mode, c, x[k][c], s[k][c]);
            if constexpr (VEC) {
#pragma unroll
                for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(oframe + c * plane + p) = make_float4(s[0][c], s[1][c], s[2][c], s[3][c]);
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) oframe[c * plane + p] = s[0][c];
            }
        }
        if (state) {
            if constexpr (VEC) {
#pragma unroll
                for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(state + c * plane + p) = make_float4(s[0][c], s[1][c], s[2][c], s[3][c]);
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) state[c * plane + p] = s[0][c];
            }
        }
    }
}

bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

MixRow mix_row(const float* row) {
    MixRow m;
    for (int c = 0; c < 3; ++c) m.g[c] = row[FR_GAIN] * row[FR_TINT + c];
    m.dry = row[FR_DRY], m.limit = row[FR_LIMIT];
    m.neutral = row[FR_GAIN] == 0.f && row[FR_DRY] == 1.f;
    return m;
}

// still: the flag is set AND the matrix is exactly the identity (a flag on another matrix is not believed)
bool is_still(const float* row) {
    return row[FR_STILL] != 0.f && row[FR_A] == 1.f && row[FR_B] == 0.f && row[FR_TX] == 0.f && row[FR_C] == 0.f && row[FR_D] == 1.f &&
           row[FR_TY] == 0.f;
}

// the end (exclusive) of the launch that starts at frame i: a still run of at most STILL_MAX frames, or the one moving frame
int launch_end(const float* rows, int row_stride, int batch, int i, bool* still) {
    *still = rows && is_still(rows + (int64_t)i * row_stride);
    if (!*still) return i + 1;
    int j = i + 1;
    while (j < batch && j - i < STILL_MAX && is_still(rows + (int64_t)j * row_stride)) ++j;
    return j;
}

unsigned grid_of(int64_t items) {
    const int64_t blocks = ceil_div64(items, 256), cap = g_grid_cap > 0 ? g_grid_cap : GRID_CAP;
    return (unsigned)(blocks < cap ? blocks : cap);
}

int check_shape(int batch, int h, int w, int row_stride) {
    if (batch < 1 || h <= 0 || w <= 0 || row_stride < FR_ROW) return MAUA_EINVAL;
    if ((int64_t)h * w > 0x7fffff00ll) return MAUA_ENOSYS;  // the 32-bit item index
    return 0;
}
}  // namespace

extern "C" int maua_feedback_test_grid_cap(int cap) {
    const int before = g_grid_cap;
    g_grid_cap = cap > 0 ? cap : 0;
    return before;
}

extern "C" int maua_feedback_plan(int batch, int h, int w, const float* host_rows, int row_stride, const float* img, int* plan) {
    if (!plan || !img) return MAUA_EINVAL;
    if (int rc = check_shape(batch, h, w, row_stride)) return rc;
    int launches = 0, still_launches = 0;
    unsigned long long kinds = 0;  // bit k: launch k is a still run (the first 64 launches)
    bool first_moving = true;
    for (int i = 0; i < batch;) {
        bool still;
        const int j = launch_end(host_rows, row_stride, batch, i, &still);
        if (i == 0) first_moving = !still;
        if (still) {
            ++still_launches;
            if (launches < 64) kinds |= 1ull << launches;
        }
        ++launches;
        i = j;
    }
    plan[0] = launches;
    plan[1] = still_launches;
    plan[2] = (w % 4 == 0 && (((uintptr_t)img) & 15) == 0) ? 1 : 0;  // the instance, as far as img decides it (the entry also asks out and state)
    plan[3] = (int)(kinds & 0xffffffffull);
    plan[4] = (int)(kinds >> 32);
    plan[5] = (batch == 1 && first_moving) ? 1 : 0;  // a single moving frame cannot store the state it gathers from: one device copy follows
    plan[6] = (int)grid_of((int64_t)(plan[2] ? w / 4 : w) * h);
    plan[7] = STILL_MAX;
    return 0;
}

extern "C" int maua_feedback_f32(const float* img, float* out, float* state, int state_valid, int batch, int h, int w, const float* rows,
                                 int row_stride, int mode, int border, void* stream) {
    if (!img || !out || !state || !rows) return MAUA_EINVAL;
    if (mode < 0 || mode >= N_MODES || border < 0 || border >= N_BORDERS) return MAUA_EINVAL;
    if (int rc = check_shape(batch, h, w, row_stride)) return rc;
    const int64_t plane = (int64_t)h * w, frame = 3 * plane;
    const size_t bytes = (size_t)batch * frame * 4, state_bytes = (size_t)frame * 4;
    if (out != img && overlap(img, bytes, out, bytes)) return MAUA_EINVAL;  // overlapping, and not the whole batch in place
    if (overlap(state, state_bytes, img, bytes) || overlap(state, state_bytes, out, bytes)) return MAUA_EINVAL;
    const bool vec = w % 4 == 0 && ((((uintptr_t)img) | ((uintptr_t)out) | ((uintptr_t)state)) & 15) == 0;
    const int64_t per_row = vec ? w / 4 : w, items = per_row * h;
    const dim3 grid(grid_of(items));
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < batch;) {
        bool still;
        const int j = launch_end(rows, row_stride, batch, i, &still);
        const float* prev = i > 0 ? out + (int64_t)(i - 1) * frame : state_valid ? state : nullptr;
        const float* cur = img + (int64_t)i * frame;
        float* dst = out + (int64_t)i * frame;
        const bool last = j == batch;
        if (still) {
            StillRun run;
            run.n = j - i;
            for (int f = i; f < j; ++f) run.r[f - i] = mix_row(rows + (int64_t)f * row_stride);
            float* store = last ? state : nullptr;  // (a lane reads its own pixels of the state before it writes them)
            if (vec) hipLaunchKernelGGL((feedback_still_kernel<true>), grid, dim3(256), 0, st, cur, dst, prev, store, plane, (uint32_t)items, run, mode);
            else hipLaunchKernelGGL((feedback_still_kernel<false>), grid, dim3(256), 0, st, cur, dst, prev, store, plane, (uint32_t)items, run, mode);
            MAUA_LAUNCH_CHECK();
        } else {
            const float* row = rows + (int64_t)i * row_stride;
            WarpRow r;
            r.a = row[FR_A], r.b = row[FR_B], r.tx = row[FR_TX], r.c = row[FR_C], r.d = row[FR_D], r.ty = row[FR_TY];
            r.m = mix_row(row);
            // the frame that gathers from the state must not store it in the same launch (other lanes still read it): a batch of one
            // moving frame stores `out` alone and a device copy on the same stream follows
            const bool gathers_state = prev == state && !r.m.neutral;
            float* store = last && !gathers_state ? state : nullptr;
            if (vec) hipLaunchKernelGGL((feedback_warp_kernel<true>), grid, dim3(256), 0, st, cur, dst, prev, store, h, w, (uint32_t)items, (uint32_t)per_row, r, mode, border);
            else hipLaunchKernelGGL((feedback_warp_kernel<false>), grid, dim3(256), 0, st, cur, dst, prev, store, h, w, (uint32_t)items, (uint32_t)per_row, r, mode, border);
            MAUA_LAUNCH_CHECK();
            if (last && gathers_state) {
                const hipError_t e = hipMemcpyAsync(state, dst, state_bytes, hipMemcpyDeviceToDevice, st);
                if (e != hipSuccess) return (int)e;
            }
        }
        i = j;
    }
    return 0;
}
