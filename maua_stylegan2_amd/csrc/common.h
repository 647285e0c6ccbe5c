// Shared helpers for libmaua_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/maua_hip.h"

#define MAUA_LAUNCH_CHECK()                       \
    do {                                          \
        hipError_t e__ = hipGetLastError();       \
        if (e__ != hipSuccess) return (int)e__;   \
    } while (0)

// hipFuncAttributeMaxDynamicSharedMemorySize for a kernel that uses more than the default 64 KB of LDS.  The attribute belongs to
// (function, device): SUCCESS is remembered per device in the caller's `done` bit mask (maua_launch_conv's, one per instance), a failure is
// returned as the launch's hipError_t (> 0, the contract of include/maua_hip.h) and retried by the next call instead of being cached
// for the life of the process.  Relaxed atomics: two threads racing on the first call both set the attribute, which is harmless.
static inline int maua_allow_full_lds(const void* kern, unsigned long long* done, int bytes = 160 * 1024) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    const unsigned long long bit = 1ull << (dev & 63);
    if (__atomic_load_n(done, __ATOMIC_RELAXED) & bit) return 0;
    e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return (int)e;
    __atomic_fetch_or(done, bit, __ATOMIC_RELAXED);
    return 0;
}

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Grid of a grid-stride kernel (weight packers, reducers, frame conversion): one 256-thread block per 256 elements, at most `cap` blocks.
static inline unsigned pack_grid(int64_t total, int64_t cap = 4096) {
    const int64_t blocks = ceil_div64(total, 256);
    return (unsigned)(blocks < cap ? blocks : cap);
}

// An operand the kernels address through a raw buffer descriptor (conv_device.h) with 32-bit byte offsets: descriptors carry 2^31 - 1
// checked bytes and the offset 2^31 means "outside" (the source of the zero padding), so every real byte offset must stay below that.
static inline bool fits_raw_descriptor(int64_t bytes) { return bytes <= 0x7fffffffLL; }

// Name of the kernel template instance that the last convolution launch of this process ran, as rocprofv3 prints it
// (maua_modconv_last_instance): bench.py, tools/microbench.py and the tables under profiles/ join on it.  A launch that is followed by
// helper kernels (edge lines, seam pass, reducers) keeps its main kernel's name.  (The generic kernel's names come from its instance
// tables, modconv_m0.hip .. modconv_m4.hip kConvInstances, which maua_modconv_plan_instance answers from without launching.)
inline char g_conv_instance[96] = "";

// THE launch of a convolution kernel instance (256 threads, dynamic LDS beyond the default 64 KB allowed): attribute, name, launch,
// check.  The kernel is a template argument, never a host function-pointer variable (build.py on -fsanitize=function says why), which
// also gives every instance its own `lds_ok` mask.
template <auto Kern, typename... Args>
int maua_launch_conv(const char* name, int64_t blocks, size_t lds_bytes, hipStream_t st, const Args&... args) {
    static unsigned long long lds_ok = 0;  // devices on which the attribute has been set
    if (int rc = maua_allow_full_lds(reinterpret_cast<const void*>(Kern), &lds_ok)) return rc;
    snprintf(g_conv_instance, sizeof(g_conv_instance), "%s", name);
    hipLaunchKernelGGL(Kern, dim3((unsigned)blocks), dim3(256), lds_bytes, st, args...);
    MAUA_LAUNCH_CHECK();
    return 0;
}

// Bijective XCD-aware remap (cdna_hip_programming.md §5 "XCD swizzle must be bijective"): block b runs on
// XCD b % 8; give every XCD one contiguous chunk of the logical tile range so that neighbouring tiles
// (which share halos / weight panels) hit the same 4 MiB L2.  Speed only, never correctness.
__device__ __forceinline__ int xcd_remap(int bid, int nblocks) {
    const int NX = 8;
    int q = nblocks / NX, r = nblocks % NX;
    int xcd = bid % NX, idx = bid / NX;
    int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}

// sqrt(2): the gain of the leaky ReLU (FusedLeakyReLU's scale).  Every tail folds it into gain, bias and noise weight once.
constexpr float kSqrt2 = 1.41421356237309515f;

__device__ __forceinline__ float lrelu_gain(float v) { return (v > 0.f ? v : v * 0.2f) * kSqrt2; }

// ---- the StyledConv tail (noise, bias, leaky ReLU * sqrt2) as every convolution / blur entry receives it
// Where this launch's noise comes from: the caller's map, or — with a frame source (include/maua_hip.h) — slot `noise_slot` of the
// HBM-resident sequence at the launch's first frame.  Uniform scalar loads; the ONE place that knows the frame source's layout.
template <typename NoisePtr>  // const float*, with or without __restrict__
__device__ __forceinline__ void maua_noise_source(NoisePtr& noise, int64_t& batch_stride, const maua_frame_source_t* src, int noise_slot) {
    if (src) {
        batch_stride = src->noise_stride[noise_slot];
        noise = src->noise[noise_slot];
        if (noise) noise += (int64_t)src->frame0 * batch_stride;
    }
}

struct TailArgs {
    const float* noise;          // [B or 1, H, W] or null
    const float* noise_w;        // [1]
    const float* bias;           // [Cout] or null
    int64_t noise_batch_stride;
    const maua_frame_source_t* src;  // when set: noise / noise_batch_stride come from src->noise[noise_slot] at frame src->frame0
    int noise_slot;

    // The entries' argument check (0 or MAUA_EINVAL).  tail_applied = false: this launch stores the raw map, a frame source's noise is
    // not read and its weight may be absent (maua_modconv3x3_f32 without fuse_act).
    int check(bool tail_applied = true) const {
        if ((noise || (src && tail_applied)) && !noise_w) return MAUA_EINVAL;
        if (src && (noise_slot < 0 || noise_slot >= MAUA_MAX_NOISE_SLOTS)) return MAUA_EINVAL;
        return 0;
    }
};

// fused ToRGB (models/stylegan2.py:346-365) of a plain StyledConv
struct RgbArgs {
    const float* w;      // [3, Cout]
    const float* s;      // styles of the ToRGB layer, [B, s_stride] (already offset to the layer's slice)
    const float* bias;   // [3]
    const float* skip;   // [B, 3, H/2, W/2] or null
    const float* k4;     // 4x4 upsample taps
    float* out;          // [B, 3, H, W]; mode 3: [B, 3 m_tiles, H, W]
    uint8_t* u8;         // when set: the image leaves as uint8 NHWC frames [B, H, W, 3] (render.py:40-43); out may then be null
    float wscale;
    int mode;            // 1 on, 2 on and the feature map itself is not stored, 3 partial: every m-tile's share of the sum goes to out (no
                         // bias, no skip; 2-D Winograd only), the feature map is stored
};

// modconv_w2d.hip (mode 5 of maua_modconv3x3_f32 / maua_styledconv_torgb_f32): 2-D Winograd F(2x4, 3x3) plain convolution
int maua_w2d_tiles(int cin, int cout, int h, int w, int* tm, int* tn);
int maua_w2d_launch(const float* x, const float* wq, const float* s, int s_stride, const float* d, float* y, int batch, int cin,
                    int cout, int h, int w, float wscale, int fuse_act, const TailArgs& tail, const RgbArgs* rgb, const float* post_s,
                    void* stream);

// modconv_up2d.hip (mode 6 of maua_modconv3x3_f32): transposed convolution with F(2,2) on both axes of its polyphase form
int64_t maua_up2d_ws_floats(int batch, int cin, int h);
int maua_up2d_launch(const float* x, const float* wq, const float* s, int s_stride, const float* d, float* y, float* ws, int batch, int cin,
                     int cout, int h, int w, float wscale, void* stream);

// ... its form for 16-wide inputs with K split over several workgroups per tile (partial raw maps in slabs; maua_upconv_blur_lowres_f32, up = 6)
int maua_up2d16_ok(int cin, int cout, int h, int w);
int maua_up2d16_splits(int batch, int cin, int cout, int h, int w);
int maua_up2d16_launch(const float* x, const float* wq, const float* s, int s_stride, float* y, float* xcol, int batch, int cin, int cout, int h,
                       int w, float wscale, int* splits_out, void* stream);

// modconv_sbf16.hip (mode 7 of maua_modconv3x3_f32; side measurement, off by default): plain 3x3 convolution with split-bf16 products
int maua_sbf16_ok(int cin, int cout, int h, int w);
int maua_sbf16_launch(const float* x, const void* wq, const float* s, int s_stride, const float* d, float* y, float* ws, int batch, int cin,
                      int cout, int h, int w, int up, float wscale, int fuse_act, const TailArgs& tail, void* stream);
int maua_up2d_edge_launch(const float* x, const float* edge_taps, const float* s, int s_stride, const float* d, float* y, const float* xcol,
                          int batch, int cin, int cout, int h, int w, float wscale, void* stream);
