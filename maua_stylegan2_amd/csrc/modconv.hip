// ModulatedConv2d 3x3 on the gfx950 matrix cores (fp32-in / fp32-accumulate MFMA, exact fp32).
//
// Behavioural contract: /root/reference/models/stylegan2.py:217-254 (+ StyledConv tail :338-343).
// The reference materialises per-sample weights [B,Cout,Cin,3,3] and runs a grouped cuDNN conv.  Here:
//
//     y[b,o] = d[b,o] * sum_{i,tap} (wscale * W[o,i,tap]) * (s[b,i] * x[b,i, . + tap])
//
// i.e. input-scale -> SHARED-weight implicit GEMM -> output-demod, so one weight panel
// serves the whole batch of frames and stays L2-resident across pixel tiles.
//
// Implicit GEMM on v_mfma_f32_32x32x2_f32:  M = Cout, N = pixels, K = Cin x taps.
//   A (weights)  : tap-major repack wp[tap][cin][cout_pad] (maua_pack_weight_f32) -> LDS As[tap][c][BM], lanes read
//                  consecutive cout -> conflict-free ds_read_b32 with immediate offsets.
//   B (features) : the workgroup stages ONE halo patch per 8-channel chunk (scaled by s[b,i] on the way in);
//                  the 9 taps are 9 shifted views of the same patch — no im2col replication, in HBM or in LDS.
//   C            : 64 accumulator VGPRs per wave; epilogue applies demod, noise, bias, leaky-ReLU*sqrt2 in-register
//                  and stores 128-byte row segments (lane = pixel column).
// Transposed (stride-2) convolution (:229-237) is evaluated polyphase: the 9 taps split into output parities
// (4/2/2/1 taps), every workgroup owns a tile of input positions and accumulates all four parities from the same
// staged patch — 9 MACs per input pixel per channel pair, exactly the reference's FLOPs, no zero-stuffing.
// Small feature maps (4^2..32^2) are weight-streaming bound: K is split across workgroups (deterministic two-pass
// split-K through a caller-owned workspace, reduced by reduce_tail_kernel together with the tail).
//
// Kernel modes (template MODE = the `up` argument of maua_modconv3x3_f32), all on the same tile / pipeline skeleton:
//   0  direct 3x3                      9 weight rows per channel, 1 accumulator tile per position group
//   1  transposed, polyphase           9 rows, 4 tiles (output parities); tiles = flat runs of the (H+1)x(W+1) grid
//   2  Winograd F(2,3) along x         12 rows (3 ky x 4 frequencies), positions = output pairs, 4 tiles
//   3  Winograd F(4,3) along x         18 rows (3 ky x 6 frequencies), positions = output quads, 6 tiles
//   4  transposed + F(2,2) on the even x-phase   12 rows, positions = position pairs, 10 tiles
// Both operands reach LDS by global_load_lds DMA, double buffered, one barrier per K chunk; the style scale of the
// input channel is applied when the B operand is read (a register-staged, pre-scaled patch remains for tiles that hold
// several images and for the 32-channel F(2,3) config).  Measured rule of this chip that shapes everything above: VALU /
// SALU instructions of co-resident waves do NOT hide under the 64-cycle MFMAs (profiles/r01_pmc_modconv.md) — fewer
// MFMAs per output (Winograd) and fewer non-MFMA instructions are what pay, not occupancy or prefetch depth.
//
// Where the pieces live: this file is the host side — make_plan (shape -> instance, geometry, grid), the entries, and the split-K
// reducers with the entries that launch them.  The kernel template is modconv_kernel.h, instantiated by modconv_m0.hip ..
// modconv_m4.hip (one unit per mode, each with the table of its instances); modconv_plan.h holds what those units and this file share;
// the weight packs are modconv_pack.hip.
#include "modconv_plan.h"
#include "epilogue.h"

#include <cstdio>

namespace {

// The tail behind a slab sum, with every rounding spelled out (no fp contraction): reduce_tail_kernel and reduce_tail_rgbpart_kernel must
// store the same bits for the same slabs, whatever the compiler would fuse in either context.
__device__ __forceinline__ float slab_tail(float v, float dv, float nw, float nzv, float bv, bool act) {
#pragma clang fp contract(off)  // (HIP's __fmul_rn / __fadd_rn are plain operators: they do not stop the contraction)
    v = v * dv;
    if (!act) return v;
    const float nz = nw * nzv;
    const float t = v + nz;
    return lrelu_gain(t + bv);
}

// Sum split-K slabs and apply the same tail as the fused epilogue.
__global__ __launch_bounds__(256) void reduce_tail_kernel(const float* __restrict__ ws, int splits, int64_t slab,
                                                          float* __restrict__ y, const float* __restrict__ d,
                                                          const float* __restrict__ noise, int64_t noise_batch_stride,
                                                          const float* __restrict__ noise_w,
                                                          const float* __restrict__ bias, int fuse_act, int cout,
                                                          int64_t plane, int64_t total,
                                                          const maua_frame_source_t* __restrict__ src, int noise_slot) {
    maua_noise_source(noise, noise_batch_stride, src, noise_slot);
    const float nw = (fuse_act && noise) ? noise_w[0] : 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        // every operand of this element is fetched before the first use: the slab values (up to 32, all in flight: with four at a time a
        // 32-way split was eight dependent round trips, 8 us per launch on maps of a few KB), the demodulation factor, the noise value, the bias
        const int64_t bc = i / plane;
        const int64_t pix = i - bc * plane;
        const int b = (int)(bc / cout), o = (int)(bc - (int64_t)b * cout);
        const float dv = d ? d[bc] : 1.f;
        const float nzv = nw != 0.f ? noise[(size_t)b * noise_batch_stride + pix] : 0.f;
        const float bv = (fuse_act && bias) ? bias[o] : 0.f;
        float v = 0.f;
        int s = 0;
        for (; s + 32 <= splits; s += 32) {
            float a[32];
#pragma unroll
            for (int k = 0; k < 32; ++k) a[k] = ws[(size_t)(s + k) * slab + i];
#pragma unroll
            for (int k = 0; k < 32; k += 4) v += (a[k] + a[k + 1]) + (a[k + 2] + a[k + 3]);  // (slab_sum's association, epilogue.h; 32 / 16 slabs in flight)
        }
        if (s + 16 <= splits) {
            float a[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) a[k] = ws[(size_t)(s + k) * slab + i];
#pragma unroll
            for (int k = 0; k < 16; k += 4) v += (a[k] + a[k + 1]) + (a[k + 2] + a[k + 3]);
            s += 16;
        }
        for (; s + 4 <= splits; s += 4) {
            const float a0 = ws[(size_t)s * slab + i], a1 = ws[(size_t)(s + 1) * slab + i];
            const float a2 = ws[(size_t)(s + 2) * slab + i], a3 = ws[(size_t)(s + 3) * slab + i];
            v += (a0 + a1) + (a2 + a3);
        }
        for (; s < splits; ++s) v += ws[(size_t)s * slab + i];
        y[i] = slab_tail(v, dv, nw, nzv, bv, fuse_act != 0);
    }
}

// ---- low-resolution layers (4^2 .. 32^2 outputs): the split-K reduction fused with what follows it -----------------------------------------
// On these maps every launch is a fixed cost of 5 .. 20 us whatever it computes (tools/rocpd_timeline.py): the transposed layers ran
// convolution -> reduce_tail -> blur + noise + act (three launches, 22 .. 33 us for the last two), the plain ones convolution -> reduce_tail ->
// ToRGB (16 .. 29 us).  The two kernels below take the workspace slabs of the convolution directly.
//
// Up-sampling layer: one workgroup per (image, channel) plane.  The raw (2H+1) x (2W+1) plane — the sum of the split-K slabs times the
// demodulation factor, exactly reduce_tail_kernel's value — is formed in LDS, then the 4 x 4 blur (pad (1, 1)), noise, bias, leaky ReLU and the
// style fold's scale are applied in the arithmetic order of fir_tile_kernel: the result is bit-identical to the three-launch path.
__global__ __launch_bounds__(256) void reduce_blur_tail_kernel(const float* __restrict__ ws, int splits, int64_t slab, float* __restrict__ y,
                                                               const float* __restrict__ d, const float* __restrict__ k4,
                                                               const float* __restrict__ noise, int64_t noise_batch_stride,
                                                               const float* __restrict__ noise_w, const float* __restrict__ bias,
                                                               const float* __restrict__ post_s, int post_stride, int cout, int h, int w,
                                                               const maua_frame_source_t* __restrict__ src, int noise_slot, int edge_slab0) {
    // edge_slab0 (the F(2,2)^2 form, modconv_up2d.hip): raw row 2h and column 2w are written by the edge kernel, into slab 0 only
    extern __shared__ __attribute__((aligned(16))) float raw[];  // [(2h + 3)][(2w + 3)]: the raw plane inside a border of zeros (the blur's padding)
    const int RH = 2 * h + 1, RW = 2 * w + 1, OH = 2 * h, OW = 2 * w, PW = RW + 2;
    const int bc = blockIdx.x, b = bc / cout, c = bc - b * cout;
    const int tid = threadIdx.x;
    maua_noise_source(noise, noise_batch_stride, src, noise_slot);
    float kf[4][4];  // flipped taps (uniform loads)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) kf[i][j] = k4[(3 - i) * 4 + (3 - j)];
    const float dv = d ? d[bc] : 1.f;
    const float g = kSqrt2;
    const float nw = noise ? noise_w[0] * kSqrt2 : 0.f;
    const float bs = bias ? bias[c] * kSqrt2 : 0.f;
    const float post = post_s ? post_s[(size_t)b * post_stride + c] : 1.f;
    const float* wp = ws + (size_t)bc * RH * RW;
    const int n_raw = RH * RW, n_out = OH * OW;
    // the lane's noise values (at most four outputs per thread: 2h x 2w <= 1024, checked by the launcher) travel with the slab loads
    float nzv[4] = {0.f, 0.f, 0.f, 0.f};
    if (noise)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (tid + 256 * k < n_out) nzv[k] = noise[(size_t)b * noise_batch_stride + tid + 256 * k];
    {
        // a thread owns raw elements tid, tid + 256, ... (at most five: (2h + 1)(2w + 1) <= 33 x 33): the slab loads of ALL of them are issued
        // before the first add, eight slabs at a time (element by element the plane took five dependent round trips)
        constexpr int NE = 5;
        float v[NE];
        int nsl[NE];  // slabs that hold this element
#pragma unroll
        for (int q = 0; q < NE; ++q) {
            v[q] = 0.f;
            const int e = tid + 256 * q, r = e / RW;
            nsl[q] = e >= n_raw ? 0 : (edge_slab0 && (r == RH - 1 || e - r * RW == RW - 1)) ? 1 : splits;
        }
        slab_sum(v, splits, [&](int q, int sp) { return (sp < nsl[q]) ? wp[(size_t)sp * slab + tid + 256 * q] : 0.f; });
#pragma unroll
        for (int q = 0; q < NE; ++q) {
            const int e = tid + 256 * q;
            if (e < n_raw) {
                const int r = e / RW;
                raw[(r + 1) * PW + (e - r * RW) + 1] = v[q] * dv;
            }
        }
        // the border: rows 0 and RH + 1, columns 0 and RW + 1 of the rows between
        for (int e = tid; e < 2 * PW + 2 * RH; e += 256) {
            const int cell = e < PW ? e : e < 2 * PW ? (RH + 1) * PW + (e - PW) : (1 + ((e - 2 * PW) >> 1)) * PW + ((e & 1) ? RW + 1 : 0);
            raw[cell] = 0.f;
        }
    }
    __syncthreads();
    float* yp = y + (size_t)bc * n_out;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int o = tid + 256 * k;
        if (o >= n_out) break;
        const int Y = o / OW, X = o - Y * OW;
        float acc = 0.f;
        const float* win = raw + Y * PW + X;  // raw[Y - 1 + i][X - 1 + j] of the un-bordered plane
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = (i == 0 && j == 0) ? kf[0][0] * win[0] : fmaf(kf[i][j], win[i * PW + j], acc);
        const float tt = fmaf(acc, g, fmaf(nw, nzv[k], bs));
        yp[o] = fmaxf(tt, 0.2f * tt) * post;
    }
}

// Plain layer followed by a ToRGB: one workgroup per (image, group of 32 output channels, PT pixels; PT = 32, or 16 on 4 x 4 maps).  A thread
// sums the slabs of 32 PT / 256 elements (channels cl, cl + 256 / PT, ... of the group at one pixel: a wave instruction reads whole 128-byte
// rows of PT pixels), applies reduce_tail_kernel's tail (the stored feature map is bit-identical to that kernel's) and multiplies the activated
// values by their channels' three modulated ToRGB weights; the 32 channels of the group meet in LDS and leave as three partial planes
// rgb_part [B][3 * (cout / 32)][H][W] (plane 3 g + colour), which maua_torgb_f32's plane-sum form (5 us) turns into the image — instead of
// a ToRGB pass that re-reads the feature map (10 .. 22 us on these maps).
template <int PT>
__global__ __launch_bounds__(256) void reduce_tail_rgbpart_kernel(const float* __restrict__ ws, int splits, int64_t slab, float* __restrict__ y,
                                                                  const float* __restrict__ d, const float* __restrict__ noise,
                                                                  int64_t noise_batch_stride, const float* __restrict__ noise_w,
                                                                  const float* __restrict__ bias, const float* __restrict__ rgb_w,
                                                                  const float* __restrict__ rgb_s, int s_stride, float rgb_wscale,
                                                                  float* __restrict__ rgb_part, int cout, int plane,
                                                                  const maua_frame_source_t* __restrict__ src, int noise_slot) {
    constexpr int CL = 256 / PT;   // channel lanes
    constexpr int NC = 32 / CL;    // channels per thread
    __shared__ float part[3][CL][PT];
    const int tid = threadIdx.x, px = tid % PT, cl = tid / PT;
    const int ptiles = plane / PT, groups = cout / 32;
    int t = blockIdx.x;
    const int pt = t % ptiles;
    t /= ptiles;
    const int gidx = t % groups, b = t / groups;
    const int pix = pt * PT + px;
    maua_noise_source(noise, noise_batch_stride, src, noise_slot);
    const float nw = noise ? noise_w[0] : 0.f;
    const float nzv = nw != 0.f ? noise[(size_t)b * noise_batch_stride + pix] : 0.f;
    float dv[NC], bv[NC], ms[NC], w0[NC], w1[NC], w2[NC], v[NC];
    int64_t idx[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) {
        const int c = gidx * 32 + cl + CL * q;
        const int64_t bc = (int64_t)b * cout + c;
        idx[q] = bc * plane + pix;
        dv[q] = d ? d[bc] : 1.f;
        bv[q] = bias ? bias[c] : 0.f;
        ms[q] = rgb_s[(size_t)b * s_stride + c];
        w0[q] = rgb_w[c], w1[q] = rgb_w[cout + c], w2[q] = rgb_w[2 * cout + c];
        v[q] = 0.f;
    }
    slab_sum(v, splits, [&](int q, int sp) { return ws[(size_t)sp * slab + idx[q]]; });
    float r0 = 0.f, r1 = 0.f, r2 = 0.f;
#pragma unroll
    for (int q = 0; q < NC; ++q) {
        const float t2 = slab_tail(v[q], dv[q], nw, nzv, bv[q], true);
        y[idx[q]] = t2;
        // modulated ToRGB weights as torgb_kernel forms them: (wscale * w) * s
        r0 = fmaf((rgb_wscale * w0[q]) * ms[q], t2, r0);
        r1 = fmaf((rgb_wscale * w1[q]) * ms[q], t2, r1);
        r2 = fmaf((rgb_wscale * w2[q]) * ms[q], t2, r2);
    }
    part[0][cl][px] = r0, part[1][cl][px] = r1, part[2][cl][px] = r2;
    __syncthreads();
    if (tid < 3 * PT) {
        const int col = tid / PT, q = tid % PT;
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < CL; ++k) a += part[col][k][q];
        rgb_part[((size_t)b * 3 * groups + 3 * gidx + col) * plane + pt * PT + q] = a;
    }
}

inline int ilog2(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}
inline int pow2_ceil(int v) { return 1 << ilog2(v); }

// The launcher of a key: looked up in the table of the key's mode (modconv_m0.hip .. modconv_m4.hip).
const ConvInstance* find_instance(const ConvKey& key) {
    const ConvTable t = key.mode == 0   ? maua_conv_table_m0()
                        : key.mode == 1 ? maua_conv_table_m1()
                        : key.mode == 2 ? maua_conv_table_m2()
                        : key.mode == 3 ? maua_conv_table_m3()
                        : key.mode == 4 ? maua_conv_table_m4()
                                        : ConvTable{nullptr, 0};
    for (int i = 0; i < t.count; ++i)
        if (t.rows[i].key == key) return &t.rows[i];
    return nullptr;
}

struct Plan {
    ConvKey key;               // the instance; tile config = key.bm x key.bn, key.wm wave rows
    const ConvInstance* inst;  // its table entry (null: rc != 0)
    int rc;                    // 0, or why no launch serves the shape (MAUA_EINVAL: refused; MAUA_ENOSYS: no such instance in this build)
    ConvGeom g;
    size_t lds_bytes;
    int64_t blocks;
};

#ifdef MAUA_EXPERIMENTS
int g_conv_debug = 0;
int g_conv_cfg = 0;  // tuning key 2: bit0 -> Cout<=64 uses 64x128 (WM 2); bit1 -> Cout<=32 uses 32x512; bit2 -> no flat runs
#endif

// Shape -> instance, geometry, grid and LDS size (host; positive sizes, mode 0 .. 4).  BM follows Cout; the pixel tile is a stack of
// 32-pixel MFMA groups.  mode 0 plain, 1 transposed stride 2, 2 / 3 plain through Winograd F(2,3) / F(4,3) along x, 4 transposed with
// F(2,2) on the even x-phase.  Every refusal of a shape is decided here (Plan::rc); the geometry is filled in either way, so that
// maua_modconv_ws_floats answers for any shape.
//
// What the key sees of a shape (why a bounded enumeration of shapes reaches every key, tests/test_conv_instances_host.py):
//   * cin only as "a multiple of the K chunk (4 or 8)", cout as <= 32 / <= 64 / above and as "CoutPad a multiple of BM"; batch not at all:
//     MULTI is "the tile has room for several images" (ni > 1), a property of the map, and the patch is sized for ni images whether
//     the batch fills them or not;
//   * h and w through the position grid GH x GW (w, w / 2, w / 4, h + 1, w + 1, w / 2 + 1) and that grid only through pow2_ceil() of
//     itself or of its quotient by a power of two, each capped by the tile: a sub-tile is at most 32 positions wide, a tile at most 16
//     sub-tiles (BN <= 512).  So a key changes with h or w only where a grid dimension passes a power of two, and not beyond
//     GW = 32 x 16 (w = 4 x 512 in mode 3) or GH = 32 x 16: every h in 1 .. 139 and w in 1 .. 299 plus 2^k - 1, 2^k, 2^k + 1 (and the
//     next even width and multiple of four) up to 1025 and two sizes beyond it cover every threshold;
//   * as GH GW > BN (flat runs), with BN <= 128 in the transposed modes: a flat run's geometry depends on BN alone (and its patch,
//     2 (BN + 2) or 2 (2 BN + 2) floats, is inside the limit: a flat run never falls back), and the maps that are not flat have
//     (h + 1) (w + 1) <= 128, in mode 4 (h + 1) (w / 2 + 1) <= 128: w <= 126, inside the dense range;
//   * as the width rules of modes 2, 3 and 4, and as the 2^31 element limit (a refusal, not a key).
Plan make_plan(int batch, int cin, int cout, int h, int w, int mode) {
    Plan pl{};
    ConvKey& k = pl.key;
    ConvGeom& g = pl.g;
    const bool up = mode == 1 || mode == 4, uw = mode == 4, wino = mode == 2 || mode == 3, w43 = mode == 3;
    const int wx = w43 ? 4 : 2;  // outputs per Winograd position
    k.mode = mode;
    if ((int64_t)batch * cin * h * w > 0x7fffffffLL) pl.rc = MAUA_EINVAL;                             // 32-bit patch offsets
    if (((mode == 2 || mode == 4) && (w & 1)) || (mode == 3 && (w & 3))) pl.rc = MAUA_EINVAL;         // whole output pairs / quads
    g.B = batch, g.Cin = cin, g.Cout = cout, g.CoutPad = wino ? wino_cout_pad(cout) : pad32(cout), g.H = h, g.W = w;
    if (w43) {
        g.GH = h, g.GW = w / 4, g.OH = h, g.OW = w;  // positions are output quads
        if (cout <= 32) k.bm = 32, k.wm = 1, k.bn = 128;
        else k.bm = 64, k.wm = 1, k.bn = 128;  // (a 128-row tile holds 192 accumulator registers per wave as well, but its 18-row weight
                                               // tile only leaves room for 2-channel chunks: 4-7 % slower.  Dropped, with its chunk size.)
    } else if (wino) {
        g.GH = h, g.GW = w / 2, g.OH = h, g.OW = w;  // positions are output pairs
        if (cout <= 32) k.bm = 32, k.wm = 1, k.bn = MAUA_CFG(2) ? 256 : 128;
        else if (cout <= 64) k.bm = 64, k.wm = 1, k.bn = 128;
        else k.bm = 128, k.wm = 2, k.bn = 64;
    } else if (uw) {
        g.GH = h + 1, g.GW = w / 2 + 1, g.OH = 2 * h + 1, g.OW = 2 * w + 1;  // positions are pairs; W + 2 positions per row
        if (cout <= 32) k.bm = 32, k.wm = 1, k.bn = 128;
        else k.bm = 64, k.wm = 2, k.bn = 64;
    } else if (up) {
        g.GH = h + 1, g.GW = w + 1, g.OH = 2 * h + 1, g.OW = 2 * w + 1;
        if (cout <= 32) k.bm = 32, k.wm = 1, k.bn = 128;
        else k.bm = 64, k.wm = 2, k.bn = 64;
    } else {
        g.GH = h, g.GW = w, g.OH = h, g.OW = w;
        if (cout <= 32) k.bm = 32, k.wm = 1, k.bn = MAUA_CFG(2) ? 512 : 256;
        else if (cout <= 64) k.bm = 64, k.wm = MAUA_CFG(1) ? 2 : 1, k.bn = MAUA_CFG(1) ? 128 : 256;
        else k.bm = 128, k.wm = 2, k.bn = 128;
    }
    auto shape = [&](int bn) {
        const int nsub = bn / 32;
        int sw = up ? 8 : (wino ? 16 : 32);
        if (sw > pow2_ceil(g.GW)) sw = pow2_ceil(g.GW);
        const int sh = 32 / sw;
        int nsx = pow2_ceil(ceil_div(g.GW, sw));
        if (nsx > nsub) nsx = nsub;
        if (!up && nsx > 1) nsx = 1;  // plain: keep 32-wide row segments, stack rows instead
        int nsy = pow2_ceil(ceil_div(g.GH, sh));
        if (nsy > nsub / nsx) nsy = nsub / nsx;
        const int ni = nsub / (nsx * nsy);
        g.lsw = ilog2(sw), g.lsh = ilog2(sh), g.lnsx = ilog2(nsx), g.lnsy = ilog2(nsy), g.lni = ilog2(ni);
        const int tw = sw * nsx, th = sh * nsy;
        g.tiles_x = ceil_div(g.GW, tw), g.tiles_y = ceil_div(g.GH, th), g.img_groups = ceil_div(batch, ni);
        g.PH = th + 2, g.PW = (wino ? wx * tw : tw) + 2;
        // LDS row stride: with sub-tiles narrower than 32 pixels the 32 lanes of one MFMA group read SH rows at once;
        // a stride of SW * odd puts the rows on disjoint bank groups (conflict-free ds_read_b32)
        g.PWS = g.PW;
        if (sw < 32 && !wino) {  // (Winograd reads 8-byte pairs: the even PW is kept)
            while (g.PWS % (2 * sw) != sw) ++g.PWS;
            if (ni * g.PH * g.PWS > 512) g.PWS = g.PW;  // tiny maps, many images per tile: take the conflicts
        }
        g.PSTRIDE = ni * g.PH * g.PWS;
    };
    shape(k.bn);
    if (up && g.GH * g.GW > k.bn && !MAUA_CFG(4)) {
        // The (H+1)x(W+1) position grid never fits power-of-two 2-D tiles (29 % idle MFMA columns at 65x65); tiles are
        // instead runs of BN consecutive positions of the flattened grid, one image each.  A position reads inputs
        // p, p-1, p-GW, p-GW-1 of the pitch-GW flattened (zero-padded) input: two runs of BN+1 floats per channel.
        // (From two runs per image on — round 6: the 9 x 9 grid of the 8^2 -> 16^2 layer took 16 x 16 = 256 slots as a 2-D tile, 32 % of its
        // MFMA columns useful; as two runs of 64 it is 63 %.)
        g.flat = 1;
        g.lsw = 5, g.lsh = 0, g.lnsx = ilog2(k.bn / 32), g.lnsy = 0, g.lni = 0;
        g.tiles_x = ceil_div(g.GH * g.GW, k.bn), g.tiles_y = 1, g.img_groups = batch;
        g.PH = 2, g.PW = (uw ? 2 : 1) * k.bn + 1, g.PWS = (uw ? 2 : 1) * k.bn + 2;
        g.PSTRIDE = g.PH * g.PWS;
    }
    if (g.PSTRIDE > patch_limit(mode, k.bn)) {  // tiny feature maps under a wide-N config: fall back to the 128-pixel tile
        if (w43) k.bm = 64, k.wm = 1, k.bn = 128;
        else if (wino) k.bm = 128, k.wm = 2, k.bn = 64;
        else if (up) k.bm = 64, k.wm = 2, k.bn = 64;
        else k.bm = 128, k.wm = 2, k.bn = 128;
        shape(k.bn);
    }
    if (uw && !g.flat) pl.rc = MAUA_EINVAL;                        // mode 4 has no 2-D tiles: grids too small for flat pair runs use mode 1
    if (g.PSTRIDE > patch_limit(mode, k.bn)) pl.rc = MAUA_EINVAL;  // no tile of the mode holds this map's patch
    const int CC = chunk_channels(k.bm, k.bn, mode);
    k.multi = g.lni > 0;
    k.fast = cin % CC == 0 && g.CoutPad % k.bm == 0;
    k.maxp = g.PSTRIDE <= 256 ? 1 : (g.PSTRIDE <= 512 ? 2 : 3);
    if (!pl.rc && !(pl.inst = find_instance(k))) pl.rc = MAUA_ENOSYS;
    g.n_chunks = ceil_div(cin, CC);
    g.m_tiles = ceil_div(g.CoutPad, k.bm);
    g.n_tiles = g.tiles_x * g.tiles_y * g.img_groups;
    // split-K until the grid covers the chip ~2x (256 CUs), never below 2 chunks per split
    const int64_t base_blocks = (int64_t)g.m_tiles * g.n_tiles;
    int splits = 1;
    while (base_blocks * splits < 512 && g.n_chunks / (splits * 2) >= 2) splits *= 2;
    g.splits = splits;
    g.chunks_per_split = ceil_div(g.n_chunks, splits);
    g.splits = ceil_div(g.n_chunks, g.chunks_per_split);
    g.ws_slab = (int64_t)batch * cout * g.OH * g.OW;
    pl.blocks = base_blocks * g.splits;
    pl.lds_bytes = 2 * ((size_t)(w43 ? 18 : (wino || uw) ? 12 : 9) * CC * k.bm + (size_t)CC * g.PSTRIDE) * sizeof(float);
    if (g.lni == 0)  // the DMA patch path also stages the styles of one image
        pl.lds_bytes += (size_t)cin * sizeof(float);
    if (pl.lds_bytes < (size_t)2 * k.bm * sizeof(float)) pl.lds_bytes = (size_t)2 * k.bm * sizeof(float);
    return pl;
}

}  // namespace

#ifdef MAUA_EXPERIMENTS
int maua_conv_debug_set(int v) { g_conv_debug = v; return 0; }
int maua_conv_cfg_set(int v) { g_conv_cfg = v; return 0; }
#endif

extern "C" int64_t maua_modconv_ws_floats(int batch, int cin, int cout, int h, int w, int up) {
    if (batch <= 0 || cin <= 0 || cout <= 0 || h <= 0 || w <= 0 || up == 5 || up == 7) return 0;
    if (up == 6 || up == 8) return maua_up2d_ws_floats(batch, cin, h);  // the exported last input column
    Plan pl = make_plan(batch, cin, cout, h, w, up);
    return pl.g.splits > 1 ? pl.g.ws_slab * pl.g.splits : 0;
}

// Name of the kernel template instance the LAST maua_modconv3x3_f32 / maua_styledconv_torgb_f32 call of this process
// launched, as rocprofv3 prints it ("modconv_mfma_kernel<BM, BN, WM, MODE, MULTI, FAST, MAXP>"): lets bench.py join its live
// timings with the per-instance PMC tables under profiles/ without re-implementing the plan.
extern "C" int maua_modconv_last_instance(char* buf, int buf_len) {
    if (!buf || buf_len <= 0) return MAUA_EINVAL;
    snprintf(buf, (size_t)buf_len, "%s", g_conv_instance);
    return 0;
}

// The plan without a launch: which instance maua_modconv3x3_f32 would run for this shape, or the shape's refusal.  No HIP call.
extern "C" int maua_modconv_plan_instance(int batch, int cin, int cout, int h, int w, int up, char* buf, int buf_len) {
    if (!buf || buf_len <= 0 || batch <= 0 || cin <= 0 || cout <= 0 || h <= 0 || w <= 0 || up < 0 || up > 4) return MAUA_EINVAL;
    const Plan pl = make_plan(batch, cin, cout, h, w, up);
    if (pl.rc) return pl.rc;
    snprintf(buf, (size_t)buf_len, "%s", pl.inst->name);
    return 0;
}

namespace {
int modconv_impl(const float* x, const float* wp, const float* s, int s_stride, const float* d, float* y, int batch,
                 int cin, int cout, int h, int w, int up, float wscale, int fuse_act, const TailArgs& tail, float* ws, const RgbArgs* rgb,
                 const float* post_s, void* stream, int* partial_splits = nullptr) {
    // partial_splits != NULL (modes 0 .. 3, the low-resolution entries): the convolution leaves its split-K slabs (one slab when K is not
    // split) in ws and the caller reduces them; *partial_splits receives the slab count
    if (!x || !wp || !y || batch <= 0 || cin <= 0 || cout <= 0 || h <= 0 || w <= 0) return MAUA_EINVAL;
    if (partial_splits && (up > 3 || rgb || !ws)) return MAUA_EINVAL;
    // the style fold (include/maua_hip.h): s == NULL = x arrives multiplied by this layer's styles — the 2-D Winograd and the F(2,2)^2
    // transposed kernels have instances without the multiply; post_s = the consumer's styles, applied to the stored map by the
    // 2-D Winograd kernels' epilogue
    if ((!s && up != 5 && up != 6) || (post_s && up != 5)) return MAUA_ENOSYS;
    if (int rc = tail.check(fuse_act != 0)) return rc;  // (without fuse_act a frame source's noise is not read: its weight may be absent)
    if (up == 5)  // 2-D Winograd F(2x4, 3x3), modconv_w2d.hip
        return maua_w2d_launch(x, wp, s, s_stride, d, y, batch, cin, cout, h, w, wscale, fuse_act, tail, rgb, post_s, stream);
    if (up == 7 || up == 8) {  // plain (7) / transposed (8) conv with split-bf16 products (side measurement), modconv_sbf16.hip
        if (rgb) return MAUA_ENOSYS;
        return maua_sbf16_launch(x, wp, s, s_stride, d, y, ws, batch, cin, cout, h, w, up == 8, wscale, fuse_act, tail, stream);
    }
    if (up == 6) {  // transposed conv, F(2,2) on both axes, modconv_up2d.hip: raw output only (the blur kernel applies the tail)
        if (fuse_act || rgb) return MAUA_EINVAL;
        return maua_up2d_launch(x, wp, s, s_stride, d, y, ws, batch, cin, cout, h, w, wscale, stream);
    }
    if (up < 0 || up > 4) return MAUA_EINVAL;
    if (up == 4 && (fuse_act || rgb)) return MAUA_EINVAL;  // raw output only: the blur kernel applies the tail
    Plan pl = make_plan(batch, cin, cout, h, w, up);
    if (pl.rc) return pl.rc;  // the shape's own refusals (width rules, 2^31 elements, no tile for its patch) and a key without instance
    if (pl.g.splits > 1 && !ws) return MAUA_EINVAL;
    pl.g.force_ws = partial_splits ? 1 : 0;
    pl.g.s_stride = s_stride;
    pl.g.wscale = wscale;
    pl.g.fuse_act = fuse_act;
    pl.g.noise_batch_stride = tail.noise_batch_stride;
#ifdef MAUA_EXPERIMENTS
    pl.g.debug = g_conv_debug;
#endif
    pl.g.rgb = 0;
    pl.g.rgb_wscale = 0.f;
    ConvPtrs ptrs{x, wp, s, d, tail.noise, tail.noise_w, tail.bias, y, ws, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, tail.src, tail.noise_slot};
    if (rgb) {
        // fusable only when one workgroup holds every channel of its pixels in a single wave row (BM >= Cout, WM == 1),
        // no split-K, one image per tile, the tail fused
        const bool ok = up != 1 && up != 4 && fuse_act && pl.key.wm == 1 && pl.g.m_tiles == 1 && pl.g.splits == 1 && pl.g.lni == 0 &&
                        rgb->w && rgb->s && rgb->bias && (rgb->out || rgb->u8) && (!rgb->skip || (rgb->k4 && !(h & 1) && !(w & 1)));
        if (!ok) return MAUA_ENOSYS;
        pl.g.rgb = rgb->mode;
        pl.g.rgb_wscale = rgb->wscale;
        ptrs.rgb_w = rgb->w, ptrs.rgb_s = rgb->s, ptrs.rgb_bias = rgb->bias, ptrs.rgb_skip = rgb->skip;
        ptrs.rgb_k4 = rgb->k4, ptrs.rgb_out = rgb->out, ptrs.rgb_u8 = rgb->u8;
    }
    hipStream_t st = (hipStream_t)stream;
    if (int rc = pl.inst->launch(pl.inst->name, pl.blocks, pl.lds_bytes, st, pl.g, ptrs)) return rc;
    if (partial_splits) {
        *partial_splits = pl.g.splits;
        return 0;
    }
    if (pl.g.splits > 1) {
        const int64_t total = pl.g.ws_slab;
        hipLaunchKernelGGL(reduce_tail_kernel, dim3(pack_grid(total, 2048)), dim3(256), 0, st, ws,
                           pl.g.splits, pl.g.ws_slab, y, d, tail.noise, tail.noise_batch_stride, tail.noise_w, tail.bias, fuse_act, cout,
                           (int64_t)pl.g.OH * pl.g.OW, total, tail.src, tail.noise_slot);
        MAUA_LAUNCH_CHECK();
    }
    return 0;
}
}  // namespace

extern "C" int maua_modconv3x3_f32(const float* x, const float* wp, const float* s, int s_stride, const float* d,
                                   float* y, int batch, int cin, int cout, int h, int w, int up, float wscale,
                                   int fuse_act, const float* noise, int64_t noise_batch_stride, const float* noise_w,
                                   const float* bias, float* ws, const maua_frame_source_t* src, int noise_slot, void* stream) {
    const TailArgs tail{noise, noise_w, bias, noise_batch_stride, src, noise_slot};
    return modconv_impl(x, wp, s, s_stride, d, y, batch, cin, cout, h, w, up, wscale, fuse_act, tail, ws, nullptr, nullptr, stream);
}

// ---- low-resolution entries: convolution (modes 0 / 1) + the fused reducers above
extern "C" int maua_lowres_ok(int cin, int cout, int h, int w, int up) {
    if (cin <= 0 || cout <= 0 || h <= 0 || w <= 0 || (up != 0 && up != 1 && up != 2 && up != 3 && up != 6)) return 0;
    if (up == 6) return 4 * h * w <= 1024 && maua_up2d16_ok(cin, cout, h, w);  // the F(2,2)^2 kernel's 16-column tiles (modconv_up2d.hip)
    if (up == 1) return 4 * h * w <= 1024;                              // reduce_blur_tail_kernel: at most four outputs per thread
    if ((up == 2 && (w & 1)) || (up == 3 && (w & 3))) return 0;         // plain layer through Winograd F(2,3) / F(4,3) along x
    return cout % 32 == 0 && (h * w) % 16 == 0 && h * w <= 1024;        // reduce_tail_rgbpart_kernel: 32-channel groups, 16 / 32-pixel tiles
}

extern "C" int64_t maua_lowres_ws_floats(int batch, int cin, int cout, int h, int w, int up) {
    if (batch <= 0 || !maua_lowres_ok(cin, cout, h, w, up)) return 0;
    if (up == 6)  // slabs + the exported last input column
        return (int64_t)maua_up2d16_splits(batch, cin, cout, h, w) * batch * cout * (2 * h + 1) * (2 * w + 1) + maua_up2d_ws_floats(batch, cin, h);
    Plan pl = make_plan(batch, cin, cout, h, w, up);
    return pl.g.ws_slab * pl.g.splits;
}

extern "C" int maua_upconv_blur_lowres_f32(const float* x, const float* wp, const float* s, int s_stride, const float* d, float* y, float* ws,
                                           const float* k4, const float* noise, int64_t noise_batch_stride, const float* noise_w,
                                           const float* bias, const maua_frame_source_t* src, int noise_slot, int batch, int cin, int cout,
                                           int h, int w, int up, float wscale, const float* post_s, void* stream) {
    if (!x || !wp || !s || !y || !ws || !k4 || batch <= 0 || (up != 1 && up != 6)) return MAUA_EINVAL;
    if (!maua_lowres_ok(cin, cout, h, w, up)) return MAUA_ENOSYS;
    const TailArgs tail{noise, noise_w, bias, noise_batch_stride, src, noise_slot};
    if (int rc = tail.check()) return rc;
    int splits = 0;
    const int64_t slab = (int64_t)batch * cout * (2 * h + 1) * (2 * w + 1);
    if (up == 6) {  // F(2,2) on both axes (wp = maua_pack_weight_up2d_f32), K split over workgroups; the exported column behind the slabs
        float* xcol = ws + (int64_t)maua_up2d16_splits(batch, cin, cout, h, w) * slab;
        if (int rc = maua_up2d16_launch(x, wp, s, s_stride, ws, xcol, batch, cin, cout, h, w, wscale, &splits, stream)) return rc;
    } else if (int rc = modconv_impl(x, wp, s, s_stride, nullptr, y, batch, cin, cout, h, w, 1, wscale, 0, TailArgs{}, ws, nullptr, nullptr, stream,
                                     &splits))  // (the convolution writes slabs only: y is a placeholder)
        return rc;
    const size_t lds = (size_t)(2 * h + 3) * (2 * w + 3) * sizeof(float);
    hipLaunchKernelGGL(reduce_blur_tail_kernel, dim3((unsigned)(batch * cout)), dim3(256), lds, (hipStream_t)stream, ws, splits, slab, y, d, k4,
                       noise, noise_batch_stride, noise_w, bias, post_s, s_stride, cout, h, w, src, noise_slot, up == 6 ? 1 : 0);
    MAUA_LAUNCH_CHECK();
    return 0;
}

extern "C" int maua_styledconv_rgbpart_lowres_f32(const float* x, const float* wp, const float* s, int s_stride, const float* d, float* y,
                                                  float* ws, const float* noise, int64_t noise_batch_stride, const float* noise_w,
                                                  const float* bias, const float* rgb_w, const float* rgb_s, float rgb_wscale,
                                                  float* rgb_partial, const maua_frame_source_t* src, int noise_slot, int batch, int cin,
                                                  int cout, int h, int w, int mode, float wscale, void* stream) {
    if (!x || !wp || !s || !y || !ws || !rgb_w || !rgb_s || !rgb_partial || batch <= 0 || (mode != 0 && mode != 2 && mode != 3)) return MAUA_EINVAL;
    if (!maua_lowres_ok(cin, cout, h, w, mode)) return MAUA_ENOSYS;
    const TailArgs tail{noise, noise_w, bias, noise_batch_stride, src, noise_slot};
    if (int rc = tail.check()) return rc;
    int splits = 0;
    if (int rc = modconv_impl(x, wp, s, s_stride, nullptr, y, batch, cin, cout, h, w, mode, wscale, 0, TailArgs{}, ws, nullptr, nullptr, stream, &splits))
        return rc;
    const int64_t slab = (int64_t)batch * cout * h * w;
    const int pt = (h * w) % 32 == 0 ? 32 : 16;
    const int64_t blocks = (int64_t)batch * (cout / 32) * (h * w / pt);
    if (pt == 32)
        hipLaunchKernelGGL(reduce_tail_rgbpart_kernel<32>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ws, splits, slab, y, d, noise,
                           noise_batch_stride, noise_w, bias, rgb_w, rgb_s, s_stride, rgb_wscale, rgb_partial, cout, h * w, src, noise_slot);
    else
        hipLaunchKernelGGL(reduce_tail_rgbpart_kernel<16>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ws, splits, slab, y, d, noise,
                           noise_batch_stride, noise_w, bias, rgb_w, rgb_s, s_stride, rgb_wscale, rgb_partial, cout, h * w, src, noise_slot);
    MAUA_LAUNCH_CHECK();
    return 0;
}

extern "C" int maua_styledconv_torgb_partial_f32(const float* x, const float* wp, const float* s, int s_stride, const float* d,
                                                 float* y, int batch, int cin, int cout, int h, int w, int mode, float wscale,
                                                 const float* noise, int64_t noise_batch_stride, const float* noise_w,
                                                 const float* bias, const float* rgb_w, const float* rgb_s, float rgb_wscale,
                                                 float* rgb_partial, const maua_frame_source_t* src, int noise_slot,
                                                 const float* post_s, void* stream) {
    if (mode != 5) return MAUA_ENOSYS;  // only the 2-D Winograd kernel leaves partial ToRGB sums
    if (!x || !wp || !y || batch <= 0 || cin <= 0 || cout <= 0 || h <= 0 || w <= 0) return MAUA_EINVAL;
    const TailArgs tail{noise, noise_w, bias, noise_batch_stride, src, noise_slot};
    if (int rc = tail.check()) return rc;
    const RgbArgs rgb{rgb_w, rgb_s, nullptr, nullptr, nullptr, rgb_partial, nullptr, rgb_wscale, 3};
    return maua_w2d_launch(x, wp, s, s_stride, d, y, batch, cin, cout, h, w, wscale, 1, tail, &rgb, post_s, stream);
}

extern "C" int maua_styledconv_torgb_f32(const float* x, const float* wp, const float* s, int s_stride, const float* d,
                                         float* y, int batch, int cin, int cout, int h, int w, int mode, float wscale,
                                         const float* noise, int64_t noise_batch_stride, const float* noise_w,
                                         const float* bias, const float* rgb_w, const float* rgb_s, float rgb_wscale,
                                         const float* rgb_bias, const float* rgb_skip, const float* rgb_k4, float* rgb_out,
                                         int store_features, uint8_t* frames_u8, const maua_frame_source_t* src, int noise_slot,
                                         const float* post_s, void* stream) {
    const TailArgs tail{noise, noise_w, bias, noise_batch_stride, src, noise_slot};
    const RgbArgs rgb{rgb_w, rgb_s, rgb_bias, rgb_skip, rgb_k4, rgb_out, frames_u8, rgb_wscale, store_features ? 1 : 2};
    if (mode == 1) return MAUA_ENOSYS;
    return modconv_impl(x, wp, s, s_stride, d, y, batch, cin, cout, h, w, mode, wscale, 1, tail, nullptr, &rgb, post_s, stream);
}
