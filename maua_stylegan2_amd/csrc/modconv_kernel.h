// The generic 3x3 modulated convolution kernel (design: the comment at the head of modconv.hip) and the macros that turn rows of
// template arguments into table entries.  Included by the instance units modconv_m0.hip .. modconv_m4.hip only, one per MODE: the
// host side (modconv.hip) sees modconv_plan.h and never this template.
#pragma once
#include "modconv_plan.h"
#include "conv_device.h"
#include "epilogue.h"

namespace {

// UP = false : plain 3x3, pad 1.           per wave: TM x TN MFMA tiles.
// UP = true  : stride-2 transposed 3x3.    per wave: TM x (TN position groups x 4 output parities).
// FAST (Cin a multiple of the K chunk and the padded weight covers whole BM tiles — every layer of a real generator): both
// operands come in by LDS DMA (or, on the register-staged patch path, by unconditional loads masked by multiplication at
// LDS-write time), addressed as uniform base + 32-bit lane offset, which removes the exec-mask / 64-bit-address scalar work
// that dominated the short-K (32/64-channel) layers.  Everything else (ragged channel counts) takes the generic path.
// MODE 2 (WINO): plain 3x3 through Winograd F(2,3) along x — two adjacent output columns share four "frequency" products
//   m0 = (d0-d2) g0, m1 = (d1+d2)(g0+g1+g2)/2, m2 = (d2-d1)(g0-g1+g2)/2, m3 = (d1-d3) g2;  y0 = m0+m1+m2, y1 = m1-m2-m3
// so a pair of outputs costs 4 MFMA K-steps per (channel, ky) instead of 6: 1.5x fewer matrix-core cycles on the
// MFMA-bound >= 128-channel layers.  A "position" is an output PAIR; the four frequencies take the place of the four
// parities of the transposed mode (same accumulator layout), weights are pre-transformed (pack_weight_wino_kernel),
// the B operand is formed from two 8-byte LDS reads of the ordinary patch, the epilogue undoes the transform in
// registers and stores 8 bytes per lane.  fp32 F(2,3) has transform constants {1, 1/2}: error stays at the 1e-6 level.
// MODE 3 / MODE 4: see the comments at their mfma_chunk branches (F(4,3) on output quads; transposed conv with F(2,2)).
template <int BM, int BN, int WM, int MODE, bool MULTI, bool FAST, int MAXP>
__global__ __launch_bounds__(256, ((MODE == 3 && BM >= 64) || MODE == 4) ? 2
                                            : ((BM / WM / 32) * (BN / (4 / WM) / 32) * (MODE ? 4 : 1) >= 8 || BM * BN > 8192 ? 2 : 3))
void modconv_mfma_kernel(ConvGeom g, ConvPtrs p) {
    constexpr bool UP = MODE == 1 || MODE == 4;
    constexpr bool UW = MODE == 4;  // transposed conv with Winograd F(2,2) on the even x-phase: positions are position PAIRS
    constexpr bool W23 = MODE == 2;             // Winograd F(2,3): positions are output pairs, 4 frequencies
    constexpr bool W43 = MODE == 3;             // Winograd F(4,3): positions are output quads, 6 frequencies
    constexpr bool WINO = W23 || W43;
    constexpr int WX = W43 ? 4 : ((W23 || UW) ? 2 : 1);  // patch columns advanced per position
    constexpr int NFREQ = W43 ? 6 : 4;
    constexpr int NTAPS = WINO ? 3 * NFREQ : (UW ? 12 : 9);  // weight rows per channel: 9 taps, or 3 ky x NFREQ frequencies
    constexpr int CC = chunk_channels(BM, BN, MODE);
    constexpr int WN = 4 / WM;
    constexpr int TM = BM / WM / 32;
    constexpr int TN = BN / WN / 32;
    constexpr int NPH = UW ? 10 : (UP ? 4 : (WINO ? NFREQ : 1));
    constexpr int A_FLOATS = NTAPS * CC * BM;
    constexpr int A_VEC_ITERS = (A_FLOATS / 4 + 255) / 256;
    constexpr int MAX_POS = MAXP;  // patch positions per thread (PSTRIDE <= 256 * MAX_POS)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // LDS: As[2][A_FLOATS] | Ps[2][CC * PSTRIDE]   (the generic path only uses buffer 0 of each)
    float* As = lds;
    float* Ps = lds + 2 * A_FLOATS;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: everything derived from it stays in SGPRs
    const int l31 = lane & 31, hi = lane >> 5;
    const int wm = wave % WM, wn = wave / WM;

    // ---- which tile
    int t = xcd_remap(blockIdx.x, gridDim.x);
    const int nt_id = t % g.n_tiles;
    t /= g.n_tiles;
    const int mt_id = t % g.m_tiles;
    const int split = t / g.m_tiles;
    int r = nt_id;
    const int tile_x = r % g.tiles_x;
    r /= g.tiles_x;
    const int tile_y = r % g.tiles_y;
    const int img_group = r / g.tiles_y;

    const int SW = 1 << g.lsw, SH = 1 << g.lsh;
    const int TWd = SW << g.lnsx, THt = SH << g.lnsy;
    const int NI = 1 << g.lni;
    const int ty0 = tile_y * THt, tx0 = tile_x * TWd, b0 = img_group * NI;
    const int m0 = mt_id * BM;
    const size_t plane_in = (size_t)g.H * g.W;

    // ---- per-thread patch positions (decoded once)
    int src_off[MAX_POS];    // offset of (b, ch 0, y, x) in x; -1 (slow path) / 0 (FAST) when outside the image
    float src_mask[MAX_POS]; // 1 inside the image, 0 outside (FAST path multiplies instead of branching)
    int sb_off[MAX_POS];     // b * s_stride
#pragma unroll
    for (int i = 0; i < MAX_POS; ++i) {
        const int pp = tid + i * 256;
        src_off[i] = FAST ? 0 : -1;
        src_mask[i] = 0.f;
        sb_off[i] = 0;
        if (pp < g.PSTRIDE) {
            const int per_img = g.PH * g.PWS;
            const int img = pp / per_img;
            const int rem = pp - img * per_img;
            const int pr = rem / g.PWS, pc = rem - pr * g.PWS;
            const int b = b0 + img;
            int yy = ty0 + pr - 1, xx = WX * tx0 + pc - 1;
            if (UP && g.flat) {
                // flat run: patch row 1 holds positions p0-1 .. p0+BN-1 of the pitch-(W+1) flattened input (column W and
                // row H are the zero padding), patch row 0 the same run one input row up (p - GW)
                // (UW: g.GW counts position pairs per row, the flattened input pitch is 2 * g.GW = W + 2)
                const int pitch = UW ? 2 * g.GW : g.GW;
                const int fi = WX * tx0 + pc - 1 - (1 - pr) * pitch;
                yy = fi >= 0 ? fi / pitch : -1;
                xx = fi - yy * pitch;
            }
            if (pc < g.PW && img < NI && b < g.B && yy >= 0 && yy < g.H && xx >= 0 && xx < g.W) {
                src_off[i] = ((b * g.Cin * g.H + yy) * g.W + xx);  // < 2^31: checked on the host
                src_mask[i] = 1.f;
                sb_off[i] = b * g.s_stride;
            }
        }
    }

    if (MAUA_DBG(128)) {
#pragma unroll
        for (int i = 0; i < MAX_POS; ++i) src_off[i] = src_off[i] < 0 ? src_off[i] : (src_off[i] & 0x3ff);
    }

    // ---- per-lane B-fragment base offsets (top-left of the 3x3 window of this lane's pixel, channel parity hi)
    int boff[TN];
#pragma unroll
    for (int n = 0; n < TN; ++n) {
        const int sub = wn * TN + n;
        const int jx = l31 & (SW - 1), jy = l31 >> g.lsw;
        const int sx = sub & ((1 << g.lnsx) - 1);
        const int sy = (sub >> g.lnsx) & ((1 << g.lnsy) - 1);
        const int img = sub >> (g.lnsx + g.lnsy);
        const int tyy = sy * SH + jy, txx = sx * SW + jx;
        boff[n] = hi * g.PSTRIDE + (img * g.PH + tyy) * g.PWS + WX * txx;
    }
    const int aoff = hi * BM + wm * (TM * 32) + l31;
    const int aoff2 = hi * BM + wm * (TM * 32) + 2 * l31;  // interleaved [lane][mt] layout of the Winograd weight packs

    f32x16 acc[TM][TN * NPH];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int n = 0; n < TN * NPH; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][n][e] = 0.f;

    const int chunk_begin = split * g.chunks_per_split;
    int chunk_end = chunk_begin + g.chunks_per_split;
    if (chunk_end > g.n_chunks) chunk_end = g.n_chunks;

    // Software pipeline (issue-early / write-late): the global loads of chunk c+1 are issued right after the barrier
    // that publishes chunk c and stay in flight underneath chunk c's 36*TM*TN*NPH' MFMAs; they are only waited for
    // when their registers are written to LDS at the top of the next iteration.
    f32x4 av[A_VEC_ITERS];
    float pv[MAX_POS][CC];
    constexpr bool one_image = !MULTI;  // every patch position belongs to image b0: styles are block-uniform
    auto issue_loads = [&](int chunk) {  // generic path only (the FAST path below has its own DMA pipeline)
        const int c0 = chunk * CC;
        {
#pragma unroll
        for (int it = 0; it < A_VEC_ITERS; ++it) {
            const int f = tid + it * 256;  // float4 index in As
            const int row = f / (BM / 4);  // tap*CC + c
            const int col = (f - row * (BM / 4)) * 4;
            const int tap = row / CC, c = row - tap * CC;
            const int ch = c0 + c, o = m0 + col;
            av[it] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (WINO && TM == 2 && g.CoutPad < 64) {
                // A layer of <= 32 channels on a two-M-tile config (the fallback plan of a map too flat or too narrow for the 32-row
                // tile's patch): its pack has 32 plain columns (wino_cout_pad), while the A reads below expect the [lane][m-tile]
                // interleave.  Interleave here: tile column 2 l holds channel l, the odd columns (m-tile 1) are padding.
                if (f < A_FLOATS / 4 && ch < g.Cin && col < 64) {
                    const float* rowp = p.wp + ((size_t)tap * g.Cin + ch) * g.CoutPad;
                    av[it] = f32x4{rowp[col >> 1], 0.f, rowp[(col >> 1) + 1], 0.f};
                }
            } else if (f < A_FLOATS / 4 && ch < g.Cin && o < g.CoutPad) {
                av[it] = *reinterpret_cast<const f32x4*>(p.wp + ((size_t)tap * g.Cin + ch) * g.CoutPad + o);
            }
        }
#pragma unroll
        for (int i = 0; i < MAX_POS; ++i)
#pragma unroll
            for (int c = 0; c < CC; ++c) {
                const int ch = c0 + c;
                float v = 0.f;
                if (src_off[i] >= 0 && ch < g.Cin) {
                    v = p.x[(size_t)src_off[i] + ch * plane_in];
                    if (!one_image) v *= p.s[sb_off[i] + ch];
                }
                pv[i][c] = v;
            }
        }
    };
    auto write_lds = [&](int chunk) {
        const int c0 = chunk * CC;
        float sc[CC];
#pragma unroll
        for (int c = 0; c < CC; ++c)  // uniform address -> scalar loads
            sc[c] = (one_image && c0 + c < g.Cin && b0 < g.B) ? p.s[b0 * g.s_stride + c0 + c] : 1.f;
#pragma unroll
        for (int it = 0; it < A_VEC_ITERS; ++it) {
            const int f = tid + it * 256;
            if (f < A_FLOATS / 4) reinterpret_cast<f32x4*>(As)[f] = av[it];
        }
#pragma unroll
        for (int i = 0; i < MAX_POS; ++i) {
            const int pp = tid + i * 256;
            if (pp < g.PSTRIDE) {
#pragma unroll
                for (int c = 0; c < CC; ++c) Ps[c * g.PSTRIDE + pp] = pv[i][c] * sc[c];
            }
        }
    };

    // ---- MFMA phase over one staged chunk
    // Sc != nullptr: the staged patch holds RAW features (DMA path) and the style of channel 2q+hi is applied to the B
    // operand here, one VALU multiply per operand next to a 64-cycle MFMA.
    auto mfma_chunk = [&](const float* __restrict__ Ac, const float* __restrict__ Pc, const float* __restrict__ Sc) {
        if (UW) {
            // Polyphase transposed conv, x direction through F(2,2): for the position pair (p, p+1) with inputs
            // d0 = x[p-1], d1 = x[p], d2 = x[p+1] of one input row and the kernel row (g0, g1, g2):
            //   even columns  e_p = g0 d1 + g2 d0,  e_p+1 = g0 d2 + g2 d1   =  (m0 + m1, m1 + m2) with
            //                 m0 = g2 (d0 - d1),  m1 = (g0 + g2) d1,  m2 = g0 (d2 - d1)            (3 products instead of 4)
            //   odd columns   o_p = g1 d1,  o_p+1 = g1 d2
            // 5 MFMA K-steps per (kernel row, channel pair) instead of 6.  Kernel row 0 / 1 read input row y (output row
            // parity 0 / 1), kernel row 2 reads input row y-1 (parity 0): accumulator slots [parity][m0, m1, m2, o_p, o_p+1].
            // Weight rows per kernel row (maua_pack_weight_upwino_f32): g2, g0 + g2, g0, g1.
#pragma unroll
            for (int q = 0; q < CC / 2; ++q) {
                float tb[2][TN][4];  // [patch row][n][d0-d1, d1, d2-d1, d2]
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int n = 0; n < TN; ++n) {
                        const float* dp = Pc + 2 * q * g.PSTRIDE + boff[n] + r * g.PWS;  // even float offset
                        const f32x2 d01 = *reinterpret_cast<const f32x2*>(dp);
                        const float d2 = dp[2];
                        tb[r][n][0] = d01.x - d01.y;
                        tb[r][n][1] = d01.y;
                        tb[r][n][2] = d2 - d01.y;
                        tb[r][n][3] = d2;
                        if (Sc) {
                            const float sc = Sc[2 * q + hi];
#pragma unroll
                            for (int k = 0; k < 4; ++k) tb[r][n][k] *= sc;
                        }
                    }
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    const int r = ky == 2 ? 0 : 1;       // patch row: 1 = input row y, 0 = input row y-1
                    const int base = ky == 1 ? 5 : 0;    // accumulator slots of the output-row parity
#pragma unroll
                    for (int j = 0; j < 5; ++j) {
                        const int wrow = j < 3 ? j : 3;              // weight row within the kernel row
                        const int bk = j < 3 ? j : (j == 3 ? 1 : 3);  // which transformed input
                        float a[TM];
#pragma unroll
                        for (int mt = 0; mt < TM; ++mt) a[mt] = Ac[((ky * 4 + wrow) * CC + 2 * q) * BM + mt * 32 + aoff];
#pragma unroll
                        for (int mt = 0; mt < TM; ++mt)
#pragma unroll
                            for (int n = 0; n < TN; ++n)
                                acc[mt][n * NPH + base + j] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                                    a[mt], tb[r][n][bk], acc[mt][n * NPH + base + j], 0, 0, 0);
                    }
                }
            }
            return;
        }
        if (W43) {
            // B^T d for F(4,3) (interpolation points 0, +-1, +-2, inf) on six consecutive patch floats:
            //   t0 = 4 d0 - 5 d2 + d4          t1 = (d4 - 4 d2) + (d3 - 4 d1)     t2 = (d4 - 4 d2) - (d3 - 4 d1)
            //   t5 = 4 d1 - 5 d3 + d5          t3 = (d4 - d2) + 2 (d3 - d1)       t4 = (d4 - d2) - 2 (d3 - d1)
            // Explicit software pipeline over the (ky, channel pair) groups of a chunk.  A naive schedule starts every group
            // with "B reads -> wait -> 13 VALU -> first MFMA" and every frequency with "A read -> wait -> MFMA": two LDS round
            // trips and ~80 VALU cycles with at most two MFMAs (128 cycles) in flight (profiles/r01_isa_modconv.md).  Here the
            // raw window of group g+1 is read under the first MFMAs of group g, transformed under its middle ones, and the
            // weight row of the next frequency is read one step ahead; sched_barrier(0) pins that order.  Measured against the
            // naive schedule (profiles/r02_ab_variants.md): -5..8 % per launch on the 64..512-channel layers.
            constexpr int NG = 3 * (CC / 2);
            float bvp[2][TN][6];
            f32x2 raw[TN][3];
            auto read_raw = [&](int gq) {
                const int ky = gq / (CC / 2), q = gq % (CC / 2);
#pragma unroll
                for (int n = 0; n < TN; ++n) {
                    const float* dp = Pc + 2 * q * g.PSTRIDE + boff[n] + ky * g.PWS;
                    raw[n][0] = *reinterpret_cast<const f32x2*>(dp);
                    raw[n][1] = *reinterpret_cast<const f32x2*>(dp + 2);
                    raw[n][2] = *reinterpret_cast<const f32x2*>(dp + 4);
                }
            };
            auto transform = [&](int gq, float (&bv)[TN][6]) {
                const int q = gq % (CC / 2);
#pragma unroll
                for (int n = 0; n < TN; ++n) {
                    const f32x2 d01 = raw[n][0], d23 = raw[n][1], d45 = raw[n][2];
                    float a_ = fmaf(-4.f, d23.x, d45.x);
                    asm volatile("" : "+v"(a_));
                    const float b_ = fmaf(-4.f, d01.y, d23.y);
                    const float c_ = d45.x - d23.x, e_ = d23.y - d01.y;
                    bv[n][0] = fmaf(4.f, d01.x, fmaf(-5.f, d23.x, d45.x));
                    bv[n][1] = a_ + b_;
                    bv[n][2] = a_ - b_;
                    bv[n][3] = fmaf(2.f, e_, c_);
                    bv[n][4] = fmaf(-2.f, e_, c_);
                    bv[n][5] = fmaf(4.f, d01.y, fmaf(-5.f, d23.y, d45.y));
                    if (Sc) {
                        const float sc = Sc[2 * q + hi];
#pragma unroll
                        for (int k = 0; k < 6; ++k) bv[n][k] *= sc;
                    }
                }
            };
            auto read_a = [&](int step, float (&a)[TM]) {  // step = gq * 6 + xi
                const int gq = step / 6, xi = step % 6;
                const int ky = gq / (CC / 2), q = gq % (CC / 2);
                if (TM == 2) {
                    const f32x2 a2 = *reinterpret_cast<const f32x2*>(Ac + ((ky * 6 + xi) * CC + 2 * q) * BM + aoff2);
                    a[0] = a2.x, a[TM - 1] = a2.y;
                } else {
#pragma unroll
                    for (int mt = 0; mt < TM; ++mt) a[mt] = Ac[((ky * 6 + xi) * CC + 2 * q) * BM + mt * 32 + aoff];
                }
            };
            float a_cur[TM], a_nxt[TM];
            read_raw(0);
            read_a(0, a_cur);
            transform(0, bvp[0]);
#pragma unroll
            for (int gq = 0; gq < NG; ++gq) {
                const int ky = gq / (CC / 2);
                (void)ky;
#pragma unroll
                for (int xi = 0; xi < 6; ++xi) {
                    const int step = gq * 6 + xi;
                    if (step + 1 < NG * 6) read_a(step + 1, a_nxt);
                    if (xi == 0 && gq + 1 < NG) read_raw(gq + 1);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int mt = 0; mt < TM; ++mt)
#pragma unroll
                        for (int n = 0; n < TN; ++n)
                            acc[mt][n * NPH + xi] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[mt], bvp[gq & 1][n][xi],
                                                                                         acc[mt][n * NPH + xi], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    if (xi == 2 && gq + 1 < NG) {
                        transform(gq + 1, bvp[(gq + 1) & 1]);
                        __builtin_amdgcn_sched_barrier(0);
                    }
#pragma unroll
                    for (int mt = 0; mt < TM; ++mt) a_cur[mt] = a_nxt[mt];
                }
            }
            return;
        }
        if (W23) {
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
                for (int q = 0; q < CC / 2; ++q) {
                    float bv[TN][4];
#pragma unroll
                    for (int n = 0; n < TN; ++n) {
                        const float* dp = Pc + 2 * q * g.PSTRIDE + boff[n] + ky * g.PWS;  // even float offset: 8-byte aligned
                        const f32x2 d01 = *reinterpret_cast<const f32x2*>(dp);
                        const f32x2 d23 = *reinterpret_cast<const f32x2*>(dp + 2);
                        bv[n][0] = d01.x - d23.x;
                        bv[n][1] = d01.y + d23.x;
                        bv[n][2] = d23.x - d01.y;
                        bv[n][3] = d01.y - d23.y;
                        if (Sc) {
                            const float sc = Sc[2 * q + hi];
#pragma unroll
                            for (int k = 0; k < 4; ++k) bv[n][k] *= sc;
                        }
                    }
#pragma unroll
                    for (int xi = 0; xi < 4; ++xi) {
                        float a[TM];
                        if (TM == 2) {  // weight rows are packed [lane][mt] per 64 output channels: one 8-byte read, immediate offset
                            const f32x2 a2 = *reinterpret_cast<const f32x2*>(Ac + ((ky * 4 + xi) * CC + 2 * q) * BM + aoff2);
                            a[0] = a2.x, a[TM - 1] = a2.y;
                        } else {
#pragma unroll
                            for (int mt = 0; mt < TM; ++mt) a[mt] = Ac[((ky * 4 + xi) * CC + 2 * q) * BM + mt * 32 + aoff];
                        }
#pragma unroll
                        for (int mt = 0; mt < TM; ++mt)
#pragma unroll
                            for (int n = 0; n < TN; ++n)
                                acc[mt][n * NPH + xi] =
                                    __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt], bv[n][xi], acc[mt][n * NPH + xi], 0, 0, 0);
                    }
                }
            }
            return;
        }
        {
            // direct / polyphase branch: one-step look-ahead of both operands over the 9 x CC/2 (tap, channel pair) steps; the
            // style multiply of the next B operand runs behind the current MFMAs (-5..7 % on the 512-channel layers).
            constexpr int NS = 9 * (CC / 2);
            float a_c[TM], b_c[TN], a_n[TM], b_n[TN];
            auto fetch = [&](int st, float (&a)[TM], float (&b)[TN]) {
                const int tap = st / (CC / 2), q = st % (CC / 2);
                const int ky = tap / 3, kx = tap % 3;
                const int dy = UP ? (ky == 2 ? 0 : 1) : ky;
                const int dx = UP ? (kx == 2 ? 0 : 1) : kx;
                const int tapoff = dy * g.PWS + dx;
#pragma unroll
                for (int mt = 0; mt < TM; ++mt) a[mt] = Ac[(tap * CC + 2 * q) * BM + mt * 32 + aoff];
#pragma unroll
                for (int n = 0; n < TN; ++n) b[n] = Pc[2 * q * g.PSTRIDE + boff[n] + tapoff];
            };
            auto scale = [&](int st, float (&b)[TN]) {
                if (Sc) {
                    const float sc = Sc[2 * (st % (CC / 2)) + hi];
#pragma unroll
                    for (int n = 0; n < TN; ++n) b[n] *= sc;
                }
            };
            fetch(0, a_c, b_c);
            scale(0, b_c);
#pragma unroll
            for (int st = 0; st < NS; ++st) {
                const int tap = st / (CC / 2);
                const int ky = tap / 3, kx = tap % 3;
                const int ph = UP ? ((ky == 1 ? 2 : 0) + (kx == 1 ? 1 : 0)) : 0;
                if (st + 1 < NS) fetch(st + 1, a_n, b_n);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int mt = 0; mt < TM; ++mt)
#pragma unroll
                    for (int n = 0; n < TN; ++n)
                        acc[mt][n * NPH + ph] =
                            __builtin_amdgcn_mfma_f32_32x32x2f32(a_c[mt], b_c[n], acc[mt][n * NPH + ph], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (st + 1 < NS) scale(st + 1, b_n);
#pragma unroll
                for (int mt = 0; mt < TM; ++mt) a_c[mt] = a_n[mt];
#pragma unroll
                for (int n = 0; n < TN; ++n) b_c[n] = b_n[n];
            }
            return;
        }
    };

    if (FAST) {
        // Double-buffered pipeline, ONE barrier per chunk.  The weight tile goes HBM/L2 -> LDS by DMA
        // (global_load_lds, 1 KiB per wave instruction, no staging registers, no ds_write); the feature patch goes
        // through registers because it is scaled by the style and masked at the image border on the way in.
        constexpr int RPI = 256 / BM;              // weight rows (BM floats) per 1-KiB DMA instruction
        constexpr int LPR = 64 / RPI;              // lanes per row
        constexpr int A_INSTR = (NTAPS * CC + RPI - 1) / RPI;  // DMA instructions per tile (the last one may be partial)
        constexpr int A_PER_WAVE = (A_INSTR + 3) / 4;
        int a_goff[A_PER_WAVE];
#pragma unroll
        for (int k = 0; k < A_PER_WAVE; ++k) {
            const int row = (wave + 4 * k) * RPI + lane / LPR;
            const int col = (lane % LPR) * 4;
            const int tap = row / CC, c = row - tap * CC;
            a_goff[k] = row < NTAPS * CC ? (tap * g.Cin + c) * g.CoutPad + col : -1;  // -1: lane past the tile, masked off
        }
        // Both DMAs are MUBUF `buffer_load ... lds` through raw buffer descriptors: while a FLAT-encoded global_load_lds is
        // in flight the compiler's wait insertion treats the LGKM counter as out of order and turns EVERY LDS wait of the
        // chunk into lgkmcnt(0) (profiles/r01_isa_modconv.md); with the buffer form it emits partial counts, which is what
        // the look-ahead LDS reads of the pipelined MFMA phases need.
        const buffer_rsrc_t w_rsrc = raw_buffer(p.wp);
        auto issue_dma = [&](int chunk, int buf) {
            float* dst = As + buf * A_FLOATS;
#pragma unroll
            for (int k = 0; k < A_PER_WAVE; ++k) {
                const int i = wave + 4 * k;  // scalar
                constexpr bool RAGGED = (NTAPS * CC) % RPI != 0;  // only then can lanes of the last instruction be masked
                if (i < A_INSTR && (!RAGGED || a_goff[k] >= 0))
                    lds_dma16(w_rsrc, dst + i * 256, a_goff[k] * 4, (int)(((size_t)chunk * CC * g.CoutPad + m0) * 4));
            }
        };
        auto load_patch = [&](int chunk) {
            const int c0 = chunk * CC;
#pragma unroll
            for (int c = 0; c < CC; ++c) {
                const float* __restrict__ xbase = p.x + (size_t)(c0 + c) * plane_in;  // uniform
#pragma unroll
                for (int i = 0; i < MAX_POS; ++i)
                    if (i == 0 || tid + i * 256 < g.PSTRIDE) pv[i][c] = xbase[(unsigned)src_off[i]];
            }
            if (MULTI) {
#pragma unroll
                for (int i = 0; i < MAX_POS; ++i)
#pragma unroll
                    for (int c = 0; c < CC; ++c) pv[i][c] *= p.s[sb_off[i] + c0 + c];
            }
        };
        auto write_patch = [&](int chunk, int buf) {
            const int c0 = chunk * CC;
            float* Pd = Ps + buf * (CC * g.PSTRIDE);
            float sc[CC];
#pragma unroll
            for (int c = 0; c < CC; ++c) sc[c] = (one_image && b0 < g.B) ? p.s[b0 * g.s_stride + c0 + c] : 1.f;
#pragma unroll
            for (int i = 0; i < MAX_POS; ++i) {
                const int pp = tid + i * 256;
                if (pp < g.PSTRIDE) {
#pragma unroll
                    for (int c = 0; c < CC; ++c) Pd[c * g.PSTRIDE + pp] = pv[i][c] * (sc[c] * src_mask[i]);
                }
            }
        };
        int cur = 0;
        // measured (30-launch averages): -6..7 % on the transposed 64-row configs, -4 % on the transposed 32-row config,
        // -3 % on the 64/128-row Winograd configs, +1 % on the 32-channel 1024^2 Winograd layer (its features stream from
        // HBM; the register-staged patch tolerates that latency better), which keeps the register path
        constexpr bool PDMA = !MULTI && !(W23 && BM == 32);
        if (PDMA) {
            // Feature patch by DMA as well: raw features go L2/HBM -> LDS without staging registers or ds_write, double
            // buffered like the weight tile.  Out-of-image patch elements are never written: their lanes are masked out of
            // the DMA and their LDS slots are zeroed once by the owning thread.  The style scale moves to the B-operand read (mfma_chunk Sc).
            // (A three-deep patch ring with a two-chunk prefetch distance measured the same and was dropped.)
            const int PBUF = CC * g.PSTRIDE;
            float* Ss = Ps + 2 * PBUF;
            bool pvalid[MAX_POS];
#pragma unroll
            for (int i = 0; i < MAX_POS; ++i) {
                pvalid[i] = src_mask[i] != 0.f;
                const int pp = tid + i * 256;
                if (!pvalid[i] && pp < g.PSTRIDE) {  // border / padding element of this thread: zero in both buffers, for good
#pragma unroll
                    for (int c = 0; c < CC; ++c) Ps[c * g.PSTRIDE + pp] = 0.f, Ps[PBUF + c * g.PSTRIDE + pp] = 0.f;
                }
            }
            const int nK = (chunk_end - chunk_begin) * CC;
            for (int e = tid; e < nK; e += 256) Ss[e] = p.s[b0 * g.s_stride + chunk_begin * CC + e];
            // lane offsets relative to the image (bytes, < 4 MiB) on a scalar running channel pointer: the DMA address is
            // SGPR base + 32-bit VGPR offset, two scalar adds per channel
            unsigned rel_bytes[MAX_POS];
#pragma unroll
            for (int i = 0; i < MAX_POS; ++i)
                rel_bytes[i] = pvalid[i] ? (unsigned)(src_off[i] - b0 * g.Cin * (int)plane_in) * 4u : 0u;
            const char* ximg = reinterpret_cast<const char*>(p.x + (size_t)b0 * g.Cin * plane_in);
            const size_t plane_bytes = plane_in * sizeof(float);
            (void)plane_bytes;  // (its one use is the device pass's 4-byte DMA below)
            // one image's features (Cin planes, < 2 GiB: checked on the host) behind a raw buffer descriptor
            const buffer_rsrc_t x_rsrc = raw_buffer(ximg);
            auto issue_patch = [&](int chunk, int buf) {
                float* dst = Ps + buf * PBUF + wave * 64;
                (void)dst;
#pragma unroll
                for (int c = 0; c < CC; ++c) {
#pragma unroll
                    for (int i = 0; i < MAX_POS; ++i)
                        if (pvalid[i]) {
#ifdef MAUA_DEVICE_PASS
                            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                                x_rsrc, (__attribute__((address_space(3))) void*)(dst + c * g.PSTRIDE + i * 256), 4,
                                (int)rel_bytes[i], (int)((size_t)(chunk * CC + c) * plane_bytes), 0, 0);
#endif
                        }
                }
            };
            if (chunk_begin < chunk_end) {
                issue_dma(chunk_begin, 0);
                issue_patch(chunk_begin, 0);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            for (int chunk = chunk_begin; chunk < chunk_end; ++chunk) {
                if (chunk + 1 < chunk_end) {
                    if (!MAUA_DBG(32)) issue_dma(chunk + 1, cur ^ 1);
                    if (!MAUA_DBG(64)) issue_patch(chunk + 1, cur ^ 1);
                }
                if (!MAUA_DBG(2)) mfma_chunk(As + cur * A_FLOATS, Ps + cur * PBUF, Ss + (chunk - chunk_begin) * CC);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                cur ^= 1;
            }
        } else {
        if (chunk_begin < chunk_end) {
            issue_dma(chunk_begin, 0);
            load_patch(chunk_begin);
            write_patch(chunk_begin, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int chunk = chunk_begin; chunk < chunk_end; ++chunk) {
            const bool more = chunk + 1 < chunk_end;
            if (more && !MAUA_DBG(4)) {
                if (!MAUA_DBG(32)) issue_dma(chunk + 1, cur ^ 1);
                if (!MAUA_DBG(64)) load_patch(chunk + 1);
            }
            if (!MAUA_DBG(2)) mfma_chunk(As + cur * A_FLOATS, Ps + cur * (CC * g.PSTRIDE), nullptr);
            if (more && !MAUA_DBG(4 | 64)) write_patch(chunk + 1, cur ^ 1);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            cur ^= 1;
        }
        }
    } else {
    if (chunk_begin < chunk_end) issue_loads(chunk_begin);
    for (int chunk = chunk_begin; chunk < chunk_end; ++chunk) {
        write_lds(chunk);
        __syncthreads();
        if (chunk + 1 < chunk_end) issue_loads(chunk + 1);

        mfma_chunk(As, Ps, nullptr);
        __syncthreads();
    }
    }

    // ---- epilogue
    // Per-channel epilogue operands (wscale * demod, bias) go through LDS: fetched once per workgroup with all loads in
    // flight together.  (Loading them per accumulator element from global memory serialises ~64 dependent L2 round
    // trips behind the stores — that was ~45 % of the lifetime of a 32-channel 1024^2 workgroup.)
    const bool to_ws = g.splits > 1 || g.force_ws;
    float* outp = to_ws ? (p.ws + (size_t)split * g.ws_slab) : p.y;
    const float* noise_base = p.noise;
    int64_t noise_bstride = g.noise_batch_stride;
    maua_noise_source(noise_base, noise_bstride, p.src, p.noise_slot);
    const float nw = (!to_ws && g.fuse_act && noise_base) ? p.noise_w[0] : 0.f;  // (scaled by act_gain where it is applied)
    const size_t plane_out = (size_t)g.OH * g.OW;
    float* Eg = lds;        // [BM] gain
    float* Eb = lds + BM;   // [BM] bias
    // leaky ReLU is positively homogeneous: its sqrt(2) gain is folded into gain, bias and noise once, and the activation
    // itself is max(t, 0.2 t) — 4 instead of 7 VALU operations per output value
    const float act_gain = (!to_ws && g.fuse_act) ? kSqrt2 : 1.f;
    if (!MULTI) {
        for (int i = tid; i < BM; i += 256) {
            const int o = m0 + i;
            float gain = g.wscale, bias = 0.f;
            if (!to_ws && o < g.Cout && b0 < g.B) {
                if (p.d) gain *= p.d[b0 * g.Cout + o];
                if (g.fuse_act && p.bias) bias = p.bias[o];
            }
            Eg[i] = gain * act_gain;
            Eb[i] = bias * act_gain;
            if (!UP && WM == 1 && g.rgb) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    lds[(2 + c) * BM + i] = (o < g.Cout && b0 < g.B)
                                                ? g.rgb_wscale * p.rgb_w[c * g.Cout + o] * p.rgb_s[b0 * g.s_stride + o]
                                                : 0.f;
            }
        }
        __syncthreads();
    }
    // every noise value this lane needs, fetched before the first store (loads cannot be hoisted above stores later)
    float nz_all[TN][NPH];
#pragma unroll
    for (int n = 0; n < TN; ++n) {
        const int sub = wn * TN + n;
        const int jx = l31 & (SW - 1), jy = l31 >> g.lsw;
        const int sx = sub & ((1 << g.lnsx) - 1);
        const int sy = (sub >> g.lnsx) & ((1 << g.lnsy) - 1);
        const int b = b0 + (sub >> (g.lnsx + g.lnsy));
        int gy = ty0 + sy * SH + jy, gx = tx0 + sx * SW + jx;
        if (UP && g.flat) gy = gx / g.GW, gx -= gy * g.GW;
#pragma unroll
        for (int ph = 0; ph < NPH; ++ph) {
            const int oy = UP ? 2 * gy + ((ph >> 1) & 1) : gy, ox = UP ? 2 * gx + (ph & 1) : (WINO ? WX * gx + (ph < WX ? ph : 0) : gx);
            nz_all[n][ph] = 0.f;
            if (WINO && ph >= WX) continue;
            if (nw != 0.f && b < g.B && gy < g.GH && gx < g.GW && oy < g.OH && ox < g.OW)
                nz_all[n][ph] = nw * act_gain * (MULTI ? noise_base[(size_t)b * noise_bstride + (size_t)oy * g.OW + ox]
                                                       : (noise_base + (size_t)b0 * noise_bstride)[(unsigned)(oy * g.OW + ox)]);
        }
    }
#pragma unroll
    for (int n = 0; n < TN; ++n) {
        const int sub = wn * TN + n;
        const int jx = l31 & (SW - 1), jy = l31 >> g.lsw;
        const int sx = sub & ((1 << g.lnsx) - 1);
        const int sy = (sub >> g.lnsx) & ((1 << g.lnsy) - 1);
        const int img = sub >> (g.lnsx + g.lnsy);
        const int b = b0 + img;
        int gy = ty0 + sy * SH + jy, gx = tx0 + sx * SW + jx;
        if (UP && g.flat) gy = gx / g.GW, gx -= gy * g.GW;
        const bool pos_ok = (b < g.B) && (gy < g.GH) && (gx < g.GW);
        // transposed conv: the two x-parities of a position are adjacent in memory -> one 8-byte store per lane
        // (rows of the (2W+1)-wide plane are only 4-byte aligned: f32x2u is an align-4 vector type)
        constexpr int PXN = UW ? 4 : (UP ? 2 : WX);  // outputs per position along x (pairs / quads in the Winograd modes)
#pragma unroll
        for (int py = 0; py < (UP ? 2 : 1); ++py) {
            const int oy = UP ? 2 * gy + py : gy;
            const int ox = UW ? 4 * gx : (UP ? 2 * gx : WX * gx);
            const bool ok0 = pos_ok && oy < g.OH && ox < g.OW;
            const bool ok1 = (UP || WINO) && ok0 && (ox + PXN - 1 < g.OW);  // the whole pair / quad is inside the row
            float nzv[PXN];
#pragma unroll
            for (int px = 0; px < PXN; ++px) nzv[px] = UW ? 0.f : nz_all[n][UP ? py * 2 + px : (WINO ? px : 0)];
            // row pointer of this wave's first output channel (block-uniform unless several images share a tile) + a
            // 32-bit lane offset: the per-element address is scalar base + VGPR offset, no 64-bit vector arithmetic
            float* blk = outp + ((size_t)(MULTI ? b : b0) * g.Cout + m0 + wm * (TM * 32)) * plane_out;
            const unsigned lane_off = (unsigned)oy * (unsigned)g.OW + (unsigned)ox + (unsigned)(4 * hi) * (unsigned)plane_out;
            float rgbp[PXN][3];
#pragma unroll
            for (int px = 0; px < PXN; ++px) rgbp[px][0] = rgbp[px][1] = rgbp[px][2] = 0.f;
            // Everything that does not depend on the accumulator element is decided once per (n, py): whether the tail is
            // applied, whether the feature map is stored, and the lane's store class.  Tiles that lie completely inside the
            // image and the channel range (every tile of the power-of-two plain layers) take the INTERIOR instance of the
            // element loop, which has no per-lane predication at all — on the 32/64-channel 1024^2/512^2 layers (4-8 K-chunks
            // per workgroup) the epilogue's instruction count is a first-order cost.
            const bool apply_act = !to_ws && g.fuse_act;
            const bool do_rgb = !UP && WM == 1 && !MULTI && g.rgb;
            const bool store_feat = !(do_rgb && g.rgb == 2) && !MAUA_DBG(1);
            const int n_ok = g.Cout - m0 - wm * (TM * 32) - 4 * hi;  // this lane's channel rows oe < n_ok exist
            const unsigned lane_bytes = lane_off * 4u;
            auto elements = [&](auto interior_tag) {
                constexpr bool IN = decltype(interior_tag)::value;
#pragma unroll
                for (int mt = 0; mt < TM; ++mt) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int oe = mt * 32 + (e & 3) + 8 * (e >> 2);
                        const int ol = wm * (TM * 32) + oe + 4 * hi;
                        const int o = m0 + ol;
                        float gain, bias;
                        if (MULTI) {
                            gain = g.wscale, bias = 0.f;
                            if (!to_ws && ok0 && o < g.Cout) {
                                if (p.d) gain *= p.d[b * g.Cout + o];
                                if (g.fuse_act && p.bias) bias = p.bias[o];
                            }
                            gain *= act_gain, bias *= act_gain;
                        } else {
                            gain = Eg[ol], bias = Eb[ol];
                        }
                        float v[PXN];
#pragma unroll
                        for (int px = 0; px < PXN; ++px) {
                            float raw;
                            if (UW) {  // columns 4 gx .. 4 gx + 3 = e_p, o_p, e_p+1, o_p+1
                                const int sb = n * NPH + py * 5;
                                raw = px == 0 ? acc[mt][sb + 0][e] + acc[mt][sb + 1][e]
                                    : px == 1 ? acc[mt][sb + 3][e]
                                    : px == 2 ? acc[mt][sb + 1][e] + acc[mt][sb + 2][e] : acc[mt][sb + 4][e];
                            } else if (W43) {
                                // A^T m: y0 = m0+m1+m2+m3+m4, y1 = (m1-m2) + 2(m3-m4), y2 = (m1+m2) + 4(m3+m4),
                                //        y3 = (m1-m2) + 8(m3-m4) + m5
                                const float m0_ = acc[mt][n * NPH + 0][e], m1_ = acc[mt][n * NPH + 1][e];
                                const float m2_ = acc[mt][n * NPH + 2][e], m3_ = acc[mt][n * NPH + 3][e];
                                const float m4_ = acc[mt][n * NPH + 4][e], m5_ = acc[mt][n * NPH + 5][e];
                                const float s12 = m1_ + m2_, d12 = m1_ - m2_, s34 = m3_ + m4_, d34 = m3_ - m4_;
                                raw = px == 0 ? (m0_ + s12) + s34 : px == 1 ? fmaf(2.f, d34, d12)
                                    : px == 2 ? fmaf(4.f, s34, s12) : fmaf(8.f, d34, d12) + m5_;
                            } else if (W23) {  // inverse transform: y0 = m0 + m1 + m2, y1 = m1 - m2 - m3
                                const float m0_ = acc[mt][n * NPH + 0][e], m1_ = acc[mt][n * NPH + 1][e];
                                const float m2_ = acc[mt][n * NPH + 2][e], m3_ = acc[mt][n * NPH + 3][e];
                                raw = px == 0 ? (m0_ + m1_) + m2_ : (m1_ - m2_) - m3_;
                            } else {
                                raw = acc[mt][n * NPH + (UP ? py * 2 + px : 0)][e];
                            }
                            const float t = fmaf(raw, gain, nzv[px] + bias);  // bias and noise are 0 unless the tail is fused
                            v[px] = apply_act ? fmaxf(t, 0.2f * t) : t;
                        }
                        if (do_rgb) {
#pragma unroll
                            for (int c = 0; c < 3; ++c) {
                                const float rw = lds[(2 + c) * BM + ol];
#pragma unroll
                                for (int px = 0; px < PXN; ++px) rgbp[px][c] = fmaf(rw, v[px], rgbp[px][c]);
                            }
                        }
                        if (!store_feat) continue;
                        // scalar row base + 32-bit lane byte offset
                        char* rowb = reinterpret_cast<char*>(blk + (size_t)oe * plane_out);
                        float* dst = reinterpret_cast<float*>(rowb + lane_bytes);
                        auto store_all = [&]() {
                            if (PXN == 4) *reinterpret_cast<f32x4u*>(dst) = f32x4{v[0], v[1 % PXN], v[2 % PXN], v[3 % PXN]};
                            else *reinterpret_cast<f32x2u*>(dst) = f32x2{v[0], v[PXN - 1]};
                        };
                        if (IN) {
                            if (UP || WINO) store_all();
                            else dst[0] = v[0];
                        } else if (oe < n_ok) {
                            if ((UP || WINO) && ok1) store_all();
                            else if (ok0) dst[0] = v[0];
                        }
                    }
                }
            };
            const bool interior = !UP && !MULTI && (m0 + BM <= g.Cout) && (ty0 + THt <= g.GH) && (tx0 + TWd <= g.GW) &&
                                  (!WINO || g.OW % WX == 0);
            // (the 64-row F(4,3) config is at the register limit: with two instances of the element loop the compiler
            // spills 42 accumulator registers, with one it spills none and runs 4 % faster)
            if (interior && !(W43 && TM == 2 && WM == 1)) elements(std::true_type{});
            else elements(std::false_type{});
            if (!UP && WM == 1 && !MULTI && g.rgb) {
                // all channels of a pixel live in one wave: lanes l and l+32 hold the two halves of the channel set
#pragma unroll
                for (int px = 0; px < PXN; ++px)
#pragma unroll
                    for (int c = 0; c < 3; ++c) rgbp[px][c] += __shfl_xor(rgbp[px][c], 32, 64);
                if (hi == 0 && ok0) {
                    // upfirdn2d(skip, k4, up=2, pad=(2,1)) at (oy, x): exactly two source rows / columns are live,
                    // iy0 = floor((oy-1)/2), iy0+1 (taps k4[1]/k4[3] for even oy, k4[0]/k4[2] for odd) — all loads
                    // (3 channels x 2 x 2 per pixel) are unconditional (clamped) and in flight together, masked by weight 0.
                    const int sh = g.H >> 1, sw = g.W >> 1;
                    const int iy0 = (oy - 1) >> 1;
                    const int ty_ = (oy & 1) ? 2 : 3;  // tap index of the FIRST live row
                    float wy[2];
                    int ry[2];
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const int yy = iy0 + q;
                        ry[q] = min(max(yy, 0), sh - 1);
                        wy[q] = (yy >= 0 && yy < sh) ? 1.f : 0.f;
                    }
                    float wgt[PXN][2][2];
                    float sv[PXN][3][2][2];
                    // (this branch is only compiled for single-image tiles: b == b0, bases are scalar, offsets 32-bit)
                    const float* __restrict__ skip_img = p.rgb_skip ? p.rgb_skip + (size_t)b0 * 3 * sh * sw : nullptr;
#pragma unroll
                    for (int px = 0; px < PXN; ++px) {
                        const int x = ox + px;
                        const int ix0 = (x - 1) >> 1;
                        const int tx_ = (x & 1) ? 2 : 3;
                        float wx[2];
                        int rx[2];
#pragma unroll
                        for (int q = 0; q < 2; ++q) {
                            const int xx = ix0 + q;
                            rx[q] = min(max(xx, 0), sw - 1);
                            wx[q] = (xx >= 0 && xx < sw) ? 1.f : 0.f;
                        }
#pragma unroll
                        for (int qy = 0; qy < 2; ++qy)
#pragma unroll
                            for (int qx = 0; qx < 2; ++qx) {
                                wgt[px][qy][qx] = 0.f;
#pragma unroll
                                for (int c = 0; c < 3; ++c) sv[px][c][qy][qx] = 0.f;
                            }
                        if (skip_img) {
#pragma unroll
                            for (int qy = 0; qy < 2; ++qy)
#pragma unroll
                                for (int qx = 0; qx < 2; ++qx) {
                                    wgt[px][qy][qx] = p.rgb_k4[(ty_ - 2 * qy) * 4 + (tx_ - 2 * qx)] * wy[qy] * wx[qx];
#pragma unroll
                                    for (int c = 0; c < 3; ++c)
                                        sv[px][c][qy][qx] = skip_img[(unsigned)((c * sh + ry[qy]) * sw + rx[qx])];
                                }
                        }
                    }
                    float* __restrict__ rgb_img = p.rgb_out + (size_t)b0 * 3 * plane_out;
                    const unsigned rgb_off = (unsigned)(oy * g.OW + ox);
                    uint32_t pix[PXN];  // packed frame bytes (R | G << 8 | B << 16) when the frame epilogue is fused
#pragma unroll
                    for (int px = 0; px < PXN; ++px) pix[px] = 0u;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        float val[PXN];
#pragma unroll
                        for (int px = 0; px < PXN; ++px) {
                            val[px] = rgbp[px][c] + p.rgb_bias[c];
#pragma unroll
                            for (int qy = 0; qy < 2; ++qy)
#pragma unroll
                                for (int qx = 0; qx < 2; ++qx) val[px] = fmaf(wgt[px][qy][qx], sv[px][c][qy][qx], val[px]);
                        }
                        if (p.rgb_u8) {  // render.py:40-43: clamp(-1, 1), (x + 1) * 127.5, truncating cast
#pragma unroll
                            for (int px = 0; px < PXN; ++px)
                                pix[px] |= rgb8_quant(val[px]) << (8 * c);
                            if (!p.rgb_out) continue;  // (both given: the fp32 planes are written as well — the parity tests' tap)
                        }
                        float* ro = rgb_img + (size_t)c * plane_out + rgb_off;
                        if (PXN == 4 && ok1) *reinterpret_cast<f32x4u*>(ro) = f32x4{val[0], val[1 % PXN], val[2 % PXN], val[3 % PXN]};
                        else if (PXN == 2 && ok1) *reinterpret_cast<f32x2u*>(ro) = f32x2{val[0], val[PXN - 1]};
                        else ro[0] = val[0];
                    }
                    if (p.rgb_u8) {
                        uint8_t* fo = p.rgb_u8 + ((size_t)b0 * plane_out + rgb_off) * 3;
                        if (PXN == 4 && ok1) {
                            store_rgb8x4(fo, pix[0], pix[1 % PXN], pix[2 % PXN], pix[3 % PXN]);
                        } else {
#pragma unroll
                            for (int px = 0; px < PXN; ++px)
                                if (px == 0 || ok1) fo[3 * px] = (uint8_t)pix[px], fo[3 * px + 1] = (uint8_t)(pix[px] >> 8), fo[3 * px + 2] = (uint8_t)(pix[px] >> 16);
                        }
                    }
                }
            }
        }
    }
}

}  // namespace

// Rows (BM, BN, WM, MODE, MULTI, MAXP) of an instance unit's MAUA_CONV_ROWS (modconv_m0.hip .. modconv_m4.hip), each instantiated with FAST and without.  These are the keys make_plan() can return, no
// others: tests/test_conv_instances_host.py enumerates the plan over the range its saturation argument (at make_plan) names and
// tests/test_isa_checks.py compares the compiled set with the same table.  Why the other MULTI x MAXP combinations of a config cannot
// occur is listed in DESIGN.md 4.0 (smallest / largest patch of each tile, flat runs hold one image).
#define MAUA_CONV_BOTH(X, bm, bn, wm, mode, maxp) X(bm, bn, wm, mode, true, maxp) X(bm, bn, wm, mode, false, maxp)
#define MAUA_CONV_ENTRY1(BM, BN, WM, MODE, MULTI, FAST, MAXP)                                              \
    {{BM, BN, WM, MODE, MULTI, FAST, MAXP}, "modconv_mfma_kernel<" #BM ", " #BN ", " #WM ", " #MODE ", " #MULTI ", " #FAST ", " #MAXP ">", \
     &maua_launch_conv<modconv_mfma_kernel<BM, BN, WM, MODE, MULTI, FAST, MAXP>, ConvGeom, ConvPtrs>},
#define MAUA_CONV_ENTRY(BM, BN, WM, MODE, MULTI, MAXP) \
    MAUA_CONV_ENTRY1(BM, BN, WM, MODE, MULTI, true, MAXP) MAUA_CONV_ENTRY1(BM, BN, WM, MODE, MULTI, false, MAXP)
