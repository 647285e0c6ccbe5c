// Predominant local pulse for gfx950 (Grosche & Mueller, IEEE TASLP 2011) — the device side of audioreactive.beat.raw_plp.
// Two entries; their definitions are their comments in include/maua_hip.h and DESIGN.md 4.20, tests/pulse_ref.py restates both in numpy.
//
// maua_tempogram_peak_f32: one workgroup of sixteen waves owns a tile of 64 consecutive frames, lane l of every wave frame l of the tile.
//   The tile's 64 + win - 1 envelope samples are staged in LDS once (zeros outside [0, n): a clipped tap is an added zero, so a
//   frame's sum does not depend on where it falls).  Wave w takes the tempo groups w, w + 16, ... of PULSE_BT consecutive tempi; for a
//   group it walks k = 0 .. win - 1 with one conflict-free LDS read x[l + k] and PULSE_BT complex FMAs against table values that are
//   the same for the whole wave: the row pointers are wave-uniform (readfirstlane), so the table streams from L2 through the scalar
//   cache and never touches LDS or vector registers.  One accumulator chain per (frame, tempo) in ascending k: nothing reassociates.
//   A lane walks its tempi upwards taking S > best, the waves' winners meet in LDS and wave 0 takes the larger S, the LOWER bin
//   on equal S — written out, not left to a reduction tree.  The [n][n_tempi] map is stored only when asked for.
//
// maua_pulse_synth_f32: gather form, no atomics.  One workgroup owns 128 output samples; the (omega, phase, state) of the
//   128 + win - 1 covering frames and the window are staged in LDS; thread m walks k = 0 .. win - 1 (frame t = m + win / 2 - k, the
//   lanes read neighbouring frames) and adds w[k] to den and w[k] cosf(omega k + phase) to num.  cosf, not the hardware cosine: the
//   arguments reach win * omega_max + pi.
#include <math.h>

#include "common.h"

namespace {

constexpr int PULSE_TILE = 64;   // frames per workgroup of entry A (one per lane)
constexpr int PULSE_WAVES = 16;  // waves per workgroup of entry A: they split the tempo groups (four a SIMD hide the table's latency)
constexpr int PULSE_BT = 3;      // tempi a wave accumulates at a time: three rows of eight taps fill the scalar registers without a spill
constexpr int PULSE_BLOCK = 128; // output samples per workgroup of entry B

__global__ __launch_bounds__(PULSE_TILE * PULSE_WAVES) void tempogram_peak_kernel(const float* __restrict__ env, int n,
                                                                                   const float2* __restrict__ table, int win, int n_tempi,
                                                                                   const float* __restrict__ prior, int* __restrict__ bin,
                                                                                   float* __restrict__ phase, float* __restrict__ power,
                                                                                   float* __restrict__ tgram) {
#pragma clang fp contract(off)  // the sums are explicit fmaf chains, the score is (re re + im im) p with every operation rounded
    __shared__ float x[PULSE_TILE + MAUA_PULSE_MAX_WIN - 1];
    __shared__ float best_s[PULSE_WAVES][PULSE_TILE], re_s[PULSE_WAVES][PULSE_TILE], im_s[PULSE_WAVES][PULSE_TILE];
    __shared__ int bin_s[PULSE_WAVES][PULSE_TILE];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t t0 = (int64_t)blockIdx.x * PULSE_TILE;
    const int64_t first = t0 - win / 2;  // the sample behind x[0]
    for (int i = threadIdx.x; i < PULSE_TILE + win - 1; i += PULSE_TILE * PULSE_WAVES) {
        const int64_t at = first + i;
        x[i] = at >= 0 && at < n ? env[at] : 0.f;
    }
    __syncthreads();

    const int64_t t = t0 + lane;
    const float* xl = x + lane;
    float best = 0.f, best_re = 0.f, best_im = 0.f;
    int best_bin = -1;
    for (int b0 = wave * PULSE_BT; b0 < n_tempi; b0 += PULSE_WAVES * PULSE_BT) {
        const float2* row[PULSE_BT];
        float re[PULSE_BT], im[PULSE_BT];
#pragma unroll
        for (int j = 0; j < PULSE_BT; ++j) {
            row[j] = table + (size_t)min(b0 + j, n_tempi - 1) * win;  // (a group's tail repeats the last row; its results are dropped)
            re[j] = 0.f, im[j] = 0.f;
        }
#pragma unroll 8
        for (int k = 0; k < win; ++k) {
            const float v = xl[k];
#pragma unroll
            for (int j = 0; j < PULSE_BT; ++j) {
                const float2 c = row[j][k];
                re[j] = fmaf(v, c.x, re[j]);
                im[j] = fmaf(v, c.y, im[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < PULSE_BT; ++j) {
            const int b = b0 + j;
            if (b < n_tempi) {
                const float s = (re[j] * re[j] + im[j] * im[j]) * (prior ? prior[b] : 1.f);
                if (tgram && t < n) tgram[t * n_tempi + b] = s;
                if (s > best) best = s, best_bin = b, best_re = re[j], best_im = im[j];
            }
        }
    }
    best_s[wave][lane] = best, bin_s[wave][lane] = best_bin, re_s[wave][lane] = best_re, im_s[wave][lane] = best_im;
    __syncthreads();
    if (wave == 0 && t < n) {
#pragma unroll
        for (int w = 1; w < PULSE_WAVES; ++w) {
            const float s = best_s[w][lane];
            const int b = bin_s[w][lane];
            if (b >= 0 && (s > best || (s == best && b < best_bin))) best = s, best_bin = b, best_re = re_s[w][lane], best_im = im_s[w][lane];
        }
        bin[t] = best_bin;
        phase[t] = best_bin >= 0 ? atan2f(best_im, best_re) : 0.f;
        power[t] = best;
    }
}

__global__ __launch_bounds__(PULSE_BLOCK) void pulse_synth_kernel(const int* __restrict__ bin, const float* __restrict__ phase, int n,
                                                                  const float* __restrict__ window, int win,
                                                                  const float* __restrict__ omega, int n_tempi, float* __restrict__ pulse) {
#pragma clang fp contract(off)  // arg = fl(fl(omega k) + phase), num = fl(num + fl(w cos)): the order the header states
    __shared__ float om[PULSE_BLOCK + MAUA_PULSE_MAX_WIN - 1], ph[PULSE_BLOCK + MAUA_PULSE_MAX_WIN - 1], w[MAUA_PULSE_MAX_WIN];
    __shared__ int state[PULSE_BLOCK + MAUA_PULSE_MAX_WIN - 1];  // 0 outside [0, n), 1 a frame without a tempo, 2 a frame with one
    const int64_t m0 = (int64_t)blockIdx.x * PULSE_BLOCK;
    const int64_t first = m0 + win / 2 - (win - 1);  // the frame behind index 0: thread i reads index i + win - 1 - k at tap k
    for (int i = threadIdx.x; i < PULSE_BLOCK + win - 1; i += PULSE_BLOCK) {
        const int64_t t = first + i;
        int st = 0;
        float o = 0.f, p = 0.f;
        if (t >= 0 && t < n) {
            const int b = bin[t];
            st = 1;
            if (b >= 0 && b < n_tempi) st = 2, o = omega[b], p = phase[t];
        }
        state[i] = st, om[i] = o, ph[i] = p;
    }
    for (int k = threadIdx.x; k < win; k += PULSE_BLOCK) w[k] = window[k];
    __syncthreads();
    const int64_t m = m0 + threadIdx.x;
    if (m >= n) return;
    const int top = threadIdx.x + win - 1;
    float num = 0.f, den = 0.f;
    for (int k = 0; k < win; ++k) {
        const int i = top - k;
        const int st = state[i];
        if (st == 0) continue;
        const float wk = w[k];
        den = den + wk;
        if (st == 2) num = num + wk * cosf(om[i] * (float)k + ph[i]);
    }
    const float r = num / den;
    pulse[m] = den > 0.f && r > 0.f ? r : 0.f;
}

bool pulse_sizes_ok(int n, int win, int n_tempi) {
    return n >= 1 && n <= MAUA_PULSE_MAX_FRAMES && win >= 2 && win <= MAUA_PULSE_MAX_WIN && n_tempi >= 1 && n_tempi <= MAUA_PULSE_MAX_TEMPI;
}

}  // namespace

extern "C" int maua_tempogram_peak_f32(const float* env, int n, const float* table, int win, int n_tempi, const float* prior, int* bin,
                                       float* phase, float* power, float* tgram, void* stream) {
    if (!env || !table || !bin || !phase || !power) return MAUA_EINVAL;
    if (!pulse_sizes_ok(n, win, n_tempi)) return MAUA_EINVAL;
    hipLaunchKernelGGL(tempogram_peak_kernel, dim3((unsigned)ceil_div(n, PULSE_TILE)), dim3(PULSE_TILE * PULSE_WAVES), 0,
                       (hipStream_t)stream, env, n, reinterpret_cast<const float2*>(table), win, n_tempi, prior, bin, phase, power, tgram);
    MAUA_LAUNCH_CHECK();
    return 0;
}

extern "C" int maua_pulse_synth_f32(const int* bin, const float* phase, int n, const float* window, int win, const float* omega, int n_tempi,
                                    float* pulse, void* stream) {
    if (!bin || !phase || !window || !omega || !pulse) return MAUA_EINVAL;
    if (!pulse_sizes_ok(n, win, n_tempi)) return MAUA_EINVAL;
    hipLaunchKernelGGL(pulse_synth_kernel, dim3((unsigned)ceil_div(n, PULSE_BLOCK)), dim3(PULSE_BLOCK), 0, (hipStream_t)stream, bin, phase, n,
                       window, win, omega, n_tempi, pulse);
    MAUA_LAUNCH_CHECK();
    return 0;
}
