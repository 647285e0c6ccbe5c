// Monophonic pitch tracking for gfx950: YIN (de Cheveigne & Kawahara, JASA 111(4), 2002, steps 1-5) on centred frames — the device side of
// audioreactive.signal.raw_pitch / pitch.  The definition (framing, difference function, cumulative-mean normalisation, pick, parabolic
// refinement) is the comment of maua_yin_f32 in include/maua_hip.h and DESIGN.md 4.16; tests/pitch_ref.py restates it in float64.
//
// One workgroup per frame.  The L = frame + tau_max samples of the frame are staged once in LDS (zeros outside the signal), then
//   * difference function: a lane owns YIN_R = 4 CONSECUTIVE lags tau0 .. tau0 + 3, tau0 = 1 + 4 g, and walks j four samples at a time:
//     x[j .. j+3] are four broadcast reads, x[j + tau0 .. j + tau0 + 7] is one new aligned 16-byte read per step (the other half is the
//     previous step's), and the 8 + 4 values feed 16 subtract + fma pairs.  The staged copy starts 3 floats into the allocation so that
//     x[1 + 4 g] sits on a 16-byte boundary.  Each lag is summed over j in ascending order in one fp32 accumulator (the direct sum of
//     squares: the energy form 2 r(0) - 2 r(tau) cancels).  The workgroup is 64, 128 or 256 lanes — the smallest that covers
//     ceil(tau_max / 4) lag groups — and a lane takes a second group (a second pass over j) once tau_max exceeds 1024.
//   * running sum: wave 0, lane l owns the ceil(tau_max / 64) consecutive lags behind 1 + l * that, sums them, the 64 partial sums are
//     scanned with shuffles, and the lane walks its lags again writing d'(tau) = d(tau) tau / sum in place.
//   * pick and refinement: wave 0 (first lag under the threshold by a strided search and a wave minimum, the descent by a uniform loop,
//     otherwise a (value, index) arg-min with ties to the lower index), lane 0 writes the three per-frame outputs; all lanes copy the
//     d' row out when the caller wants it.
// No atomics, no workspace, fixed summation order: the result is a function of the arguments alone.
#include <math.h>

#include "common.h"
#include "wave.h"

namespace {

constexpr int YIN_R = 4;         // consecutive lags per lane and pass
constexpr int YIN_X_PAD = 8;     // zeros behind the L staged samples: the last 16-byte read of the last lag group ends at L + 3
constexpr int YIN_X_SHIFT = 3;   // x[0] sits 3 floats into the (16-byte aligned) allocation, so x[1 + 4 g] is 16-byte aligned

__host__ __device__ inline int yin_x_floats(int frame, int tau_max) { return (YIN_X_SHIFT + frame + tau_max + YIN_X_PAD + 3) & ~3; }

__global__ __launch_bounds__(256) void yin_kernel(const float* __restrict__ y, int64_t n_samples, int frame, int hop, int tau_min,
                                                  int tau_max, float threshold, float* __restrict__ lag, float* __restrict__ aperiodicity,
                                                  int32_t* __restrict__ tau_int, float* __restrict__ cmndf) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const int L = frame + tau_max;
    float* xs = sm + YIN_X_SHIFT;                  // [L + YIN_X_PAD]
    float* dp = sm + yin_x_floats(frame, tau_max); // [tau_max + 1]: d, then d' in place
    const int tid = threadIdx.x, nt = blockDim.x;
    const int t = blockIdx.x;
    const int64_t start = (int64_t)t * hop - L / 2;
    for (int i = tid; i < L + YIN_X_PAD; i += nt) {
        const int64_t s = start + i;
        xs[i] = (i < L && s >= 0 && s < n_samples) ? y[s] : 0.f;
    }
    __syncthreads();

    const int frame4 = frame & ~3;
    for (int g = tid; 1 + YIN_R * g <= tau_max; g += nt) {
        const int tau0 = 1 + YIN_R * g;
        const float* xv = xs + tau0;  // 16-byte aligned
        float acc[YIN_R] = {0.f, 0.f, 0.f, 0.f};
        f32x4 lo = *reinterpret_cast<const f32x4*>(xv);
        for (int j = 0; j < frame4; j += 4) {
            const f32x4 hi = *reinterpret_cast<const f32x4*>(xv + j + 4);
            const float a[4] = {xs[j], xs[j + 1], xs[j + 2], xs[j + 3]};
            const float w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};  // x[j + tau0 + k]
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int r = 0; r < YIN_R; ++r) {
                    const float diff = a[jj] - w[jj + r];
                    acc[r] = fmaf(diff, diff, acc[r]);
                }
            lo = hi;
        }
        for (int j = frame4; j < frame; ++j) {
            const float a = xs[j];
#pragma unroll
            for (int r = 0; r < YIN_R; ++r) {
                const float diff = a - xv[j + r];
                acc[r] = fmaf(diff, diff, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < YIN_R; ++r)
            if (tau0 + r <= tau_max) dp[tau0 + r] = acc[r];
    }
    __syncthreads();

    if (tid < 64) {  // wave 0: d'(tau) = d(tau) tau / sum_{k <= tau} d(k)
        const int per_lane = (tau_max + 63) / 64;
        const int first = 1 + tid * per_lane;
        float own = 0.f;
        for (int k = 0; k < per_lane; ++k)
            if (first + k <= tau_max) own += dp[first + k];
        float inc = own;  // (wave_incl_sum of wave.h, spelled out: the call reschedules this kernel)
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float v = __shfl_up(inc, off, 64);
            if (tid >= off) inc += v;
        }
        float run = __shfl_up(inc, 1, 64);
        if (tid == 0) run = 0.f;
        for (int k = 0; k < per_lane; ++k) {
            const int tau = first + k;
            if (tau <= tau_max) {
                const float d = dp[tau];
                run += d;
                dp[tau] = run > 0.f ? d * (float)tau / run : 1.f;
            }
        }
        if (tid == 0) dp[0] = 1.f;
    }
    __syncthreads();

    if (cmndf) {
        float* row = cmndf + (int64_t)t * (tau_max + 1);
        for (int i = tid; i <= tau_max; i += nt) row[i] = dp[i];
    }
    if (tid >= 64) return;

    int found = 0x7fffffff;  // smallest lag in [tau_min, tau_max] under the threshold
    for (int tau = tau_min + tid; tau <= tau_max; tau += 64)
        if (dp[tau] < threshold) {
            found = tau;
            break;
        }
    found = wave_min(found);
    int tau;
    if (found != 0x7fffffff) {
        tau = found;
        while (tau + 1 <= tau_max && dp[tau + 1] < dp[tau]) ++tau;  // down to the local minimum
    } else {  // first global minimum (a lane without a candidate, or with NaNs only, holds (inf, tau_min))
        float bv = INFINITY;
        int bi = tau_min;
        for (int i = tau_min + tid; i <= tau_max; i += 64) {
            const float v = dp[i];
            if (v < bv) bv = v, bi = i;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (ov < bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
        }
        tau = bi;
    }
    const float b = dp[tau];
    float lg = (float)tau, ap = b;
    if (tau - 1 >= 1 && tau + 1 <= tau_max) {
        const float a = dp[tau - 1], c = dp[tau + 1];
        const float curv = a - 2.f * b + c;
        if (curv > 0.f) {
            const float shift = fminf(fmaxf(0.5f * (a - c) / curv, -0.5f), 0.5f);
            lg = (float)tau + shift;
            ap = fmaxf(0.f, b - 0.25f * (a - c) * shift);  // (the parabola's minimum dips below 0 on clean tones)
        }
    }
    if (tid == 0) {
        lag[t] = lg;
        aperiodicity[t] = ap;
        tau_int[t] = tau;
    }
}

}  // namespace

extern "C" int maua_yin_f32(const float* y, int64_t n_samples, int frame, int hop, int tau_min, int tau_max, float threshold, float* lag,
                            float* aperiodicity, int32_t* tau_int, float* cmndf, int n_frames, void* stream) {
    if (!y || !lag || !aperiodicity || !tau_int) return MAUA_EINVAL;
    if (frame < 16 || frame > MAUA_YIN_MAX_FRAME || tau_min < 1 || tau_min >= tau_max || tau_max > MAUA_YIN_MAX_LAG || hop < 1 || n_samples < 1)
        return MAUA_EINVAL;
    if (!isfinite(threshold) || threshold < 0.f) return MAUA_EINVAL;
    if ((int64_t)n_frames != 1 + n_samples / hop) return MAUA_EINVAL;
    const int groups = ceil_div(tau_max, YIN_R);
    const int block = groups <= 64 ? 64 : (groups <= 128 ? 128 : 256);
    const size_t lds = (size_t)(yin_x_floats(frame, tau_max) + tau_max + 1) * sizeof(float);  // 32.8 KB at the limits
    hipLaunchKernelGGL(yin_kernel, dim3((unsigned)n_frames), dim3(block), lds, (hipStream_t)stream, y, n_samples, frame, hop, tau_min,
                       tau_max, threshold, lag, aperiodicity, tau_int, cmndf);
    MAUA_LAUNCH_CHECK();
    return 0;
}
