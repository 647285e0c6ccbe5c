// Probabilistic YIN for gfx950 (Mauch & Dixon, ICASSP 2014) — the device side of audioreactive.signal.raw_pyin / pitch(method="pyin").
// Two entries behind the d' rows that maua_yin_f32 (pitch.hip) writes; their definitions are their comments in include/maua_hip.h and
// DESIGN.md 4.19, tests/pyin_ref.py restates both in numpy.
//
// maua_pyin_candidates_f32: one wave per frame.  The d' row is staged in LDS; lane l owns the ceil((tau_max - tau_min) / 64) consecutive
//   lags behind tau_min + l * that and walks them three times: (1) the minimum height of its troughs, turned into "the minimum of every
//   earlier trough" by an exclusive prefix-min over the lanes (shuffles); (2) the count of its record troughs (lower than everything
//   before them: only those own thresholds), turned into offsets by a prefix sum; (3) the records, with their table difference, written
//   to an LDS list in lag order.  Lane 0 then walks the list — a handful of entries on real audio — adds the fallback mass to the last
//   record (the first trough of smallest height), refines, bins by a binary search of the edge table and accumulates into LDS rows of
//   obs / period, which all lanes copy out.  No atomics, no workspace, one fixed order of summation.
//
// maua_pyin_viterbi_f64: one workgroup runs the whole decode, lane j owns pitch bin j in both voicings (they share the window) and keeps
//   its two delta in registers.  Per frame the lanes publish e = delta - log_norm in an LDS buffer (two buffers in turn, so one barrier
//   per frame is enough; W elements of -inf either side, so the scan has no bounds to check), then scan their window: the offset
//   d = i - j runs over the same range in every lane, so log_tri[W - d] (staged in LDS) is one broadcast read and e[j + d] one
//   conflict-free 8-byte read of neighbouring lanes.  Back pointers go to global memory; after the last
//   frame lane 0 takes the first maximum and walks them back.  Only double additions, subtractions and compares: nothing to contract.
#include <math.h>

#include "common.h"
#include "wave.h"

namespace {

constexpr int PYIN_MAX_TROUGHS = MAUA_YIN_MAX_LAG / 2;  // troughs need a higher left neighbour: at most every other lag

__device__ __forceinline__ int pyin_idx(float x, int n_thr) {  // number of thresholds k / n_thr at or below x; NaN and +inf: all of them
    const float v = floorf(x * (float)n_thr);
    if (v >= (float)n_thr || v != v) return n_thr;
    return v > 0.f ? (int)v : 0;
}

__device__ __forceinline__ bool pyin_trough(const float* r, int tau, int tau_min) {
    const float left = tau == tau_min ? INFINITY : r[tau - 1];
    return r[tau] < left && r[tau] <= r[tau + 1];
}

__global__ __launch_bounds__(64) void pyin_candidates_kernel(const float* __restrict__ cmndf, int tau_min, int tau_max,
                                                             const float* __restrict__ cum_prior, int n_thr, float no_trough_prob,
                                                             const float* __restrict__ edge, int n_bins, float* __restrict__ obs,
                                                             float* __restrict__ period, float* __restrict__ voiced_prob) {
#pragma clang fp contract(off)  // every product and sum below is rounded on its own, as the header defines them
    __shared__ float r[MAUA_YIN_MAX_LAG + 1];
    __shared__ int rec_tau[PYIN_MAX_TROUGHS];
    __shared__ float rec_p[PYIN_MAX_TROUGHS];
    __shared__ float obs_s[MAUA_PYIN_MAX_BINS], per_s[MAUA_PYIN_MAX_BINS], best_s[MAUA_PYIN_MAX_BINS];
    const int lane = threadIdx.x;
    const int64_t t = blockIdx.x;
    const float* row = cmndf + t * (tau_max + 1);
    for (int i = lane; i <= tau_max; i += 64) r[i] = row[i];
    for (int b = lane; b < n_bins; b += 64) obs_s[b] = 0.f, per_s[b] = 0.f, best_s[b] = 0.f;
    __syncthreads();

    const int per_lane = (tau_max - tau_min + 63) / 64;
    const int first = min(tau_min + lane * per_lane, tau_max), last = min(first + per_lane, tau_max);  // lags [first, last)
    float own = INFINITY;
    for (int tau = first; tau < last; ++tau)
        if (pyin_trough(r, tau, tau_min) && r[tau] < own) own = r[tau];
    const float inc = wave_incl_min(own, lane);  // inclusive prefix-min over the lanes
    float before = __shfl_up(inc, 1, 64);
    if (lane == 0) before = INFINITY;

    int n_own = 0;
    float m = before;
    for (int tau = first; tau < last; ++tau)
        if (pyin_trough(r, tau, tau_min) && r[tau] < m) m = r[tau], ++n_own;
    int at = wave_incl_sum(n_own, lane);  // inclusive prefix sum of the record counts
    const int n_rec = __shfl(at, 63, 64);
    at -= n_own;
    m = before;
    for (int tau = first; tau < last; ++tau)
        if (pyin_trough(r, tau, tau_min) && r[tau] < m) {
            const float h = r[tau];
            rec_tau[at] = tau;
            rec_p[at] = cum_prior[pyin_idx(m, n_thr)] - cum_prior[pyin_idx(h, n_thr)];
            m = h;
            ++at;
        }
    __syncthreads();

    if (lane == 0) {
        float total = 0.f;
        for (int i = 0; i < n_rec; ++i) {
            const int tau = rec_tau[i];
            float p = rec_p[i];
            const float b = r[tau];
            if (i == n_rec - 1) p = p + no_trough_prob * cum_prior[pyin_idx(b, n_thr)];  // the absolute-threshold fallback
            if (!(p > 0.f)) continue;
            float lg = (float)tau;
            if (tau - 1 >= 1) {  // (tau + 1 <= tau_max holds for every trough) the parabola of maua_yin_f32
                const float a = r[tau - 1], c = r[tau + 1];
                const float curv = a - 2.f * b + c;
                if (curv > 0.f) lg = (float)tau + fminf(fmaxf(0.5f * (a - c) / curv, -0.5f), 0.5f);
            }
            int lo = 0, hi = n_bins - 1;  // the first bin whose lower edge lies below the period, the last bin when none does
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (edge[mid + 1] < lg)
                    hi = mid;
                else
                    lo = mid + 1;
            }
            obs_s[lo] = obs_s[lo] + p;
            total = total + p;
            if (p > best_s[lo]) best_s[lo] = p, per_s[lo] = lg;
        }
        voiced_prob[t] = fminf(1.f, total);
    }
    __syncthreads();
    for (int b = lane; b < n_bins; b += 64) {
        obs[t * n_bins + b] = obs_s[b];
        period[t * n_bins + b] = per_s[b];
    }
}

__global__ __launch_bounds__(1024) void pyin_viterbi_kernel(const float* __restrict__ lov, const float* __restrict__ lou, int T, int P,
                                                            int W, const double* __restrict__ log_tri, const double* __restrict__ log_norm,
                                                            double log_init, double log_stay, double log_switch,
                                                            double* __restrict__ delta_last, uint16_t* backptr,
                                                            int32_t* __restrict__ states) {
    // [2 frames in turn][e_v, e_u][W + P + W]: W elements of -inf either side of a row stand for the sources outside [0, P - 1], so the
    // window scan needs no bounds; behind them log_tri [2 W + 1]
    extern __shared__ __attribute__((aligned(16))) double e[];
    const int j = threadIdx.x;
    const bool live = j < P;
    const int jj = live ? j : 0;
    const int stride = P + 2 * W;
    double* tri = e + 4 * stride;
    for (int i = j; i < 4 * stride; i += blockDim.x) e[i] = -INFINITY;
    for (int i = j; i <= 2 * W; i += blockDim.x) tri[i] = log_tri[i];
    const int reach = W < P - 1 ? W : P - 1;          // offsets beyond it leave [0, P - 1] for every lane
    const int i0 = jj - W > 0 ? jj - W : 0;           // the window's first source bin: it starts the search whatever it holds
    const double norm = log_norm[jj];
    double dv = (double)lov[jj] + log_init, du = (double)lou[0] + log_init;
    if (live) backptr[j] = (uint16_t)j, backptr[P + j] = (uint16_t)(P + j);
    __syncthreads();
    const double first_w = tri[jj - i0 + W];
    for (int t = 1; t < T; ++t) {
        const double ov = (double)lov[(int64_t)t * P + jj], ou = (double)lou[t];
        double* ev = e + (size_t)(t & 1) * 2 * stride + W;
        double* eu = ev + stride;
        if (live) ev[j] = dv - norm, eu[j] = du - norm;
        __syncthreads();
        // The search starts from (-inf, i0) and not from the window's first candidate: the same thing unless that candidate is a NaN,
        // which nothing replaces — put back below.  Padding gives -inf + weight = -inf, never strictly greater than anything.
        const double* pv = ev + jj;
        const double* pu = eu + jj;
        const double* pw = tri + W;
        double bv = -INFINITY, bu = -INFINITY;
        int kv = i0 - jj, ku = i0 - jj;
#pragma unroll 4
        for (int d = -reach; d <= reach; ++d) {
            const double w = pw[-d];
            const double cv = pv[d] + w, cu = pu[d] + w;
            if (cv > bv) bv = cv, kv = d;
            if (cu > bu) bu = cu, ku = d;
        }
        const double fv = ev[i0] + first_w, fu = eu[i0] + first_w;
        if (fv != fv) bv = fv, kv = i0 - jj;
        if (fu != fu) bu = fu, ku = i0 - jj;
        const int iv = jj + kv, iu = jj + ku;
        double a = bv + log_stay, b = bu + log_switch;
        int from = iv;
        if (b > a) a = b, from = P + iu;
        dv = ov + a;
        double a2 = bv + log_switch, b2 = bu + log_stay;
        int from2 = iv;
        if (b2 > a2) a2 = b2, from2 = P + iu;
        du = ou + a2;
        if (live) {
            uint16_t* bp = backptr + (int64_t)t * 2 * P;
            bp[j] = (uint16_t)from;
            bp[P + j] = (uint16_t)from2;
        }
    }
    __syncthreads();  // (the last frame's window reads are done: e is free)
    if (live) {
        delta_last[j] = dv, delta_last[P + j] = du;
        e[j] = dv, e[P + j] = du;
    }
    __threadfence();  // the back pointers of every wave, before lane 0 reads them
    __syncthreads();
    if (j == 0) {
        double best = e[0];  // (first_max of wave.h, spelled out: the call reschedules this kernel)
        int s = 0;
        for (int k = 1; k < 2 * P; ++k)
            if (e[k] > best) best = e[k], s = k;
        states[T - 1] = s;
        for (int t = T - 1; t >= 1; --t) {
            s = backptr[(int64_t)t * 2 * P + s];
            states[t - 1] = s;
        }
    }
}

}  // namespace

extern "C" int maua_pyin_candidates_f32(const float* cmndf, int n_frames, int tau_min, int tau_max, const float* cum_prior, int n_thr,
                                        float no_trough_prob, const float* bin_edge_period, int n_bins, float* obs, float* period,
                                        float* voiced_prob, void* stream) {
    if (!cmndf || !cum_prior || !bin_edge_period || !obs || !period || !voiced_prob) return MAUA_EINVAL;
    if (n_frames < 1 || tau_min < 1 || tau_min >= tau_max || tau_max > MAUA_YIN_MAX_LAG) return MAUA_EINVAL;
    if (n_thr < 1 || n_thr > MAUA_PYIN_MAX_THRESHOLDS || n_bins < 1 || n_bins > MAUA_PYIN_MAX_BINS) return MAUA_EINVAL;
    if (!isfinite(no_trough_prob) || no_trough_prob < 0.f || no_trough_prob > 1.f) return MAUA_EINVAL;
    hipLaunchKernelGGL(pyin_candidates_kernel, dim3((unsigned)n_frames), dim3(64), 0, (hipStream_t)stream, cmndf, tau_min, tau_max, cum_prior,
                       n_thr, no_trough_prob, bin_edge_period, n_bins, obs, period, voiced_prob);
    MAUA_LAUNCH_CHECK();
    return 0;
}

extern "C" int maua_pyin_viterbi_f64(const float* logobs_voiced, const float* logobs_unvoiced, int n_frames, int n_bins, int width,
                                     const double* log_tri, const double* log_norm, double log_init, double log_stay, double log_switch,
                                     double* delta_last, uint16_t* backptr, int32_t* states, void* stream) {
    if (!logobs_voiced || !logobs_unvoiced || !log_tri || !log_norm || !delta_last || !backptr || !states) return MAUA_EINVAL;
    if (n_frames < 1 || n_bins < 1 || n_bins > MAUA_PYIN_MAX_BINS || width < 0 || width > MAUA_PYIN_MAX_WIDTH) return MAUA_EINVAL;
    const int block = ceil_div(n_bins, 64) * 64;
    const size_t lds = ((size_t)4 * (n_bins + 2 * width) + 2 * width + 1) * sizeof(double);  // 43 KB at the limits
    hipLaunchKernelGGL(pyin_viterbi_kernel, dim3(1), dim3(block), lds, (hipStream_t)stream, logobs_voiced, logobs_unvoiced, n_frames, n_bins,
                       width, log_tri, log_norm, log_init, log_stay, log_switch, delta_last, backptr, states);
    MAUA_LAUNCH_CHECK();
    return 0;
}
