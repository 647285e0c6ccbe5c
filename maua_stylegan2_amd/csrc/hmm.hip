// Hidden Markov models with a dense transition matrix for gfx950 — the device side of audioreactive.harmony (viterbi, hmm_posterior,
// raw_chords).  Two entries; their definitions are their comments in include/maua_hip.h and DESIGN.md 4.21, tests/hmm_ref.py restates
// both in numpy.
//
// Both run in ONE workgroup of ceil(S / 64) waves, lane j owning state j: the recursion over the frames is serial, and the work of a
// frame (S^2 multiply-adds, 16 K at the limit) is too small to spread over more than one CU without paying a device-scope hand-off
// per frame.  The transition matrix is staged once in LDS with a row stride of S | 1 doubles (S, or S + 1 where S is even):
//   forward (Viterbi, alpha): lane j walks the sources i = 0 .. S - 1 in order and reads tr[i * stride + j] — neighbouring lanes read
//     neighbouring doubles (conflict-free) — against delta[i] / alpha[i], one broadcast read.  The walk IS the defined order of the
//     sum and of the ties: nothing is reduced across lanes.
//   backward (beta): lane i walks the targets j and reads tr[i * stride + j]: the lanes of a 32-lane group are an odd number of
//     doubles apart, so their 64 dwords fall on 64 different banks.  One copy serves both sweeps.
// c_t, a chain of S dependent additions, is redone by every lane from LDS (broadcast reads): cheaper than a second barrier to publish it.
// At S = 128 the matrix takes 129 KiB of the CU's 160 KiB, which needs the dynamic-LDS attribute (common.h).
//
// maua_hmm_viterbi_f64 keeps delta in registers, publishes it in two LDS buffers in turn (one barrier per frame) and writes one byte of
// back pointer per state and frame.  The walk back is a chain of T dependent reads: it runs on lane 0 out of LDS, the rows brought in
// 1024 frames at a time by all lanes (coalesced) and the states written out the same way — a dependent LDS read is far cheaper than
// a dependent read of global memory.
// maua_hmm_posterior_f64 stores alpha in gamma, then walks back with beta in registers and multiplies in place.
#include <math.h>

#include "common.h"
#include "wave.h"

namespace {

constexpr int HMM_BLOCK = 128;          // MAUA_HMM_MAX_STATES lanes: two waves
constexpr int HMM_TRACE_ROWS = 1024;    // frames of back pointers per LDS chunk of the walk back
static_assert(MAUA_HMM_MAX_STATES <= HMM_BLOCK && MAUA_HMM_MAX_STATES <= 256, "a lane per state, a byte per back pointer");

__global__ __launch_bounds__(HMM_BLOCK) void hmm_viterbi_kernel(const float* __restrict__ logobs, const double* __restrict__ log_trans,
                                                                const double* __restrict__ log_init, int T, int S,
                                                                double* __restrict__ delta_last, uint8_t* backptr, int32_t* __restrict__ states) {
    // forward: tr [S][stride], behind it delta [2 frames in turn][S]; walk back: rows [HMM_TRACE_ROWS][S] bytes, behind them their states
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int j = threadIdx.x;
    const bool live = j < S;
    const int jj = live ? j : 0;
    const int stride = dense_stride(S);
    double* tr = lds;
    double* dl = lds + S * stride;
    stage_dense(tr, log_trans, S, stride);
    double d = log_init[jj] + (double)logobs[jj];
    if (live) backptr[j] = (uint8_t)j;
    const double* col = tr + jj;
    for (int t = 1; t < T; ++t) {
        double* e = dl + (t & 1) * S;
        if (live) e[j] = d;
        const double o = (double)logobs[(int64_t)t * S + jj];
        __syncthreads();  // (the first one also ends the staging)
        double best = e[0] + col[0];
        int k = 0;
#pragma unroll 4
        for (int i = 1; i < S; ++i) {
            const double c = e[i] + col[i * stride];
            if (c > best) best = c, k = i;
        }
        d = best + o;
        if (live) backptr[(int64_t)t * S + j] = (uint8_t)k;
    }
    double* fin = dl + (T & 1) * S;  // the buffer the last frame did not read
    if (live) delta_last[j] = d, fin[j] = d;
    __threadfence();  // the back pointers of both waves, before they are read back
    __syncthreads();
    int s = 0;
    if (j == 0) first_max(fin, S, s);
    __syncthreads();  // fin is read: the chunks may overlay everything
    uint8_t* rows = reinterpret_cast<uint8_t*>(lds);
    int32_t* st = reinterpret_cast<int32_t*>(rows + HMM_TRACE_ROWS * S);
    for (int hi = T - 1; hi >= 0; hi -= HMM_TRACE_ROWS) {
        const int lo = hi - (HMM_TRACE_ROWS - 1) > 0 ? hi - (HMM_TRACE_ROWS - 1) : 0;
        const int n = hi - lo + 1;
        const uint8_t* src = backptr + (int64_t)lo * S;
        for (int idx = j; idx < n * S; idx += blockDim.x) rows[idx] = src[idx];
        __syncthreads();
        if (j == 0)
            for (int r = n - 1; r >= 0; --r) {
                st[r] = s;
                s = rows[r * S + s];  // (row 0 of backptr holds each state's own index)
            }
        __syncthreads();
        for (int r = j; r < n; r += blockDim.x) states[lo + r] = st[r];
        __syncthreads();
    }
}

__global__ __launch_bounds__(HMM_BLOCK) void hmm_posterior_kernel(const float* __restrict__ obs, const double* __restrict__ trans,
                                                                  const double* __restrict__ init, int T, int S, double* gamma, double* scale) {
#pragma clang fp contract(off)  // every product and sum below is rounded on its own, as the header defines them
    extern __shared__ __attribute__((aligned(16))) double lds[];  // tr [S][stride], two vectors [S]
    const int j = threadIdx.x;
    const bool live = j < S;
    const int jj = live ? j : 0;
    const int stride = dense_stride(S);
    double* tr = lds;
    double* va = lds + S * stride;  // forward: alpha of the frame before; backward: u of the odd frames
    double* vs = va + S;            // forward: a of this frame;           backward: u of the even frames
    stage_dense(tr, trans, S, stride);
    const double* col = tr + jj;
    double a = init[jj] * (double)obs[jj];
    for (int t = 0; t < T; ++t) {
        if (t > 0) {
            const double o = (double)obs[(int64_t)t * S + jj];
            double p = 0.0;
#pragma unroll 4
            for (int i = 0; i < S; ++i) p = p + va[i] * col[i * stride];
            a = p * o;
        }
        if (live) vs[j] = a;
        __syncthreads();  // (the first one also ends the staging)
        double c = 0.0;
        for (int k = 0; k < S; ++k) c = c + vs[k];
        const double alpha = a / c;
        if (live) gamma[(int64_t)t * S + j] = alpha, va[j] = alpha;
        if (j == 0) scale[t] = c;
        __syncthreads();
    }
    __threadfence();  // scale, written by lane 0, before the other wave reads it
    __syncthreads();
    const double* row = tr + jj * stride;
    double beta = 1.0;
    for (int t = T - 2; t >= 0; --t) {
        double* u = (t & 1) ? va : vs;
        const double o = (double)obs[(int64_t)(t + 1) * S + jj];
        if (live) u[j] = o * beta;
        const double c = scale[t + 1];
        const double alpha = gamma[(int64_t)t * S + jj];
        __syncthreads();
        double q = 0.0;
#pragma unroll 4
        for (int k = 0; k < S; ++k) q = q + row[k] * u[k];
        beta = q / c;
        if (live) gamma[(int64_t)t * S + j] = alpha * beta;
    }
}

bool hmm_shape_ok(int n_frames, int n_states) {
    return n_frames >= 1 && n_frames <= MAUA_HMM_MAX_FRAMES && n_states >= 1 && n_states <= MAUA_HMM_MAX_STATES;
}

}  // namespace

extern "C" int maua_hmm_viterbi_f64(const float* logobs, const double* log_trans, const double* log_init, int n_frames, int n_states,
                                    double* delta_last, uint8_t* backptr, int32_t* states, void* stream) {
    if (!logobs || !log_trans || !log_init || !delta_last || !backptr || !states) return MAUA_EINVAL;
    if (!hmm_shape_ok(n_frames, n_states)) return MAUA_EINVAL;
    const int S = n_states;
    const size_t forward = ((size_t)S * dense_stride(S) + 2 * S) * sizeof(double);                  // 131 KiB at S = 128
    const size_t walk = (size_t)HMM_TRACE_ROWS * S + (size_t)HMM_TRACE_ROWS * sizeof(int32_t);    // 132 KiB at S = 128
    const size_t lds = ((forward > walk ? forward : walk) + 15) / 16 * 16;
    static unsigned long long lds_ok = 0;
    if (int rc = maua_allow_full_lds(reinterpret_cast<const void*>(hmm_viterbi_kernel), &lds_ok)) return rc;
    hipLaunchKernelGGL(hmm_viterbi_kernel, dim3(1), dim3(ceil_div(S, 64) * 64), lds, (hipStream_t)stream, logobs, log_trans, log_init,
                       n_frames, S, delta_last, backptr, states);
    MAUA_LAUNCH_CHECK();
    return 0;
}

extern "C" int maua_hmm_posterior_f64(const float* obs, const double* trans, const double* init, int n_frames, int n_states, double* gamma,
                                      double* scale, void* stream) {
    if (!obs || !trans || !init || !gamma || !scale) return MAUA_EINVAL;
    if (!hmm_shape_ok(n_frames, n_states)) return MAUA_EINVAL;
    const int S = n_states;
    const size_t lds = (((size_t)S * dense_stride(S) + 2 * S) * sizeof(double) + 15) / 16 * 16;
    static unsigned long long lds_ok = 0;
    if (int rc = maua_allow_full_lds(reinterpret_cast<const void*>(hmm_posterior_kernel), &lds_ok)) return rc;
    hipLaunchKernelGGL(hmm_posterior_kernel, dim3(1), dim3(ceil_div(S, 64) * 64), lds, (hipStream_t)stream, obs, trans, init, n_frames, S,
                       gamma, scale);
    MAUA_LAUNCH_CHECK();
    return 0;
}
