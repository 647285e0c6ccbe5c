// The bar-pointer model for gfx950 — the device side of audioreactive.bars (bar_viterbi, raw_bars).  One entry; its definition is its
// comment in include/maua_hip.h and DESIGN.md 4.23, tests/bar_ref.py restates it in numpy.
//
// The model has sum(interval) * B states (4,000 for the default tempo range and a 4-beat bar) but only the K * B states that begin a
// beat have more than one predecessor: inside a beat the path is forced and its observations are two differences of prefix sums.  So
// the recursion runs over ENTRY values V[t][k][b] alone — an explicit-duration Viterbi — with K * K * B additions per frame.
//
// One workgroup per model (blockIdx.x), lane = k * B + b, everything the recursion touches per frame in LDS:
//   lc    [K][K | 1]      log_change, staged once; lane (k, b) walks the sources k' in order and reads lc[k' * stride + k]: the lanes of
//                         one k broadcast, neighbouring k are neighbouring doubles (dense_stride of wave.h, conflict-free).
//   X     [2][lanes]      the exit values of the frame, published in two buffers in turn: one barrier per frame.  Lane (k, b) reads
//                         X[k' * B + b']: B distinct runs, broadcast within each.
//   ring  [slot][lanes]   per lane its last interval[k] entry values, slot = t mod interval[k]: V[t - interval[k]] is read from the
//                         slot that V[t] then overwrites.  Lane-private: no barrier guards it.
// The walk is the defined order of the compares: nothing is reduced across lanes until the final state, where every lane's first
// maximum is walked by lane 0 in lane order — the same first maximum in ascending (k, b, j).
// The prefix sums are three serial chains on lanes 0 .. 2 (that IS their definition) in the workspace; the four of them a lane needs
// for frame t + 1 are loaded before the barrier of frame t, off the recursion's critical path.  Back pointers: one byte per
// (t, k, b) in the workspace.  The walk back is a chain of at most T / interval[0] dependent reads on lane 0, which leaves a segment
// list; every lane then fills the path of whole segments.
#include <math.h>

#include "common.h"
#include "wave.h"

namespace {

constexpr int BAR_LDS_LIMIT = 160 * 1024;
static_assert(MAUA_BAR_MAX_TEMPI <= 256, "a byte per back pointer");
static_assert(MAUA_BAR_MAX_TEMPI * MAUA_BAR_MAX_BEATS <= 1024, "a lane per (k, b)");
static_assert(MAUA_BAR_MAX_INTERVAL <= 65535, "intervals travel as uint16");

struct BarModel {  // by value in the kernarg segment: 544 bytes
    uint16_t interval[MAUA_BAR_MAX_TEMPI];
    uint16_t width[MAUA_BAR_MAX_TEMPI];
    int32_t beats[MAUA_BAR_MAX_MODELS];
};

struct BarSegment {  // frames max(e, 0) .. end of the path are (k, b, f - e)
    int32_t e, end, k, b;
};

// per-model regions of the workspace, in this order for all models: P [3][T + 1] doubles, segments [T + 1], back pointers [T][lanes]
__host__ __device__ inline int64_t bar_ws_p(int T) { return 3 * ((int64_t)T + 1) * (int64_t)sizeof(double); }
__host__ __device__ inline int64_t bar_ws_seg(int T) { return ((int64_t)T + 1) * (int64_t)sizeof(BarSegment); }
__host__ __device__ inline int64_t bar_ws_back(int T, int lanes) { return ((int64_t)T * lanes + 15) / 16 * 16; }

__global__ __launch_bounds__(1024) void bar_viterbi_kernel(const float* __restrict__ logobs, int T, const double* __restrict__ log_change,
                                                           int K, int max_lanes, int ring_len, int n_models, BarModel model,
                                                           unsigned char* __restrict__ ws, double* __restrict__ score,
                                                           int32_t* __restrict__ path) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int m = blockIdx.x;
    const int B = model.beats[m];
    const int L = K * B;
    const int lane = threadIdx.x;
    const bool live = lane < L;
    const int ll = live ? lane : 0;
    const int k = ll / B, b = ll % B;
    const int I = model.interval[k], W = model.width[k];
    const int stride = dense_stride(K);
    double* lc = lds;
    double* X = lc + K * stride;
    double* ring = X + 2 * max_lanes;
    double* P = reinterpret_cast<double*>(ws + m * bar_ws_p(T));
    BarSegment* seg = reinterpret_cast<BarSegment*>(ws + n_models * bar_ws_p(T) + m * bar_ws_seg(T));
    uint8_t* back = ws + n_models * (bar_ws_p(T) + bar_ws_seg(T)) + m * bar_ws_back(T, max_lanes);
    path += (int64_t)m * T * 3;

    // ---- prefix sums (lanes 0 .. 2: the block has at least 64), the matrix and the ring's zeros (everyone)
    if (lane < 3) {
        double* p = P + (int64_t)lane * (T + 1);
        double acc = 0.0;
        p[0] = acc;
        for (int n = 0; n < T; ++n) {
            acc = acc + (double)logobs[(int64_t)n * 3 + lane];
            p[n + 1] = acc;
        }
    }
    stage_dense(lc, log_change, K, stride);
    for (int idx = lane; idx < L * ring_len; idx += blockDim.x) ring[idx] = 0.0;
    __threadfence();  // the prefix sums, before the other waves read them
    __syncthreads();

    const double* P0 = P;
    const double* Pc = P + (int64_t)(b == 0 ? 2 : 1) * (T + 1);
    auto seg_sum = [&](int e, int end) {
        const int a0 = e > 0 ? e : 0;
        int a1 = e + W > 0 ? e + W : 0;
        a1 = a1 < end ? a1 : end;
        return (Pc[a1] - Pc[a0]) + (P0[end] - P0[a1]);
    };

    // ---- forward
    const int bp = b == 0 ? B - 1 : b - 1;
    const double* col = lc + k;
    double* mine = ring + ll;
    int slot = 0;  // t mod I
    double s = T > 1 ? seg_sum(1 - I, 1) : 0.0;
    for (int t = 1; t < T; ++t) {
        slot = slot + 1 == I ? 0 : slot + 1;
        double* pub = X + (t & 1) * max_lanes;
        if (live) pub[lane] = mine[slot * L] + s;
        if (t + 1 < T) s = seg_sum(t + 1 - I, t + 1);  // in flight across the barrier
        __syncthreads();
        const double* xs = pub + bp;
        double best = xs[0] + col[0];
        int arg = 0;
#pragma unroll 4
        for (int q = 1; q < K; ++q) {
            const double c = xs[q * B] + col[q * stride];
            if (c > best) best = c, arg = q;
        }
        if (live) {
            mine[slot * L] = best;
            back[(int64_t)t * L + lane] = (uint8_t)arg;
        }
    }

    // ---- the final state: every lane's first maximum over j, then lane 0 over the lanes
    double top = -INFINITY;
    int top_j = 0;
    for (int j = 0; j < I; ++j) {
        const int e = T - 1 - j;
        const double v = (e >= 1 ? mine[(e % I) * L] : 0.0) + seg_sum(e, T);
        if (v > top) top = v, top_j = j;
    }
    __syncthreads();  // X of the last frame is read
    int* xi = reinterpret_cast<int*>(X + max_lanes);  // [max_lanes] first maxima, behind them the segment count
    if (live) X[lane] = top, xi[lane] = top_j;
    __threadfence();  // the back pointers of every wave, before lane 0 reads them
    __syncthreads();
    if (lane == 0) {
        double best = -INFINITY;  // (not first_max: a NaN in X[0] is stepped over here and would stay there)
        int at = 0;
        for (int q = 0; q < L; ++q)
            if (X[q] > best) best = X[q], at = q;
        score[m] = best;
        int kk = at / B, bb = at % B, j = xi[at], t = T - 1, n = 0;
        for (;;) {
            const int e = t - j;
            seg[n++] = BarSegment{e, t, kk, bb};
            if (e <= 0) break;
            kk = back[(int64_t)e * L + kk * B + bb];
            bb = bb == 0 ? B - 1 : bb - 1;
            j = model.interval[kk] - 1;
            t = e - 1;
        }
        xi[max_lanes] = n;
    }
    __threadfence();  // the segments
    __syncthreads();
    const int n_seg = xi[max_lanes];
    for (int n = lane; n < n_seg; n += blockDim.x) {
        const BarSegment g = seg[n];
        for (int f = g.e > 0 ? g.e : 0; f <= g.end; ++f) {
            int32_t* dst = path + (int64_t)f * 3;
            dst[0] = g.k, dst[1] = g.b, dst[2] = f - g.e;
        }
    }
}

bool bar_counts_ok(int n_tempi, int max_beats) {
    return n_tempi >= 1 && n_tempi <= MAUA_BAR_MAX_TEMPI && max_beats >= 1 && max_beats <= MAUA_BAR_MAX_BEATS && n_tempi * max_beats <= 1024;
}

}  // namespace

extern "C" int64_t maua_bar_lds_bytes(int n_tempi, int max_beats, int max_interval) {
    if (!bar_counts_ok(n_tempi, max_beats) || max_interval < 1 || max_interval > MAUA_BAR_MAX_INTERVAL) return 0;
    const int64_t lanes = (int64_t)n_tempi * max_beats;
    // (two buffers of `lanes` doubles hold the lanes' first maxima as doubles, as ints, and one int more at the end: lanes >= 1)
    const int64_t bytes = ((int64_t)n_tempi * dense_stride(n_tempi) + 2 * lanes + lanes * max_interval) * (int64_t)sizeof(double);
    const int64_t padded = (bytes + 15) / 16 * 16;
    return padded <= BAR_LDS_LIMIT ? padded : 0;
}

extern "C" int64_t maua_bar_ws_bytes(int n_frames, int n_tempi, int max_beats, int n_models) {
    if (!bar_counts_ok(n_tempi, max_beats) || n_frames < 1 || n_frames > MAUA_BAR_MAX_FRAMES || n_models < 1 || n_models > MAUA_BAR_MAX_MODELS)
        return -1;
    return n_models * (bar_ws_p(n_frames) + bar_ws_seg(n_frames) + bar_ws_back(n_frames, n_tempi * max_beats));
}

extern "C" int maua_bar_viterbi_f64(const float* logobs, int n_frames, const int32_t* interval, const int32_t* width, const double* log_change,
                                    int n_tempi, const int32_t* beats_per_bar, int n_models, void* ws, double* score, int32_t* path,
                                    void* stream) {
    if (!logobs || !interval || !width || !log_change || !beats_per_bar || !ws || !score || !path) return MAUA_EINVAL;
    if (n_frames < 1 || n_frames > MAUA_BAR_MAX_FRAMES || n_tempi < 1 || n_tempi > MAUA_BAR_MAX_TEMPI) return MAUA_EINVAL;
    if (n_models < 1 || n_models > MAUA_BAR_MAX_MODELS) return MAUA_EINVAL;
    BarModel model = {};
    int max_beats = 0;
    for (int m = 0; m < n_models; ++m) {
        if (beats_per_bar[m] < 1 || beats_per_bar[m] > MAUA_BAR_MAX_BEATS) return MAUA_EINVAL;
        model.beats[m] = beats_per_bar[m];
        max_beats = beats_per_bar[m] > max_beats ? beats_per_bar[m] : max_beats;
    }
    for (int k = 0; k < n_tempi; ++k) {
        if (interval[k] < 1 || interval[k] > MAUA_BAR_MAX_INTERVAL || (k > 0 && interval[k] <= interval[k - 1])) return MAUA_EINVAL;
        if (width[k] < 1 || width[k] > interval[k]) return MAUA_EINVAL;
        model.interval[k] = (uint16_t)interval[k];
        model.width[k] = (uint16_t)width[k];
    }
    if (!bar_counts_ok(n_tempi, max_beats)) return MAUA_EINVAL;
    const int ring_len = interval[n_tempi - 1];
    const int64_t lds = maua_bar_lds_bytes(n_tempi, max_beats, ring_len);
    if (lds == 0) return MAUA_EINVAL;
    const int max_lanes = n_tempi * max_beats;
    static unsigned long long lds_ok = 0;
    if (int rc = maua_allow_full_lds(reinterpret_cast<const void*>(bar_viterbi_kernel), &lds_ok)) return rc;
    hipLaunchKernelGGL(bar_viterbi_kernel, dim3(n_models), dim3(ceil_div(max_lanes, 64) * 64), (size_t)lds, (hipStream_t)stream, logobs,
                       n_frames, log_change, n_tempi, max_lanes, ring_len, n_models, model, static_cast<unsigned char*>(ws), score, path);
    MAUA_LAUNCH_CHECK();
    return 0;
}
