// Structural segmentation kernels for gfx950 (the device side of audioreactive/segment.py, laplacian_segmentation).
//
//   tempogram       <- librosa.feature.tempogram (autocorrelation, Hann window, max-normalised) averaged over frames
//   beat_track      <- librosa.beat's local score (Gaussian-smoothed envelope) + the dynamic-programming beat search
//   beat_sync       <- librosa.util.sync (np.median / np.mean over variable spans of frames)
//   knn_links       <- librosa.segment.recurrence_matrix's k-nearest-neighbour search outside a diagonal band
//   rec_affinity    <- mutual links -> exp(-d / bandwidth), then timelag_filter(median_filter, size=(1, 7))
//
// Every kernel is deterministic: reductions run in a fixed order (xor-butterfly trees, per-block partials summed in block order),
// the only atomics are integer histogram counts in LDS.
#include <float.h>
#include <math.h>

#include "common.h"
#include "wave.h"

namespace {

// ------------------------------------------------------------------------------------------------ wave / block helpers

// Order-preserving map of a float onto an unsigned key (negative values reversed below the positive ones).
__device__ __forceinline__ unsigned fkey(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float funkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// ------------------------------------------------------------------------------------------------ tempogram
constexpr int TG_MAX_WIN = 1024;
constexpr int TG_MAX_BLOCKS = 512;
constexpr int TG_LAGS = TG_MAX_WIN / 256;

// Onset envelope padded by win/2 on each side with numpy's linear ramp to 0 (np.pad mode="linear_ramp").
__device__ __forceinline__ double tg_padded(const float* env, int n, int pad, int p) {
    const int e = p - pad;
    if (e < 0) return (double)p * ((double)env[0] / pad);
    if (e >= n) return (double)(pad - 1 - (e - n)) * ((double)env[n - 1] / pad);
    return (double)env[e];
}

// Block b takes frames b, b + G, b + 2G ... : frame t in LDS (fp64, windowed), one lag per thread (4 per thread for win <= 1024),
// direct sums, block max |ac|, normalised frames accumulated per lag in fp64 registers -> part[b][win].
__global__ __launch_bounds__(256) void tempogram_kernel(const float* __restrict__ env, int n, int win, double* __restrict__ part) {
    __shared__ double f[TG_MAX_WIN];
    __shared__ double wmax[4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int pad = win / 2;
    double acc[TG_LAGS];
    double wv[TG_LAGS];
#pragma unroll
    for (int m = 0; m < TG_LAGS; ++m) {
        acc[m] = 0.0;
        const int q = tid + 256 * m;
        wv[m] = 0.5 - 0.5 * cos(2.0 * M_PI * (double)q / (double)win);  // periodic Hann
    }
    for (int t = blockIdx.x; t < n; t += gridDim.x) {
        __syncthreads();  // the previous frame is no longer read
#pragma unroll
        for (int m = 0; m < TG_LAGS; ++m) {
            const int q = tid + 256 * m;
            if (q < win) f[q] = tg_padded(env, n, pad, t + q) * wv[m];
        }
        __syncthreads();
        double ac[TG_LAGS];
        double mx = 0.0;
#pragma unroll
        for (int m = 0; m < TG_LAGS; ++m) {
            const int l = tid + 256 * m;
            double s = 0.0;
            if (l < win)
                for (int q = 0; q + l < win; ++q) s = fma(f[q], f[q + l], s);
            ac[m] = s;
            mx = fmax(mx, fabs(s));
        }
        mx = wave_max(mx);
        if (lane == 0) wmax[wid] = mx;
        __syncthreads();
        mx = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
        const double norm = mx < (double)FLT_MIN ? 1.0 : mx;  // util.normalize leaves a (near-)silent frame as it is
#pragma unroll
        for (int m = 0; m < TG_LAGS; ++m) acc[m] += ac[m] / norm;
    }
#pragma unroll
    for (int m = 0; m < TG_LAGS; ++m) {
        const int l = tid + 256 * m;
        if (l < win) part[(int64_t)blockIdx.x * win + l] = acc[m];
    }
}

__global__ __launch_bounds__(256) void tempogram_mean_kernel(const double* __restrict__ part, int blocks, int win, int n,
                                                             float* __restrict__ tg) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= win) return;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += part[(int64_t)b * win + l];
    tg[l] = (float)(s / n);
}

static int tg_blocks(int n) { return n < TG_MAX_BLOCKS ? n : TG_MAX_BLOCKS; }

// ------------------------------------------------------------------------------------------------ beat tracking
constexpr int BT_MAX_PERIOD = 2000;
constexpr int BT_MAX_W = 3072;   // 2 period - round(period / 2) + 1 candidates
constexpr int BT_RING = 4096;    // cumulative scores of the last BT_RING frames (> 2 BT_MAX_PERIOD)

// localscore[i] = sum_j x[i + j] exp(-0.5 (j 32 / period)^2), j = -period .. period, zero outside (scipy.signal.convolve 'same').
__global__ __launch_bounds__(256) void beat_localscore_kernel(const double* __restrict__ x, int n, int period, double* __restrict__ ls) {
    __shared__ double taps[2 * BT_MAX_PERIOD + 1];
    for (int j = threadIdx.x; j <= 2 * period; j += 256) {
        const double a = (double)(j - period) * 32.0 / (double)period;
        taps[j] = exp(-0.5 * (a * a));
    }
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int lo = i - period < 0 ? period - i : 0;
    const int hi = i + period >= n ? period + (n - 1 - i) : 2 * period;
    double s = 0.0;
    for (int j = lo; j <= hi; ++j) s = fma(x[i - period + j], taps[j], s);
    ls[i] = s;
}

// The dynamic programme as one wave stepping through the frames.  Candidate j of frame i is the predecessor i + w0 + j,
// w0 = -2 period; it scores txwt[j] (+ cumscore of the predecessor when it exists).  Each lane scores the candidates
// j = lane, lane + 64 ..., keeping its first maximum; a xor butterfly then takes the larger score, the lower j on a tie — the
// first maximum, as np.argmax.  Cumulative scores live in an LDS ring; localscore is staged 64 frames at a time.
__global__ __launch_bounds__(64) void beat_dp_kernel(const double* __restrict__ ls, int n, int period, double* __restrict__ cum,
                                                     int* __restrict__ back) {
    __shared__ double txwt[BT_MAX_W];
    __shared__ double ring[BT_RING];
    __shared__ double lsbuf[64];
    const int lane = threadIdx.x;
    const int w0 = -2 * period;
    const int w1 = -(int)rint((double)period / 2.0);  // np.round: half to even
    const int W = w1 - w0 + 1;
    for (int j = lane; j < W; j += 64) {
        const double r = log((double)(-(w0 + j)) / (double)period);
        txwt[j] = -100.0 * (r * r);
    }
    double mx = -INFINITY;
    for (int i = lane; i < n; i += 64) mx = fmax(mx, ls[i]);
    const double thr = 0.01 * wave_max(mx);
    bool first = true;
    for (int i0 = 0; i0 < n; i0 += 64) {
        __syncthreads();
        lsbuf[lane] = i0 + lane < n ? ls[i0 + lane] : 0.0;
        __syncthreads();
        const int steps = n - i0 < 64 ? n - i0 : 64;
        for (int ii = 0; ii < steps; ++ii) {
            const int i = i0 + ii;
            double best = -INFINITY;
            int bj = W;
            for (int j = lane; j < W; j += 64) {
                const int idx = i + w0 + j;
                const double c = idx >= 0 ? txwt[j] + ring[idx & (BT_RING - 1)] : txwt[j];
                if (c > best) best = c, bj = j;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double ob = __shfl_xor(best, off);
                const int oj = __shfl_xor(bj, off);
                if (ob > best || (ob == best && oj < bj)) best = ob, bj = oj;
            }
            const double score = lsbuf[ii];
            const double ci = score + best;
            const bool none = first && score < thr;
            __syncthreads();  // every lane has read the ring for this frame
            if (lane == 0) {
                ring[i & (BT_RING - 1)] = ci;
                cum[i] = ci;
                back[i] = none ? -1 : i + w0 + bj;
            }
            first = none;
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------------ beat-synchronous aggregation
// k-th smallest (0-based rank) of src[0 .. L) by a 4-pass 8-bit radix select over the float keys; one wave, hist = 256 ints of LDS
// owned by the wave.  Every wave of the block runs the same passes (the block barriers are shared).
__device__ unsigned wave_select(const float* __restrict__ src, int L, int rank, int* hist, int lane, bool active) {
    unsigned prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int b = lane; b < 256; b += 64) hist[b] = 0;
        __syncthreads();
        if (active)
            for (int i = lane; i < L; i += 64) {
                const unsigned key = fkey(src[i]);
                if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
            }
        __syncthreads();
        const int c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
        const int incl = wave_incl_sum(c0 + c1 + c2 + c3, lane);
        const int excl = incl - (c0 + c1 + c2 + c3);
        const unsigned long long hit = __ballot(excl <= rank && rank < incl);
        int bin = 0, before = excl;
        if (rank < excl + c0) bin = 0;
        else if (rank < excl + c0 + c1) bin = 1, before += c0;
        else if (rank < excl + c0 + c1 + c2) bin = 2, before += c0 + c1;
        else bin = 3, before += c0 + c1 + c2;
        const int src_lane = hit ? __ffsll((long long)hit) - 1 : 0;
        bin = __shfl(4 * lane + bin, src_lane);
        before = __shfl(before, src_lane);
        prefix |= (unsigned)bin << shift;
        mask |= 255u << shift;
        rank -= before;
    }
    return prefix;
}

// out[r][s] = aggregate of x[r][bounds[s] .. bounds[s + 1]); one wave per row, four rows per block, one span per blockIdx.x.
__global__ __launch_bounds__(256) void beat_sync_kernel(const float* __restrict__ x, int rows, int n_frames, const int* __restrict__ bounds,
                                                        int n_spans, int median, float* __restrict__ out) {
    __shared__ int hist[4][256];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int s = blockIdx.x;
    const int r = blockIdx.y * 4 + wid;
    const bool active = r < rows;
    // the bounds table clamped as a table: each bound inside [0, n_frames] and not below any bound before it (a span never starts
    // before the end of the one before it)
    int b0 = 0;
    for (int q = lane; q <= s; q += 64) b0 = max(b0, bounds[q]);
    b0 = wave_max(b0);
    b0 = b0 > n_frames ? n_frames : b0;
    int b1 = bounds[s + 1];
    b1 = b1 < b0 ? b0 : (b1 > n_frames ? n_frames : b1);
    const int L = b1 - b0;
    const float* src = x + (int64_t)(active ? r : 0) * n_frames + b0;
    float v;
    if (L == 0) {
        v = __uint_as_float(0x7fc00000u);  // empty span: NaN, as np.median / np.mean of nothing
    } else if (median) {
        const float hi = funkey(wave_select(src, L, L / 2, hist[wid], lane, active));
        if (L & 1) {
            v = hi;
        } else {
            const float lo = funkey(wave_select(src, L, L / 2 - 1, hist[wid], lane, active));
            v = (lo + hi) * 0.5f;
        }
    } else {
        double sum = 0.0;
        if (active)
            for (int i = lane; i < L; i += 64) sum += (double)src[i];
        sum = wave_sum(sum);
        v = (float)(sum / L);
    }
    if (active && lane == 0) out[(int64_t)r * n_spans + s] = v;
}

// ------------------------------------------------------------------------------------------------ k-nearest-neighbour links
constexpr int KNN_MAX_S = 8192;
constexpr int KNN_MAX_D = 1024;

// Block-wide exclusive scan of one int per thread (256 threads); wsum = 4 ints of LDS.
__device__ __forceinline__ int block_excl_scan(int v, int* wsum, int* total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int incl = wave_incl_sum(v, lane);
    __syncthreads();
    if (lane == 63) wsum[wid] = incl;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wid; ++w) base += wsum[w];
    *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    return base + incl - v;
}

// One row i per block: d[j] = sqrt(sum_f (x[f][i] - x[f][j])^2) in LDS (the same operation order for (i, j) and (j, i): d is exactly
// symmetric), then the k smallest (d, j) pairs among |i - j| >= width: the k-th smallest distance by radix select, the ties at it
// given to the lowest j by an ordered block scan.  out[i][j] = d[j] on a link, -1 elsewhere.
__global__ __launch_bounds__(256) void knn_links_kernel(const float* __restrict__ x, int D, int S, int k, int width, float* __restrict__ out) {
    __shared__ float dist[KNN_MAX_S];
    __shared__ float xi[KNN_MAX_D];
    __shared__ int hist[256];
    __shared__ int wsum[4];
    __shared__ int sel[2];
    const int tid = threadIdx.x;
    const int i = blockIdx.x;
    for (int f = tid; f < D; f += 256) xi[f] = x[(int64_t)f * S + i];
    __syncthreads();
    for (int j = tid; j < S; j += 256) {
        float acc = 0.f;
        for (int f = 0; f < D; ++f) {
            const float diff = xi[f] - x[(int64_t)f * S + j];
            acc = fmaf(diff, diff, acc);
        }
        dist[j] = sqrtf(acc);
    }
    __syncthreads();
    const int band_lo = i - width + 1 < 0 ? 0 : i - width + 1;
    const int band_hi = i + width - 1 > S - 1 ? S - 1 : i + width - 1;
    const int n_valid = S - (band_hi - band_lo + 1);
    const int kk = k < n_valid ? k : n_valid;
    unsigned vstar = 0xffffffffu;
    int need_equal = S;  // kk == n_valid: every valid j is a link
    if (kk < n_valid) {
        int rank = kk - 1;
        unsigned prefix = 0, mask = 0;
        for (int shift = 24; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            for (int j = tid; j < S; j += 256) {
                if (j >= band_lo && j <= band_hi) continue;
                const unsigned key = fkey(dist[j]);
                if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
            }
            __syncthreads();
            const int c = hist[tid];
            int total;
            const int excl = block_excl_scan(c, wsum, &total);
            if (excl <= rank && rank < excl + c) sel[0] = tid, sel[1] = excl;
            __syncthreads();
            prefix |= (unsigned)sel[0] << shift;
            mask |= 255u << shift;
            rank -= sel[1];
            __syncthreads();  // sel is rewritten by the next pass
        }
        vstar = prefix;
        need_equal = rank + 1;  // links among the distances equal to the k-th one
    }
    // ordered pass: thread t owns the contiguous j range [t chunk, (t + 1) chunk)
    const int chunk = (S + 255) / 256;
    const int j0 = tid * chunk, j1 = j0 + chunk < S ? j0 + chunk : S;
    int eq = 0;
    for (int j = j0; j < j1; ++j)
        if ((j < band_lo || j > band_hi) && fkey(dist[j]) == vstar) ++eq;
    int total;
    int before = block_excl_scan(eq, wsum, &total);
    __syncthreads();
    for (int j = j0; j < j1; ++j) {
        bool link = false;
        if (j < band_lo || j > band_hi) {
            const unsigned key = fkey(dist[j]);
            if (key < vstar) link = true;
            else if (key == vstar) link = before++ < need_equal;
        }
        if (!link) dist[j] = -1.f;
    }
    __syncthreads();
    for (int j = tid; j < S; j += 256) out[(int64_t)i * S + j] = dist[j];
}

// ------------------------------------------------------------------------------------------------ affinity + time-lag median
// rec[i][j] = exp(-d / bandwidth) where i links j AND j links i, 0 elsewhere; 32 x 32 tiles, the transposed tile through LDS.
__global__ __launch_bounds__(256) void rec_affinity_kernel(const float* __restrict__ lnk, int S, float bandwidth, float* __restrict__ rec) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int bi = blockIdx.y * 32, bj = blockIdx.x * 32;
    for (int r = ty; r < 32; r += 8) {
        const int row = bj + r, col = bi + tx;
        tile[r][tx] = (row < S && col < S) ? lnk[(int64_t)row * S + col] : -1.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int i = bi + r, j = bj + tx;
        if (i >= S || j >= S) continue;
        const float a = lnk[(int64_t)i * S + j];
        const float b = tile[tx][r];  // lnk[j][i]
        rec[(int64_t)i * S + j] = (a >= 0.f && b >= 0.f) ? expf(a / -bandwidth) : 0.f;
    }
}

// timelag_filter(median_filter, size=(1, 7)): filt[i][j] = median over s = -3..3 of rec[i - j + j'][j'], j' = j + s reflected at the
// edges (scipy 'reflect': d c b a | a b c d), 0 for a row outside [0, S) (the zero rows of the padded lag matrix).
__global__ __launch_bounds__(256) void rec_timelag_median_kernel(const float* __restrict__ rec, int S, float* __restrict__ filt) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= S) return;
    float v[7];
#pragma unroll
    for (int s = 0; s < 7; ++s) {
        int jp = j + s - 3;
        jp = jp < 0 ? -jp - 1 : (jp >= S ? 2 * S - jp - 1 : jp);
        const int row = i - j + jp;
        v[s] = (row >= 0 && row < S) ? rec[(int64_t)row * S + jp] : 0.f;
    }
    // the element of rank 3 (ties broken by position)
    float med = v[0];
#pragma unroll
    for (int a = 0; a < 7; ++a) {
        int rank = 0;
#pragma unroll
        for (int b = 0; b < 7; ++b) rank += (v[b] < v[a]) || (v[b] == v[a] && b < a);
        if (rank == 3) med = v[a];
    }
    filt[(int64_t)i * S + j] = med;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int64_t maua_tempogram_ws_doubles(int n_frames, int win) {
    if (n_frames <= 0 || win <= 0) return 0;
    return (int64_t)tg_blocks(n_frames) * win;
}

extern "C" int maua_tempogram_f32(const float* env, int n_frames, int win, double* ws, float* tg, void* stream) {
    if (!env || !ws || !tg || n_frames <= 0 || win < 2 || win > TG_MAX_WIN) return MAUA_EINVAL;
    const int blocks = tg_blocks(n_frames);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tempogram_kernel, dim3(blocks), dim3(256), 0, st, env, n_frames, win, ws);
    MAUA_LAUNCH_CHECK();
    hipLaunchKernelGGL(tempogram_mean_kernel, dim3(ceil_div(win, 256)), dim3(256), 0, st, ws, blocks, win, n_frames, tg);
    MAUA_LAUNCH_CHECK();
    return 0;
}

extern "C" int maua_beat_track_f64(const double* onset, int n_frames, int period, double* localscore, double* cumscore, int* backlink,
                                   void* stream) {
    if (!onset || !localscore || !cumscore || !backlink || n_frames <= 0 || period < 2 || period > BT_MAX_PERIOD) return MAUA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(beat_localscore_kernel, dim3(ceil_div(n_frames, 256)), dim3(256), 0, st, onset, n_frames, period, localscore);
    MAUA_LAUNCH_CHECK();
    hipLaunchKernelGGL(beat_dp_kernel, dim3(1), dim3(64), 0, st, localscore, n_frames, period, cumscore, backlink);
    MAUA_LAUNCH_CHECK();
    return 0;
}

extern "C" int maua_beat_sync_f32(const float* x, int rows, int n_frames, const int* bounds, int n_spans, int median, float* out,
                                  void* stream) {
    if (!x || !bounds || !out || rows <= 0 || n_frames <= 0 || n_spans <= 0 || (median != 0 && median != 1)) return MAUA_EINVAL;
    hipLaunchKernelGGL(beat_sync_kernel, dim3(n_spans, ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, rows, n_frames, bounds,
                       n_spans, median, out);
    MAUA_LAUNCH_CHECK();
    return 0;
}

extern "C" int maua_knn_links_f32(const float* x, int d, int s, int k, int width, float* links, void* stream) {
    if (!x || !links || d <= 0 || d > KNN_MAX_D || s <= 1 || s > KNN_MAX_S || k <= 0 || width < 1) return MAUA_EINVAL;
    hipLaunchKernelGGL(knn_links_kernel, dim3(s), dim3(256), 0, (hipStream_t)stream, x, d, s, k, width, links);
    MAUA_LAUNCH_CHECK();
    return 0;
}

extern "C" int maua_rec_affinity_f32(const float* links, int s, float bandwidth, float* rec, float* rec_filt, void* stream) {
    if (!links || !rec || !rec_filt || s < 4 || s > KNN_MAX_S || !(bandwidth > 0.f) || !isfinite(bandwidth)) return MAUA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rec_affinity_kernel, dim3(ceil_div(s, 32), ceil_div(s, 32)), dim3(256), 0, st, links, s, bandwidth, rec);
    MAUA_LAUNCH_CHECK();
    hipLaunchKernelGGL(rec_timelag_median_kernel, dim3(ceil_div(s, 256), s), dim3(256), 0, st, rec, s, rec_filt);
    MAUA_LAUNCH_CHECK();
    return 0;
}
