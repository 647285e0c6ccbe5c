// Wave-wide (64-lane) reductions and scans, and the few lines the dense decoders (hmm.hip, bar.hip) share.  The shuffle order
// of every helper is part of its definition: the sums and the ties of the kernels that use them are pinned bit for bit by their tests.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

// ---- xor butterflies, offsets 32, 16, 8, 4, 2, 1: every lane ends with the result
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        if constexpr (std::is_floating_point_v<T>)
            v = fmax(v, __shfl_xor(v, off, 64));
        else
            v = max(v, __shfl_xor(v, off, 64));
    }
    return v;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

// ---- inclusive scans over the lanes by __shfl_up, distances 1, 2, ... 32
template <typename T>
__device__ __forceinline__ T wave_incl_sum(T v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

__device__ __forceinline__ float wave_incl_min(float v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float o = __shfl_up(v, off, 64);
        if (lane >= off && o < v) v = o;
    }
    return v;
}

// ---- dense decoders: an [n][n] double matrix in LDS with a row stride of n | 1 (n, or n + 1 where n is even): lanes that walk a column
// read neighbouring doubles, lanes that walk a row are an odd number of doubles apart — conflict-free both ways
__host__ __device__ constexpr int dense_stride(int n) { return n | 1; }

__device__ __forceinline__ void stage_dense(double* dst, const double* __restrict__ src, int n, int stride) {
    for (int idx = threadIdx.x; idx < n * n; idx += blockDim.x) dst[(idx / n) * stride + idx % n] = src[idx];
}

// the first maximum of v[0 .. n - 1], walked by one lane in index order: strict >, so the lowest index wins and a NaN in v[0] stays
__device__ __forceinline__ double first_max(const double* v, int n, int& arg) {
    double best = v[0];
    arg = 0;
    for (int k = 1; k < n; ++k)
        if (v[k] > best) best = v[k], arg = k;
    return best;
}
