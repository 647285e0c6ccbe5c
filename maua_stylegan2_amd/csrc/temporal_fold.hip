// Temporal supersampling: fold `subframes` consecutive uint8 frames into one by a weighted average (a shutter), the first per-frame step
// behind the generator's frame epilogue (render.py fold_frames): N sub-frames are synthesised per delivered frame, one leaves the device.
//
// A frame is a flat run of `frame_bytes` bytes; nothing here knows about pixels.  With weights w_i (0 .. 255, N <= 16) and W = sum w_i:
//   encoded light   out[g][j] = (sum_i w_i * in[g N + i][j] + W / 2) / W                                   (`/` is floor: half up)
//   linear light    L = (sum_i w_i * decode[in[g N + i][j]] + W / 2) / W,   out[g][j] = max{ v : encode_threshold[v] <= L }
// in integers only.  The largest numerator is 16 * 255 * 65535 + 2040 < 2^28, so 32-bit unsigned sums are exact, and the division by the
// per-launch constant W <= 4080 < 2^12 is an exact multiply-shift (Granlund & Montgomery, "Division by invariant integers using
// multiplication", 1994, theorem 4.2 with 28-bit numerators and l = 12): floor(n / W) = (n * ceil(2^40 / W)) >> 40 for every n < 2^28;
// n * magic < W * 2^16 * (2^40 / W + 1) < 2^57 fits 64 bits.
//
// Memory-bound: N bytes read per byte written.  A thread owns one 16-byte column and walks the N frames of its group: N 16-byte loads,
// one 16-byte store, 16 accumulators in registers.  Columns are cut on the 16-byte grid of the ADDRESSES: when every frame of `in` and
// `out` starts at the same offset from that grid (frame_bytes % 16 == 0 and in, out congruent modulo 16 — the render path: H * W * 3
// bytes, allocator-aligned buffers) the first and the last column of a frame may be partial (the head and the tail, done byte by byte
// by their thread) and every other column is one aligned vector access.  Any other layout (a frame size off the grid leaves every
// frame at another offset) takes the byte path, chosen per launch: one thread per output byte.  No access leaves [in, in + groups * N *
// frame_bytes) or [out, out + groups * frame_bytes) on either path.
// Linear light keeps both 256-entry tables in LDS (2 x 512 bytes); the threshold search is 8 halving steps.
#include "common.h"

namespace {
constexpr int MAX_SUBFRAMES = 16;

struct FoldWeights {
    uint32_t w[MAX_SUBFRAMES];  // by value in the kernel arguments: a captured launch carries them
};

// numerator -> output byte.  thr: the threshold table in LDS (LINEAR only)
template <bool LINEAR>
__device__ __forceinline__ uint32_t fold_finish(uint32_t acc, uint32_t half, uint64_t magic, const uint16_t* thr) {
    const uint32_t q = (uint32_t)(((uint64_t)(acc + half) * magic) >> 40);
    if constexpr (LINEAR) {
        uint32_t v = 0;  // thr[0] == 0 <= q; v + step <= 255
#pragma unroll
        for (uint32_t step = 128; step >= 1; step >>= 1)
            if (thr[v + step] <= q) v += step;
        return v;
    } else {
        return q;
    }
}

// one output byte: frame byte j of the group whose first sub-frame starts at src
template <bool LINEAR>
__device__ __forceinline__ uint8_t fold_byte(const uint8_t* __restrict__ src, int64_t j, int n, int64_t frame_bytes, const FoldWeights& wt,
                                             uint32_t half, uint64_t magic, const uint16_t* dec, const uint16_t* thr) {
    uint32_t acc = 0;
    for (int i = 0; i < n; ++i) {
        const uint32_t b = src[i * frame_bytes + j];
        acc += wt.w[i] * (LINEAR ? (uint32_t)dec[b] : b);
    }
    return (uint8_t)fold_finish<LINEAR>(acc, half, magic, thr);
}

// grid: y = group, x walks the group's units.  VEC: a unit is a 16-byte column of the address grid — unit u holds the frame bytes
// [16 u - lead, 16 u - lead + 16) that exist, lead = in & 15 = out & 15; units = ceil((lead + frame_bytes) / 16).  !VEC: a unit is a byte.
template <bool LINEAR, bool VEC>
__global__ __launch_bounds__(256) void temporal_fold_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int n,
                                                            int64_t frame_bytes, int64_t units, int lead, FoldWeights wt, uint32_t half,
                                                            uint64_t magic, const uint16_t* __restrict__ decode,
                                                            const uint16_t* __restrict__ encode_threshold) {
    __shared__ uint16_t dec[LINEAR ? 256 : 1], thr[LINEAR ? 256 : 1];
    if constexpr (LINEAR) {
        dec[threadIdx.x] = decode[threadIdx.x];
        thr[threadIdx.x] = encode_threshold[threadIdx.x];
        __syncthreads();
    }
    const int64_t g = blockIdx.y;
    const uint8_t* __restrict__ src = in + g * n * frame_bytes;
    uint8_t* __restrict__ dst = out + g * frame_bytes;
    for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < units; u += (int64_t)gridDim.x * 256) {
        if constexpr (VEC) {
            const int64_t j0 = 16 * u - lead;
            if (j0 >= 0 && j0 + 16 <= frame_bytes) {
                uint32_t acc[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) acc[k] = 0;
                for (int i = 0; i < n; ++i) {
                    const uint4 v = *reinterpret_cast<const uint4*>(src + i * frame_bytes + j0);
                    const uint32_t w = wt.w[i];
                    const uint32_t word[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        const uint32_t b = (word[k >> 2] >> ((k & 3) * 8)) & 0xffu;
                        acc[k] += w * (LINEAR ? (uint32_t)dec[b] : b);
                    }
                }
                uint32_t packed[4] = {0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < 16; ++k) packed[k >> 2] |= fold_finish<LINEAR>(acc[k], half, magic, thr) << ((k & 3) * 8);
                *reinterpret_cast<uint4*>(dst + j0) = make_uint4(packed[0], packed[1], packed[2], packed[3]);
            } else {  // the head or the tail of the frame: only the bytes that exist
                const int64_t lo = j0 > 0 ? j0 : 0, hi = j0 + 16 < frame_bytes ? j0 + 16 : frame_bytes;
                for (int64_t j = lo; j < hi; ++j) dst[j] = fold_byte<LINEAR>(src, j, n, frame_bytes, wt, half, magic, dec, thr);
            }
        } else {
            dst[u] = fold_byte<LINEAR>(src, u, n, frame_bytes, wt, half, magic, dec, thr);
        }
    }
}

template <bool LINEAR, bool VEC>
int launch_fold(const uint8_t* in, uint8_t* out, int groups, int n, int64_t frame_bytes, int64_t units, int lead, const FoldWeights& wt,
                uint32_t half, uint64_t magic, const uint16_t* decode, const uint16_t* encode_threshold, hipStream_t st) {
    const int64_t blocks = ceil_div64(units, 256);
    const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536), (unsigned)groups);
    hipLaunchKernelGGL((temporal_fold_kernel<LINEAR, VEC>), grid, dim3(256), 0, st, in, out, n, frame_bytes, units, lead, wt, half, magic,
                       decode, encode_threshold);
    MAUA_LAUNCH_CHECK();
    return 0;
}
}  // namespace

extern "C" int maua_temporal_fold_u8(const uint8_t* in, uint8_t* out, int groups, int subframes, int64_t frame_bytes, const uint8_t* weights,
                                     const uint16_t* decode, const uint16_t* encode_threshold, void* stream) {
    if (subframes < 1 || subframes > MAX_SUBFRAMES || frame_bytes <= 0 || groups < 0 || !weights) return MAUA_EINVAL;
    if ((decode == nullptr) != (encode_threshold == nullptr)) return MAUA_EINVAL;
    FoldWeights wt = {};
    uint32_t total = 0;
    for (int i = 0; i < subframes; ++i) total += (wt.w[i] = weights[i]);
    if (total == 0) return MAUA_EINVAL;
    if (groups == 0) return 0;
    if (!in || !out) return MAUA_EINVAL;
    // (the group is the grid's y; the byte ranges below stay far inside int64)
    if (groups > 65535 || frame_bytes > (int64_t)1 << 40) return MAUA_ENOSYS;
    const uintptr_t in_lo = (uintptr_t)in, in_hi = in_lo + (uintptr_t)((int64_t)groups * subframes * frame_bytes);
    const uintptr_t out_lo = (uintptr_t)out, out_hi = out_lo + (uintptr_t)((int64_t)groups * frame_bytes);
    if (in_lo < out_hi && out_lo < in_hi) return MAUA_EINVAL;  // a group's output would overwrite another group's input
    const uint32_t half = total / 2;
    const uint64_t magic = (((uint64_t)1 << 40) + total - 1) / total;
    const int lead = (int)(in_lo & 15);
    const bool vec = frame_bytes % 16 == 0 && lead == (int)(out_lo & 15);
    const int64_t units = vec ? ceil_div64(lead + frame_bytes, 16) : frame_bytes;
    const hipStream_t st = (hipStream_t)stream;
    if (decode) {
        return vec ? launch_fold<true, true>(in, out, groups, subframes, frame_bytes, units, lead, wt, half, magic, decode, encode_threshold, st)
                   : launch_fold<true, false>(in, out, groups, subframes, frame_bytes, units, 0, wt, half, magic, decode, encode_threshold, st);
    }
    return vec ? launch_fold<false, true>(in, out, groups, subframes, frame_bytes, units, lead, wt, half, magic, nullptr, nullptr, st)
               : launch_fold<false, false>(in, out, groups, subframes, frame_bytes, units, 0, wt, half, magic, nullptr, nullptr, st);
}
