// Looping latent sequences (audioreactive/latent.py: spline_loops, slerp_loops, loop_sections) as one gather-and-blend launch.
//
// Both loop kinds are LINEAR in their keys once the knot count and the period (spline) or the leg angles (slerp) are known: a frame is a
// row of a small weight matrix times the keys of its section,
//   out[f, :] = sum_i weights[row_of_frame[f], i] * bank[key_idx[sec_of_frame[f], i], :],
// so a whole sectioned sequence is one launch whose only real traffic is the write of out [n_frames, feats] (18 x 512 floats per frame);
// the bank (a latent selection, a few hundred KB) is re-read from L2, the tables are a few KB.  No LDS: a frame's weight row and key
// indices are uniform across its workgroup and arrive through the scalar cache, every lane streams its own 16 bytes of the keys.
#include "common.h"

namespace {

__device__ __forceinline__ int clamp_index(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// grid-stride over tiles = (frame, chunk of blockDim.x quads); a thread owns 4 consecutive features (a quad) of one frame.  VEC (feats % 4
// == 0, bank and out 16-byte aligned): 16-byte loads and one 16-byte store; otherwise element by element.  Both forms run the same chain
// per element — acc = fmaf(w_i, key_i, acc) for i ascending from acc = 0, a zero weight leaving acc as it is (so columns a shorter
// section does not use, and whatever key they point at, never touch the value) — and give the same bits.  The keys are fetched four
// at a time before their multiply-adds so that four L2 round trips overlap.  Indices read from the tables are clamped into their
// tables: a bad table gives a wrong frame, never an access outside bank / weights / key_idx.
template <bool VEC>
__global__ __launch_bounds__(256) void keyframe_blend_kernel(const float* __restrict__ bank, int n_bank, int feats,
                                                             const int* __restrict__ key_idx, const float* __restrict__ weights,
                                                             const int* __restrict__ row_of_frame, const int* __restrict__ sec_of_frame,
                                                             float* __restrict__ out, int n_sections, int n_rows, int kmax, int chunks,
                                                             int64_t tiles) {
    const int quads = (feats + 3) / 4;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int f = (int)(tile / chunks);
        const int q = (int)(tile - (int64_t)f * chunks) * (int)blockDim.x + (int)threadIdx.x;
        if (q >= quads) continue;
        const float* w = weights + (size_t)clamp_index(row_of_frame[f], n_rows) * kmax;
        const int* ki = key_idx + (size_t)clamp_index(sec_of_frame[f], n_sections) * kmax;
        const int e = q * 4;
        const int n = feats - e < 4 ? feats - e : 4;  // (VEC: always 4)
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i0 = 0; i0 < kmax; i0 += 4) {
            float wv[4], v[4][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {  // past kmax: weight 0 on the last key again (no branch around the load)
                const int i = i0 + j < kmax ? i0 + j : kmax - 1;
                wv[j] = i0 + j < kmax ? w[i] : 0.f;
                const float* src = bank + (size_t)clamp_index(ki[i], n_bank) * feats + e;
                if (VEC) {
                    const float4 t = *reinterpret_cast<const float4*>(src);
                    v[j][0] = t.x, v[j][1] = t.y, v[j][2] = t.z, v[j][3] = t.w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[j][k] = k < n ? src[k] : 0.f;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (wv[j] != 0.f) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[k] = fmaf(wv[j], v[j][k], acc[k]);
                }
        }
        float* dst = out + (size_t)f * feats + e;
        if (VEC) {
            *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) dst[k] = acc[k];
        }
    }
}

}  // namespace

extern "C" int maua_keyframe_blend_f32(const float* bank, int n_bank, int feats, const int* key_idx, const float* weights,
                                       const int* row_of_frame, const int* sec_of_frame, float* out, int n_frames, int n_sections, int n_rows,
                                       int kmax, void* stream) {
    if (n_bank <= 0 || feats <= 0 || n_frames < 0 || n_sections <= 0 || n_rows <= 0 || kmax <= 0 || kmax > MAUA_LOOP_MAX_KEYS) return MAUA_EINVAL;
    if (n_frames == 0) return 0;
    if (!bank || !key_idx || !weights || !row_of_frame || !sec_of_frame || !out) return MAUA_EINVAL;
    const int quads = (feats + 3) / 4;
    const int threads = quads <= 64 ? 64 : 256;
    const int chunks = ceil_div(quads, threads);
    const int64_t tiles = (int64_t)n_frames * chunks;
    const dim3 grid((unsigned)(tiles < 2048 ? tiles : 2048));  // 8 workgroups of 4 waves per CU, the rest by the grid stride
    const bool vec = feats % 4 == 0 && (((uintptr_t)bank | (uintptr_t)out) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(keyframe_blend_kernel<true>, grid, dim3(threads), 0, (hipStream_t)stream, bank, n_bank, feats, key_idx, weights,
                           row_of_frame, sec_of_frame, out, n_sections, n_rows, kmax, chunks, tiles);
    else
        hipLaunchKernelGGL(keyframe_blend_kernel<false>, grid, dim3(threads), 0, (hipStream_t)stream, bank, n_bank, feats, key_idx, weights,
                           row_of_frame, sec_of_frame, out, n_sections, n_rows, kmax, chunks, tiles);
    MAUA_LAUNCH_CHECK();
    return 0;
}
