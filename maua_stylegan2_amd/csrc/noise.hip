// Seeded per-frame N(0,1) noise maps, generated on the device (include/maua_hip.h, "counter-based noise"): the map of
// (seed, absolute frame, slot) is a pure function — Philox4x32-10 (Salmon et al., SC'11) + Box-Muller — so one table-driven launch at
// the head of a captured forward fills the maps of every randomised layer of one batch, identically for every batch size, lane and shard.
#include "common.h"
#include "philox.h"  // philox4x32_10, box_muller: shared with csrc/noise_synth.hip

namespace {

using namespace maua_philox;

// One thread = four consecutive floats of one map.  The table lives in device memory, so the host cannot size the grid by it: every
// workgroup builds the prefix sums of the slots' quad counts (<= 32 entries) in LDS and the grid strides over their total.
__global__ __launch_bounds__(256) void randn_frames_kernel(const maua_randn_slot_t* __restrict__ table, int n_slots, int batch,
                                                           uint32_t key0, uint32_t key1, int frame0, maua_frame_source_t* src) {
    __shared__ int64_t first_quad[MAUA_MAX_NOISE_SLOTS + 1];
    __shared__ maua_randn_slot_t slots[MAUA_MAX_NOISE_SLOTS];
    if (threadIdx.x == 0) {
        int64_t acc = 0;
        for (int i = 0; i < n_slots; ++i) {
            maua_randn_slot_t e = table[i];
            if (!e.dst || e.hw < 1) e.hw = 0;  // an empty entry produces nothing
            slots[i] = e;
            first_quad[i] = acc;
            acc += (int64_t)batch * ((e.hw + 3) / 4);
        }
        first_quad[n_slots] = acc;
    }
    __syncthreads();
    // frames of this launch: [first, first + batch).  With a frame source the sequences it points at start at absolute frame `frame0`
    // (0 unless the caller holds one shard of a job) and the launch at src->frame0 inside them.
    const int64_t local0 = src ? (int64_t)src->frame0 : 0;
    const uint32_t first = (uint32_t)(local0 + frame0);
    if (src && blockIdx.x == 0 && (int)threadIdx.x < n_slots) {
        // the layers read noise[slot] + (src->frame0 + b) * noise_stride[slot]: bias the pointer so that this lands on dst + b * hw.
        // Integer arithmetic: the biased value is only ever an operand of that sum, never dereferenced.
        const maua_randn_slot_t e = slots[threadIdx.x];
        if (e.hw > 0 && e.slot >= 0 && e.slot < MAUA_MAX_NOISE_SLOTS) {
            const uint64_t biased = (uint64_t)(uintptr_t)e.dst - (uint64_t)local0 * (uint64_t)e.hw * sizeof(float);
            src->noise[e.slot] = (const float*)(uintptr_t)biased;
            src->noise_stride[e.slot] = e.hw;
        }
    }
    const int64_t total = first_quad[n_slots];
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        int lo = 0, hi = n_slots - 1;  // last slot whose first quad is <= q (empty slots share their successor's start and lose)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (first_quad[mid] <= q) lo = mid; else hi = mid - 1;
        }
        const maua_randn_slot_t e = slots[lo];
        const int64_t r = q - first_quad[lo];
        const uint32_t quads = (uint32_t)(e.hw + 3) / 4u;
        uint32_t b, i;
        if (r <= 0xFFFFFFFFll) {
            b = (uint32_t)r / quads;
            i = (uint32_t)r - b * quads;
        } else {
            b = (uint32_t)(r / quads);
            i = (uint32_t)(r - (int64_t)b * quads);
        }
        const U4 x = philox4x32_10(U4{i, first + b, (uint32_t)e.slot, 0u}, key0, key1);
        float4 z;
        box_muller(x.x, x.y, z.x, z.y);
        box_muller(x.z, x.w, z.z, z.w);
        // (a pointer that went through LDS has lost its address space: say that it is global memory, or the stores become flat ones)
        global_float* p = (global_float*)e.dst + (int64_t)b * e.hw + 4 * (int64_t)i;
        const int left = e.hw - 4 * (int)i;  // >= 1
        if (left >= 4 && ((uintptr_t)p & 15) == 0) {
            *(global_vec4f*)p = vec4f{z.x, z.y, z.z, z.w};
        } else {
            p[0] = z.x;
            if (left > 1) p[1] = z.y;
            if (left > 2) p[2] = z.z;
            if (left > 3) p[3] = z.w;
        }
    }
}

}  // namespace

extern "C" int maua_randn_frames_f32(const maua_randn_slot_t* table, int n_slots, int batch, uint64_t seed, int frame0,
                                     maua_frame_source_t* src, void* stream) {
    if (!table || n_slots < 1 || n_slots > MAUA_MAX_NOISE_SLOTS || batch < 1 || frame0 < 0) return MAUA_EINVAL;
    // 2048 workgroups = 8 per compute unit: enough to keep every unit storing on the 1024^2 maps, and a grid whose surplus workgroups
    // leave after the table scan on the small ones
    hipLaunchKernelGGL(randn_frames_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream, table, n_slots, batch, (uint32_t)seed,
                       (uint32_t)(seed >> 32), frame0, src);
    MAUA_LAUNCH_CHECK();
    return 0;
}
