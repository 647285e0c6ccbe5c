// Synthesised noise slots (include/maua_hip.h, "synthesised noise"): the maps of a noise slot as a sum of up to four terms
//   dst[b, e] = gain * sum_k envelope_k[f] * mask_k[e] * v_k[e],   v_k = a row of a short loop bank, or the counter-based N(0,1) map,
// produced per launch from a table in device memory: one launch at the head of a captured forward fills the maps of every synthesised
// layer of one batch, so a 1024^2 layer reacts to the audio from a loop of a few hundred frames instead of a resident per-frame sequence.
// A streaming kernel: per element one 4-byte store and one 4-byte load per bank and mask operand.
#include "common.h"
#include "philox.h"

namespace {

using namespace maua_philox;

// one workgroup pass = 1024 quads (16 KiB) of one map, four per thread a workgroup's width apart: what is found per pass (slot, sample, bank
// rows, alignment) is wave-uniform and spread over four quads, and a thread has the loads of four quads in flight
constexpr int QUADS_PER_THREAD = 4;
constexpr int CHUNK_QUADS = 256 * QUADS_PER_THREAD;

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// four consecutive floats at p (16-byte aligned when `vec`), the last `left` < 4 of a map element by element; absent ones read as 0
__device__ __forceinline__ vec4f load4(const global_float* p, int left, bool vec) {
    if (vec && left >= 4) return *(const global_vec4f*)p;
    vec4f v = {p[0], 0.f, 0.f, 0.f};
    if (left > 1) v.y = p[1];
    if (left > 2) v.z = p[2];
    if (left > 3) v.w = p[3];
    return v;
}

// One thread = four consecutive floats of one map, one workgroup pass = one chunk of one (slot, sample).  The table lives in device memory,
// so the host cannot size the grid by it: every workgroup copies it to LDS (one entry per thread), builds the prefix sums of the slots'
// chunk counts there and the grid strides over their total.  Slot, sample, the bank rows ((F + phase) mod period) and the alignment of the
// operands are found once per chunk from wave-uniform values, not per element.
__global__ __launch_bounds__(256) void noise_synth_kernel(const maua_noise_synth_slot_t* __restrict__ table, int n_slots, int batch, int frame0,
                                                          maua_frame_source_t* src) {
    __shared__ int64_t first_chunk[MAUA_MAX_NOISE_SLOTS + 1];
    __shared__ maua_noise_synth_slot_t slots[MAUA_MAX_NOISE_SLOTS];
    if ((int)threadIdx.x < n_slots) {
        maua_noise_synth_slot_t e = table[threadIdx.x];
        if (!e.dst || e.hw < 1 || e.n_terms < 1) e.hw = 0;  // an empty entry produces nothing
        if (e.n_terms > MAUA_NOISE_SYNTH_MAX_TERMS) e.n_terms = MAUA_NOISE_SYNTH_MAX_TERMS;
        for (int k = 0; k < MAUA_NOISE_SYNTH_MAX_TERMS; ++k) {  // (the host validates: a period below 1 must still not divide by zero)
            if (e.term[k].period < 1) e.term[k].period = 1;
            if (e.term[k].phase < 0) e.term[k].phase = 0;
        }
        slots[threadIdx.x] = e;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t acc = 0;
        for (int i = 0; i < n_slots; ++i) {
            first_chunk[i] = acc;
            const int quads = (slots[i].hw + 3) / 4;
            acc += (int64_t)batch * ((quads + CHUNK_QUADS - 1) / CHUNK_QUADS);
        }
        first_chunk[n_slots] = acc;
    }
    __syncthreads();
    // frames of this launch: local [local0, local0 + batch) inside the bound sequences (the envelopes), absolute frame0 + local
    const int64_t local0 = src ? (int64_t)src->frame0 : 0;
    if (src && blockIdx.x == 0 && (int)threadIdx.x < n_slots) {
        // the layers read noise[slot] + (src->frame0 + b) * noise_stride[slot]: bias the pointer so that this lands on dst + b * hw.
        // Integer arithmetic: the biased value is only ever an operand of that sum, never dereferenced.
        const int hw = slots[threadIdx.x].hw, slot = slots[threadIdx.x].slot;
        if (hw > 0 && slot >= 0 && slot < MAUA_MAX_NOISE_SLOTS) {
            const uint64_t biased = (uint64_t)(uintptr_t)slots[threadIdx.x].dst - (uint64_t)local0 * (uint64_t)hw * sizeof(float);
            src->noise[slot] = (const float*)(uintptr_t)biased;
            src->noise_stride[slot] = hw;
        }
    }
    const int64_t total = first_chunk[n_slots];
    for (int64_t c = blockIdx.x; c < total; c += gridDim.x) {
        int lo = 0, hi = n_slots - 1;  // last slot whose first chunk is <= c (empty slots share their successor's start and lose)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (first_chunk[mid] <= c) lo = mid; else hi = mid - 1;
        }
        lo = uniform(lo);
        const maua_noise_synth_slot_t& e = slots[lo];
        const int hw = uniform(e.hw), n_terms = uniform(e.n_terms);
        const int quads = (hw + 3) / 4;
        const uint32_t chunks = (uint32_t)(quads + CHUNK_QUADS - 1) / CHUNK_QUADS;
        const int64_t r = c - first_chunk[lo];  // < batch * chunks
        const int b = uniform((int)(r / chunks));
        const int chunk = uniform((int)(r - (int64_t)b * chunks));
        const int64_t f = local0 + b;                          // local frame: index into the envelopes
        const int64_t F = f + frame0;                          // absolute frame: loop position and counter word
        // (a pointer that went through LDS has lost its address space: say that it is global memory, or the accesses become flat ones)
        global_float* dst = (global_float*)e.dst + (int64_t)b * hw;
        const global_float* bank[MAUA_NOISE_SYNTH_MAX_TERMS];
        const global_float* mask[MAUA_NOISE_SYNTH_MAX_TERMS];
        float env[MAUA_NOISE_SYNTH_MAX_TERMS];
        uintptr_t align = (uintptr_t)dst;
        bool counter_term = false;  // a NULL-bank term among them (at most one per slot: its quad is generated once)
#pragma unroll
        for (int k = 0; k < MAUA_NOISE_SYNTH_MAX_TERMS; ++k) {
            bank[k] = mask[k] = nullptr;
            env[k] = 1.0f;
            if (k < n_terms) {
                const maua_noise_term_t& t = e.term[k];
                if (t.bank) {
                    const uint64_t at = (uint64_t)F + (uint32_t)t.phase;  // 32-bit division wherever it fits: always, in practice
                    const uint32_t row = at <= 0xFFFFFFFFull ? (uint32_t)at % (uint32_t)t.period : (uint32_t)(at % (uint32_t)t.period);
                    bank[k] = (const global_float*)t.bank + (int64_t)row * hw;
                } else {
                    counter_term = true;
                }
                mask[k] = (const global_float*)t.mask;
                if (t.envelope) env[k] = ((const global_float*)t.envelope)[f];
                align |= (uintptr_t)bank[k] | (uintptr_t)mask[k];
            }
        }
        const bool vec = (align & 15) == 0;  // every operand of this (slot, sample) on a 16-byte boundary (NULL counts as aligned)
#pragma unroll
        for (int j = 0; j < QUADS_PER_THREAD; ++j) {
            const int i = chunk * CHUNK_QUADS + j * 256 + (int)threadIdx.x;  // a quad of this thread
            if (i >= quads) break;
            const int left = hw - 4 * i;  // >= 1
            const int64_t off = 4 * (int64_t)i;
            vec4f acc = {0.f, 0.f, 0.f, 0.f}, z = acc;
            if (counter_term) {
                const float4 n = randn_quad((uint32_t)i, (uint32_t)F, (uint32_t)e.slot, (uint32_t)e.seed, (uint32_t)(e.seed >> 32));
                z = vec4f{n.x, n.y, n.z, n.w};
            }
#pragma unroll
            for (int k = 0; k < MAUA_NOISE_SYNTH_MAX_TERMS; ++k) {
                if (k < n_terms) {
                    const vec4f v = bank[k] ? load4(bank[k] + off, left, vec) : z;
                    vec4f m = {1.f, 1.f, 1.f, 1.f};
                    if (mask[k]) m = load4(mask[k] + off, left, vec);
                    // the term order and these two roundings per term are the definition: the same bits from either access width
                    acc.x = fmaf(__fmul_rn(env[k], m.x), v.x, acc.x);
                    acc.y = fmaf(__fmul_rn(env[k], m.y), v.y, acc.y);
                    acc.z = fmaf(__fmul_rn(env[k], m.z), v.z, acc.z);
                    acc.w = fmaf(__fmul_rn(env[k], m.w), v.w, acc.w);
                }
            }
            const float gain = e.gain;
            acc = vec4f{__fmul_rn(gain, acc.x), __fmul_rn(gain, acc.y), __fmul_rn(gain, acc.z), __fmul_rn(gain, acc.w)};
            global_float* p = dst + off;
            if (vec && left >= 4) {
                *(global_vec4f*)p = acc;
            } else {
                p[0] = acc.x;
                if (left > 1) p[1] = acc.y;
                if (left > 2) p[2] = acc.z;
                if (left > 3) p[3] = acc.w;
            }
        }
    }
}

}  // namespace

extern "C" int maua_noise_synth_f32(const maua_noise_synth_slot_t* table, int n_slots, int batch, int frame0, maua_frame_source_t* src,
                                    void* stream) {
    if (!table || n_slots < 1 || n_slots > MAUA_MAX_NOISE_SLOTS || batch < 1 || frame0 < 0) return MAUA_EINVAL;
    // 2048 workgroups = 8 per compute unit, as maua_randn_frames_f32: enough loads in flight on the 1024^2 maps, and a grid whose surplus
    // workgroups leave after the table scan on the small ones
    hipLaunchKernelGGL(noise_synth_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream, table, n_slots, batch, frame0, src);
    MAUA_LAUNCH_CHECK();
    return 0;
}
