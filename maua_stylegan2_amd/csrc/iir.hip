// Recursive (IIR) filters for gfx950 — the device side of audioreactive.filters (sosfilt, sosfiltfilt, bandpass, bands, envelope).
// Two entries; their definitions are their comments in include/maua_hip.h and DESIGN.md 4.22, tests/iir_ref.py restates both in numpy.
//
// maua_sosfilt_f64 — a cascade of biquads is linear in its state, so time is cut into chunks that are filtered independently and
// stitched together by a short serial carry (four launches, all on the caller's stream):
//   sos_trans_kernel   one workgroup per filter, lane j < 2 n_sections: the recurrence over one chunk of zero input from the unit state
//                      e_j gives column j of the chunk's transition matrix A.
//   sos_pass_kernel<false>  zero-state pass: one LANE per chunk, one wave per 64 neighbouring chunks of one filter.  The lane keeps
//                      the 2 n_sections state values in registers (n_sections is a template argument: no indexed register arrays) and
//                      walks its chunk sample by sample, all sections per sample; only the final state Z_c is stored.
//   sos_carry_kernel   one wave per filter, lane i owns row i of A in registers: S_{c+1}[i] = (sum_j A[i][j] S_c[j]) + Z_c[i], the sum one
//                      chain of fma in ascending j, S_c[j] taken from lane j with v_readlane (no LDS, no barrier).  Z is fetched eight
//                      chunks ahead so that the dependent chain never waits for memory.
//   sos_pass_kernel<true>   final pass: the same walk from the true state S_c, y written.
// A lane that walks its own chunk would read with a stride of `chunk` samples across the wave.  Both passes therefore move 64 x 16
// tiles through LDS: the wave loads 16 consecutive samples of four chunks per instruction (64-byte / 128-byte segments), the tile of the
// NEXT 16 samples is already in registers while the current one is computed, and y leaves through a second tile the same way.  Tile
// rows are 17 doubles apart: lane r reads tile[r][k] — with ds_read_b64 the 32 lanes of a half fall on 32 different bank pairs.
// Z and S are laid out [filter][state][chunk]: coalesced for the passes (lane = chunk), contiguous per lane for the carry's prefetch.
//
// maua_env_follow_f32 — one lane per column, the frames in order; the loads of a frame do not depend on the chain and are unrolled.
#include <math.h>

#include "common.h"

namespace {

constexpr int SOS_TILE = 16;              // samples per LDS tile
constexpr int SOS_ROW = SOS_TILE + 1;     // doubles between tile rows
constexpr int SOS_LANES = 64;             // chunks per workgroup: one wave
constexpr int SOS_AHEAD = 8;              // chunks of Z the carry fetches ahead
static_assert(2 * MAUA_SOS_MAX_SECTIONS <= SOS_LANES, "the carry and the transition matrix run a lane per state in one wave");

// One sample through section `c` (b0 b1 b2 a1 a2): the arithmetic of the header, every operation a single fma.
__device__ __forceinline__ double sos_section(const double (&c)[5], double x, double& z1, double& z2) {
    const double y = fma(c[0], x, z1);
    z1 = fma(-c[3], y, fma(c[1], x, z2));
    z2 = fma(-c[4], y, c[2] * x);
    return y;
}

// The coefficients are the same in every lane, and the compiler would keep them in scalar registers: 5 n_sections doubles are more
// than the scalar file holds beyond 8 sections, and every use of a spilled one costs two v_readlane in front of the fma that waits
// for it (four per fma in the 12-section pass).  An index the compiler cannot see through makes them per-lane loads into vector registers.
template <int NS>
__device__ __forceinline__ void sos_load_coeffs(double (&co)[NS][5], const double* __restrict__ sos) {
    int opaque_zero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(opaque_zero));
    sos += opaque_zero;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        co[s][0] = sos[s * 6 + 0], co[s][1] = sos[s * 6 + 1], co[s][2] = sos[s * 6 + 2];
        co[s][3] = sos[s * 6 + 4], co[s][4] = sos[s * 6 + 5];
    }
}

template <int NS>
__global__ __launch_bounds__(SOS_LANES) void sos_trans_kernel(const double* __restrict__ sos, int chunk, double* __restrict__ A) {
    constexpr int D = 2 * NS;
    const int f = blockIdx.x, j = threadIdx.x;
    if (j >= D) return;
    double co[NS][5];
    sos_load_coeffs<NS>(co, sos + (int64_t)f * NS * 6);
    double z[NS][2];
#pragma unroll
    for (int s = 0; s < NS; ++s) z[s][0] = (j == 2 * s) ? 1.0 : 0.0, z[s][1] = (j == 2 * s + 1) ? 1.0 : 0.0;
    for (int t = 0; t < chunk; ++t) {
        double v = 0.0;
#pragma unroll
        for (int s = 0; s < NS; ++s) v = sos_section(co[s], v, z[s][0], z[s][1]);
    }
    double* col = A + (int64_t)f * D * D + j;  // A[f][i][j]
#pragma unroll
    for (int s = 0; s < NS; ++s) col[(2 * s) * D] = z[s][0], col[(2 * s + 1) * D] = z[s][1];
}

// The wave's share of a tile: element e = lane + 64 i, i < 16, is sample (e % 16) of tile row (e / 16).
__device__ __forceinline__ void sos_fetch(double (&pre)[SOS_TILE], const float* __restrict__ xf, const double* __restrict__ xd, int64_t sig,
                                          int c0, int nc, int chunk, int n, int t0) {
    const int lane = threadIdx.x, k = lane % SOS_TILE, r0 = lane / SOS_TILE;
#pragma unroll
    for (int i = 0; i < SOS_TILE; ++i) {
        const int c = c0 + r0 + (SOS_LANES / SOS_TILE) * i;
        const int64_t g = (int64_t)c * chunk + t0 + k;
        const bool ok = c < nc && t0 + k < chunk && g < n;
        pre[i] = !ok ? 0.0 : xf ? (double)xf[sig + g] : xd[sig + g];
    }
}

template <int NS, bool FINAL>
__global__ __launch_bounds__(SOS_LANES) void sos_pass_kernel(const double* __restrict__ sos, const float* __restrict__ xf,
                                                             const double* __restrict__ xd, int shared_signal, int n, int chunk, int nc,
                                                             const double* __restrict__ S, double* __restrict__ Z, double* __restrict__ yd,
                                                             float* __restrict__ yf, double* __restrict__ zf) {
    constexpr int D = 2 * NS;
    __shared__ double tin[SOS_LANES * SOS_ROW];
    __shared__ double tout[FINAL ? SOS_LANES * SOS_ROW : 1];
    const int f = blockIdx.y, lane = threadIdx.x, c0 = blockIdx.x * SOS_LANES, c = c0 + lane;
    const int n_run = FINAL ? nc : nc - 1;  // the zero-state pass has no use for the last chunk
    const bool live = c < n_run;
    const int64_t sig = shared_signal ? 0 : (int64_t)f * n, out = (int64_t)f * n;
    const int64_t left = (int64_t)n - (int64_t)c * chunk;
    const int len = !live ? 0 : left < chunk ? (int)left : chunk;  // samples of this lane's chunk
    double co[NS][5];
    sos_load_coeffs<NS>(co, sos + (int64_t)f * NS * 6);
    double z[NS][2];
    const int cc = live ? c : 0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        z[s][0] = FINAL ? S[((int64_t)f * D + 2 * s) * nc + cc] : 0.0;
        z[s][1] = FINAL ? S[((int64_t)f * D + 2 * s + 1) * nc + cc] : 0.0;
    }
    const int k = lane % SOS_TILE, r0 = lane / SOS_TILE;
    double pre[SOS_TILE];
    sos_fetch(pre, xf, xd, sig, c0, n_run, chunk, n, 0);
    for (int t0 = 0; t0 < chunk; t0 += SOS_TILE) {
#pragma unroll
        for (int i = 0; i < SOS_TILE; ++i) tin[(r0 + (SOS_LANES / SOS_TILE) * i) * SOS_ROW + k] = pre[i];
        __syncthreads();
        if (t0 + SOS_TILE < chunk) sos_fetch(pre, xf, xd, sig, c0, n_run, chunk, n, t0 + SOS_TILE);
#pragma unroll 4
        for (int u = 0; u < SOS_TILE; ++u) {
            if (t0 + u < len) {  // (a lane past the end of its chunk keeps its state: the last chunk's is zf)
                double v = tin[lane * SOS_ROW + u];
#pragma unroll
                for (int s = 0; s < NS; ++s) v = sos_section(co[s], v, z[s][0], z[s][1]);
                if (FINAL) tout[lane * SOS_ROW + u] = v;
            }
        }
        __syncthreads();
        if (FINAL) {
#pragma unroll
            for (int i = 0; i < SOS_TILE; ++i) {
                const int r = r0 + (SOS_LANES / SOS_TILE) * i;
                const int64_t g = (int64_t)(c0 + r) * chunk + t0 + k;
                if (c0 + r < nc && t0 + k < chunk && g < n) {
                    const double v = tout[r * SOS_ROW + k];
                    if (yd) yd[out + g] = v;
                    if (yf) yf[out + g] = (float)v;  // round to nearest even, once, from the double
                }
            }
            __syncthreads();
        }
    }
    if (!live) return;
    if (!FINAL) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            Z[((int64_t)f * D + 2 * s) * nc + c] = z[s][0];
            Z[((int64_t)f * D + 2 * s + 1) * nc + c] = z[s][1];
        }
    } else if (zf && c == nc - 1) {
#pragma unroll
        for (int s = 0; s < NS; ++s) zf[(int64_t)f * D + 2 * s] = z[s][0], zf[(int64_t)f * D + 2 * s + 1] = z[s][1];
    }
}

__device__ __forceinline__ double sos_from_lane(double v, int src) {  // src is a constant after unrolling: two v_readlane
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}

template <int NS>
__global__ __launch_bounds__(SOS_LANES) void sos_carry_kernel(const double* __restrict__ A, const double* __restrict__ zi,
                                                              const double* __restrict__ Z, double* __restrict__ S, int nc) {
    constexpr int D = 2 * NS;
    const int f = blockIdx.x, i = threadIdx.x;
    const bool live = i < D;
    const int ii = live ? i : 0;
    double a[D];
#pragma unroll
    for (int j = 0; j < D; ++j) a[j] = A[((int64_t)f * D + ii) * D + j];
    const double* zrow = Z + ((int64_t)f * D + ii) * nc;
    double* srow = S + ((int64_t)f * D + ii) * nc;
    double s = zi ? zi[(int64_t)f * D + ii] : 0.0;
    double next[SOS_AHEAD];
#pragma unroll
    for (int u = 0; u < SOS_AHEAD; ++u) next[u] = u < nc - 1 ? zrow[u] : 0.0;
    for (int c0 = 0; c0 < nc; c0 += SOS_AHEAD) {
        double cur[SOS_AHEAD];
#pragma unroll
        for (int u = 0; u < SOS_AHEAD; ++u) cur[u] = next[u];
#pragma unroll
        for (int u = 0; u < SOS_AHEAD; ++u) next[u] = c0 + SOS_AHEAD + u < nc - 1 ? zrow[c0 + SOS_AHEAD + u] : 0.0;
#pragma unroll
        for (int u = 0; u < SOS_AHEAD; ++u) {
            const int c = c0 + u;  // (uniform: every lane of the wave takes the same way)
            if (c < nc) {
                if (live) srow[c] = s;
                double acc = 0.0;
#pragma unroll
                for (int j = 0; j < D; ++j) acc = fma(a[j], sos_from_lane(s, j), acc);
                s = acc + cur[u];
            }
        }
    }
}

__global__ void sos_copy_state_kernel(const double* __restrict__ zi, double* __restrict__ zf, int count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) zf[i] = zi ? zi[i] : 0.0;
}

__global__ __launch_bounds__(64) void env_follow_kernel(const float* __restrict__ x, const float* __restrict__ y0, float* __restrict__ y, int T,
                                                        int C, float ca, float cr) {
#pragma clang fp contract(off)  // the product and the sum below are rounded on their own (__fmul_rn / __fadd_rn are inlined operators
                                // that the compiler fuses all the same: the pragma on plain operators is what holds)
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    float prev = y0 ? y0[c] : x[c];
#pragma unroll 8
    for (int t = 0; t < T; ++t) {
        const float v = x[(int64_t)t * C + c];
        const float k = v > prev ? ca : cr;  // a NaN compares false: release
        const float d = v - prev;
        const float step = k * d;
        prev = prev + step;
        y[(int64_t)t * C + c] = prev;
    }
}

// nc = ceil(n / chunk) and the workgroups of a pass over `chunks` chunks, a lane each, for any n an int holds (n + chunk - 1 and
// nc + 63 need not fit one).
int sos_chunks(int n, int chunk) { return (int)ceil_div64(n, chunk); }
int sos_groups(int chunks) { return (int)ceil_div64(chunks, SOS_LANES); }

struct SosArgs {
    const double* sos;
    const float* xf;
    const double* xd;
    int shared_signal, n, chunk, nc, F;
    const double* zi;
    double *yd;
    float* yf;
    double *zf, *A, *Z, *S;
    hipStream_t st;
};

template <int NS>
int sos_launch(const SosArgs& a) {
    const dim3 grid_final(sos_groups(a.nc), a.F);
    if (a.nc > 1) {
        hipLaunchKernelGGL(sos_trans_kernel<NS>, dim3(a.F), dim3(SOS_LANES), 0, a.st, a.sos, a.chunk, a.A);
        MAUA_LAUNCH_CHECK();
        const dim3 grid_zero(sos_groups(a.nc - 1), a.F);
        hipLaunchKernelGGL((sos_pass_kernel<NS, false>), grid_zero, dim3(SOS_LANES), 0, a.st, a.sos, a.xf, a.xd, a.shared_signal, a.n, a.chunk,
                           a.nc, (const double*)nullptr, a.Z, (double*)nullptr, (float*)nullptr, (double*)nullptr);
        MAUA_LAUNCH_CHECK();
    }
    // (with a single chunk the carry only writes S_0 = zi: A and Z are not read)
    hipLaunchKernelGGL(sos_carry_kernel<NS>, dim3(a.F), dim3(SOS_LANES), 0, a.st, (const double*)a.A, a.zi, (const double*)a.Z, a.S, a.nc);
    MAUA_LAUNCH_CHECK();
    hipLaunchKernelGGL((sos_pass_kernel<NS, true>), grid_final, dim3(SOS_LANES), 0, a.st, a.sos, a.xf, a.xd, a.shared_signal, a.n, a.chunk, a.nc,
                       (const double*)a.S, (double*)nullptr, a.yd, a.yf, a.zf);
    MAUA_LAUNCH_CHECK();
    return 0;
}

bool sos_shape_ok(int F, int ns, int n, int chunk) {
    return F >= 1 && F <= MAUA_SOS_MAX_FILTERS && ns >= 1 && ns <= MAUA_SOS_MAX_SECTIONS && n >= 0 && chunk >= 0 && chunk <= MAUA_SOS_MAX_CHUNK;
}

}  // namespace

extern "C" int maua_sosfilt_default_chunk(int n) {
    int p = 64;
    while (p < 4096 && (int64_t)p * p * MAUA_SOS_CHUNK_BALANCE < (int64_t)n) p *= 2;
    return p;
}

extern "C" int64_t maua_sosfilt_ws_doubles(int n_filters, int n_sections, int n, int chunk) {
    if (!sos_shape_ok(n_filters, n_sections, n, chunk)) return -1;
    if (chunk == 0) chunk = maua_sosfilt_default_chunk(n);
    const int64_t D = 2 * n_sections, nc = sos_chunks(n, chunk);
    return n_filters * (D * D + 2 * nc * D);
}

// What a call with these shape arguments does, from the constants and the checks of the entry below; nothing is launched.
extern "C" int maua_sosfilt_plan(int n_filters, int n_sections, int n, int chunk, int32_t* out) {
    if (!out || !sos_shape_ok(n_filters, n_sections, n, chunk)) return MAUA_EINVAL;
    if (chunk == 0) chunk = maua_sosfilt_default_chunk(n);
    const int nc = sos_chunks(n, chunk);
    const int last_tile = chunk % SOS_TILE ? chunk % SOS_TILE : SOS_TILE;
    out[0] = chunk;
    out[1] = nc;
    out[2] = n == 0 ? 1 : nc == 1 ? 2 : 4;                    // (at n == 0 the one launch copies zi to zf, where zf is asked for)
    out[3] = n == 0 ? 0 : sos_groups(nc - 1);                 // zero-state pass, grid.x (none at nc == 1)
    out[4] = n == 0 ? 0 : sos_groups(nc);                     // final pass, grid.x
    out[5] = ceil_div(chunk, SOS_TILE);                       // LDS tiles a lane walks per full chunk
    out[6] = last_tile;                                       // samples in the last of them
    out[7] = n == 0 ? 0 : n - (nc - 1) * chunk;               // length of the last chunk
    return 0;
}

extern "C" int maua_sosfilt_f64(const double* sos, int n_filters, int n_sections, const float* x_f32, const double* x_f64, int n_signals,
                                int n, int chunk, const double* zi, double* y_f64, float* y_f32, double* zf, double* ws, void* stream) {
    if (!sos || !ws || !sos_shape_ok(n_filters, n_sections, n, chunk)) return MAUA_EINVAL;
    if ((x_f32 != nullptr) == (x_f64 != nullptr) || (!y_f64 && !y_f32)) return MAUA_EINVAL;
    if (n_signals != 1 && n_signals != n_filters) return MAUA_EINVAL;
    const int F = n_filters, D = 2 * n_sections;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (zf) {
            hipLaunchKernelGGL(sos_copy_state_kernel, dim3(ceil_div(F * D, 256)), dim3(256), 0, st, zi, zf, F * D);
            MAUA_LAUNCH_CHECK();
        }
        return 0;
    }
    if (chunk == 0) chunk = maua_sosfilt_default_chunk(n);
    const int nc = sos_chunks(n, chunk);
    SosArgs a{sos, x_f32, x_f64, n_signals == 1 ? 1 : 0, n, chunk, nc, F, zi, y_f64, y_f32, zf, ws, ws + (int64_t)F * D * D,
              ws + (int64_t)F * D * D + (int64_t)F * nc * D, st};
    switch (n_sections) {
#define MAUA_SOS_CASE(NS) \
    case NS:              \
        return sos_launch<NS>(a);
        MAUA_SOS_CASE(1) MAUA_SOS_CASE(2) MAUA_SOS_CASE(3) MAUA_SOS_CASE(4) MAUA_SOS_CASE(5) MAUA_SOS_CASE(6) MAUA_SOS_CASE(7) MAUA_SOS_CASE(8)
        MAUA_SOS_CASE(9) MAUA_SOS_CASE(10) MAUA_SOS_CASE(11) MAUA_SOS_CASE(12) MAUA_SOS_CASE(13) MAUA_SOS_CASE(14) MAUA_SOS_CASE(15)
        MAUA_SOS_CASE(16)
#undef MAUA_SOS_CASE
    }
    return MAUA_EINVAL;
}

extern "C" int maua_env_follow_f32(const float* x, const float* y0, float* y, int n_frames, int n_cols, float attack_coef, float release_coef,
                                   void* stream) {
    if (!x || !y || n_frames < 0 || n_cols < 1) return MAUA_EINVAL;
    if (!(attack_coef >= 0.f && attack_coef <= 1.f) || !(release_coef >= 0.f && release_coef <= 1.f)) return MAUA_EINVAL;  // (a NaN too)
    if (n_frames == 0) return 0;
    hipLaunchKernelGGL(env_follow_kernel, dim3(ceil_div(n_cols, 64)), dim3(64), 0, (hipStream_t)stream, x, y0, y, n_frames, n_cols, attack_coef,
                       release_coef);
    MAUA_LAUNCH_CHECK();
    return 0;
}
