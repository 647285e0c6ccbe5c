// Frame delivery at any size (render.py FrameResize / resize_frames): a separable resampler on packed 3-channel frames of 8 or 16 bits.
//   maua_resample_coeffs    host: the integer weight and bounds tables of one axis
//   maua_resample_u8 / _u16 the launch: in[B,in_h,in_w,3] -> a window of out[B,out_h,out_w,3]
//   maua_resample_ws_bytes  the workspace of the two-launch path (0 where the fused kernel serves the geometry)
//   maua_resample_plan      the entry's dispatch as text, without a launch
//
// Definition (Pillow's Image.resize(size, resample, box) on 8-bit images, restated in integers; tests/resample_ref.py is its numpy twin).
// Per axis, for a source length n, a source interval [in0, in1), an output length m and a filter f of support s:
//   scale = (in1 - in0) / m, fs = max(scale, 1), support = s * fs, ksize = 2 * ceil(support) + 1                  (double)
//   output j: center = in0 + (j + 0.5) * scale, xmin = max(0, (int)(center - support + 0.5)),
//             xmax = min(n, (int)(center + support + 0.5)) - xmin
//   w_x = f((x + xmin - center + 0.5) / fs) for x < xmax, each divided by their sequential sum when that is non-zero
//   k_x = (int)(w_x * 2^22 +- 0.5) (the sign of w_x);  bounds_j = (xmin, xmax)
//   a pass: out_j = clamp((2^21 + sum_x in[xmin + x] * k_x) >> 22, 0, top), an arithmetic shift; top = 255 / 65535
// The horizontal pass runs first and is rounded to the sample type; the vertical pass runs on that.  8-bit sums are 32 bits wide (as
// Pillow's), 16-bit sums 64.  A NULL table copies its axis (= one tap of weight 2^22).
//
// Kernels.  The work is per output sample ksize_x + ksize_y multiply-adds on data that is read once, so the kernel is meant to be bound by
// the bytes it moves; the horizontal intermediate must then not travel through HBM.
//   fused    a workgroup of 256 threads owns a tile of 64 x th output pixels of one frame's window, th = 64, 32 or 16: the tallest whose
//            LDS stays within a CU's share for 8 workgroups (a workgroup's phases are a chain of dependent loads and barriers: more rows
//            per tile amortise that latency and shrink the overlap of neighbouring tiles' row spans).  It copies the tile's
//            slices of the four tables to LDS (weight rows at an odd stride: lanes of a wave read different columns' rows), takes the
//            union [lo, hi) of the source rows its output rows need from the vertical bounds, resamples those rows horizontally for its 64
//            columns into LDS (8 or 16 bits, the rounding of the definition; a pixel's taps are read four at a time as whole dwords at its
//            own unaligned address, tap_sums below), then runs the vertical pass out of LDS — the weights of an
//            output row are the same address for the lanes that share it, an LDS broadcast — and stores packed RGB rows, 4 bytes per lane
//            where the alignment allows (.vec) or sample by sample (.scalar).  Rows are taken in groups whose span fits the LDS rows the
//            launch was given, so tables of any origin are served without leaving the allocation; the planner sizes the allocation so that
//            tables made by maua_resample_coeffs need one group.  x = tiles (at most FUSED_GRID_CAP workgroups walking them), y = frame.
//   twopass  where the bound on a tile's row span, ceil(15 * in_h / dst_h) + ksize_y + 1 at th = 16, does not fit the 64 KB of LDS next to the
//            tables (large down-scales): a horizontal launch into ws[B, in_h, dst_w, 3] and a vertical launch out of it, one thread per
//            pixel, grid-stride.  The same integers, so the same bits.
// No atomics; every output sample is written by exactly one thread, so results are identical from run to run.
#include <math.h>
#include <string.h>

#include "common.h"

namespace {
constexpr int BITS = 22;
constexpr int MAX_TAPS = MAUA_RESAMPLE_MAX_TAPS;
constexpr int TW = 64;                   // the fused tile's width, output pixels
constexpr int TILE_HEIGHTS[3] = {64, 32, 16};  // its height: the tallest whose LDS stays within LDS_SHARE, else 16
constexpr int LDS_SHARE = 20 * 1024;     // 160 KB of LDS for the 8 workgroups of 256 threads a CU can hold
constexpr int LDS_BUDGET = 64 * 1024;    // dynamic LDS a fused launch may ask for (the default limit: no attribute is set)
constexpr int FUSED_GRID_CAP = 2048;     // workgroups per frame of the fused kernel
constexpr int PASS_GRID_CAP = 1024;      // workgroups of a two-pass launch

// ---------------------------------------------------------------------------------------------------------------- host: the tables
double f_box(double x) { return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0; }
double f_bilinear(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}
double f_hamming(double x) {
    if (x < 0.0) x = -x;
    if (x == 0.0) return 1.0;
    if (x >= 1.0) return 0.0;
    x = x * M_PI;
    return sin(x) / x * (0.54f + 0.46f * cos(x));  // (float literals, as Pillow writes them)
}
double f_bicubic(double x) {
    constexpr double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
double f_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}
double f_lanczos(double x) { return (-3.0 <= x && x < 3.0) ? f_sinc(x) * f_sinc(x / 3) : 0.0; }

struct Filter {
    double (*f)(double);
    double support;
};
const Filter kFilters[5] = {{f_box, 0.5}, {f_bilinear, 1.0}, {f_hamming, 1.0}, {f_bicubic, 2.0}, {f_lanczos, 3.0}};

// ---------------------------------------------------------------------------------------------------------------- device
template <typename T>
struct Sample;
template <>
struct Sample<uint8_t> {
    using acc = int32_t;
    static constexpr int TOP = 255, G = 4;  // G: samples of one 4-byte store
};
template <>
struct Sample<uint16_t> {
    using acc = int64_t;
    static constexpr int TOP = 65535, G = 2;
};

template <typename T>
__device__ __forceinline__ T finish(typename Sample<T>::acc s) {
    s = (s + (1 << (BITS - 1))) >> BITS;
    return (T)(s < 0 ? 0 : (s > Sample<T>::TOP ? Sample<T>::TOP : s));
}

// a bounds pair as the kernels use it: inside [0, n] and at most `ksize` taps, whatever the table holds
__device__ __forceinline__ void clamp_bounds(const int32_t* b, int j, int n, int ksize, int& lo, int& cnt) {
    lo = min(max(b[2 * j], 0), n - 1);
    cnt = min(max(b[2 * j + 1], 0), min(ksize, n - lo));
}

// The horizontal sums of one intermediate pixel: `cnt` taps of three samples each from `src`, weights k[0 .. cnt).  The loads, not the
// arithmetic, bound this pass (one load instruction per sample keeps the texture path busy whatever the cache hit rate), so where
// `whole_blocks` says that the taps rounded up to a multiple of 4 still lie inside the frame, 4 taps = 12 samples are read as 3 (8 bits) or
// 6 (16 bits) whole dwords at the pixel's own, generally unaligned, address and taken apart in registers; weights past cnt count as zero,
// whatever the table holds there.  Otherwise (the last pixels of a frame) sample by sample.  Both forms add the same integers.
template <typename T>
__device__ __forceinline__ void tap_sums(const T* __restrict__ src, const int32_t* k, int cnt, bool whole_blocks,
                                         typename Sample<T>::acc& a0, typename Sample<T>::acc& a1, typename Sample<T>::acc& a2) {
    using acc_t = typename Sample<T>::acc;
    if (whole_blocks) {
        constexpr int ND = 12 * (int)sizeof(T) / 4, PER = 4 / (int)sizeof(T), SHIFT = 8 * (int)sizeof(T);
        for (int t = 0; t < cnt; t += 4) {
            uint32_t d[ND];
            __builtin_memcpy(d, src + 3 * t, sizeof(d));
            acc_t w[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) w[i] = t + i < cnt ? k[t + i] : 0;
            acc_t s[3] = {0, 0, 0};
#pragma unroll
            for (int i = 0; i < 12; ++i)  // sample i of the block: tap i / 3, channel i % 3
                s[i % 3] += w[i / 3] * (acc_t)((d[i / PER] >> (SHIFT * (i % PER))) & (uint32_t)Sample<T>::TOP);
            a0 += s[0], a1 += s[1], a2 += s[2];
        }
    } else {
        for (int t = 0; t < cnt; ++t) {
            const acc_t w = k[t];
            a0 += w * src[3 * t], a1 += w * src[3 * t + 1], a2 += w * src[3 * t + 2];
        }
    }
}

struct Geo {
    int in_h, in_w, out_h, out_w, dst_x0, dst_y0, dst_w, dst_h;
    int ksx, ksy;        // taps per output column / row; 0: the axis is copied (NULL tables)
    int strx, stry;      // stride of a weight row in LDS: max(ks, 1) | 1
    int cap_rows;        // rows of the horizontal intermediate the launch's LDS holds (>= max(ksy, 1))
    int tiles_x, tiles;  // tiles per window row, per window
    int th;              // tile height (TILE_HEIGHTS)
};

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void resample_fused_kernel(const T* __restrict__ in, T* __restrict__ out, const int32_t* __restrict__ kx,
                                                             const int32_t* __restrict__ bx, const int32_t* __restrict__ ky,
                                                             const int32_t* __restrict__ by, Geo g) {
    using acc_t = typename Sample<T>::acc;
    constexpr int G = Sample<T>::G, PITCH = TW * 3;  // samples of an LDS row; PITCH % G == 0
    extern __shared__ __align__(16) unsigned char lds[];
    int32_t* s_kx = reinterpret_cast<int32_t*>(lds);  // [TW][strx]
    int32_t* s_bx = s_kx + TW * g.strx;               // [TW][2]
    int32_t* s_ky = s_bx + TW * 2;                    // [th][stry]
    int32_t* s_by = s_ky + g.th * g.stry;             // [th][2]
    T* s_h = reinterpret_cast<T*>(s_by + g.th * 2);   // [cap_rows][PITCH]
    const int tid = threadIdx.x;
    const int ksx = max(g.ksx, 1), ksy = max(g.ksy, 1);
    const T* fin = in + (int64_t)blockIdx.y * g.in_h * g.in_w * 3;
    T* fout = out + (int64_t)blockIdx.y * g.out_h * g.out_w * 3;
    for (int tile = blockIdx.x; tile < g.tiles; tile += gridDim.x) {
        const int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
        const int x0 = tx * TW, y0 = ty * g.th;
        const int tw = min(TW, g.dst_w - x0), th = min(g.th, g.dst_h - y0);
        __syncthreads();  // (the previous tile's readers are done with the tables)
        for (int i = tid; i < tw * ksx; i += 256) {
            const int c = i / ksx, t = i - c * ksx;
            s_kx[c * g.strx + t] = kx ? kx[(int64_t)(x0 + c) * ksx + t] : (1 << BITS);
        }
        for (int i = tid; i < th * ksy; i += 256) {
            const int r = i / ksy, t = i - r * ksy;
            s_ky[r * g.stry + t] = ky ? ky[(int64_t)(y0 + r) * ksy + t] : (1 << BITS);
        }
        if (tid < tw) {
            int lo = x0 + tid, cnt = 1;
            if (bx) clamp_bounds(bx, x0 + tid, g.in_w, ksx, lo, cnt);
            s_bx[2 * tid] = lo, s_bx[2 * tid + 1] = cnt;
        } else if (tid >= 64 && tid - 64 < th) {
            const int r = tid - 64;
            int lo = y0 + r, cnt = 1;
            if (by) clamp_bounds(by, y0 + r, g.in_h, ksy, lo, cnt);
            s_by[2 * r] = lo, s_by[2 * r + 1] = cnt;
        }
        __syncthreads();
        for (int ry = 0; ry < th;) {
            // the group of output rows [ry, re) whose source rows [lo, hi) fit the intermediate (one row always does: cnt <= ksy <= cap_rows)
            int lo = s_by[2 * ry], hi = lo + s_by[2 * ry + 1], re = ry + 1;
            while (re < th) {
                const int nlo = min(lo, s_by[2 * re]), nhi = max(hi, s_by[2 * re] + s_by[2 * re + 1]);
                if (nhi - nlo > g.cap_rows) break;
                lo = nlo, hi = nhi, ++re;
            }
            const int nrows = hi - lo;
            // horizontal pass: source rows [lo, hi) at the tile's columns -> LDS
            for (int e = tid; e < nrows * tw; e += 256) {
                const int r = e / tw, c = e - r * tw;
                const int xmin = s_bx[2 * c], xmax = s_bx[2 * c + 1];
                const int64_t first = (int64_t)(lo + r) * g.in_w + xmin;  // pixel index inside the frame
                acc_t a0 = 0, a1 = 0, a2 = 0;
                tap_sums<T>(fin + first * 3, s_kx + c * g.strx, xmax, first + ((xmax + 3) & ~3) <= (int64_t)g.in_h * g.in_w, a0, a1, a2);
                T* d = s_h + r * PITCH + c * 3;
                d[0] = finish<T>(a0), d[1] = finish<T>(a1), d[2] = finish<T>(a2);
            }
            __syncthreads();
            // vertical pass: G consecutive samples of one output row per thread
            const int samples = tw * 3, groups = (samples + G - 1) / G;
            for (int e = tid; e < (re - ry) * groups; e += 256) {
                const int j = e / groups, s0 = (e - j * groups) * G;
                const int ymin = s_by[2 * (ry + j)] - lo, ymax = s_by[2 * (ry + j) + 1];
                const int32_t* k = s_ky + (ry + j) * g.stry;
                acc_t a[G];
#pragma unroll
                for (int q = 0; q < G; ++q) a[q] = 0;
                for (int t = 0; t < ymax; ++t) {
                    const acc_t w = k[t];
                    // (PITCH % G == 0: the 4 bytes lie inside the row even where s0 + G > samples)
                    uint32_t word;  // (memcpy: the row was written as samples; one 4-byte LDS read)
                    __builtin_memcpy(&word, __builtin_assume_aligned(s_h + (ymin + t) * PITCH + s0, 4), 4);
#pragma unroll
                    for (int q = 0; q < G; ++q) a[q] += w * (acc_t)((word >> (q * (32 / G))) & (uint32_t)Sample<T>::TOP);
                }
                T* dst = fout + ((int64_t)(g.dst_y0 + y0 + ry + j) * g.out_w + g.dst_x0 + x0) * 3 + s0;
                if (VEC && s0 + G <= samples) {
                    uint32_t word = 0;
#pragma unroll
                    for (int q = 0; q < G; ++q) {
                        // The finished sample goes through an empty asm statement before it is packed: without it the compiler joins the
                        // shift, the clamp and the packing of two samples into one v_ashr_pk_u8_i32 and ORs the other two samples onto
                        // its result as if bits 31:16 were zero; on the MI355X those samples then came out wrong (the samples 2 and 3 of
                        // every 4-byte store, found by the red-zone tests).  Shift, clamp and pack stay separate instructions this way.
                        uint32_t v = finish<T>(a[q]);
                        asm volatile("" : "+v"(v));
                        word |= v << (q * (32 / G));
                    }
                    __builtin_memcpy(__builtin_assume_aligned(dst, 4), &word, 4);  // one 4-byte store
                } else {
#pragma unroll
                    for (int q = 0; q < G; ++q)
                        if (s0 + q < samples) dst[q] = finish<T>(a[q]);
                }
            }
            __syncthreads();  // (the next group overwrites the intermediate)
            ry = re;
        }
    }
}

// two-pass, horizontal: in[rows = B * in_h, in_w, 3] -> ws[rows, dst_w, 3]; one thread per pixel
template <typename T>
__global__ __launch_bounds__(256) void resample_h_kernel(const T* __restrict__ in, T* __restrict__ ws, const int32_t* __restrict__ kx,
                                                         const int32_t* __restrict__ bx, int in_w, int dst_w, int ksx, int64_t total) {
    using acc_t = typename Sample<T>::acc;
    const int64_t rows = total / dst_w;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int c = (int)(idx % dst_w);
        const int64_t row = idx / dst_w;
        int xmin, xmax;
        clamp_bounds(bx, c, in_w, ksx, xmin, xmax);
        const int64_t first = row * in_w + xmin;  // pixel index inside the batch (rows = B * in_h)
        acc_t a0 = 0, a1 = 0, a2 = 0;
        tap_sums<T>(in + first * 3, kx + (int64_t)c * ksx, xmax, first + ((xmax + 3) & ~3) <= rows * in_w, a0, a1, a2);
        T* d = ws + idx * 3;
        d[0] = finish<T>(a0), d[1] = finish<T>(a1), d[2] = finish<T>(a2);
    }
}

// two-pass, vertical: src[B, in_h, dst_w, 3] (the workspace, or the input itself where the x axis is copied) -> the window of out
template <typename T>
__global__ __launch_bounds__(256) void resample_v_kernel(const T* __restrict__ src, T* __restrict__ out, const int32_t* __restrict__ ky,
                                                         const int32_t* __restrict__ by, Geo g, int64_t total) {
    using acc_t = typename Sample<T>::acc;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int c = (int)(idx % g.dst_w);
        const int j = (int)((idx / g.dst_w) % g.dst_h);
        const int64_t b = idx / ((int64_t)g.dst_w * g.dst_h);
        int ymin, ymax;
        clamp_bounds(by, j, g.in_h, g.ksy, ymin, ymax);
        const int64_t pitch = (int64_t)g.dst_w * 3;
        const T* p = src + ((b * g.in_h + ymin) * g.dst_w + c) * 3;
        const int32_t* k = ky + (int64_t)j * g.ksy;
        acc_t a0 = 0, a1 = 0, a2 = 0;
        for (int t = 0; t < ymax; ++t) {
            const acc_t w = k[t];
            a0 += w * p[t * pitch], a1 += w * p[t * pitch + 1], a2 += w * p[t * pitch + 2];
        }
        T* d = out + ((b * g.out_h + g.dst_y0 + j) * g.out_w + g.dst_x0 + c) * 3;
        d[0] = finish<T>(a0), d[1] = finish<T>(a1), d[2] = finish<T>(a2);
    }
}

// ---------------------------------------------------------------------------------------------------------------- host: the dispatch
struct Plan {
    Geo g;
    bool twopass, vec;
    size_t lds;
    unsigned grid_x;
    int trips;                  // fused: trips of the tile loop
    int64_t h_total, v_total;   // two-pass: threads' work items
    int h_trips, v_trips;
    int64_t ws_bytes;
};

// The one place that decides.  sz: bytes per sample (1 / 2); ksx / ksy: 0 for a copied axis; out_misalign: the output pointer's low bits.
// Returns 0, MAUA_EINVAL or MAUA_ENOSYS; batch == 0 is planned like batch == 1 (the entry returns before launching).
int make_plan(int sz, int batch, int in_h, int in_w, int out_h, int out_w, int dst_x0, int dst_y0, int dst_w, int dst_h, int ksx, int ksy,
              unsigned out_misalign, Plan* p) {
    if ((sz != 1 && sz != 2) || batch < 0 || in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1 || dst_w < 1 || dst_h < 1) return MAUA_EINVAL;
    if (dst_x0 < 0 || dst_y0 < 0 || dst_x0 > out_w - dst_w || dst_y0 > out_h - dst_h) return MAUA_EINVAL;
    if (ksx < 0 || ksx > MAX_TAPS || ksy < 0 || ksy > MAX_TAPS) return MAUA_EINVAL;
    if ((ksx == 0 && dst_w != in_w) || (ksy == 0 && dst_h != in_h)) return MAUA_EINVAL;
    if (batch > 65535) return MAUA_ENOSYS;
    Geo& g = p->g;
    g = Geo{in_h, in_w, out_h, out_w, dst_x0, dst_y0, dst_w, dst_h, ksx, ksy, (ksx > 1 ? ksx : 1) | 1, (ksy > 1 ? ksy : 1) | 1, 0, 0, 0, 0};
    const int64_t row_bytes = (int64_t)TW * 3 * sz;
    int64_t tables = 0, span = 0;
    for (int th : TILE_HEIGHTS) {
        g.th = th;
        tables = 4ll * (TW * g.strx + TW * 2 + th * g.stry + th * 2);
        // rows of the source one tile can need: (th - 1) output steps of at most in_h / dst_h rows, plus one row's taps, plus one for the rounding
        span = ksy == 0 ? th : ceil_div64((int64_t)(th - 1) * in_h, dst_h) + ksy + 1;
        if (tables + span * row_bytes <= LDS_SHARE && (th == 16 || dst_h > th / 2)) break;  // (a taller tile than the window has rows gains nothing)
    }
    const int64_t tiles_x = ceil_div(dst_w, TW), tiles = tiles_x * ceil_div(dst_h, g.th);
    if (tiles > 0x7fffffffll) return MAUA_ENOSYS;
    g.tiles_x = (int)tiles_x, g.tiles = (int)tiles;
    p->twopass = tables + span * row_bytes > LDS_BUDGET;
    p->vec = (out_misalign & 3) == 0 && ((int64_t)out_w * 3 * sz) % 4 == 0 && ((int64_t)dst_x0 * 3 * sz) % 4 == 0;
    p->lds = 0, p->trips = 0, p->grid_x = 0, p->h_total = p->v_total = 0, p->h_trips = p->v_trips = 0, p->ws_bytes = 0;
    const int nb = batch > 0 ? batch : 1;
    if (!p->twopass) {
        g.cap_rows = (int)span;
        p->lds = (size_t)(tables + span * row_bytes);
        p->grid_x = (unsigned)(tiles < FUSED_GRID_CAP ? tiles : FUSED_GRID_CAP);
        p->trips = (int)ceil_div64(tiles, p->grid_x);
    } else {
        p->h_total = ksx ? (int64_t)nb * in_h * dst_w : 0;
        p->v_total = (int64_t)nb * dst_h * dst_w;
        p->h_trips = (int)ceil_div64(ceil_div64(p->h_total, 256), PASS_GRID_CAP);
        p->v_trips = (int)ceil_div64(ceil_div64(p->v_total, 256), PASS_GRID_CAP);
        p->ws_bytes = p->h_total * 3 * sz;
    }
    return 0;
}

template <typename T>
int resample(const T* in, T* out, int batch, int in_h, int in_w, int out_h, int out_w, int dst_x0, int dst_y0, int dst_w, int dst_h,
             const int32_t* kx, const int32_t* bx, int ksize_x, const int32_t* ky, const int32_t* by, int ksize_y, void* ws, void* stream) {
    if (!in || !out || (kx == nullptr) != (bx == nullptr) || (ky == nullptr) != (by == nullptr)) return MAUA_EINVAL;
    if ((kx && (ksize_x < 1 || ksize_x > MAX_TAPS)) || (ky && (ksize_y < 1 || ksize_y > MAX_TAPS))) return MAUA_EINVAL;
    Plan p;
    if (int rc = make_plan((int)sizeof(T), batch, in_h, in_w, out_h, out_w, dst_x0, dst_y0, dst_w, dst_h, kx ? ksize_x : 0, ky ? ksize_y : 0,
                           (unsigned)((uintptr_t)out & 3), &p))
        return rc;
    if (batch == 0) return 0;
    const uintptr_t a0 = (uintptr_t)in, a1 = a0 + (uintptr_t)batch * in_h * in_w * 3 * sizeof(T);
    const uintptr_t b0 = (uintptr_t)out, b1 = b0 + (uintptr_t)batch * out_h * out_w * 3 * sizeof(T);
    if (a0 < b1 && b0 < a1) return MAUA_EINVAL;  // out overlaps in
    hipStream_t st = (hipStream_t)stream;
    if (!p.twopass) {
        const dim3 grid(p.grid_x, (unsigned)batch);
        if (p.vec) {
            hipLaunchKernelGGL((resample_fused_kernel<T, true>), grid, dim3(256), p.lds, st, in, out, kx, bx, ky, by, p.g);
        } else {
            hipLaunchKernelGGL((resample_fused_kernel<T, false>), grid, dim3(256), p.lds, st, in, out, kx, bx, ky, by, p.g);
        }
        MAUA_LAUNCH_CHECK();
        return 0;
    }
    const T* mid = in;  // (a copied x axis: the vertical pass reads the input itself)
    if (kx) {
        if (!ws) return MAUA_EINVAL;
        const uintptr_t w0 = (uintptr_t)ws, w1 = w0 + (uintptr_t)p.ws_bytes;
        if ((w0 < b1 && b0 < w1) || (w0 < a1 && a0 < w1) || (w0 & (sizeof(T) - 1))) return MAUA_EINVAL;
        hipLaunchKernelGGL(resample_h_kernel<T>, dim3(pack_grid(p.h_total, PASS_GRID_CAP)), dim3(256), 0, st, in, (T*)ws, kx, bx, in_w, dst_w,
                           ksize_x, p.h_total);
        MAUA_LAUNCH_CHECK();
        mid = (const T*)ws;
    }
    hipLaunchKernelGGL(resample_v_kernel<T>, dim3(pack_grid(p.v_total, PASS_GRID_CAP)), dim3(256), 0, st, mid, out, ky, by, p.g, p.v_total);
    MAUA_LAUNCH_CHECK();
    return 0;
}
}  // namespace

extern "C" int maua_resample_coeffs(int in_size, int in0, int in1, int out_size, int filter, int32_t* h_k, int32_t* h_bounds, int cap) {
    if (in_size < 1 || out_size < 1 || in0 < 0 || in0 >= in1 || in1 > in_size || filter < 0 || filter > 4) return MAUA_EINVAL;
    const Filter& flt = kFilters[filter];
    const double scale = (double)(in1 - in0) / out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = flt.support * fs;
    const double taps = 2.0 * ceil(support) + 1.0;
    if (taps > MAX_TAPS) return MAUA_ENOSYS;
    const int ksize = (int)taps;
    if (!h_k || !h_bounds || (int64_t)out_size * ksize > (int64_t)cap) return MAUA_EINVAL;
    double w[MAX_TAPS];
    for (int j = 0; j < out_size; ++j) {
        const double center = in0 + (j + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            w[x] = flt.f((x + xmin - center + 0.5) / fs);
            ww += w[x];
        }
        int32_t* k = h_k + (int64_t)j * ksize;
        for (int x = 0; x < xmax; ++x) {
            const double v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = v < 0 ? (int32_t)(-0.5 + v * (double)(1 << BITS)) : (int32_t)(0.5 + v * (double)(1 << BITS));
        }
        for (int x = xmax; x < ksize; ++x) k[x] = 0;
        h_bounds[2 * j] = xmin, h_bounds[2 * j + 1] = xmax;
    }
    return ksize;
}

extern "C" int maua_resample_u8(const uint8_t* in, uint8_t* out, int batch, int in_h, int in_w, int out_h, int out_w, int dst_x0, int dst_y0,
                                int dst_w, int dst_h, const int32_t* kx, const int32_t* bx, int ksize_x, const int32_t* ky, const int32_t* by,
                                int ksize_y, void* ws, void* stream) {
    return resample<uint8_t>(in, out, batch, in_h, in_w, out_h, out_w, dst_x0, dst_y0, dst_w, dst_h, kx, bx, ksize_x, ky, by, ksize_y, ws, stream);
}

extern "C" int maua_resample_u16(const uint16_t* in, uint16_t* out, int batch, int in_h, int in_w, int out_h, int out_w, int dst_x0,
                                 int dst_y0, int dst_w, int dst_h, const int32_t* kx, const int32_t* bx, int ksize_x, const int32_t* ky,
                                 const int32_t* by, int ksize_y, void* ws, void* stream) {
    if ((((uintptr_t)in) | ((uintptr_t)out)) & 1) return MAUA_EINVAL;  // 16-bit samples at an odd address
    return resample<uint16_t>(in, out, batch, in_h, in_w, out_h, out_w, dst_x0, dst_y0, dst_w, dst_h, kx, bx, ksize_x, ky, by, ksize_y, ws,
                              stream);
}

extern "C" int64_t maua_resample_ws_bytes(int sample_bytes, int batch, int in_h, int in_w, int dst_w, int dst_h, int ksize_x, int ksize_y) {
    Plan p;
    if (make_plan(sample_bytes, batch, in_h, in_w, dst_h, dst_w, 0, 0, dst_w, dst_h, ksize_x, ksize_y, 0, &p)) return 0;
    return p.ws_bytes;
}

extern "C" int maua_resample_plan(int sample_bytes, int batch, int in_h, int in_w, int out_h, int out_w, int dst_x0, int dst_y0, int dst_w,
                                  int dst_h, int ksize_x, int ksize_y, int out_misalign, char* buf, int buf_len) {
    Plan p;
    if (int rc = make_plan(sample_bytes, batch, in_h, in_w, out_h, out_w, dst_x0, dst_y0, dst_w, dst_h, ksize_x, ksize_y,
                           (unsigned)out_misalign, &p))
        return rc;
    char text[96];
    const char* type = sample_bytes == 1 ? "u8" : "u16";
    if (!p.twopass)
        snprintf(text, sizeof(text), "fused.%s.%s %dx%d tiles=%d trips=%d rows=%d lds=%d", type, p.vec ? "vec" : "scalar", TW, p.g.th, p.g.tiles,
                 p.trips, p.g.cap_rows, (int)p.lds);
    else
        snprintf(text, sizeof(text), "twopass.%s trips=%d,%d ws=%lld", type, p.h_trips, p.v_trips, (long long)p.ws_bytes);
    if (!buf || buf_len <= (int)strlen(text)) return MAUA_EINVAL;
    memcpy(buf, text, strlen(text) + 1);
    return 0;
}
