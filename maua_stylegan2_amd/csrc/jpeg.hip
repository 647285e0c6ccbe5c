// Packed RGB frames -> one baseline JPEG per frame (render.py FrameSink, pix_fmt mjpeg): the frame leaves the device at roughly a tenth of
// its rgb24 size and describes itself, so that the host can write a playable Motion-JPEG .avi without an encoder (avi.py).
//
// THE STREAM, in integers only (tests/jpeg_ref.py restates it in numpy; the device output equals it byte for byte):
//   Structure   baseline sequential DCT, 8 bit, 3 components: Y sampled 2 x 2 with quantisation table 0, Cb and Cr 1 x 1 with table 1; one
//               interleaved scan, MCU = 16 x 16 pixels = blocks Y00 Y01 Y10 Y11 Cb Cr.  Markers: SOI, APP0 (JFIF 1.01, density 1:1),
//               DQT 0, DQT 1, SOF0, DHT x 4 (the standard ITU-T T.81 Annex K.3 tables: DC0, AC0, DC1, AC1), DRI, SOS, entropy data, EOI.
//   Dimensions  any 1 <= w, h <= 65535 (SOF0); partial MCUs are filled by replicating the last column / row of the frame.
//   Quantiser   Annex K.1 / K.2 scaled the IJG way: scale = 5000 / q for q < 50, else 200 - 2 q; t' = clamp((t scale + 50) / 100, 1, 255);
//               quality q in 1 .. 95.
//   Colour      JFIF full-range BT.601, 16-bit fixed point, per pixel:
//                 Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
//                 Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16
//                 Cr = ( 32768 R - 27439 G -  5329 B + 8388608 + 32767) >> 16
//               every 2 x 2 block of Cb / Cr averaged as (sum + 2) >> 2; level shift -128.
//   DCT         the Loeffler-Ligtenberg-Moschytz 8-point form with 13-bit constants, int32 throughout, rows then columns (dct8 below).
//               With t0..t3 = d0+d7, d1+d6, d2+d5, d3+d4, t7..t4 = d0-d7, d1-d6, d2-d5, d3-d4, t10 = t0+t3, t13 = t0-t3, t11 = t1+t2,
//               t12 = t1-t2 and R(x, n) = (x + (1 << (n-1))) >> n (arithmetic shift):
//                 row pass    o0 = (t10+t11) << 2, o4 = (t10-t11) << 2, every other output R(., 11)
//                 column pass o0 = R(t10+t11, 2),  o4 = R(t10-t11, 2),  every other output R(., 15)
//                 z = (t12+t13) 4433:  o2 = z + t13 6270,  o6 = z - t12 15137
//                 z5 = (t4+t5+t6+t7) 9633, z1 = -(t4+t7) 7373, z2 = -(t5+t6) 20995, z3 = z5 - (t4+t6) 16069, z4 = z5 - (t5+t7) 3196
//                 o7 = t4 2446 + z1 + z3, o5 = t5 16819 + z2 + z4, o3 = t6 25172 + z2 + z3, o1 = t7 12299 + z1 + z4
//               The result c is 8 times the orthonormal DCT.  Quantised value v = sign(c) ((|c| + d / 2) / d), d = 8 t'.
//   Entropy     zig-zag order; DC differences per component; AC with ZRL and EOB; a negative value v is sent as the low bits of v - 1.
//   Restarts    interval length restart_mcus in 1 .. 65535 (an interval may span MCU rows and need not divide the MCU count); every
//               interval starts with the three DC predictors at 0, is padded with 1-bits to a byte boundary and, the last excepted, is
//               followed by RSTm, m = 0 .. 7 cyclically; every 0xFF byte of entropy data is followed by 0x00.
// The restart intervals make the entropy coding parallel: every interval is byte-aligned and independent of the others.
//
// THREE KERNELS on the caller's stream, through the workspace ws = coefficients | interval segments | interval lengths:
//   jpeg_dct_quant_kernel  a workgroup per 4 MCUs of an MCU row: 16 rows x 64 pixels read as 12-byte segments (consecutive lanes own
//                          consecutive segments of a row), colour + chroma average + DCT + quantiser through LDS, the 24 blocks' zig-zag
//                          int16 coefficients stored as one contiguous 3 KiB run of ws [frame][MCU][6][64].  3 B/px in, 3 B/px out.
//   jpeg_entropy_kernel    a workgroup per restart interval, a thread per block, 256 blocks at a time: bit lengths, a workgroup prefix sum
//                          for every block's bit offset, the bits assembled in LDS (a block's DC predictor is the DC of the block
//                          before it of the same component: read directly), then byte stuffing by a second prefix over the 0xFF counts.
//                          Segment size: a block is at most 11 + 11 bits of DC (the longest DC code has 11 bits) and 63 x (16 + 10) bits of
//                          AC = 1660 bits; 6 blocks = 1245 bytes, doubled by stuffing = 2490, rounded to kSegBytesPerMcu = 2496 per
//                          MCU, plus 16 bytes for the padded last byte (2 after stuffing).
//   jpeg_pack_kernel       per frame: sum of the interval lengths (overflow test), exclusive scan, then header, segments, RSTm and EOI to
//                          their offsets in the slot, the 16-byte slot header last.
#include <algorithm>
#include <initializer_list>

#include "common.h"
#include "wave.h"

namespace {
constexpr int kSegBytesPerMcu = 2496;
constexpr int kSegBytesExtra = 16;
constexpr int kMaxBlockBits = 22 + 63 * 26;
constexpr int kHeaderBytes = 2 + 18 + 2 * 69 + 19 + 2 * 33 + 2 * 183 + 6 + 14;  // 629

struct JpegTables {
    uint8_t quant[2][64];    // Annex K.1 / K.2, natural order
    uint8_t zigzag[64];      // natural index of the k-th coefficient in zig-zag order
    uint8_t unzigzag[64];    // zig-zag position of natural index n
    uint8_t bits[4][16];     // Annex K.3 in stream order: DC0, AC0, DC1, AC1
    uint8_t vals[4][162];
    uint8_t n_vals[4];
    uint32_t codes[4][256];  // [table][symbol] = code << 8 | length (0: no such symbol)
};

constexpr JpegTables make_tables() {
    constexpr uint8_t luma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                  69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                                  81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99};
    constexpr uint8_t chroma[16] = {17, 18, 24, 47, 18, 21, 26, 66, 24, 26, 56, 99, 47, 66, 99, 99};  // top-left 4 x 4, everything else 99
    constexpr uint8_t dc_bits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
    constexpr uint8_t ac_bits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
    constexpr uint8_t ac_vals[2][162] = {
        {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
         0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
         0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
         0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
         0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
         0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
         0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
         0xfa},
        {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
         0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
         0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
         0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
         0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
         0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
         0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
         0xfa}};
    JpegTables t{};
    for (int n = 0; n < 64; ++n) {
        t.quant[0][n] = luma[n];
        t.quant[1][n] = (n / 8 < 4 && n % 8 < 4) ? chroma[(n / 8) * 4 + n % 8] : 99;
    }
    for (int k = 0, x = 0, y = 0; k < 64; ++k) {  // the zig-zag walk of an 8 x 8 block
        t.zigzag[k] = (uint8_t)(y * 8 + x);
        t.unzigzag[y * 8 + x] = (uint8_t)k;
        if ((x + y) % 2 == 0) {  // moving up and to the right
            if (x == 7) ++y;
            else if (y == 0) ++x;
            else ++x, --y;
        } else {
            if (y == 7) ++x;
            else if (x == 0) ++y;
            else --x, ++y;
        }
    }
    for (int tab = 0; tab < 4; ++tab) {
        const bool ac = tab & 1;
        const int which = tab >> 1;
        t.n_vals[tab] = ac ? 162 : 12;
        for (int i = 0; i < 16; ++i) t.bits[tab][i] = ac ? ac_bits[which][i] : dc_bits[which][i];
        for (int i = 0; i < t.n_vals[tab]; ++i) t.vals[tab][i] = ac ? ac_vals[which][i] : (uint8_t)i;
        uint32_t code = 0;
        for (int len = 1, k = 0; len <= 16; ++len) {  // T.81 Annex C
            for (int i = 0; i < t.bits[tab][len - 1]; ++i) t.codes[tab][t.vals[tab][k++]] = (code++ << 8) | (uint32_t)len;
            code <<= 1;
        }
    }
    return t;
}

constexpr JpegTables kTables = make_tables();
__constant__ JpegTables d_tables = make_tables();

constexpr int scaled_quant(int base, int quality) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int q = (base * scale + 50) / 100;
    return q < 1 ? 1 : (q > 255 ? 255 : q);
}

// ------------------------------------------------------------------------------------------------ colour, DCT, quantiser
__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one 8-point pass (header comment): FIRST = the row pass
template <bool FIRST>
__device__ __forceinline__ void dct8(int (&d)[8]) {
    constexpr int S = FIRST ? 11 : 15;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = FIRST ? (t10 + t11) << 2 : descale(t10 + t11, 2);
    d[4] = FIRST ? (t10 - t11) << 2 : descale(t10 - t11, 2);
    const int z = (t12 + t13) * 4433;
    d[2] = descale(z + t13 * 6270, S);
    d[6] = descale(z - t12 * 15137, S);
    const int z5 = (t4 + t5 + t6 + t7) * 9633;
    const int z1 = -(t4 + t7) * 7373, z2 = -(t5 + t6) * 20995;
    const int z3 = z5 - (t4 + t6) * 16069, z4 = z5 - (t5 + t7) * 3196;
    d[7] = descale(t4 * 2446 + z1 + z3, S);
    d[5] = descale(t5 * 16819 + z2 + z4, S);
    d[3] = descale(t6 * 25172 + z2 + z3, S);
    d[1] = descale(t7 * 12299 + z1 + z4, S);
}

constexpr int GROUP = 4;         // MCUs per workgroup
constexpr int WS_STRIDE = 72;    // dwords per block of the row-pass results: 64 + 8, so that the column reads of 4 blocks hit 32 banks

__global__ __launch_bounds__(256) void jpeg_dct_quant_kernel(const uint8_t* __restrict__ rgb, int16_t* __restrict__ coef, int h, int w, int mw,
                                                             int groups_per_row, int quality, int dword_rows) {
    __shared__ int16_t s_y[16][GROUP * 16], s_cb[16][GROUP * 16], s_cr[16][GROUP * 16];
    __shared__ int s_rows[GROUP * 6 * WS_STRIDE];
    __shared__ int s_div[2][64];
    __shared__ __attribute__((aligned(16))) int16_t s_out[GROUP * 6 * 64];
    const int tid = threadIdx.x;
    const int64_t frame = blockIdx.y;
    const int my = blockIdx.x / groups_per_row;
    const int mx0 = (blockIdx.x - my * groups_per_row) * GROUP;
    const int n_mcu = min(GROUP, mw - mx0);
    if (tid < 128) s_div[tid >> 6][tid & 63] = 8 * scaled_quant(d_tables.quant[tid >> 6][tid & 63], quality);
    {   // 16 rows x 16 segments of 4 pixels
        const int row = tid >> 4, x = mx0 * 16 + (tid & 15) * 4, y = my * 16 + row;
        const uint8_t* src = rgb + frame * h * w * 3;
        int px[12];
        if (dword_rows && y < h && x + 4 <= w) {
            const uint32_t* p = reinterpret_cast<const uint32_t*>(src + ((int64_t)y * w + x) * 3);
            const uint32_t d[3] = {p[0], p[1], p[2]};
#pragma unroll
            for (int k = 0; k < 12; ++k) px[k] = (int)((d[k >> 2] >> ((k & 3) * 8)) & 0xffu);
        } else {  // the frame's edge, or rows off the dword grid: byte loads, the last row / column replicated
            const uint8_t* line = src + (int64_t)min(y, h - 1) * w * 3;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint8_t* p = line + (int64_t)min(x + i, w - 1) * 3;
                px[3 * i] = p[0], px[3 * i + 1] = p[1], px[3 * i + 2] = p[2];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = px[3 * i], g = px[3 * i + 1], b = px[3 * i + 2];
            const int col = (tid & 15) * 4 + i;
            s_y[row][col] = (int16_t)(((19595 * r + 38470 * g + 7471 * b + 32768) >> 16) - 128);
            s_cb[row][col] = (int16_t)((-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16);
            s_cr[row][col] = (int16_t)((32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16);
        }
    }
    __syncthreads();
    const int blk = tid >> 3, lane8 = tid & 7;  // 24 blocks x 8 rows / columns on the first 192 threads
    const int mcu = blk / 6, comp = blk - mcu * 6;
    if (tid < GROUP * 6 * 8) {
        int d[8];
        if (comp < 4) {
            const int16_t* p = &s_y[(comp >> 1) * 8 + lane8][mcu * 16 + (comp & 1) * 8];
#pragma unroll
            for (int i = 0; i < 8; ++i) d[i] = p[i];
        } else {
            const int16_t(*c)[GROUP * 16] = comp == 4 ? s_cb : s_cr;
            const int16_t *p0 = &c[2 * lane8][mcu * 16], *p1 = &c[2 * lane8 + 1][mcu * 16];
#pragma unroll
            for (int i = 0; i < 8; ++i) d[i] = ((p0[2 * i] + p0[2 * i + 1] + p1[2 * i] + p1[2 * i + 1] + 2) >> 2) - 128;
        }
        dct8<true>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) s_rows[blk * WS_STRIDE + lane8 * 8 + i] = d[i];
    }
    __syncthreads();
    if (tid < GROUP * 6 * 8) {
        int d[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) d[r] = s_rows[blk * WS_STRIDE + r * 8 + lane8];
        dct8<false>(d);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int n = r * 8 + lane8;
            const uint32_t div = (uint32_t)s_div[comp >= 4][n];
            const int v = (int)(((uint32_t)abs(d[r]) + div / 2) / div);
            s_out[blk * 64 + d_tables.unzigzag[n]] = (int16_t)(d[r] < 0 ? -v : v);
        }
    }
    __syncthreads();
    if (tid < n_mcu * 48) {  // 768 bytes per MCU, 16 per thread
        const int mh = gridDim.x / groups_per_row;
        uint4* dst = reinterpret_cast<uint4*>(coef + ((frame * mh + my) * mw + mx0) * 384);
        dst[tid] = reinterpret_cast<const uint4*>(s_out)[tid];
    }
}

// ------------------------------------------------------------------------------------------------ entropy coding
// exclusive prefix sum over the 256 threads of a workgroup; every thread calls it; `part` is 4 words of LDS
template <typename T>
__device__ __forceinline__ T block_scan(T v, T* part, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T x = wave_incl_sum(v, lane);
    if (lane == 63) part[wave] = x;
    __syncthreads();
    T base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i < wave) base += part[i];
        total += part[i];
    }
    __syncthreads();  // (part is free again)
    return base + x - v;
}

// Bits go into LDS words MSB first: stream bit p is bit 31 - p % 32 of word p / 32.  Neighbouring blocks share words: atomic OR into
// zeroed words.
struct BitWriter {
    uint32_t* words;
    uint64_t acc;
    int n, word;
    __device__ __forceinline__ void start(uint32_t* w, int bit) { words = w, acc = 0, n = bit & 31, word = bit >> 5; }
    __device__ __forceinline__ void put(uint32_t bits, int len) {  // len <= 26
        acc = (acc << len) | bits;
        n += len;
        if (n >= 32) {
            n -= 32;
            atomicOr(&words[word++], (uint32_t)(acc >> n));
        }
    }
    __device__ __forceinline__ void finish() {
        if (n > 0) atomicOr(&words[word], (uint32_t)(acc << (32 - n)));
    }
};

// a value's size category and the bits behind its code
__device__ __forceinline__ void magnitude(int v, int& size, uint32_t& extra) {
    size = 32 - __clz(abs(v));
    extra = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
}

// One block's code: returns its length in bits; EMIT writes it as well.  `block`: 64 zig-zag coefficients (128 bytes, 16-byte aligned).
template <bool EMIT>
__device__ __forceinline__ int encode_block(const uint4* __restrict__ block, int dc_diff, const uint32_t* dc, const uint32_t* ac, BitWriter& bw) {
    int size;
    uint32_t extra;
    magnitude(dc_diff, size, extra);
    uint32_t e = dc[size];
    int total = (int)(e & 0xffu) + size;
    if (EMIT) bw.put(((e >> 8) << size) | extra, (int)(e & 0xffu) + size);
    int run = 0;
    for (int g = 0; g < 8; ++g) {
        const uint4 q = block[g];
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (g == 0 && j == 0) continue;  // the DC
            const int v = (int)(int16_t)(w[j >> 1] >> ((j & 1) * 16));
            if (v == 0) {
                ++run;
                continue;
            }
            while (run > 15) {  // ZRL
                e = ac[0xf0];
                total += (int)(e & 0xffu);
                if (EMIT) bw.put(e >> 8, (int)(e & 0xffu));
                run -= 16;
            }
            magnitude(v, size, extra);
            e = ac[(run << 4) | size];
            total += (int)(e & 0xffu) + size;
            if (EMIT) bw.put(((e >> 8) << size) | extra, (int)(e & 0xffu) + size);
            run = 0;
        }
    }
    if (run > 0) {  // EOB
        e = ac[0];
        total += (int)(e & 0xffu);
        if (EMIT) bw.put(e >> 8, (int)(e & 0xffu));
    }
    return total;
}

constexpr int CHUNK = 256;                                              // blocks coded at a time = threads
constexpr int BIT_WORDS = (CHUNK * kMaxBlockBits + 7 + 31) / 32 + 1;    // 7: the carried bits of the chunk before

__global__ __launch_bounds__(256) void jpeg_entropy_kernel(const int16_t* __restrict__ coef, uint8_t* __restrict__ segs, uint32_t* __restrict__ lens,
                                                           int mcus, int restart_mcus, int n_intervals, int64_t seg_cap) {
    __shared__ uint32_t s_bits[BIT_WORDS];
    __shared__ uint32_t s_codes[4 * 256];
    __shared__ int s_part[4];
    const int tid = threadIdx.x;
    const int interval = blockIdx.x;
    const int64_t frame = blockIdx.y;
    const int first_mcu = interval * restart_mcus;
    const int n_blocks = min(restart_mcus, mcus - first_mcu) * 6;
    const int16_t* blocks = coef + (frame * mcus + first_mcu) * 384;
    uint8_t* out = segs + (frame * n_intervals + interval) * seg_cap;
    for (int i = tid; i < 4 * 256; i += 256) s_codes[i] = d_tables.codes[i >> 8][i & 255];
    __syncthreads();
    int64_t out_pos = 0;
    int carry_bits = 0;       // bits of the last, incomplete byte of the chunk before ...
    uint32_t carry_byte = 0;  // ... and that byte (its unused low bits zero)
    for (int chunk = 0; chunk < n_blocks; chunk += CHUNK) {
        const int k = chunk + tid;
        const bool valid = k < n_blocks;
        int len = 0, diff = 0, tab = 0;
        BitWriter bw;
        bw.start(s_bits, 0);
        if (valid) {
            const int m = k / 6, j = k - m * 6;
            // the block before this one of the same component: Y within the MCU, else the last block of that component one MCU back
            const int before = j >= 1 && j <= 3 ? k - 1 : (m > 0 ? (j == 0 ? k - 3 : k - 6) : -1);
            diff = blocks[(int64_t)k * 64] - (before >= 0 ? blocks[(int64_t)before * 64] : 0);
            tab = j >= 4;
            len = encode_block<false>(reinterpret_cast<const uint4*>(blocks + (int64_t)k * 64), diff, s_codes + tab * 512, s_codes + tab * 512 + 256, bw);
        }
        int total;
        const int offset = block_scan(len, s_part, total);
        int n_bits = carry_bits + total;
        for (int i = tid; i <= (n_bits >> 5) + 1 && i < BIT_WORDS; i += 256) s_bits[i] = i == 0 ? carry_byte << 24 : 0u;
        __syncthreads();
        if (valid) {
            bw.start(s_bits, carry_bits + offset);
            encode_block<true>(reinterpret_cast<const uint4*>(blocks + (int64_t)k * 64), diff, s_codes + tab * 512, s_codes + tab * 512 + 256, bw);
            bw.finish();
        }
        __syncthreads();
        const bool last = chunk + CHUNK >= n_blocks;
        if (last && (n_bits & 7)) {  // pad the interval with 1-bits (inside one byte, hence one word)
            const int pad = 8 - (n_bits & 7);
            if (tid == 0) s_bits[n_bits >> 5] |= ((1u << pad) - 1u) << (32 - (n_bits & 31) - pad);
            n_bits += pad;
        }
        __syncthreads();
        const int n_bytes = n_bits >> 3;
        auto byte_at = [&](int i) { return (s_bits[i >> 2] >> (24 - 8 * (i & 3))) & 0xffu; };
        carry_bits = n_bits & 7;
        carry_byte = carry_bits ? byte_at(n_bytes) : 0u;
        // byte stuffing: a thread owns a run of bytes, the prefix over the 0xFF counts gives the run's place
        const int per = (n_bytes + 255) / 256;
        const int lo = min(tid * per, n_bytes), hi = min(lo + per, n_bytes);
        int n_ff = 0;
        for (int i = lo; i < hi; ++i) n_ff += byte_at(i) == 0xffu;
        int total_ff;
        int64_t dst = out_pos + lo + block_scan(n_ff, s_part, total_ff);
        for (int i = lo; i < hi; ++i) {
            const uint32_t b = byte_at(i);
            if (dst < seg_cap) out[dst] = (uint8_t)b;  // (seg_cap is the worst case: the tests never see these bounds refuse a byte)
            ++dst;
            if (b == 0xffu) {
                if (dst < seg_cap) out[dst] = 0;
                ++dst;
            }
        }
        out_pos += n_bytes + total_ff;
        __syncthreads();  // s_bits is rewritten by the next chunk
    }
    if (tid == 0) lens[frame * n_intervals + interval] = (uint32_t)min(out_pos, seg_cap);
}

// ------------------------------------------------------------------------------------------------ packing
__global__ __launch_bounds__(256) void jpeg_pack_kernel(const uint8_t* __restrict__ segs, const uint32_t* __restrict__ lens, const uint8_t* __restrict__ header,
                                                        int header_len, uint8_t* __restrict__ out, int64_t slot_bytes, int n_intervals, int64_t seg_cap) {
    __shared__ long long s_part[4];
    __shared__ long long s_off[256];
    __shared__ uint32_t s_len[256];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t frame = blockIdx.y;
    const uint32_t* len_of = lens + frame * n_intervals;
    uint8_t* slot = out + frame * slot_bytes;
    long long sum = 0, n;
    for (int i = tid; i < n_intervals; i += 256) sum += len_of[i];
    block_scan(sum, s_part, n);
    n += header_len + 2ll * (n_intervals - 1) + 2;  // + RSTm behind every interval but the last + EOI
    const bool overflow = 16 + n > slot_bytes;
    if (!overflow) {
        uint8_t* body = slot + 16 + header_len;
        long long carry = 0;
        const int my_wave = blockIdx.x * 4 + (tid >> 6), n_waves = gridDim.x * 4;
        for (int chunk = 0; chunk < n_intervals; chunk += 256) {
            const int i = chunk + tid;
            const uint32_t len = i < n_intervals ? len_of[i] : 0u;
            long long total;
            s_off[tid] = carry + block_scan((long long)len + (i < n_intervals - 1 ? 2 : 0), s_part, total);
            s_len[tid] = len;
            carry += total;
            __syncthreads();
            for (int j = my_wave; j < min(256, n_intervals - chunk); j += n_waves) {  // a wave copies an interval
                const uint8_t* src = segs + (frame * n_intervals + chunk + j) * seg_cap;
                uint8_t* dst = body + s_off[j];
                const uint32_t bytes = s_len[j];
                for (uint32_t b = lane; b < bytes; b += 64) dst[b] = src[b];
                if (lane == 0 && chunk + j < n_intervals - 1) dst[bytes] = 0xff, dst[bytes + 1] = (uint8_t)(0xd0 + ((chunk + j) & 7));
            }
            __syncthreads();
        }
        if (blockIdx.x == 0) {
            for (int b = tid; b < header_len; b += 256) slot[16 + b] = header[b];
            if (tid == 0) slot[16 + n - 2] = 0xff, slot[16 + n - 1] = 0xd9;
        }
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid < 16) slot[tid] = tid < 4 ? (uint8_t)((uint64_t)n >> (8 * tid)) : (uint8_t)(tid == 4 && overflow);
}

struct Plan {
    int mw, mh, mcus, n_intervals;
    int64_t seg_cap, coef_bytes, seg_bytes, len_bytes;
};

bool plan(int batch, int h, int w, int restart_mcus, Plan& p) {
    if (batch < 0 || h < 1 || w < 1 || h > 65535 || w > 65535 || restart_mcus < 1 || restart_mcus > 65535) return false;
    p.mw = ceil_div(w, 16), p.mh = ceil_div(h, 16), p.mcus = p.mw * p.mh;
    p.n_intervals = ceil_div(p.mcus, restart_mcus);
    p.seg_cap = (int64_t)(restart_mcus < p.mcus ? restart_mcus : p.mcus) * kSegBytesPerMcu + kSegBytesExtra;
    p.coef_bytes = (int64_t)batch * p.mcus * 768;
    p.seg_bytes = (int64_t)batch * p.n_intervals * p.seg_cap;
    p.len_bytes = (int64_t)batch * p.n_intervals * 4;
    return true;
}
}  // namespace

extern "C" int maua_jpeg_header(int h, int w, int quality, int restart_mcus, uint8_t* h_buf, int cap) {
    Plan p;
    if (!plan(0, h, w, restart_mcus, p) || quality < 1 || quality > 95 || !h_buf || cap < kHeaderBytes) return MAUA_EINVAL;
    uint8_t* o = h_buf;
    auto put = [&o](std::initializer_list<int> bytes) {
        for (int b : bytes) *o++ = (uint8_t)b;
    };
    put({0xff, 0xd8});
    put({0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int t = 0; t < 2; ++t) {
        put({0xff, 0xdb, 0, 67, t});
        for (int k = 0; k < 64; ++k) *o++ = (uint8_t)scaled_quant(kTables.quant[t][kTables.zigzag[k]], quality);
    }
    put({0xff, 0xc0, 0, 17, 8, h >> 8, h & 255, w >> 8, w & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int t = 0; t < 4; ++t) {
        const int n = kTables.n_vals[t];
        put({0xff, 0xc4, (3 + 16 + n) >> 8, (3 + 16 + n) & 255, ((t & 1) << 4) | (t >> 1)});
        for (int i = 0; i < 16; ++i) *o++ = kTables.bits[t][i];
        for (int i = 0; i < n; ++i) *o++ = kTables.vals[t][i];
    }
    put({0xff, 0xdd, 0, 4, restart_mcus >> 8, restart_mcus & 255});
    put({0xff, 0xda, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    return (int)(o - h_buf);
}

extern "C" int64_t maua_jpeg_ws_bytes(int batch, int h, int w, int restart_mcus) {
    Plan p;
    if (!plan(batch, h, w, restart_mcus, p)) return 0;
    return p.coef_bytes + p.seg_bytes + p.len_bytes;
}

extern "C" int maua_jpeg_encode_u8(const uint8_t* rgb, int batch, int h, int w, int quality, int restart_mcus, const uint8_t* header, int header_len,
                                   uint8_t* out, int64_t slot_bytes, void* ws, void* stream) {
    Plan p;
    if (!plan(batch, h, w, restart_mcus, p) || quality < 1 || quality > 95) return MAUA_EINVAL;
    if (batch == 0) return 0;
    if (!rgb || !header || !out || !ws || header_len < 1 || slot_bytes < 16 + (int64_t)header_len + 2) return MAUA_EINVAL;
    if ((uintptr_t)ws & 15) return MAUA_EINVAL;  // (the coefficients move as 16-byte words)
    if (batch > 65535) return MAUA_ENOSYS;       // (the frame is the grid's y)
    int16_t* coef = static_cast<int16_t*>(ws);
    uint8_t* segs = static_cast<uint8_t*>(ws) + p.coef_bytes;
    uint32_t* lens = reinterpret_cast<uint32_t*>(segs + p.seg_bytes);  // (coef_bytes and seg_cap are multiples of 16)
    hipStream_t st = (hipStream_t)stream;
    const int groups_per_row = ceil_div(p.mw, GROUP);
    const int dword_rows = w % 4 == 0 && ((uintptr_t)rgb & 3) == 0;
    hipLaunchKernelGGL(jpeg_dct_quant_kernel, dim3((unsigned)(groups_per_row * p.mh), (unsigned)batch), dim3(256), 0, st, rgb, coef, h, w, p.mw,
                       groups_per_row, quality, dword_rows);
    MAUA_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)p.n_intervals, (unsigned)batch), dim3(256), 0, st, coef, segs, lens, p.mcus, restart_mcus,
                       p.n_intervals, p.seg_cap);
    MAUA_LAUNCH_CHECK();
    const int pack_groups = std::min(std::max(ceil_div(p.n_intervals, 8), 1), 32);
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3((unsigned)pack_groups, (unsigned)batch), dim3(256), 0, st, segs, lens, header, header_len, out, slot_bytes,
                       p.n_intervals, p.seg_cap);
    MAUA_LAUNCH_CHECK();
    return 0;
}
