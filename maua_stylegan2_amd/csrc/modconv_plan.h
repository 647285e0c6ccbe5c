// What the host planner (modconv.hip) and the instance units of the generic convolution kernel (modconv_m0.hip .. modconv_m4.hip) share:
// the kernel's argument structs, the key and table types of its instances, and the tile constants from which both sides derive sizes.
// Plain structs and constexpr / inline functions at namespace scope, defined identically in every unit: one identity across the library.
#pragma once
#include "common.h"

// Ablation / A-B switches only exist in -DMAUA_EXPERIMENTS builds (tools/build_exp.sh): the product kernels carry no debug
// branches and the product library exports no tuning entry.
#ifdef MAUA_EXPERIMENTS
#define MAUA_DBG(mask) ((g.debug & (mask)) != 0)
#define MAUA_CFG(mask) ((g_conv_cfg & (mask)) != 0)
#else
#define MAUA_DBG(mask) false
#define MAUA_CFG(mask) false
#endif

// channels per K chunk: the weight tile As[rows][CC][BM] is kept at <= 18..24 KB so that the double buffer fits 2-3x per CU
constexpr int chunk_channels(int bm, int bn = 0, int mode = 0) {
    if (mode == 3) return 4;  // F(4,3): 18 weight rows per channel (tiles of 32 and 64 rows only: see make_plan)
    return (bm >= 128 || bn >= 512) ? 4 : 8;
}

struct ConvGeom {
    int B, Cin, Cout, CoutPad, H, W;  // input feature map
    int GH, GW;                       // per-image grid of tile positions (plain: H,W   up: H+1,W+1)
    int OH, OW;                       // output plane
    int lsw, lsh;                     // log2 sub-tile (one MFMA N=32 group) width / height, 2^(lsw+lsh) = 32
    int lnsx, lnsy;                   // log2 sub-tiles per tile along x / y
    int lni;                          // log2 images per tile
    int tiles_x, tiles_y, img_groups;
    int PH, PW, PWS, PSTRIDE;         // staged patch: rows, valid cols, LDS row stride, floats per channel (all images)
    int m_tiles, n_tiles;
    int splits, chunks_per_split, n_chunks;
    int s_stride;
    float wscale;
    int fuse_act;
    int64_t noise_batch_stride;
    int64_t ws_slab;  // floats per split slab
    int flat;         // transposed mode: tiles are runs of BN consecutive positions of the row-major (H+1)x(W+1) grid
    int rgb;          // fused ToRGB epilogue: 0 off, 1 on, 2 on and the feature map itself is not stored
    float rgb_wscale;
    int force_ws;     // the partial sums go to the workspace slabs also when K is not split (the low-resolution entries reduce them themselves)
#ifdef MAUA_EXPERIMENTS
    int debug;        // (maua_tuning_set key 1) 1 skip stores, 2 skip MFMA, 4 skip loads, 32 skip weight DMA, 64 skip patch loads,
                      // 128 fold the patch loads onto 4 KB per channel (always cache hits; wrong results).  Not a member of the product's struct.
#endif
};

struct ConvPtrs {
    const float* x;
    const float* wp;
    const float* s;
    const float* d;
    const float* noise;
    const float* noise_w;
    const float* bias;
    float* y;
    float* ws;
    // fused ToRGB (models/stylegan2.py:346-365) — only for single-M-tile plain configs
    const float* rgb_w;     // [3, Cout]
    const float* rgb_s;     // styles of the ToRGB layer, [B, s_stride] (already offset to the layer's slice)
    const float* rgb_bias;  // [3]
    const float* rgb_skip;  // [B, 3, H/2, W/2] or null
    const float* rgb_k4;    // 4x4 upsample taps
    float* rgb_out;         // [B, 3, H, W]
    uint8_t* rgb_u8;        // when set: the image leaves as uint8 NHWC frames [B, H, W, 3] (render.py:40-43) instead of rgb_out
    // frame source (include/maua_hip.h): when set, the noise maps are read from src->noise[noise_slot] at frame src->frame0
    const maua_frame_source_t* src;
    int noise_slot;
};

// Column layout of the Winograd weight packs (modes 2 and 3).  Layers above 32 output channels run with two 32-channel
// M-tiles per wave; their columns are interleaved [lane][m-tile] inside every group of 64 channels (and padded to a multiple
// of 64) so that a lane fetches both A operands with one 8-byte LDS read.  (Destination column -> source channel:
// wino_src_channel, modconv_pack.hip.)
__host__ __device__ inline int wino_cout_pad(int cout) { return cout > 32 ? (cout + 63) / 64 * 64 : (cout + 31) / 32 * 32; }

// Floats per channel the staged patch of a config may hold.  A thread stages MAXP positions of it (PSTRIDE <= 256 MAXP); the instances
// with MAXP = 3 exist for the wide-N configs only.
constexpr int patch_limit(int mode, int bn) {
    return (bn >= 512 || (mode == 2 && bn >= 256) || ((mode == 3 || mode == 4) && bn >= 128)) ? 768 : 512;
}

inline int pad32(int c) { return (c + 31) / 32 * 32; }

// ---- which instance a shape runs: ONE table per mode of the instances the library holds, ONE host function that picks among them
// The template arguments of an instance.  make_plan() derives the key of a shape; the table of its mode finds its launcher.
struct ConvKey {
    int bm, bn, wm, mode;
    bool multi, fast;
    int maxp;
    bool operator==(const ConvKey& o) const {
        return bm == o.bm && bn == o.bn && wm == o.wm && mode == o.mode && multi == o.multi && fast == o.fast && maxp == o.maxp;
    }
};

struct ConvInstance {
    ConvKey key;
    const char* name;  // as rocprofv3 prints it: bench.py and tests/golden/conv_instances.json join on it
    int (*launch)(const char* name, int64_t blocks, size_t lds_bytes, hipStream_t st, const ConvGeom& g, const ConvPtrs& p);
};

// The table of mode M is defined by modconv_m<M>.hip, the only unit that instantiates the kernel template for that mode, and handed out by
// a host function: a const array with external linkage would also be emitted into the unit's device code, where its launchers do not exist.
// (Hidden: the functions are the library's own business, its dynamic symbols stay those of include/maua_hip.h and common.h.)
struct ConvTable {
    const ConvInstance* rows;
    int count;
};
__attribute__((visibility("hidden"))) ConvTable maua_conv_table_m0(), maua_conv_table_m1(), maua_conv_table_m2(), maua_conv_table_m3(), maua_conv_table_m4();
