/*
 * maua_hip.h — C ABI of libmaua_hip.so, the MI355X (gfx950) native library behind the audio-reactive StyleGAN2
 * inference path.  Plain pointers and sizes only; every pointer is a DEVICE pointer unless named h_*;
 * `stream` is a hipStream_t passed as void*.  Every launcher is asynchronous on `stream`, never
 * synchronises, never allocates, and returns 0 on success, a hipError_t (> 0) from the launch, or a
 * negative MAUA_E* code for rejected arguments.  All tensors are contiguous fp32 NCHW unless stated.
 *
 * Each entry point names the reference interface (file:line under /root/reference) it replaces.
 */
#ifndef MAUA_HIP_H
#define MAUA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAUA_EINVAL (-22)
#define MAUA_ENOSYS (-38)

/* ABI version of this header; bumped on any signature change. */
int maua_abi_version(void);  /* 8: + maua_bend_point_f32, maua_bend_morph_f32 (point and morphological network bends); 7: + maua_randn_frames_f32 (counter-based noise); 6: + the structural-segmentation entries (maua_tempogram_f32 ... maua_rec_affinity_f32); 5: + the low-resolution entries (maua_*_lowres_*), maua_const_styledconv_f32, maua_torgb_f32's plane-sum form; 4: the style fold (post_s arguments, s == NULL; round 6); 3: + maua_upconv_blur_f32 (round 5); 2: frame source (maua_frame_source_t) arguments; no tuning entry */
/* Number of compute units / name of device 0 (diagnostics for bench.py). */
int maua_device_info(int* cu_count, int* lds_bytes, char* name, int name_len);

/* ------------------------------------------------------------------------------------------------ ops
 * Replaces pybind `upfirdn2d.upfirdn2d(input[major,in_h,in_w,minor], kernel[kh,kw], up_x, up_y, down_x,
 * down_y, pad_x0, pad_x1, pad_y0, pad_y1)` — op/upfirdn2d.cpp:12-22, op/upfirdn2d_kernel.cu:209-369.
 * y must hold major*out_h*out_w*minor floats, out = (in*up + pad0 + pad1 - k)/down + 1 (floor).
 * `k` is the un-flipped [kh,kw] tap matrix in DEVICE memory (true convolution, as the reference).
 * Every argument combination is served; tiled HBM-rate kernels exist for the shapes the reference's own kernel tiles (modes 1-6 of
 * op/upfirdn2d_kernel.cu:313-359), with minor == 1 and planes below 2 GiB: up = down = 1 with 2..4 square taps (Blur), up = 2 / down = 1
 * and up = 1 / down = 2 with up to 4 x 4 taps (Upsample, Downsample), any pads incl. negative ones; the rest takes a one-thread-per-output gather. */
int maua_upfirdn2d_f32(const float* x, const float* k, float* y, int major, int in_h, int in_w, int minor,
                       int kh, int kw, int up_x, int up_y, int down_x, int down_y,
                       int pad_x0, int pad_x1, int pad_y0, int pad_y1, void* stream);
/* The plan alone: writes which kernel instance maua_upfirdn2d_f32 would launch for these 14 geometry integers (the same host function
 * picks it) and returns 0, or returns MAUA_EINVAL for exactly the geometries that call refuses (a negative major, a size, tap count or
 * factor below 1, a negative span on either axis, more than 2^31 - 1 tiles) and for a null or too short buf.  The text is the instance,
 * then for the tiled ones the workgroups per plane as columns x rows: "tile4.wx2 1x3" (fir_tile_kernel<4, 4, 2, false, 24>, taps 2 .. 4),
 * "up2.wx4 3x2" (fir_up2_kernel<4, 16>), "down2.wx1 1x1" (fir_down2_kernel<1, 8>), each with wx 1, 2 or 4; "generic" (fir_generic_kernel);
 * "none" for major == 0, which launches nothing.  Geometry only: no pointer of the op is looked at, no HIP call is made, nothing needs a
 * GPU.  (Additive: the ABI version is unchanged.) */
int maua_upfirdn2d_plan_instance(int major, int in_h, int in_w, int minor, int kh, int kw, int up_x, int up_y, int down_x, int down_y,
                                 int pad_x0, int pad_x1, int pad_y0, int pad_y1, char* buf, int buf_len);

/* The same op for half / double tensors — the reference dispatches half, float and double (upfirdn2d_kernel.cu:313-359,
 * fused_bias_act_kernel.cu:79).  Generic kernels (fp32 accumulation for half); the fp32 entries above are the tuned path.
 * major == 0 (an empty tensor) is a successful no-op in all three entries: 0 is returned and nothing is launched; a negative major
 * is MAUA_EINVAL. */
int maua_upfirdn2d_f16(const void* x, const void* k, void* y, int major, int in_h, int in_w, int minor, int kh, int kw, int up_x,
                       int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1, void* stream);
int maua_upfirdn2d_f64(const void* x, const void* k, void* y, int major, int in_h, int in_w, int minor, int kh, int kw, int up_x,
                       int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1, void* stream);

/* Replaces pybind `fused.fused_bias_act(input, bias, refer, act, grad, alpha, scale)` —
 * op/fused_bias_act.cpp:11-20, op/fused_bias_act_kernel.cu:18-98.  b == NULL or size_b == 0: no bias;
 * ref == NULL: no reference tensor.  bias index = (i / step_b) % size_b. In-place (y == x) is allowed. */
int maua_fused_bias_act_f32(const float* x, const float* b, const float* ref, float* y, int64_t size_x,
                            int size_b, int step_b, int act, int grad, float alpha, float scale, void* stream);

/* Half / double forms.  Half: arithmetic in fp32, and the last step — the multiply by `scale` and the rounding to half — is one
 * mixed-precision instruction, so the stored half is the exact product rounded once (not its fp32 rounding rounded again). */
int maua_fused_bias_act_f16(const void* x, const void* b, const void* ref, void* y, int64_t size_x, int size_b, int step_b,
                            int act, int grad, float alpha, float scale, void* stream);
int maua_fused_bias_act_f64(const void* x, const void* b, const void* ref, void* y, int64_t size_x, int size_b, int step_b,
                            int act, int grad, float alpha, float scale, void* stream);

/* ------------------------------------------------------------------------------------------------ frame source
 * Per-frame inputs of a generator forward, read THROUGH device memory instead of through kernel arguments, so that one
 * captured hipGraph serves every batch of a render (and every render): the sequences of render.py:140-182 — latents
 * [n_frames, n_latent, style_dim], truncation [n_frames], one noise map sequence per noise slot — stay resident in HBM and a
 * replay only moves `frame0` (maua_frame_source_seek: one 4-byte device write; the reference re-uploads every sequence slice
 * from pinned host memory per batch).  The struct lives in DEVICE memory; the host fills the pointers once per render.
 * Every launcher below that takes `src` ignores its own latents / trunc / noise / noise_batch_stride arguments when src != NULL:
 *   latent of sample b   = src->latents + (frame0 + b) * n_latent * style_dim
 *   truncation of b      = src->trunc[frame0 + b]            (src->trunc == NULL: no lerp)
 *   noise map of b       = src->noise[slot] + (frame0 + b) * src->noise_stride[slot]   (stride 0: one shared map, e.g. a
 *                          checkpoint's noises.noise_i buffer; src->noise[slot] == NULL: no noise) */
#define MAUA_MAX_NOISE_SLOTS 32
typedef struct {
    int32_t frame0;                               /* first frame of this launch inside every per-frame sequence */
    int32_t pad_;
    const float* latents;
    const float* trunc;
    const float* noise[MAUA_MAX_NOISE_SLOTS];
    int64_t noise_stride[MAUA_MAX_NOISE_SLOTS];   /* floats between the maps of consecutive frames */
} maua_frame_source_t;
/* src->frame0 = frame0, asynchronously on `stream` (a 4-byte hipMemsetD32Async: no host buffer has to outlive the call). */
int maua_frame_source_seek(maua_frame_source_t* src, int frame0, void* stream);

/* ------------------------------------------------------------------------------------------------ counter-based noise (ABI 7)
 * Seeded N(0,1) noise maps for `randomize_noise` (models/stylegan2.py:262-265, render.py:180), generated on the device: the map of
 * (seed, absolute frame f, slot s) is a pure function, so it is the same for every batch size, lane count and shard of a job, and it
 * can be produced per replay inside a captured forward instead of living in HBM as a [n_frames, 1, h, w] sequence.  Element e:
 *   x[0..3] = Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85) with
 *             key = (seed low word, seed high word) and counter = (e / 4, f, s, 0);
 *   u(x)    = ((x >> 9) + 0.5) * 2^-23      — 24 significant bits: exact in fp32, never 0 or 1, so |z| <= sqrt(48 ln 2) = 5.768;
 *   Box-Muller: element 4i = r cos(2 pi u(x[1])), 4i+1 = r sin(2 pi u(x[1])) with r = sqrt(-2 ln u(x[0])); 4i+2, 4i+3 the same from
 *             (x[2], x[3]).  A map whose hw is not a multiple of 4 drops the surplus values.
 * One launch fills the [batch, hw] maps of all `n_slots` table entries (the table lives in DEVICE memory; an entry with dst == NULL or
 * hw < 1 is skipped); frame of sample b:
 *   src == NULL: frame0 + b;
 *   src != NULL: frame0 + src->frame0 + b, read on the device, so that one captured launch serves every replay.  `frame0` is then the
 *             absolute frame at which the sequences behind `src` start: 0, unless the caller holds one shard of a job's frames.
 *             The same launch points the frame source at the generated maps, for every entry with slot in 0 .. MAUA_MAX_NOISE_SLOTS-1:
 *               src->noise[slot] = dst - src->frame0 * hw,  src->noise_stride[slot] = hw
 *             (the layers, later on the same stream, read noise[slot] + (src->frame0 + b) * noise_stride[slot] = dst + b * hw; the
 *             biased pointer itself is never dereferenced).
 * MAUA_EINVAL: table == NULL, n_slots outside 1 .. MAUA_MAX_NOISE_SLOTS, batch < 1, frame0 < 0. */
typedef struct {
    float* dst;     /* [batch, hw] */
    int32_t hw;     /* floats per map */
    int32_t slot;   /* third counter word; with src also the noise slot of the frame source */
} maua_randn_slot_t;
int maua_randn_frames_f32(const maua_randn_slot_t* table, int n_slots, int batch, uint64_t seed, int frame0, maua_frame_source_t* src,
                          void* stream);

/* Synthesised noise slots (additive to ABI 8; audioreactive/noise.py NoiseSynth, csrc/noise_synth.hip).  What an audio-reactive plugin does
 * with noise — blending short loops by envelopes, gating fields by a static mask — is a sum of at most MAUA_NOISE_SYNTH_MAX_TERMS terms, so
 * the maps of a slot are produced per launch from a recipe instead of living in HBM as a [n_frames, 1, h, w] sequence (36 GB for one 1024^2
 * slot of a 9000-frame track; a 110-frame loop is 0.45 GB).  The table lives in DEVICE memory and is read by every launch, the seed included:
 * a captured launch is re-bound to another render by rewriting the table, and only `frame0` is a kernel argument.
 * Frames: local frame of sample b  f = b (src == NULL) or src->frame0 + b (read on the device); absolute frame  F = frame0 + f, `frame0`
 * being the absolute frame at which the bound sequences (the envelopes) start, as for maua_randn_frames_f32.  For every entry with
 * n_terms >= 1, dst != NULL and hw >= 1 (others are skipped), sample b and element e:
 *   dst[b * hw + e] = gain * sum_{k < n_terms} envelope_k[f] * mask_k[e] * v_k
 *   v_k = bank_k[((F + phase_k) mod period_k) * hw + e]                                      for a bank term,
 *       = the counter-based N(0,1) value of (seed, F, slot, e) exactly as maua_randn_frames_f32 defines it   for the NULL-bank term (at most one).
 * In fp32, in term order: acc = 0; acc = fma(round(envelope_k * mask_k), v_k, acc); then round(gain * acc) — the same bits whatever the
 * batch, the access width or the launch.  16-byte loads and stores for the samples whose dst, bank rows and masks are all 16-byte aligned
 * (hw % 4 != 0 makes every odd sample unaligned), element by element otherwise.  n_terms above the maximum is clamped; the per-entry values
 * (periods, phases, envelope lengths >= the frames used) are the caller's to validate: the device only keeps a period below 1 from dividing.
 * With src the launch points the frame source at the maps as maua_randn_frames_f32 does:
 *   src->noise[slot] = dst - src->frame0 * hw,  src->noise_stride[slot] = hw        (slot in 0 .. MAUA_MAX_NOISE_SLOTS-1, entry not skipped).
 * MAUA_EINVAL, before any HIP call: table == NULL, n_slots outside 1 .. MAUA_MAX_NOISE_SLOTS, batch < 1, frame0 < 0. */
#define MAUA_NOISE_SYNTH_MAX_TERMS 4
typedef struct {
    const float* bank;      /* [period, hw] loop; NULL: the counter-based N(0,1) map of (seed, absolute frame, slot) */
    const float* envelope;  /* [n_frames of the bound sequences] or NULL (= 1) */
    const float* mask;      /* [hw] or NULL (= 1) */
    int32_t period;         /* >= 1 when bank != NULL */
    int32_t phase;          /* 0 .. period-1 */
} maua_noise_term_t;
typedef struct {
    float* dst;             /* [batch, hw] */
    int32_t hw;             /* floats per map */
    int32_t slot;           /* third counter word of the NULL-bank term; with src also the noise slot of the frame source */
    int32_t n_terms;        /* 0: entry skipped */
    float gain;
    uint64_t seed;          /* of the NULL-bank term */
    maua_noise_term_t term[MAUA_NOISE_SYNTH_MAX_TERMS];
} maua_noise_synth_slot_t;
int maua_noise_synth_f32(const maua_noise_synth_slot_t* table, int n_slots, int batch, int frame0, maua_frame_source_t* src, void* stream);

/* ------------------------------------------------------------------------------------------------ generator layers
 * THE STYLE FOLD (ABI 4).  ModulatedConv2d multiplies its input by the per-sample styles before the shared-weight contraction
 * (models/stylegan2.py:220-221, w = scale * W * s  <=>  conv(scale * W, x * s)).  Every feature map of the generator has exactly one
 * modulated 3x3 convolution as consumer (its ToRGB is computed in the producer's epilogue from the un-scaled value), so the multiply can
 * move into the PRODUCER's epilogue — once per element instead of once per element AND output-channel tile of the consumer's K loop:
 *   producers (maua_blur_noise_act_f32, maua_upconv_blur_f32, maua_styledconv_torgb_f32 and _partial_f32 in mode 5) take `post_s`
 *     = the CONSUMER's styles [B, stride] indexed by the producer's output channel, NULL = store the map as it is:
 *       y_stored[b,o] = y[b,o] * post_s[b * stride + o];
 *   consumers (maua_modconv3x3_f32 with up == 5 or 6, maua_upconv_blur_f32, the two ToRGB-fused entries in mode 5) accept s == NULL
 *     = "x arrives multiplied by my styles": kernel instances without the style multiplies in their K loop (4 of 16 transform
 *     instructions per window of the 2-D Winograd kernel, 9 of 23 per K step of the F(2,2)^2 transposed kernel).  d (demodulation)
 *     is unaffected: it is computed from the styles by maua_demod_f32 either way.
 * MAUA_ENOSYS for s == NULL / post_s != NULL in the other modes.  The caller keeps the un-folded form wherever something else reads
 * the feature map (a network bend on that layer id, return_activation_maps).
 *
 * Fused Blur -> NoiseInjection -> FusedLeakyReLU tail of an up-sampling StyledConv
 * (models/stylegan2.py:238,262-266,338-343; op/fused_act.py:74-83):
 *   y[b,c] = lrelu_0.2( upfirdn2d(x[b,c], k, pad=(pad0,pad1)) * gain[b,c] + noise_w * noise[b,0] + bias[c] ) * sqrt(2)
 * x [B,C,in_h,in_w] -> y [B,C,out_h,out_w], up = down = 1. gain (may be NULL = 1) carries the demodulation
 * factor of the preceding shared-weight convolution. noise [B or 1,1,out_h,out_w] (noise_batch_stride 0 = broadcast).
 * Limits (the kernel addresses a plane through 32-bit buffer offsets): kh == kw in 2..4, and planes below 2 GiB — MAUA_ENOSYS otherwise
 * (there is no generic fallback behind this entry: run maua_upfirdn2d_f32, which has one, and maua_fused_bias_act_f32 instead).  The noise
 * map is read as exactly out_h * out_w floats per sample from noise + b * noise_batch_stride: the CALLER guarantees that shape (the Python
 * mirror checks it against the feature map, models/stylegan2.py StyledConv.run; the reference raises a broadcast error there). */
int maua_blur_noise_act_f32(const float* x, const float* k, float* y, int batch, int channels, int in_h, int in_w,
                            int kh, int kw, int pad0, int pad1, const float* gain, const float* noise,
                            int64_t noise_batch_stride, const float* noise_w, const float* bias,
                            const maua_frame_source_t* src, int noise_slot, const float* post_s, int post_stride, void* stream);

/* The WHOLE up-sampling StyledConv in one pass (round 5): transposed 3x3 modulated convolution (stride 2) -> Blur (4x4 SEPARABLE taps, pad
 * (1, 1)) -> NoiseInjection -> FusedLeakyReLU — models/stylegan2.py:229-238,262-266,338-343 — without the raw (2H+1) x (2W+1) map that
 * maua_modconv3x3_f32 (mode 6) writes and maua_blur_noise_act_f32 reads back (548 MB per 1024^2 frame each way):
 *   y[b,o] = lrelu_0.2( blur( conv_transpose2d(x[b] * s[b], W)[o] ) * wscale * d[b,o] + noise_w * noise[b,0] + bias[o] ) * sqrt(2),  y [B,Cout,2H,2W].
 * The blur runs on the accumulators of csrc/modconv_up2d.hip (F(2,2) on both axes of the polyphase form): horizontal pass across the lanes
 * of a wave, vertical pass across the waves of a workgroup through LDS; a workgroup walks a vertical segment of tiles and keeps the three
 * halo rows in LDS; the rows either side of a segment boundary go through `ws` to a small second launch.  `wq` = maua_pack_weight_up2d_f32.
 * `k4`: the [4][4] tap matrix in DEVICE memory; it MUST be separable (outer product, as make_kernel([1,3,3,1]) is) — the caller checks.
 * `ws`: maua_upconv_blur_ws_floats(...) floats.  Shapes: maua_upconv_blur_ok (cin % 8 == 0, cin <= 256, cout % 32 == 0, h % 8 == 0,
 * w % 32 == 0); MAUA_ENOSYS otherwise (the two-launch path serves every shape). */
int maua_upconv_blur_ok(int cin, int cout, int h, int w);
int64_t maua_upconv_blur_ws_floats(int batch, int cin, int cout, int h, int w);
int maua_upconv_blur_f32(const float* x, const float* wq, const float* s, int s_stride, const float* d, float* y, float* ws,
                         const float* k4, const float* noise, int64_t noise_batch_stride, const float* noise_w, const float* bias,
                         const maua_frame_source_t* src, int noise_slot, int batch, int cin, int cout, int h, int w, float wscale,
                         const float* post_s /* [B, s_stride] or NULL */, void* stream);

/* All style affines and demodulation factors of one forward, two launches in total, table-driven.
 *  affine (EqualLinear, models/stylegan2.py:140-146,207,220), with the truncation lerp of Generator.forward
 *  (:541-543) applied to the latent first when trunc != NULL (latent' = trunc_latent + trunc[b]*(latent - trunc_latent)):
 *      s[b*s_stride + s_off_l + i] = (1/sqrt(style_dim)) * sum_j mod_w_l[i,j] * latent'[b, lat_idx_l, j] + mod_b_l[i]
 *  demod (:223-225) in the shared-weight formulation, for layers with wsq != NULL:
 *      d[d_off_l + b*cout_l + o] = rsqrt( wscale_l^2 * sum_i wsq_l[o,i] * s[b, s_off_l + i]^2 + 1e-8 )
 *  `table` lives in DEVICE memory (n_layers entries).  Any batch >= 1: both kernels walk the frames 16 at a time.
 *  trunc != NULL with trunc_latent == NULL: the lerp runs against a zero mean latent, latent' = trunc[b] * latent.  With src the
 *  latents / trunc arguments are ignored (frame source above); trunc_latent still comes from the argument.
 *  Limits.  style_dim: a multiple of 64, at most 1024 (MAUA_EINVAL otherwise).  An entry's cin is unlimited for the affine, but an
 *  entry with wsq != NULL needs cin <= 1024: the demod kernel keeps [16][cin] squared styles in 64 KB of LDS and 16 values per lane.
 *  The launcher cannot see the table, so that limit is the CALLER's to enforce where the table is built (models/stylegan2.py
 *  _style_table raises); a wider entry would write past the LDS and drop terms.  max_cin / max_cout >= every entry's cin / cout
 *  (they size the grid; rows beyond them are not computed).
 *  MAUA_EINVAL: latents and src both NULL, table / s / d NULL, batch, n_layers, max_cin or max_cout < 1. */
typedef struct {
    const float* mod_w; /* [cin, style_dim] */
    const float* mod_b; /* [cin] */
    const float* wsq;   /* [cout, cin] sum over taps of W^2 (maua_pack_weight_f32), NULL = no demodulation */
    int cin;
    int cout;
    int lat_idx;        /* which of the n_latent rows feeds this layer */
    int s_off;          /* offset of this layer's slice inside one batch row of s */
    int64_t d_off;      /* offset of this layer's [batch, cout] block inside d */
    float wscale;       /* 1/sqrt(cin * k * k) */
    int pad_;
} maua_style_layer_t;
int maua_style_affine_f32(const float* latents, int batch, int n_latent, int style_dim, const float* trunc,
                          const float* trunc_latent, const maua_style_layer_t* table, int n_layers, int max_cin,
                          float* s, int s_stride, const maua_frame_source_t* src, void* stream);
int maua_demod_f32(const maua_style_layer_t* table, int n_layers, int max_cout, const float* s, int s_stride, float* d,
                   int batch, void* stream);

/* Sum of squared taps wsq[o,i] and the tap-major repack wp[tap][i][o] of a [cout,cin,k,k] weight (one-off, at load). */
int maua_pack_weight_f32(const float* w, float* wp, float* wsq, int cout, int cin, int ktaps, void* stream);

/* Winograd F(2,3) form of the same weight, transformed along kx: wq[(ky*4+xi)][i][o_pad] (o_pad = cout padded to 32;
 * above 32 channels padded to 64 with the columns of every 64-group interleaved [o % 32][o / 32 % 2], both here and in the
 * F(4,3) pack) with
 * xi 0: g0, 1: (g0+g1+g2)/2, 2: (g0-g1+g2)/2, 3: g2.  The operand of maua_modconv3x3_f32 in mode 2. */
int maua_pack_weight_wino_f32(const float* w, float* wq, int cout, int cin, void* stream);
/* Winograd F(4,3) form (interpolation points 0, +-1, +-2, inf): wq[(ky*6+xi)][i][o_pad] with xi 0: g0/4,
 * 1: -(g0+g1+g2)/6, 2: -(g0-g1+g2)/6, 3: (g0+2g1+4g2)/24, 4: (g0-2g1+4g2)/24, 5: g2.  Operand of mode 3. */
int maua_pack_weight_wino43_f32(const float* w, float* wq, int cout, int cin, void* stream);
/* Transposed-conv form for mode 4 (F(2,2) on the even x-phase of the polyphase decomposition):
 * wq[(ky*4+j)][i][o_pad] with j 0: g2, 1: g0+g2, 2: g0, 3: g1. */
int maua_pack_weight_upwino_f32(const float* w, float* wq, int cout, int cin, void* stream);

/* Transposed-conv form for mode 6 (F(2,2) on BOTH axes of the polyphase decomposition: 25 instead of 36 products per 2x2 block of
 * positions): 16 transformed-kernel entries per (cout, cin) pair — 9 (even, even) + 3 (even row, odd column) + 3 (odd row, even
 * column) + the centre tap, one axis transforming as (tap 2, tap 0 + tap 2, tap 0) — stored as the LDS tile images
 * wq[cout/32][cin/4][16][cin%4][32 columns], followed by the five [cin][cout] tap matrices of the kernel's last row / column that
 * the edge lines (output row 2H, column 2W) use.  maua_pack_weight_up2d_floats() floats.  maua_modconv_up2d_ok(): cin % 4 == 0,
 * cout % 32 == 0, h % 8 == 0, w % 32 == 0. */
int64_t maua_pack_weight_up2d_floats(int cout, int cin);
int maua_pack_weight_up2d_f32(const float* w, float* wq, int cout, int cin, void* stream);
int maua_modconv_up2d_ok(int cin, int cout, int h, int w);
/* SIDE MEASUREMENT (off by default, never the headline): packed weight of the split-bf16 plain convolution (up == 7 below) — every
 * fp32 weight as two bf16 terms w_h + w_l in MFMA lane order, maua_pack_weight_sbf16_bytes() bytes.  maua_modconv_sbf16_ok():
 * cin % 16 == 0, cout % 128 == 0, h % 8 == 0, w % 32 == 0. */
int64_t maua_pack_weight_sbf16_bytes(int cout, int cin);
int maua_pack_weight_sbf16_f32(const float* w, void* wq, int cout, int cin, void* stream);
int maua_modconv_sbf16_ok(int cin, int cout, int h, int w);
int maua_modconv_sbf16_up_ok(int cin, int cout, int h, int w);  /* the transposed form (up == 8): cout % 32 == 0 instead of % 128 */

/* 2-D Winograd F(2x4, 3x3) form for mode 5 (F(2,3) along ky on top of F(4,3) along kx: 24 values per (cout, cin) pair),
 * stored as the LDS tile image the kernel DMAs linearly: wq[cout/BM][cin/4][fy 4][xf 6][cin%4][BM columns] (BM = 64, or 32 for
 * a 32-channel layer; m-tile pairs interleaved inside a row).  Needs 24*cin*cout floats.  maua_modconv_w2d_ok() says whether a
 * layer shape qualifies (cin % 4 == 0, cout == 32 or cout % 64 == 0, w % 32 == 0, h % 8 (16 for cout 32) == 0). */
int maua_pack_weight_wino2d_f32(const float* w, float* wq, int cout, int cin, void* stream);
int maua_modconv_w2d_ok(int cin, int cout, int h, int w);
/* number of output-channel tiles (workgroups per pixel tile) the 2-D Winograd kernel uses for this layer; 0 = shape not accepted */
int maua_modconv_w2d_mtiles(int cin, int cout, int h, int w);

/* ModulatedConv2d 3x3 (models/stylegan2.py:217-254) as input-scale -> shared-weight implicit GEMM on MFMA ->
 * output-demod, with the StyledConv tail (noise + bias + leaky ReLU, :338-343) fused when `fuse_act`:
 *   plain   : x[B,cin,H,W] -> y[B,cout,H,W]        (pad 1)
 *   up == 1 : x[B,cin,H,W] -> y[B,cout,2H+1,2W+1]  (conv_transpose2d stride 2, :229-237) — raw, un-demodulated
 *             when fuse_act == 0 (the blur kernel applies gain/noise/bias/act).
 *   up == 2 : the plain convolution evaluated through Winograd F(2,3) along x (W even): 1.5x fewer MFMA cycles,
 *             same result to fp32 rounding; wp is then the maua_pack_weight_wino_f32 weight.
 *   up == 4 : the transposed convolution of up == 1 with F(2,2) on its even x-phase (W even, fuse_act == 0): 5 instead
 *             of 6 MFMA K-steps per position pair and kernel row; wp from maua_pack_weight_upwino_f32.
 *   up == 3 : the same through Winograd F(4,3) (W % 4 == 0): 2x fewer MFMA cycles than direct, |error| ~2e-5 of
 *             the output scale; wp from maua_pack_weight_wino43_f32.
 *   up == 6 : the transposed convolution of up == 1 with F(2,2) on both axes (shapes accepted by maua_modconv_up2d_ok, fuse_act == 0):
 *             25/36 of the MFMA cycles of up == 1; wp from maua_pack_weight_up2d_f32.
 *   up == 5 : the plain convolution through 2-D Winograd F(2x4, 3x3) (shapes accepted by maua_modconv_w2d_ok): 3x fewer
 *             MFMA cycles than direct, 1.5x fewer than up == 3; wp from maua_pack_weight_wino2d_f32.
 *   up == 7 : SIDE MEASUREMENT — the plain convolution in its direct 9-tap form with split-bf16 products on the bf16 matrix cores
 *             (a b ~= a_h b_h + a_h b_l + a_l b_h, fp32 accumulation; relative error of a product <= 2^-16 + 2^-17); wp from
 *             maua_pack_weight_sbf16_f32.  Not used unless the caller asks for it; the default path computes in fp32.
 *   up == 8 : SIDE MEASUREMENT — the transposed convolution of up == 1 with split-bf16 products (four polyphase phase launches of the
 *             up == 7 kernel + fp32 edge lines), same packed weight as up == 7, fuse_act == 0, ws as for up == 6.
 * wp = tap-major packed weight from maua_pack_weight_f32; s = per-sample input scales [B, s_stride] (NULL with up == 5 / 6: x arrives
 * pre-scaled, see THE STYLE FOLD above);
 * d = demod [B,cout] (NULL = 1).  `ws` is a caller-owned fp32 workspace of at least maua_modconv_ws_floats()
 * floats used for split-K partial sums on small feature maps and, for up == 6, for the exported last input column [B, cin, H]
 * (may be NULL when that returns 0).
 * MAUA_EINVAL besides null / non-positive arguments and the width rules above: a map whose staged patch fits no tile of the mode —
 * up == 3 with W == 4, or with H <= 4 and W >= 20 (run up == 2 or 0 there); up == 4 where the (H+1) x (W/2+1) grid of position pairs
 * is a single run (at most 128 pairs up to 32 output channels, 64 above: run up == 1).  Nothing is launched.  ModulatedConv2d.conv_mode
 * never picks these; the low-resolution entries below pass the code on. */
int64_t maua_modconv_ws_floats(int batch, int cin, int cout, int h, int w, int up);
/* Name of the kernel template instance launched by the last modconv call of this process, as rocprofv3 prints it
 * ("modconv_mfma_kernel<BM, BN, WM, MODE, MULTI, FAST, MAXP>") — the key of the per-instance PMC tables in profiles/. */
int maua_modconv_last_instance(char* buf, int buf_len);
/* The plan alone, for up == 0 .. 4: writes the name of the instance maua_modconv3x3_f32 would launch for this shape (the same host
 * function picks it) and returns 0, or returns the code with which that call refuses the shape (MAUA_EINVAL: the width rules, more than
 * 2^31 - 1 input elements, a patch that fits no tile of the mode; any other up is MAUA_EINVAL here).  Shapes only: no pointer is looked
 * at, no HIP call is made, nothing needs a GPU.  The name does not depend on batch.  (Additive: the ABI version is unchanged.) */
int maua_modconv_plan_instance(int batch, int cin, int cout, int h, int w, int up, char* buf, int buf_len);
int maua_modconv3x3_f32(const float* x, const float* wp, const float* s, int s_stride, const float* d,
                        float* y, int batch, int cin, int cout, int h, int w, int up, float wscale, int fuse_act,
                        const float* noise, int64_t noise_batch_stride, const float* noise_w, const float* bias,
                        float* ws, const maua_frame_source_t* src, int noise_slot, void* stream);

/* Plain StyledConv with the following ToRGB (models/stylegan2.py:338-343 then :356-365) fused into its epilogue: the
 * activated feature map is reduced to RGB while it is still in registers (all channels of a pixel sit in one wave).
 * Only for layers whose channels fit one weight tile in a single wave row (cout <= 64); returns MAUA_ENOSYS otherwise
 * (the caller then runs maua_modconv3x3_f32 + maua_torgb_f32).  rgb_s = the ToRGB layer's styles [B, s_stride] (same
 * stride as s).  frames_u8 != NULL (last layer): the image is not written as fp32 planes at all but leaves as uint8 NHWC frames
 * [B,H,W,3] = clamp(-1,1), (x+1)*127.5, truncating cast (the frame epilogue of render.py:40-43 folded in); rgb_out may then be NULL
 * (the normal case) — when it is not, the fp32 planes are written as well (the parity tests compare them with the oracle in float).
 * mode = 0 (direct), 2, 3 or 5 (Winograd F(2,3) / F(4,3) / 2-D F(2x4,3x3), wp from the matching pack function).  store_features = 0 skips writing y (legal for the last layer: nothing downstream reads it). */
int maua_styledconv_torgb_f32(const float* x, const float* wp, const float* s, int s_stride, const float* d,
                              float* y, int batch, int cin, int cout, int h, int w, int mode, float wscale,
                              const float* noise, int64_t noise_batch_stride, const float* noise_w, const float* bias,
                              const float* rgb_w, const float* rgb_s, float rgb_wscale, const float* rgb_bias,
                              const float* rgb_skip, const float* rgb_k4, float* rgb_out, int store_features,
                              uint8_t* frames_u8, const maua_frame_source_t* src, int noise_slot,
                              const float* post_s /* [B, s_stride] or NULL; mode 5 only */, void* stream);

/* LOW-RESOLUTION LAYERS (ABI 5; the 4^2 .. 32^2 outputs of a generator).  Their convolutions are the split-K direct / polyphase kernels of
 * maua_modconv3x3_f32 (up = 0 / 1), and on maps of a few KB every launch is a fixed 5 .. 20 us whatever it computes.  These entries run the
 * convolution with its split-K slabs left in `ws` (maua_lowres_ws_floats floats: one slab when K is not split) and reduce them in the SAME
 * launch that applies what follows:
 *   maua_upconv_blur_lowres_f32   = maua_modconv3x3_f32(up = 1) + maua_blur_noise_act_f32 (4 x 4 taps, pad (1, 1)) of an up-sampling
 *       StyledConv (models/stylegan2.py:229-238, :338-343): y [B, Cout, 2H, 2W], bit-identical to that pair wherever K is split (without a
 *       split the pair applies wscale * d as one factor, this entry as two);  post_s as THE STYLE FOLD;
 *   maua_styledconv_rgbpart_lowres_f32 = maua_modconv3x3_f32(up = 0, fuse_act = 1) of a plain StyledConv — y bit-identical — that also
 *       leaves per-32-channel-group partial ToRGB sums (models/stylegan2.py:356-365) in rgb_partial [B, 3 * Cout / 32, H, W] (plane 3 g + c),
 *       which maua_torgb_f32's plane-sum form (w = s = NULL) turns into the image.
 * `up` of the up-sampling entry picks the convolution: 1 = the polyphase kernel (wp = maua_pack_weight_f32), 6 = F(2,2) on both axes of the
 * polyphase form (csrc/modconv_up2d.hip on 16 x 16-position tiles, K split over workgroups; wp = maua_pack_weight_up2d_f32): 16-wide
 * inputs, 25 instead of 36 products per 2 x 2 positions and that kernel's operand pipeline (the 16^2 -> 32^2 layer at batch 8: 129 -> 77 us).
 * maua_lowres_ok: up == 1: 2H * 2W <= 1024;  up == 6: W == 16, H % 16 == 0, Cin % 8 == 0, Cout % 32 == 0, 2H * 2W <= 1024;
 * up == 0 / 2 / 3 (the plain entry's `mode`: direct, Winograd F(2,3) / F(4,3) along x — 2 needs an even W, 3 W % 4 == 0): Cout % 32 == 0,
 * H * W % 16 == 0, H * W <= 1024.  MAUA_ENOSYS otherwise.  `wp` of the plain entry = the pack of its mode (maua_pack_weight_f32 /
 * maua_pack_weight_wino_f32 / maua_pack_weight_wino43_f32); s must not be NULL (no pre-scaled instances here). */
int maua_lowres_ok(int cin, int cout, int h, int w, int up);
int64_t maua_lowres_ws_floats(int batch, int cin, int cout, int h, int w, int up);
int maua_upconv_blur_lowres_f32(const float* x, const float* wp, const float* s, int s_stride, const float* d, float* y, float* ws,
                                const float* k4, const float* noise, int64_t noise_batch_stride, const float* noise_w, const float* bias,
                                const maua_frame_source_t* src, int noise_slot, int batch, int cin, int cout, int h, int w, int up,
                                float wscale, const float* post_s, void* stream);
int maua_styledconv_rgbpart_lowres_f32(const float* x, const float* wp, const float* s, int s_stride, const float* d, float* y, float* ws,
                                       const float* noise, int64_t noise_batch_stride, const float* noise_w, const float* bias,
                                       const float* rgb_w, const float* rgb_s, float rgb_wscale, float* rgb_partial,
                                       const maua_frame_source_t* src, int noise_slot, int batch, int cin, int cout, int h, int w,
                                       int mode, float wscale, void* stream);

/* conv1 on a ConstantInput (models/stylegan2.py:269-278, :547-549; csrc/constconv.hip).  The input of a generator's first StyledConv is
 * the learned 4 x 4 constant, the same for every frame and scaled per (frame, channel) by the styles, so
 *   y[b,o,p] = act( (wscale * sum_i T[o,p,i] s[b,i]) * d[b,o] + noise_w * noise[b,p] + bias[o] ),  T[o,p,i] = sum_taps W[o,i,ky,kx] c[i, p + (ky,kx) - 1]
 * with T a function of the checkpoint alone: maua_pack_const_conv_f32 (w [Cout,Cin,3,3], c [Cin,4,4] -> T, Cout * 16 * Cin floats, once per
 * weight version), then maua_const_styledconv_f32 per batch — 1/9 of the convolution's multiply-adds, one read of T, no split-K.
 * rgb_partial != NULL: per-32-channel-group partial ToRGB sums [B, 3 * Cout / 32, 4, 4] as maua_styledconv_rgbpart_lowres_f32 leaves them.
 * maua_const_conv_ok: h == w == 4, Cin % 8 == 0, Cout % 32 == 0 (Cin <= 1536: the styles of eight frames in LDS); MAUA_ENOSYS otherwise. */
int maua_const_conv_ok(int cin, int cout, int h, int w);
int maua_pack_const_conv_f32(const float* w, const float* c, float* T, int cout, int cin, int h, int wd, void* stream);
int maua_const_styledconv_f32(const float* T, const float* s, int s_stride, const float* d, float* y, const float* noise,
                              int64_t noise_batch_stride, const float* noise_w, const float* bias, const float* rgb_w, const float* rgb_s,
                              float rgb_wscale, float* rgb_partial, const maua_frame_source_t* src, int noise_slot, int batch, int cin,
                              int cout, int h, int w, float wscale, void* stream);

/* The same fusion for layers wider than one weight tile (128..512 output channels, mode 5 only): every output-channel tile leaves
 * its share of the ToRGB sum  sum_{i in tile} (rgb_wscale * rgb_w[c,i] * rgb_s[b,i]) * y[b,i,Y,X]  in
 * rgb_partial [B, 3 * maua_modconv_w2d_mtiles(), H, W] (plane 3 m + c), the feature map y is stored as usual.  The caller finishes with
 * maua_torgb_f32 over the 3 m_tiles planes (w = s = NULL: its plane-sum form), which adds bias and the up-sampled skip: the ToRGB of
 * models/stylegan2.py:356-365 then reads 3 m_tiles planes instead of all `cout` feature planes.  MAUA_ENOSYS for mode != 5. */
int maua_styledconv_torgb_partial_f32(const float* x, const float* wp, const float* s, int s_stride, const float* d, float* y,
                                      int batch, int cin, int cout, int h, int w, int mode, float wscale, const float* noise,
                                      int64_t noise_batch_stride, const float* noise_w, const float* bias, const float* rgb_w,
                                      const float* rgb_s, float rgb_wscale, float* rgb_partial,
                                      const maua_frame_source_t* src, int noise_slot, const float* post_s /* [B, s_stride] or NULL */,
                                      void* stream);

/* StyleGAN1 (`--stylegan1`, models/stylegan1.py:258-318 LayerEpilogue) — conv bias, per-channel-weighted noise, LeakyReLU(0.2),
 * instance norm (biased variance, eps 1e-5) and the style modulation in one launch:
 *   y[b,c] = norm( lrelu_0.2( x[b,c] + bias[c] + noise_w[c] * noise[b or 0] ) ) * (style[b, c] + 1) + style[b, C + c]
 * bias / noise / style may be NULL (skipped); instance_norm = 0 skips the normalisation; y == x is allowed. */
int maua_sg1_epilogue_f32(const float* x, const float* bias, const float* noise, int64_t noise_batch_stride,
                          const float* noise_w, const float* style, int style_stride, float* y, int batch, int channels,
                          int h, int w, int instance_norm, void* stream);

/* ToRGB (models/stylegan2.py:356-365): 1x1 modulated conv without demod + bias + 2x FIR-upsampled skip
 * (Upsample :34-52, kernel k4 = 4x4 taps in device memory, pad (2,1)).  skip == NULL: no skip.
 *   y[b,c,Y,X] = sum_i (wscale * w[c,i] * s[b,i]) * x[b,i,Y,X] + bias[c] + up2(skip)[b,c,Y,X]
 * w == NULL and s == NULL: x holds per-tile partial ToRGB sums [B, cin = 3 M, H, W] (maua_styledconv_torgb_partial_f32), plane 3 m + c
 * feeding colour c:  y[b,c] = sum_m x[b, 3 m + c] + bias[c] + up2(skip)[b,c]  (wdt % 4 == 0; one round trip of independent loads).
 * s is read as s[b * s_stride + i], s_stride >= cin (a window of a wider styles table).  A skip needs k4 and even h and wdt.
 * Limit of the general form (w != NULL): the three modulated weight rows (3 cin floats, padded to a multiple of 4) and, when the channel
 * loop is split into slices, 3072 floats of partial sums live in dynamic LDS, which must not exceed 64 KB.  The loop is split whenever
 * the grid would otherwise have fewer than 512 workgroups of 256 pixel groups, so cin <= 4437 is served at every shape and cin <= 5461
 * on maps large enough to run unsplit; MAUA_ENOSYS beyond that, before any launch. */
int maua_torgb_f32(const float* x, const float* w, const float* s, int s_stride, const float* bias,
                   const float* skip, const float* k4, float* y, int batch, int cin, int h, int wdt,
                   float wscale, void* stream);

/* Frame epilogue of render.py:40-43: [B,3,H,W] fp32 -> [B,H,W,3] uint8 via clamp(-1,1), (x+1)*127.5, truncation — bit for bit the fp32
 * statement ((clip(x, -1, 1) + 1) * 127.5).astype(uint8).  A NaN becomes 0: the clamp is fminf(fmaxf(x, -1), 1) and fmaxf returns its
 * other operand for a NaN, hence -1 (numpy's clip would propagate it).  -inf gives 0, +inf 255.  The fused epilogues of the last layer
 * share this quantiser. */
int maua_frames_to_u8(const float* img, uint8_t* out, int batch, int h, int w, void* stream);
/* Wide-output delivery of render.py:97-104 on the device: crop [y0, y0+crop_h) x [x0, x0+crop_w) of uint8 NHWC frames
 * in[B,in_h,in_w,3] and resize to out[B,out_h,out_w,3] as PIL's Image.resize(BILINEAR) does for an up-scale (2-tap triangle filter at
 * (dst + 0.5) * in/out - 0.5, clamped taps, horizontal pass rounded to 8 bits, then vertical).  MAUA_ENOSYS for a down-scale. */
int maua_crop_resize_u8(const uint8_t* in, uint8_t* out, int batch, int in_h, int in_w, int x0, int y0, int crop_w, int crop_h,
                        int out_w, int out_h, void* stream);
/* Packed uint8 frames rgb[B,h,w,3] (what the two entries above produce) -> planar YUV 4:2:0 out[B, h*w*3/2]: per frame the Y plane
 * [h, w], then U [h/2, w/2], then V [h/2, w/2] (I420, ffmpeg's rawvideo yuv420p).  ITU-R BT.601 limited range in integer arithmetic
 * (the formula is in csrc/yuv420.hip), chroma from the box average of each 2 x 2 block (centre siting).  h and w even and positive
 * (MAUA_EINVAL otherwise); batch == 0 is a successful no-op, more than 65535 frames a launch are MAUA_ENOSYS.  Any even width and any
 * alignment is served; w % 8 == 0 with 8-byte aligned buffers takes the vector path.  (Additive: the ABI version is unchanged.) */
int maua_rgb_to_yuv420p_u8(const uint8_t* rgb, uint8_t* out, int batch, int h, int w, void* stream);
/* Packed uint8 frames rgb[B,h,w,3] -> one baseline JPEG per frame (4:2:0, the standard Huffman tables, restart intervals of restart_mcus
 * 16 x 16 MCUs; the stream is defined in integers in csrc/jpeg.hip and the device reproduces that definition byte for byte).  1 <= h, w
 * <= 65535, quality in 1 .. 95, restart_mcus in 1 .. 65535: MAUA_EINVAL otherwise.  (Additive: the ABI version is unchanged.)
 *   maua_jpeg_header    host only, no HIP call: writes the bytes from SOI up to and including the SOS header (they depend on h, w, quality
 *                       and restart_mcus only) to h_buf[cap] and returns their count; MAUA_EINVAL for bad arguments or a cap too small.
 *   maua_jpeg_ws_bytes  size of the workspace of maua_jpeg_encode_u8: zig-zag int16 coefficients [B][MCU][6][64], one worst-case segment
 *                       per restart interval (2496 bytes per MCU + 16) and the intervals' lengths; a pure function of its arguments, 0
 *                       for arguments outside the ranges above.
 *   maua_jpeg_encode_u8 three launches on `stream` (colour + DCT + quantiser; entropy coding, a workgroup per restart interval; packing),
 *                       no allocation, no synchronisation.  `header`: a DEVICE copy of maua_jpeg_header's bytes for the same h, w, quality
 *                       and restart_mcus.  out[B, slot_bytes], per frame: bytes 0..3 the stream's length n (little-endian), bytes 4..7 the
 *                       status (0 ok, 1 overflow), bytes 8..15 zero, the stream from byte 16; the slot's bytes behind 16 + n are not
 *                       written.  Overflow (16 + n > slot_bytes): status 1, n is the length the stream would have had, nothing but the 16
 *                       bytes is written, the other frames of the batch are unaffected.  MAUA_EINVAL (before any HIP call) for a NULL
 *                       pointer, slot_bytes < 16 + header_len + 2 or a ws that is not 16-byte aligned; batch == 0 is a successful no-op,
 *                       more than 65535 frames a launch are MAUA_ENOSYS.  rgb and out may have any alignment. */
int maua_jpeg_header(int h, int w, int quality, int restart_mcus, uint8_t* h_buf, int cap);
int64_t maua_jpeg_ws_bytes(int batch, int h, int w, int restart_mcus);
int maua_jpeg_encode_u8(const uint8_t* rgb, int batch, int h, int w, int quality, int restart_mcus, const uint8_t* header, int header_len,
                        uint8_t* out, int64_t slot_bytes, void* ws, void* stream);
/* Temporal supersampling (csrc/temporal_fold.hip): in[groups * subframes, frame_bytes] -> out[groups, frame_bytes], every output frame the
 * weighted average of `subframes` consecutive input frames.  A frame is a flat run of bytes (H * W * 3 for packed RGB).  With weights
 * w_i and W = sum w_i, in 32-bit unsigned integers (`/` is floor, so the rounding is half up), bit for bit:
 *   both tables NULL (encoded light)  out[g][j] = (sum_i w_i * in[g N + i][j] + W / 2) / W
 *   both tables given (linear light)  L = (sum_i w_i * decode[in[g N + i][j]] + W / 2) / W,  out[g][j] = max{ v : encode_threshold[v] <= L }
 * `weights`: a HOST pointer to `subframes` bytes, copied into the kernel arguments (the launch is capturable: one launch on `stream`, no
 * allocation, no synchronisation).  decode / encode_threshold: DEVICE tables of 256 entries; the caller guarantees encode_threshold[0] ==
 * 0 and a non-decreasing table.  MAUA_EINVAL (before any HIP call) for subframes outside 1 .. 16, W == 0, frame_bytes <= 0, groups < 0,
 * exactly one table, a NULL pointer, or out overlapping in; groups == 0 is a successful no-op, more than 65535 groups a launch are
 * MAUA_ENOSYS.  Any frame size and any alignment of in and out is served: frame_bytes % 16 == 0 with in and out at the same offset from a
 * 16-byte boundary takes the 16-byte vector path, everything else goes byte by byte.  (Additive: the ABI version is unchanged.) */
int maua_temporal_fold_u8(const uint8_t* in, uint8_t* out, int groups, int subframes, int64_t frame_bytes, const uint8_t* weights,
                          const uint16_t* decode, const uint16_t* encode_threshold, void* stream);
/* Deep frame delivery (csrc/deep_frames.hip): 16-bit packed RGB and 10-bit planar YUV from the fp32 image.  (Additive: the ABI version
 * is unchanged.)
 *   maua_frames_to_u16  [B,3,H,W] fp32 -> [B,H,W,3] uint16 (ffmpeg's rgb48le), the 8-bit quantiser with the scale changed: bit for bit the
 *                       fp32 statement ((clip(x, -1, 1) + 1) * 32767.5).astype(uint16), a truncating cast; the add and the multiply are
 *                       never contracted.  NaN gives 0, -inf 0, +inf 65535, 1 gives 65535.  Arguments as maua_frames_to_u8 (batch <= 0 is
 *                       MAUA_EINVAL); plane % 4 == 0 with img 16-byte and out 8-byte aligned takes the vector path.
 *   maua_crop_resize_u16  maua_crop_resize_u8 on uint16 frames: the same taps, clamping and coefficients rounded to 22 fractional bits,
 *                       64-bit products, the horizontal pass rounded half up to 16 bits, then the vertical pass on that, clamped to
 *                       0 .. 65535.  MAUA_ENOSYS for a down-scale; MAUA_EINVAL as the 8-bit entry.
 *   maua_rgb48_to_yuv_p10  rgb[B,h,w,3] uint16 -> planar out[B, frame] uint16 with a 10-bit value in the low bits: per frame the Y plane
 *                       [h, w], then U, then V, each [h/2, w/2] for subsampling 420, [h, w/2] for 422, [h, w] for 444 (ffmpeg's
 *                       yuv420p10le / yuv422p10le / yuv444p10le).  ITU-R BT.709 limited range, the exact rational value for Kr = 0.2126,
 *                       Kg = 0.7152, Kb = 0.0722 rounded half up, in 64-bit integers (`/` is floor).  For a block of n pixels whose codes
 *                       sum to Sr, Sg, Sb (n = 1 for Y; chroma from the box sum of the 2 x 2, 2 x 1 or 1 x 1 block: centre siting):
 *                         L  = 2126 Sr + 7152 Sg + 722 Sb
 *                         Y  = 64 + (2 * 876 * L + D) / (2 D)                       D  = 10000 * 65535
 *                         Cb = (2 * (512 Eb + 896 * (10000 Sb - L)) + Eb) / (2 Eb)  Eb = 2 * 9278 * 65535 * n
 *                         Cr = (2 * (512 Er + 896 * (10000 Sr - L)) + Er) / (2 Er)  Er = 2 * 7874 * 65535 * n
 *                       MAUA_EINVAL for another subsampling, non-positive h or w, batch < 0, odd w (420, 422) or odd h (420), a NULL
 *                       buffer; batch == 0 is a successful no-op; more than 65535 frames a launch are MAUA_ENOSYS.  Any legal width and
 *                       alignment is served; w % 8 == 0 with 16-byte aligned buffers takes the vector path.
 *   maua_frames_to_yuv_p10_f32  img[B,3,h,w] fp32 -> the same planar frame in one launch: maua_rgb48_to_yuv_p10 applied to
 *                       maua_frames_to_u16, bit for bit, the 16-bit codes kept in registers.  Arguments and refusals as
 *                       maua_rgb48_to_yuv_p10; w % 4 == 0 with img 16-byte and out 8-byte aligned takes the vector path. */
int maua_frames_to_u16(const float* img, uint16_t* out, int batch, int h, int w, void* stream);
int maua_crop_resize_u16(const uint16_t* in, uint16_t* out, int batch, int in_h, int in_w, int x0, int y0, int crop_w, int crop_h,
                         int out_w, int out_h, void* stream);
int maua_rgb48_to_yuv_p10(const uint16_t* rgb, uint16_t* out, int batch, int h, int w, int subsampling, void* stream);
int maua_frames_to_yuv_p10_f32(const float* img, uint16_t* out, int batch, int h, int w, int subsampling, void* stream);
/* Colour grading of the fp32 image (csrc/grade.hip): ASC CDL, a 3 x 3 matrix and a 3-D LUT in front of the quantisers.  (Additive: the ABI
 * version is unchanged.)
 *   maua_grade_f32    img[B,3,h,w] fp32 -> out[B,3,h,w] fp32; out == img (in place) is legal
 *   maua_grade_to_u8  img[B,3,h,w] fp32 -> out[B,h,w,3] uint8: maua_frames_to_u8 applied to maua_grade_f32's result, bit for bit, the
 *                     graded value kept in registers
 * Frame b reads the 24 floats at rows + b * row_stride (row_stride >= 24): slope[3] at 0, offset[3] at 3, power[3] at 6, the matrix M[3][3]
 * row-major at 9, bias[3] at 18, lut_mix at 21, two reserved zeros.  Per pixel, in fp32, every operation rounded on its own (no multiply-add
 * is contracted), with clamp01(a) = fminf(fmaxf(a, 0), 1), which takes a NaN to 0 as the quantiser's clamp does:
 *   v_c = clamp01(x_c * 0.5f + 0.5f)
 *   t_c = clamp01(v_c * slope_c + offset_c);  t_c = power_c == 1 ? t_c : powf(t_c, power_c)       (0 stays 0)
 *   m_c = clamp01(((M[c][0] * t_0 + M[c][1] * t_1) + M[c][2] * t_2) + bias_c)
 *   lut != NULL and lut_mix != 0:  l = tetra(lut, m);  m_c = clamp01(m_c + lut_mix * (l_c - m_c))
 *   y_c = m_c * 2.0f - 1.0f
 * lut: a table of lut_n^3 entries (2 <= lut_n <= 65) over the domain [0, 1], red index fastest (.cube order), every entry PADDED to four
 * floats (r, g, b, unused) and the table 16-byte aligned: entry (ir, ig, ib) is at float offset 4 * ((ib * lut_n + ig) * lut_n + ir).
 * tetra, per axis a: p = m_a * (lut_n - 1), i_a = min((int)p, lut_n - 2), f_a = p - i_a.  The fractions are ordered hi >= mid >= lo by
 * this chain, which also resolves ties:
 *   f_r >= f_g:  f_g >= f_b ? (r, g, b) : f_r >= f_b ? (r, b, g) : (b, r, g)
 *   otherwise:   f_b >= f_g ? (b, g, r) : f_b >= f_r ? (g, b, r) : (g, r, b)
 * The vertices are v0 = c(i), v1 = v0 stepped along hi's axis, v2 = v1 stepped along mid's axis, v3 = c(i + 1), and
 *   l_c = (((1 - hi) * v0_c + (hi - mid) * v1_c) + (mid - lo) * v2_c) + lo * v3_c
 * m is clamped before it indexes the table: no index leaves it, whatever the rows and the image hold.
 * Identity: a frame whose row has slope 1, offset 0, power 1, M = I, bias 0 and (lut == NULL or lut_mix == 0) is passed through untouched —
 * out = img bit for bit, NaN payloads included; the uint8 output is maua_frames_to_u8's — because 2 * fl(0.5 x + 0.5) - 1 is not x in fp32.
 * The device does NOT check the rows (finite values, power > 0): audioreactive/grade.py's Grade does; the output is defined (clamped)
 * for any row.  One launch on `stream`, no allocation, no synchronisation: capturable.
 * Refused before any HIP call: MAUA_EINVAL for non-positive h or w, batch < 0, row_stride < 24, a lut with lut_n outside 2 .. 65 or not
 * 16-byte aligned, a NULL img, out or rows (batch > 0), an out that overlaps img other than out == img for the fp32 entry; batch == 0 is a
 * successful no-op; more than 65535 frames or more than 2^31 - 256 pixels per frame a launch are MAUA_ENOSYS.
 * Vector path (a lane takes 4 consecutive pixels: 16-byte loads, 16-byte stores or three dwords of uint8): h * w % 4 == 0, img 16-byte
 * aligned, out 16-byte (fp32) or 4-byte (uint8) aligned; anything else takes the scalar path, which serves any size and alignment. */
int maua_grade_f32(const float* img, float* out, int batch, int h, int w, const float* rows, int row_stride, const float* lut, int lut_n,
                   void* stream);
int maua_grade_to_u8(const float* img, uint8_t* out, int batch, int h, int w, const float* rows, int row_stride, const float* lut, int lut_n,
                     void* stream);
/* Lens effects on the fp32 image (csrc/lens.hip): bloom, sharpen / soften and vignette, in front of the grade and the quantisers.
 * (Additive: the ABI version is unchanged.)  Images are the generator's fp32 [B,3,h,w], raw range [-1, 1]; clamp01(a) = fminf(fmaxf(a, 0), 1)
 * takes a NaN to 0.  Frame b reads the 16 floats at rows + b * row_stride (row_stride >= 16): threshold at 0, knee at 1, bloom_rgb[3] at 2
 * (gain x tint, folded by the host), sharpen at 5 (negative softens), vignette at 6, vig_inner at 7, vig_outer at 8, seven reserved zeros.
 *
 * maua_lens_extract_f32  img[B,3,h,w] -> out[B,3,ceil(h/d),ceil(w/d)], d in {1, 2, 4, 8}.  Per pixel, in fp32, every operation rounded on
 * its own (nothing contracted):
 *   v_c = clamp01(x_c * 0.5f + 0.5f);  m = fmaxf(fmaxf(v_r, v_g), v_b);  o = m - threshold
 *   s = fminf(fmaxf(o + knee, 0), 2.0f * knee);  s = (s * s) / (4.0f * knee + 1e-5f)
 *   q = fmaxf(s, o) / fmaxf(m, 1e-5f)            (the soft-knee curve; s >= 0, so q >= 0)
 *   hl_c = v_c * q
 * An output cell is the sum of hl_c over the pixels of its d x d block that exist — accumulated from 0.0f row by row, within a row from
 * left to right — divided by their count as a float: edge blocks divide by their own count.
 *
 * maua_lens_blur_f32  src[B,planes,h,w] -> dst[B,planes,h,w], dst must not overlap src.  0 <= radius <= 64, tap_stride >= radius + 1;
 * frame b reads its half-kernel w[0 .. radius] at taps + b * tap_stride, w[0] the centre:
 *   y[i] = w[0] x[i] + sum_{k = 1 .. radius} w[k] (x[clamp(i - k)] + x[clamp(i + k)])       clamp: to 0 .. n - 1 (edges replicated)
 * along rows, then along columns of the result.  The order of the summation is NOT fixed and multiply-adds may be fused: the result is
 * within 2 (radius + 4) 2^-23 max|x| of the exact one for weights that sum to 1, and exact wherever every partial sum is representable
 * (dyadic taps on integers).  radius == 0 with w[0] == 1 copies.  The taps are not checked: the host builds them.
 * maua_lens_blur_plan reports, without launching, what the entry does for (h, w, radius, src): plan[0] the instance (1: w % 4 == 0
 * and src 16-byte aligned, the halo is staged with 16-byte loads; 0: scalar loads, any size and alignment), plan[1] x plan[2] the output
 * tile of a workgroup (64 x 64), plan[3] the workgroups per plane, plan[4] a workgroup's LDS in bytes (<= 65536 at every radius), plan[5] the
 * number of launches (1: there is no two-launch path).
 *
 * maua_lens_apply_f32  img[B,3,h,w] -> out[B,3,h,w]; out == img (in place) is legal.  bloom ([B,3,bh,bw], the blurred map of reduction d)
 * and soft ([B,3,h,w], a short-radius blur of img) may be NULL: then that term is absent.  Per pixel (px, py), in fp32, every operation
 * rounded on its own, in this order:
 *   y_c = x_c
 *   soft:   y_c = y_c + sharpen * (x_c - soft_c)
 *   bloom:  u = fminf(fmaxf((px + 0.5f) / d - 0.5f, 0), bw - 1), x0 = (int)u, x1 = min(x0 + 1, bw - 1), fx = u - x0; v, y0, y1, fy likewise
 *           with py and bh;  w00 = (1 - fx) * (1 - fy), w01 = fx * (1 - fy), w10 = (1 - fx) * fy, w11 = fx * fy;
 *           g_c = ((w00 * b[y0][x0] + w01 * b[y0][x1]) + w10 * b[y1][x0]) + w11 * b[y1][x1]
 *           y_c = y_c + (2.0f * bloom_rgb_c) * g_c                                  (2: the map lives in display range 0 .. 1)
 *   vignette != 0:  dx = ((px + 0.5f) - w * 0.5f) / (w * 0.5f), dy likewise;  r = sqrtf(dx * dx + dy * dy) * 0.70710678f   (corner: 1)
 *           t = clamp01((r - vig_inner) / (vig_outer - vig_inner));  f = 1.0f - vignette * ((t * t) * (3.0f - 2.0f * t))
 *           y_c = (y_c + 1.0f) * f - 1.0f
 * Identity: a frame whose row has bloom_rgb == 0, sharpen == 0 and vignette == 0 is passed through untouched — out = img bit for bit, NaN
 * payloads included, whatever bloom and soft hold.  The test is uniform over the frame.
 *
 * Every entry is one launch on `stream`, no allocation, no synchronisation: capturable.  The rows are not checked (audioreactive/lens.py's
 * Lens does).  Refused before any HIP call: MAUA_EINVAL for non-positive sizes, batch < 0, d outside {1, 2, 4, 8} (apply: with a bloom
 * only), radius outside 0 .. 64, tap_stride < radius + 1, row_stride < 16, a NULL img / src / out / dst / rows / taps (batch > 0), an output
 * that overlaps an input other than out == img in apply; batch == 0 is a successful no-op; more than 65535 frames (blur: or planes) or more
 * than 2^31 - 256 pixels per plane (blur: or more than 2^24 - 1 tiles of 64 x 64 per plane, which only a plane a few pixels wide or high
 * reaches) are MAUA_ENOSYS.  Vector paths (16-byte accesses, 4 consecutive pixels of a row per lane): w % 4 == 0 and
 * the image pointers 16-byte aligned (extract: img; blur: src; apply: img, out and soft); anything else takes the scalar paths. */
int maua_lens_extract_f32(const float* img, float* out, int batch, int h, int w, int d, const float* rows, int row_stride, void* stream);
int maua_lens_blur_f32(const float* src, float* dst, int batch, int planes, int h, int w, int radius, const float* taps, int tap_stride,
                       void* stream);
int maua_lens_blur_plan(int h, int w, int radius, const float* src, int* plan);
int maua_lens_apply_f32(const float* img, float* out, int batch, int h, int w, const float* rows, int row_stride, const float* bloom, int bh,
                        int bw, int d, const float* soft, void* stream);
/* Frame feedback on the fp32 image (csrc/feedback.hip): the previous OUTPUT frame, warped, scaled and combined under the new one, in front
 * of the lens, the grade and the quantisers.  (Additive: the ABI version is unchanged.)  Images are the generator's fp32 [B,3,h,w], raw
 * range [-1, 1], black = -1.  A recurrence: frame i of the call reads out[i - 1]; frame 0 reads `state` ([3,h,w]; state_valid == 0: a
 * black frame, `state` is not read); the last frame's result is also stored to `state`.
 *
 * `rows` is HOST memory, read during the call and never after it: frame i's 16 floats at rows + i * row_stride (row_stride >= 16) travel
 * to its launch by value, so a captured call keeps the values it was captured with.  A row: the INVERSE matrix in pixels a, b, tx at 0..2
 * and c, d, ty at 3..5, gain at 6, tint_rgb at 7..9, dry at 10, limit at 11, a "still" flag at 12, three reserved zeros.
 * Per output pixel (x, y), in fp32, every operation rounded on its own, in this order (nothing is fused):
 *   cx = (w - 1) * 0.5f, cy = (h - 1) * 0.5f;  dx = x - cx, dy = y - cy
 *   sx = ((a * dx + b * dy) + tx) + cx,  sy = ((c * dx + d * dy) + ty) + cy;  each clamped to +-2^30 by fminf(fmaxf(s, -2^30), 2^30)
 *   ix = (int)floorf(sx), fx = sx - floorf(sx);  iy, fy likewise;  the taps are columns ix, ix + 1 and rows iy, iy + 1, each INDEX taken
 *   through the border rule (border 0 zero: an index outside 0 .. n - 1 is a black tap, -1.0f;  1 replicate: clamped;  2 mirror: reflected
 *   about the first and last element, period 2 (n - 1), n == 1: index 0;  3 wrap: modulo n) — the same as folding the coordinate, since
 *   every rule is continuous in it
 *   top = v00 + fx * (v01 - v00), bottom = v10 + fx * (v11 - v10), p_c = top + fy * (bottom - top)
 *   u_prev = 0.5f * p_c + 0.5f;  u_cur = 0.5f * cur_c + 0.5f;  g_c = gain * tint_c (rounded once);  A = dry * u_cur, B = g_c * u_prev
 *   mode 0 add: u = A + B;  1 max: u = fmaxf(A, B);  2 screen: u = 1.0f - (1.0f - clamp01(A)) * (1.0f - clamp01(B)),
 *   clamp01(a) = fminf(fmaxf(a, 0), 1);   u = fminf(u, limit);   out_c = 2.0f * u - 1.0f
 * Neutral: a row with gain == 0 and dry == 1 passes its frame through — out = cur bit for bit, NaN payloads included; the frame is the
 * state of the next one like any other.  Still: a row whose flag is non-zero AND whose matrix is exactly 1, 0, 0, 0, 1, 0.
 *
 * Launches, in order, all on `stream`: a run of consecutive still rows (at most 64 frames, a longer run is split) is ONE launch that keeps
 * a lane's pixels in registers across the run's frames; every other frame is one launch.  The two kinds agree bit for bit on finite
 * images.  The launch of the last frame stores `out` and `state`; only a call of ONE moving, non-neutral frame with state_valid != 0 —
 * which gathers from the state it replaces — stores `out` and is followed by one device-to-device copy on `stream`.  No allocation, no
 * synchronisation: capturable.  out == img (in place) is legal.  Vector instances (16-byte accesses, 4 consecutive pixels of a row per
 * lane): w % 4 == 0 and img, out and state 16-byte aligned; anything else takes the scalar instances.
 * maua_feedback_plan reports without launching (host_rows NULL: every row counts as moving): plan[0] launches, plan[1] how many of them are
 * still runs, plan[2] 1 when w and img allow the vector instances, plan[3], plan[4] bit k set when launch k (of the first 64) is a still
 * run, plan[5] 1 when the call may be followed by the copy above, plan[6] workgroups per launch, plan[7] the longest still run of a launch.
 * Refused before any HIP call, outputs untouched: MAUA_EINVAL for a NULL img / out / state / rows (plan: img / plan), batch < 1,
 * non-positive sizes, mode outside 0 .. 2, border outside 0 .. 3, row_stride < 16, out overlapping img other than out == img, state
 * overlapping img or out; MAUA_ENOSYS for more than 2^31 - 256 pixels per plane.  The rows are not checked (audioreactive/feedback.py's
 * Feedback does).  maua_feedback_test_grid_cap (tests only) caps the workgroups of a launch (0: the default) and returns the old cap. */
int maua_feedback_f32(const float* img, float* out, float* state, int state_valid, int batch, int h, int w, const float* rows, int row_stride,
                      int mode, int border, void* stream);
int maua_feedback_plan(int batch, int h, int w, const float* host_rows, int row_stride, const float* img, int* plan);
int maua_feedback_test_grid_cap(int cap);
/* Frame delivery at any size (csrc/resample.hip): a separable resampler on packed 3-channel frames, Pillow's Image.resize(size, resample,
 * box) for 8-bit images restated in integers and extended to 16 bits.  (Additive: the ABI version is unchanged.)
 * Per axis, for a source length n, a source interval [in0, in1), an output length m and a filter f of support s (box 0.5, bilinear 1,
 * hamming 1, bicubic 2 with a = -0.5, lanczos 3), in double:
 *   scale = (in1 - in0) / m, fs = max(scale, 1), support = s * fs, ksize = 2 * ceil(support) + 1
 *   output j: center = in0 + (j + 0.5) * scale, xmin = max(0, (int)(center - support + 0.5)), xmax = min(n, (int)(center + support + 0.5)) - xmin
 *   w_x = f((x + xmin - center + 0.5) / fs) for x < xmax, each divided by their sequential sum when that is non-zero
 *   k_x = (int)(w_x * 2^22 +- 0.5) (the sign of w_x), 0 from xmax to ksize;  bounds_j = (xmin, xmax)
 *   a pass: out_j = clamp((2^21 + sum_x in[xmin + x] * k_x) >> 22, 0, top), an arithmetic shift; top = 255 or 65535
 * The horizontal pass runs first and is rounded to the sample type, the vertical pass runs on its result; 8-bit sums are 32 bits wide,
 * 16-bit sums 64.
 *   maua_resample_coeffs  host only, no HIP call: writes k[out_size, ksize] to h_k (`cap` int32 entries) and bounds[out_size, 2] to
 *                       h_bounds for `filter` (MAUA_RESAMPLE_BOX .. MAUA_RESAMPLE_LANCZOS) and returns ksize.  MAUA_EINVAL for a size below
 *                       1, an interval outside 0 <= in0 < in1 <= in_size, an unknown filter, a NULL table or cap < out_size * ksize;
 *                       MAUA_ENOSYS for ksize > MAUA_RESAMPLE_MAX_TAPS (a Lanczos down-scale beyond about 10 : 1).
 *   maua_resample_u8 / maua_resample_u16  in[B,in_h,in_w,3] -> the window [dst_y0, dst_y0 + dst_h) x [dst_x0, dst_x0 + dst_w) of every frame
 *                       of out[B,out_h,out_w,3]; no byte outside the window is written (a letterbox border is the caller's, zeroed once).
 *                       kx[dst_w, ksize_x], bx[dst_w, 2], ky[dst_h, ksize_y], by[dst_h, 2]: DEVICE copies of the tables; both tables of an
 *                       axis NULL = the axis is copied (dst_w == in_w / dst_h == in_h required, its ksize ignored).  Bounds are clamped
 *                       to the frame and to ksize on the device, so no table makes the kernels read outside `in`.  One launch (fused) or
 *                       two (through `ws`, maua_resample_ws_bytes bytes, may be NULL where that is 0) on `stream`; no allocation, no
 *                       synchronisation, capturable; no atomics, identical bits from run to run.  Any alignment (of the sample type) and
 *                       any width is served; the 4-byte store path needs out, its row pitch and the window's first column on 4-byte
 *                       boundaries.  batch == 0 is a successful no-op.  MAUA_EINVAL, before any HIP call, for a NULL buffer, one table
 *                       of an axis without the other, a size below 1, a window outside the frame, taps outside 1 .. 64, a copied axis of
 *                       unequal lengths, out (or a needed ws) overlapping in, a needed ws that is NULL; MAUA_ENOSYS above 65535 frames.
 *   maua_resample_ws_bytes  bytes of `ws` for these arguments (ksize 0 = copied axis): 0 where the fused kernel runs or the arguments are
 *                       refused, else B * in_h * dst_w * 3 samples.  A pure function of its arguments.
 *   maua_resample_plan  the entries' own dispatch without the launch (sample_bytes 1 / 2; ksize 0 = copied axis; out_misalign = the
 *                       output address modulo 4): writes "fused.u8.vec 64x64 tiles=510 trips=1 rows=49 lds=12288" (instance, tile — 64
 *                       columns by 64, 32 or 16 rows, the tallest whose LDS stays within 20 KB —, tiles per frame, trips of a workgroup's
 *                       tile loop, LDS rows of the intermediate, dynamic LDS bytes; .vec / .scalar = the store path) or "twopass.u16 trips=8,2 ws=123" (grid-stride trips of the horizontal and vertical launch, workspace
 *                       bytes) and returns 0; the entries' refusals, or MAUA_EINVAL for a short buf.  No HIP call. */
#define MAUA_RESAMPLE_MAX_TAPS 64
#define MAUA_RESAMPLE_BOX 0
#define MAUA_RESAMPLE_BILINEAR 1
#define MAUA_RESAMPLE_HAMMING 2
#define MAUA_RESAMPLE_BICUBIC 3
#define MAUA_RESAMPLE_LANCZOS 4
int maua_resample_coeffs(int in_size, int in0, int in1, int out_size, int filter, int32_t* h_k, int32_t* h_bounds, int cap);
int maua_resample_u8(const uint8_t* in, uint8_t* out, int batch, int in_h, int in_w, int out_h, int out_w, int dst_x0, int dst_y0, int dst_w,
                     int dst_h, const int32_t* kx, const int32_t* bx, int ksize_x, const int32_t* ky, const int32_t* by, int ksize_y, void* ws,
                     void* stream);
int maua_resample_u16(const uint16_t* in, uint16_t* out, int batch, int in_h, int in_w, int out_h, int out_w, int dst_x0, int dst_y0,
                      int dst_w, int dst_h, const int32_t* kx, const int32_t* bx, int ksize_x, const int32_t* ky, const int32_t* by,
                      int ksize_y, void* ws, void* stream);
int64_t maua_resample_ws_bytes(int sample_bytes, int batch, int in_h, int in_w, int dst_w, int dst_h, int ksize_x, int ksize_y);
int maua_resample_plan(int sample_bytes, int batch, int in_h, int in_w, int out_h, int out_w, int dst_x0, int dst_y0, int dst_w, int dst_h,
                       int ksize_x, int ksize_y, int out_misalign, char* buf, int buf_len);

/* ------------------------------------------------------------------------------------------------ audio / temporal
 * Circular Gaussian FIR along time (audioreactive/signal.py:319-368): x [T, F] -> y [T, F], taps[2*radius+1]
 * already normalised / causal-weighted by the host; circular index when radius <= T, else the reference's
 * single-wrap-then-zero padding (:350-355).  The taps are staged in LDS with 96 floats of zero padding: radius <=
 * MAUA_TEMPORAL_FIR_MAX_RADIUS (a Gaussian of sigma ~2000 frames), MAUA_EINVAL above.  A non-finite sample stays inside the filter's
 * support, as with the reference's conv1d. */
#define MAUA_TEMPORAL_FIR_MAX_RADIUS 8143
int maua_temporal_fir_f32(const float* x, const float* taps, float* y, int n_frames, int64_t features, int radius,
                          void* stream);

/* Power spectrogram |STFT|^2 (librosa.stft as called at audioreactive/signal.py:51,93,119): centred, reflect-padded
 * frames, window[n_fft] in device memory, n_fft a power of two <= 4096.  y[n_samples] -> p[n_bins = n_fft/2+1, n_frames]. */
int maua_stft_power_f32(const float* y, int64_t n_samples, const float* window, int n_fft, int hop, float* p,
                        int n_frames, void* stream);
/* Harmonic / percussive source separation pieces (librosa.effects.percussive / harmonic, audioreactive/signal.py:49,150):
 *   complex STFT -> re/im [n_fft/2+1, n_frames];  inverse STFT (frames_ws: n_frames*n_fft floats of workspace; window-sum-
 *   square normalised overlap-add, centre padding removed, output length n_samples);
 *   median filter of x[rows, cols] along axis 0 (frequency) or 1 (time), size in {3,5,9,17,31}, scipy 'reflect' boundary;
 *   soft mask (x / z)^p / ((x/z)^p + (x_ref*margin/z)^p) applied to the complex spectrum. */
int maua_stft_complex_f32(const float* y, int64_t n_samples, const float* window, int n_fft, int hop, float* out_re,
                          float* out_im, int n_frames, void* stream);
int maua_istft_f32(const float* in_re, const float* in_im, const float* window, int n_fft, int hop, int n_frames,
                   float* frames_ws, float* y, int64_t n_samples, void* stream);
/* Median of a centred window of `size` in {3, 5, 9, 17, 31} taps (MAUA_ENOSYS otherwise) along `axis` of x[rows, cols]: periodic symmetric
 * reflection (d c b a | a b c d | d c b a), any axis length: scipy.ndimage mode 'reflect', and numpy.pad 'symmetric' where the axis is
 * shorter than size / 2. */
int maua_median_filter_f32(const float* x, float* y, int rows, int cols, int size, int axis, void* stream);
int maua_softmask_apply_f32(const float* re, const float* im, const float* x, const float* x_ref, float margin, float power,
                            int split_zeros, float* out_re, float* out_im, int64_t n, void* stream);
/* out[M,N] = fb[M,K] @ p[K,N] (mel / chroma filterbank projection), optional 10*log10(max(amin, .)) when to_db. */
int maua_filterbank_f32(const float* fb, const float* p, float* out, int m, int k, int n, int to_db, float amin,
                        void* stream);

/* Fourier-method resampling along time, y[num, features] from x[n, features] (row-major, fp64) — scipy.signal.resample
 * as called at audioreactive/signal.py:68,152 — evaluated as a Dirichlet-kernel sum in the time domain. */
int maua_resample_f64(const double* x, int n, int64_t features, double* y, int num, void* stream);

/* |constant-Q transform| (librosa.cqt role inside chroma_cqt / chroma_cens, signal.py:115-117): out[k][t] for n_bins
 * geometrically spaced frequencies freqs[k] (Hz) with window lengths lengths[k] (samples), centred frames every `hop`
 * samples with reflect padding, periodic-Hann kernels of unit L1 norm, scaled by 1/sqrt(length). */
int maua_cqt_mag_f32(const float* y, int64_t n_samples, const float* freqs, const int* lengths, int n_bins, int hop,
                     float sr, float* out, int n_frames, void* stream);

/* Chroma post-processing for audioreactive/signal.py:102-133 (ch / out are [n_bins <= 32, n_frames], fp32):
 * CENS = per-frame L1 normalisation, 4-level quantisation, Hann smoothing over win_len (odd) frames, L2 normalisation;
 * nn_median = per-frame median over the k frames of highest cosine similarity outside |i-j| < width (the
 * aggregate=np.median, metric="cosine" nearest-neighbour filter at :131; 1 <= k < n_frames; where fewer than k frames are admissible the
 * excluded ones fill up in index order, every frame at most once).  The fp64 similarity row of a frame lives in LDS
 * while n_frames * 8 + k * (4 + 4 n_bins) bytes fit (~16k frames); longer tracks need a caller-owned workspace `ws` of
 * maua_nn_median_ws_doubles() doubles (0 = not needed, ws may be NULL).  A non-NULL ws of min(n_frames, 1024) * n_frames doubles
 * selects the workspace path at any size (same results, bit for bit). */
int maua_chroma_cens_f32(const float* ch, float* out, int n_bins, int n_frames, int win_len, void* stream);
int64_t maua_nn_median_ws_doubles(int n_bins, int n_frames, int k);
int maua_nn_median_f32(const float* ch, float* out, int n_bins, int n_frames, int k, int width, double* ws, void* stream);

/* Monophonic pitch tracking (audioreactive raw_pitch / pitch; csrc/pitch.hip; additive: the ABI version is unchanged).
 * YIN (de Cheveigne & Kawahara 2002, steps 1-5) on centred frames.  n_frames must equal 1 + n_samples / hop.
 *   Framing.  L = frame + tau_max.  Frame t reads L samples starting at t * hop - L / 2 (integer division); samples outside
 *     [0, n_samples) are 0.  x[j] below is frame-relative.
 *   Difference function.  d(0) = 0; for tau = 1 .. tau_max, d(tau) = sum_{j=0}^{frame-1} (x[j] - x[j + tau])^2, the direct sum of squares
 *     (not the energy / FFT form, which cancels).
 *   Normalised difference (CMNDF).  d'(0) = 1; for tau >= 1, d'(tau) = d(tau) tau / sum_{k=1}^{tau} d(k) when that sum is > 0, else 1.
 *   Pick.  The smallest tau in [tau_min, tau_max] with d'(tau) < threshold, then advanced while tau + 1 <= tau_max and
 *     d'(tau + 1) < d'(tau); if no lag is below the threshold, the first global minimum of d' over [tau_min, tau_max].  That is tau_int.
 *   Refine.  a, b, c = d'(tau - 1), d'(tau), d'(tau + 1).  If tau - 1 >= 1, tau + 1 <= tau_max and a - 2 b + c > 0:
 *     shift = clamp(0.5 (a - c) / (a - 2 b + c), -0.5, 0.5), lag = tau + shift, aperiodicity = max(0, b - 0.25 (a - c) shift) (the
 *     unclamped parabola dips slightly below 0 on clean tones); otherwise lag = tau and aperiodicity = b.
 *   The sample rate never enters: the host computes f0 = sr / lag.
 * MAUA_EINVAL, before any device call: a NULL y / lag / aperiodicity / tau_int, frame outside 16 .. MAUA_YIN_MAX_FRAME, not
 *   1 <= tau_min < tau_max <= MAUA_YIN_MAX_LAG, hop < 1, n_samples < 1, a threshold that is negative or not finite,
 *   n_frames != 1 + n_samples / hop.
 * Deterministic run to run, capturable, no workspace.  A non-finite sample may make the frames that cover it arbitrary, but their tau_int
 *   stays inside [tau_min, tau_max]; it never changes a frame that does not cover it. */
#define MAUA_YIN_MAX_FRAME 4096
#define MAUA_YIN_MAX_LAG 2048
int maua_yin_f32(const float* y, int64_t n_samples, int frame, int hop, int tau_min, int tau_max, float threshold,
                 float* lag /*[n_frames]*/, float* aperiodicity /*[n_frames]*/, int32_t* tau_int /*[n_frames]*/,
                 float* cmndf /*[n_frames, tau_max + 1] or NULL*/, int n_frames, void* stream);

/* Probabilistic YIN (audioreactive raw_pyin / pitch(method="pyin"); csrc/pyin.hip; additive: the ABI version is unchanged).
 * Mauch & Dixon, "pYIN: a fundamental frequency estimator using probabilistic threshold distributions", ICASSP 2014, in two entries
 * behind the d' rows of maua_yin_f32.  tests/pyin_ref.py restates both in numpy.
 *
 * maua_pyin_candidates_f32: d' rows -> per-bin voiced mass.  cmndf [n_frames, tau_max + 1] as maua_yin_f32 writes it; obs and period
 * [n_frames, n_bins]; voiced_prob [n_frames].  Per frame, with r = cmndf[t]:
 *   Troughs.  A lag tau in [tau_min, tau_max - 1] is a trough where r[tau] < r[tau - 1] and r[tau] <= r[tau + 1]; at tau_min the left
 *     neighbour counts as +inf; tau_max is never a trough.  fp32 compares of the given values (a NaN compares false).  Height h = r[tau].
 *   Threshold prior.  Thresholds k / n_thr, k = 1 .. n_thr; cum_prior[0 .. n_thr] is the running sum of their prior (cum_prior[0] = 0,
 *     non-decreasing, summed in float64 by the host and rounded once).  idx(x) = clamp((int)floorf(x * (float)n_thr), 0, n_thr), the
 *     number of thresholds at or below x; idx(+inf) = idx(NaN) = n_thr.  Walking the troughs in ascending lag with m = the minimum
 *     height of the earlier ones (+inf for the first): a trough with h < m — a record — gets p = cum_prior[idx(m)] - cum_prior[idx(h)],
 *     one fp32 subtraction (it owns every threshold for which it is the first trough below); every other trough gets 0.  The first
 *     trough of smallest height (the last record) gets p + no_trough_prob * cum_prior[idx(h)] instead: the product rounded, then one
 *     addition (YIN's fallback picks the global minimum, with that probability, under every threshold no trough gets under).  A frame
 *     without troughs has no mass.
 *   Period.  Each trough with p > 0 is refined by the parabola of maua_yin_f32: a, b, c = r[tau - 1], r[tau], r[tau + 1]; if
 *     tau - 1 >= 1 and a - 2 b + c > 0, lag = tau + fminf(fmaxf(0.5 (a - c) / (a - 2 b + c), -0.5), 0.5), otherwise lag = tau.
 *   Bin.  bin_edge_period[0 .. n_bins] is strictly decreasing; bin b holds the periods in (edge[b + 1], edge[b]]; a period above
 *     edge[0] goes to bin 0, one at or below edge[n_bins] to bin n_bins - 1.  (The host builds the edges in float64 from the bins'
 *     frequencies and rounds once: the device needs no logarithm.)
 *   Outputs.  obs[t, b] = the sum of the p that fall into b, added in ascending lag; period[t, b] = the refined lag of the heaviest
 *     trough in b (ties to the lower lag), 0 where there is none; voiced_prob[t] = min(1, the sum of all p in ascending lag).  Every
 *     element of the three outputs is written.
 * MAUA_EINVAL, without a launch: a null pointer, n_frames < 1, not 1 <= tau_min < tau_max <= MAUA_YIN_MAX_LAG, n_thr outside
 *   1 .. MAUA_PYIN_MAX_THRESHOLDS, n_bins outside 1 .. MAUA_PYIN_MAX_BINS, no_trough_prob outside [0, 1] or not finite.
 * No atomics, no workspace, capturable: the result is a function of the arguments alone.
 *
 * maua_pyin_viterbi_f64: the most probable path through 2 P states, P = n_bins: state p < P is voiced in bin p, state P + p unvoiced
 * in bin p.  logobs_voiced [T, P] and logobs_unvoiced [T] (shared by the unvoiced states of a frame) are fp32, widened exactly.
 * log_tri [2 W + 1] holds the logarithms of the triangular weights W + 1 - |d|, log_norm [P] the logarithm of source bin i's sum of those
 * weights over the targets inside [0, P - 1]; both built by the host in float64.  Every operation is a double addition, subtraction
 * or compare, in this order:
 *   Frame 0.  delta[s] = logobs(0, s) + log_init; row 0 of backptr holds each state's own index.
 *   Frame t >= 1.  e_v[i] = delta[i] - log_norm[i], e_u[i] = delta[P + i] - log_norm[i].  For target bin j the window is
 *     i in [max(0, j - W), min(P - 1, j + W)]; bv = the maximum over it of e_v[i] + log_tri[j - i + W] and iv its index, scanning
 *     ascending i from the window's first element, a later candidate replacing the best only when strictly greater (ties go to the
 *     lowest i, a NaN never replaces); bu, iu the same from e_u.
 *     Voiced target: a = bv + log_stay, b = bu + log_switch; it takes a with backptr iv unless b > a, then b with backptr P + iu;
 *       delta'[j] = logobs_voiced[t, j] + that.
 *     Unvoiced target: a = bv + log_switch, b = bu + log_stay, the same rule; delta'[P + j] = logobs_unvoiced[t] + that.
 *   End.  states[T - 1] = the first maximum of the final delta (scanning ascending from state 0, replaced only by a strictly greater
 *     one); states[t - 1] = backptr[t][states[t]].
 * delta_last [2 P], every element of backptr [T, 2 P] and of states [T] are written.  -inf in the inputs is legal (a frame of nothing
 * but -inf decodes to the lowest index); a NaN does not fault, the rules above define what it does.
 * MAUA_EINVAL, without a launch: a null pointer, n_frames < 1, n_bins outside 1 .. MAUA_PYIN_MAX_BINS, width outside
 *   0 .. MAUA_PYIN_MAX_WIDTH (width >= n_bins is fine: the window is clipped).
 * One workgroup, latency-bound by construction (one barrier per frame); capturable, no workspace. */
#define MAUA_PYIN_MAX_BINS 1024
#define MAUA_PYIN_MAX_THRESHOLDS 256
#define MAUA_PYIN_MAX_WIDTH 128
int maua_pyin_candidates_f32(const float* cmndf, int n_frames, int tau_min, int tau_max, const float* cum_prior /*[n_thr + 1]*/,
                             int n_thr, float no_trough_prob, const float* bin_edge_period /*[n_bins + 1]*/, int n_bins,
                             float* obs /*[n_frames, n_bins]*/, float* period /*[n_frames, n_bins]*/, float* voiced_prob /*[n_frames]*/,
                             void* stream);
int maua_pyin_viterbi_f64(const float* logobs_voiced, const float* logobs_unvoiced, int n_frames, int n_bins, int width,
                          const double* log_tri, const double* log_norm, double log_init, double log_stay, double log_switch,
                          double* delta_last /*[2 n_bins]*/, uint16_t* backptr /*[n_frames, 2 n_bins]*/, int32_t* states /*[n_frames]*/,
                          void* stream);

/* Predominant local pulse (audioreactive raw_plp / tempogram / pulse / tempo / beats / beat_phase; csrc/pulse.hip; additive: the ABI
 * version is unchanged).  Grosche & Mueller, "Extracting predominant local pulse information from music recordings", IEEE TASLP 2011,
 * in two entries behind an onset envelope.  tests/pulse_ref.py restates both in numpy.
 *
 * maua_tempogram_peak_f32: the strongest tempo of every frame of a Fourier tempogram on an arbitrary tempo grid.  env [n] is the
 * envelope; table [n_tempi][win][2] (8-byte aligned) holds tab[b][k] = w[k] (cos(omega_b k), -sin(omega_b k)), built by the host in
 * float64 and rounded once, w >= 0 the window and omega_b the grid in radians per frame; prior [n_tempi] >= 0, NULL for all ones.
 *   Frame t reads x[k] = env[t - win / 2 + k] (integer division), k = 0 .. win - 1, 0 outside [0, n).
 *   F[t, b] = sum_k x[k] tab[b][k]: per component one fp32 chain acc = fmaf(x[k], tab, acc) from 0 in ascending k, clipped taps added
 *     as zeros, so a frame's result does not depend on where it lies in the envelope or in the launch.
 *   S[t, b] = (Re Re + Im Im) prior[b], every operation rounded on its own (without a prior the last product is left out).
 *   Peak.  best = 0, bin = -1; walking b upwards, b is taken when S > best (an fp32 compare): the lowest b wins ties, a frame without
 *     energy and a frame whose scores are all NaN keep bin = -1.
 *   Outputs.  bin [n]; phase [n] = atan2f(Im, Re) of the winner, 0 for bin = -1; power [n] = best; tgram [n][n_tempi] = S when the
 *     pointer is not NULL.  Every element is written.  A NaN in env reaches exactly the frames whose window covers it.
 *
 * maua_pulse_synth_f32: the overlap-add of every frame's windowed sinusoid, in gather form.  bin, phase [n] as above, window [win] =
 * w, omega [n_tempi].  A bin outside [0, n_tempi) counts as -1 and indexes nothing.  For output sample m, walking k = 0 .. win - 1 and
 * t = m + win / 2 - k, frames outside [0, n) skipped:
 *     den = den + w[k];   for bin[t] >= 0:  num = num + w[k] cosf(omega[bin[t]] (float)k + phase[t])
 *   every operation an fp32 operation rounded on its own, cosf accurate to a few ulp at every argument (they reach win omega + pi).
 *   pulse[m] = num / den where den > 0 and the quotient is > 0, else 0: a steady pulse reaches about 1, and there is no normalisation
 *   over the clip.  Every element of pulse [n] is written.
 *
 * Both: MAUA_EINVAL, without a launch, on a NULL pointer (other than prior and tgram), n outside 1 .. MAUA_PULSE_MAX_FRAMES, win outside
 * 2 .. MAUA_PULSE_MAX_WIN, n_tempi outside 1 .. MAUA_PULSE_MAX_TEMPI.  No atomics, no workspace, no allocation or synchronisation:
 * capturable, and the result is a function of the arguments alone, bit for bit. */
#define MAUA_PULSE_MAX_FRAMES (1 << 22)
#define MAUA_PULSE_MAX_WIN 2048
#define MAUA_PULSE_MAX_TEMPI 1024
int maua_tempogram_peak_f32(const float* env, int n, const float* table /*[n_tempi][win][2]*/, int win, int n_tempi,
                            const float* prior /*[n_tempi] or NULL*/, int* bin /*[n]*/, float* phase /*[n]*/, float* power /*[n]*/,
                            float* tgram /*[n][n_tempi] or NULL*/, void* stream);
int maua_pulse_synth_f32(const int* bin, const float* phase, int n, const float* window /*[win]*/, int win,
                         const float* omega /*[n_tempi]*/, int n_tempi, float* pulse /*[n]*/, void* stream);

/* Hidden Markov models with a dense transition matrix (audioreactive viterbi / hmm_posterior / raw_chords / chords; csrc/hmm.hip;
 * additive: the ABI version is unchanged).  Two entries over S = n_states states and T = n_frames frames: the most probable path
 * (Viterbi) and the per-frame state posteriors (scaled forward-backward; Rabiner, "A tutorial on hidden Markov models and selected
 * applications in speech recognition", Proc. IEEE 1989, III.A-B and V.A).  Matrices are row-major with row = source state i and
 * column = target state j; observations are fp32 and widened exactly, everything else is float64.  tests/hmm_ref.py restates both in
 * numpy, bit for bit.
 *
 * maua_hmm_viterbi_f64: logobs [T, S], log_trans [S, S], log_init [S] are logarithms.  Every operation is a double addition or compare:
 *   Frame 0.  delta[j] = log_init[j] + logobs[0, j]; backptr[0, j] = j.
 *   Frame t >= 1, target j.  best = delta[0] + log_trans[0][j] with index 0; then i = 1 .. S - 1 ascending, the candidate
 *     delta[i] + log_trans[i][j] replacing best (and the index) only when strictly greater: ties go to the lowest i, a NaN never
 *     replaces (and a NaN at i = 0 is never replaced).  delta'[j] = best + logobs[t, j]; backptr[t, j] = the index.
 *   End.  states[T - 1] = the first maximum of the final delta under the same rule (from state 0, replaced only by a strictly greater
 *     one); states[t - 1] = backptr[t][states[t]].
 * delta_last [S] (the final delta), every element of backptr [T, S] and of states [T] are written.  -inf is legal anywhere (forbidden
 * transitions; a frame of nothing but -inf decodes to the lowest index); a NaN does not fault, the rules above define what it does.
 *
 * maua_hmm_posterior_f64: obs [T, S] are likelihoods >= 0 up to a factor per frame, trans [S, S] and init [S] probabilities.  Every
 * product, sum and quotient below is one float64 operation rounded on its own (no fused multiply-add anywhere):
 *   Forward, frame 0.  a[j] = init[j] * obs[0, j].
 *   Forward, frame t >= 1.  p[j] = the chain acc = acc + alpha_{t-1}[i] * trans[i][j] from acc = 0.0 over i = 0 .. S - 1 ascending;
 *     a[j] = p[j] * obs[t, j].
 *   Both.  c_t = the chain acc = acc + a[j] from 0.0 over j ascending; alpha_t[j] = a[j] / c_t.
 *   Backward, from beta_{T-1}[i] = 1, t = T - 2 .. 0.  u[j] = obs[t + 1, j] * beta_{t+1}[j]; q[i] = the chain
 *     acc = acc + trans[i][j] * u[j] from 0.0 over j ascending; beta_t[i] = q[i] / c_{t+1}.
 *   Outputs.  gamma[t, i] = alpha_t[i] * beta_t[i], not renormalised (its rows sum to 1 within rounding); gamma[T - 1] = alpha_{T-1},
 *     no product.  scale[t] = c_t: the sum of their logarithms is the log-likelihood of the observations (plus the logarithms of
 *     whatever factors the caller took out of the rows of obs).
 * gamma holds alpha between the two sweeps: there is no workspace.  Every element of gamma [T, S] and scale [T] is written.  A frame
 * whose likelihoods are all zero gives c_t = 0 and IEEE NaN from that frame on in alpha and scale, and in all of gamma; nothing faults.
 *
 * Both: MAUA_EINVAL, without a launch and with the outputs untouched, on a NULL pointer, n_frames outside 1 .. MAUA_HMM_MAX_FRAMES,
 * n_states outside 1 .. MAUA_HMM_MAX_STATES.  No atomics, no workspace, no allocation or synchronisation: capturable, and the result is
 * a function of the arguments alone, bit for bit and run to run.  One workgroup each, a lane per state, the transition matrix staged
 * once in LDS: latency-bound by construction (one or two barriers per frame), like maua_pyin_viterbi_f64. */
#define MAUA_HMM_MAX_STATES 128
#define MAUA_HMM_MAX_FRAMES (1 << 22)
int maua_hmm_viterbi_f64(const float* logobs /*[n_frames, n_states]*/, const double* log_trans /*[n_states, n_states]*/,
                         const double* log_init /*[n_states]*/, int n_frames, int n_states, double* delta_last /*[n_states]*/,
                         uint8_t* backptr /*[n_frames, n_states]*/, int32_t* states /*[n_frames]*/, void* stream);
int maua_hmm_posterior_f64(const float* obs /*[n_frames, n_states]*/, const double* trans /*[n_states, n_states]*/,
                           const double* init /*[n_states]*/, int n_frames, int n_states, double* gamma /*[n_frames, n_states]*/,
                           double* scale /*[n_frames]*/, void* stream);

/* Bar-pointer model (audioreactive bar_viterbi / raw_bars / downbeats / metre / bar_phase / bar_beats; csrc/bar.hip; additive: the ABI
 * version is unchanged).  The most probable path through the hidden Markov model over (tempo, beat in the bar, position in the beat) of
 * Whiteley, Cemgil & Godsill (ISMIR 2006) on the state space of Krebs, Boeck & Widmer (ISMIR 2015), for n_models bar lengths in one
 * call, decoded WITHOUT writing the states out.  tests/bar_ref.py restates it in numpy, bit for bit, and expands it to the dense model
 * of maua_hmm_viterbi_f64 for comparison.
 *
 * Model.  K = n_tempi tempi, tempo k a beat of interval[k] envelope frames (strictly ascending integers in 1 .. MAUA_BAR_MAX_INTERVAL);
 * B = beats_per_bar[m] beats in the bar of model m.  A state is (k, b, j), b in 0 .. B - 1, j in 0 .. interval[k] - 1.  Transitions:
 * (k, b, j - 1) -> (k, b, j) with log-probability 0, and (k', (b - 1) mod B, interval[k'] - 1) -> (k, b, 0) with log_change[k'][k]
 * (row = source, float64, -inf legal); nothing else.  Every state starts with log-probability 0.  Observations: logobs [T, 3] fp32,
 * widened exactly, column 0 "no beat", 1 "beat", 2 "downbeat"; state (k, b, j) reads column c(b) = (b == 0 ? 2 : 1) when j < width[k]
 * and column 0 otherwise, 1 <= width[k] <= interval[k].
 *
 * Every operation is a float64 addition, subtraction or compare, in this order (T = n_frames):
 *   Prefix sums.  P_c[0] = 0, P_c[n + 1] = P_c[n] + logobs[n][c] for n = 0 .. T - 1 ascending, c = 0, 1, 2.
 *   A beat (k, b) entered at frame e (any sign), seen up to frame `end` exclusive:  a0 = max(e, 0), a1 = min(max(e + width[k], 0), end),
 *     seg(k, b, e, end) = (P_c(b)[a1] - P_c(b)[a0]) + (P_0[end] - P_0[a1]).
 *   Entry values.  V[e][k][b] = 0 for e <= 0 (the path began inside that beat).  For t = 1 .. T - 1 ascending:
 *     X[k'][b'] = V[t - interval[k']][k'][b'] + seg(k', b', t - interval[k'], t)      (leaving beat (k', b') behind frame t - 1)
 *     V[t][k][b]: best = X[0][b'] + log_change[0][k] with index 0, b' = (b - 1) mod B; then k' = 1 .. K - 1 ascending, the candidate
 *     X[k'][b'] + log_change[k'][k] replacing best (and the index) only when strictly greater: ties go to the lowest k', a NaN never
 *     replaces (and a NaN at k' = 0 is never replaced).  The index is the back pointer of (t, k, b).
 *   End.  Final value of state (k, b, j), with e = T - 1 - j:  V[e][k][b] + seg(k, b, e, T).  The final state is the first maximum in
 *     ascending (k, b, j): from best = -inf at state (0, 0, 0), a value replaces only when strictly greater (so a NaN is never chosen,
 *     and nothing but -inf and NaN ends in (0, 0, 0) with score -inf).  score[m] = that best.
 *   Walk back.  The final state (k, b, j) at frame t = T - 1 entered its beat at e = t - j: path[f] = (k, b, f - e) for f = max(e, 0)
 *     .. t.  While e > 0: k = the back pointer of (e, k, b), b = (b - 1) mod B, j = interval[k] - 1, t = e - 1, and again.
 * Every element of score [n_models] and path [n_models, T, 3] is written.  Work per frame: K * K * B additions.
 *
 * ws: maua_bar_ws_bytes(n_frames, n_tempi, max_beats, n_models) bytes of device memory, 16-byte aligned (the prefix sums, a byte of
 * back pointer per (t, k, b), the segment list of the walk back; per model, so that the workgroups share nothing); -1 for arguments
 * the entry refuses.  max_beats is the largest beats_per_bar.  maua_bar_lds_bytes(n_tempi, max_beats, max_interval): the LDS of the
 * launch — log_change at a row stride of K | 1 doubles, two buffers of K * max_beats exit values, a ring of max_interval entry values
 * per lane — or 0 where the counts are outside their limits or the plan is more than the 160 KiB of one CU.
 *
 * interval, width and beats_per_bar are HOST arrays, read during the call (they travel as kernel arguments); everything else is device
 * memory.  MAUA_EINVAL, without a launch and with the outputs untouched: a NULL pointer, n_frames outside 1 .. MAUA_BAR_MAX_FRAMES,
 * n_tempi outside 1 .. MAUA_BAR_MAX_TEMPI, n_models outside 1 .. MAUA_BAR_MAX_MODELS, an interval outside 1 .. MAUA_BAR_MAX_INTERVAL or
 * not above the one before, a width outside 1 .. interval, a beats_per_bar outside 1 .. MAUA_BAR_MAX_BEATS, n_tempi * max_beats >
 * 1024, maua_bar_lds_bytes(n_tempi, max_beats, interval[n_tempi - 1]) == 0.  No atomics, no allocation, no synchronisation, no copy:
 * capturable, and the result is a function of the arguments alone, bit for bit and run to run.  One workgroup per model, a lane per
 * (k, b), one barrier per frame: latency-bound by construction, like maua_hmm_viterbi_f64. */
#define MAUA_BAR_MAX_FRAMES (1 << 22)
#define MAUA_BAR_MAX_TEMPI 128
#define MAUA_BAR_MAX_BEATS 8          /* K * B <= 1024 lanes */
#define MAUA_BAR_MAX_INTERVAL 1024
#define MAUA_BAR_MAX_MODELS 8
int64_t maua_bar_lds_bytes(int n_tempi, int max_beats, int max_interval);
int64_t maua_bar_ws_bytes(int n_frames, int n_tempi, int max_beats, int n_models);
int maua_bar_viterbi_f64(const float* logobs /*[n_frames, 3]*/, int n_frames, const int32_t* interval /*host [n_tempi]*/,
                         const int32_t* width /*host [n_tempi]*/, const double* log_change /*[n_tempi, n_tempi]*/, int n_tempi,
                         const int32_t* beats_per_bar /*host [n_models]*/, int n_models, void* ws, double* score /*[n_models]*/,
                         int32_t* path /*[n_models, n_frames, 3]*/, void* stream);

/* Spectrogram factorisation (audioreactive nmf / decompose / components; csrc/nmf.hip; additive: the ABI version is unchanged).
 * Non-negative matrix factorisation V [F, T] ~ W [F, K] . H [K, T] under the generalised Kullback-Leibler divergence by multiplicative
 * updates (Lee & Seung 2000), in place, all fp32 and contiguous: V with frames contiguous, W contiguous in k, H contiguous in t.
 * One iteration, in this order:
 *   H step (update_h != 0):  P = max(W.H, eps);  R = V / P;  H[k,t] <- H[k,t] * (sum_f W[f,k] R[f,t]) / max(sum_f W[f,k], eps)
 *   W step (update_w != 0):  P = max(W.H, eps) with the new H;  R = V / P;
 *                            W[f,k] <- W[f,k] * (sum_t R[f,t] H[k,t]) / max(sum_t H[k,t], eps)
 * Every element of W.H is the chain p = fmaf(W[f,k], H[k,t], p) for k ascending from p = 0; the quotients are IEEE divisions; the update is
 * (old * sum) / denominator, in that order.  W.H and R are never stored.
 * maua_nmf_kl_f32 enqueues n_iter iterations on `stream`; it neither synchronises nor allocates (no workspace) and can be captured.
 * update_w = 0 keeps the dictionary fixed (activations only), update_h = 0 is the mirror case.  n_iter == 0 returns 0 without a launch.
 * No atomics and no reduction across workgroups: the results of a call are bit-identical from run to run, and n calls of one iteration
 * equal one call of n.
 * Zeros absorb, bit for bit (finite input): a zero H[k,t] or W[f,k] stays exactly zero; an all-zero column of V (a silent frame) gives an
 * exactly zero column of H after one H step; an all-zero column of W gives a zero row of H.
 * Non-finite input: with update_w = 0, a NaN or an infinity in V[f,t] changes column t of H only, every other column keeps its bits; with
 * both updates on it spreads everywhere (the callers refuse such input).
 * maua_nmf_kl_div_f32: d_cols[t] = sum_f (V log(V / P) - V + P) with 0 log 0 = 0, P the same fp32 max(W.H, eps) as in the update, the
 * terms and their sum in double; the divergence is the sum of the T numbers (the host adds them).
 * MAUA_EINVAL, without a launch: a null pointer, F, T or K < 1, K > MAUA_NMF_MAX_K, F * T >= 2^31, eps not finite or <= 0, n_iter < 0,
 * both update flags zero. */
#define MAUA_NMF_MAX_K 32
int maua_nmf_kl_f32(const float* v /*[F, T]*/, float* w /*[F, K]*/, float* h /*[K, T]*/, int F, int T, int K, int n_iter, int update_w,
                    int update_h, float eps, void* stream);
int maua_nmf_kl_div_f32(const float* v, const float* w, const float* h, int F, int T, int K, float eps, double* d_cols /*[T]*/,
                        void* stream);

/* Source separation by soft masks (audioreactive separate; csrc/separate.hip; additive: the ABI version is unchanged).
 * From a factorisation V ~ W.H of a magnitude spectrogram and the complex spectrogram re + i im it was taken from to the complex
 * spectrogram of every source ("stem"): component k belongs to stem group[k] in [0, G); a group may be empty.  Layouts as in
 * maua_nmf_kl_f32: re, im [F, T] with frames contiguous, W [F, K] contiguous in k, H [K, T] contiguous in t; out_re, out_im
 * [n_out, F, T], indexed in 64 bits.  `group` is a HOST array of K entries, read before the call returns and carried in the kernel
 * arguments: one launch on `stream`, no upload, no workspace, no allocation, no synchronisation; the call can be captured.
 * Per element (f, t), all fp32, in this order:
 *   P_g = 0; for k ascending with group[k] == g:  P_g = fmaf(W[f,k], H[k,t], P_g)
 *   q_g = P_g (power == 1, the ratio mask)  or  P_g * P_g (power == 2, the Wiener mask; one rounding)
 *   D   = 0; for g ascending from 0:  D = D + q_g            (always over all G groups, whatever the window)
 *   m_g = q_g / D (IEEE division) when D > 0, else 1.0f / G  (the equal split keeps the masks a partition of unity on silent bins;
 *                                                             a NaN D compares false and takes it too)
 *   out_re[g - g0, f, t] = m_g * re[f,t],  out_im[g - g0, f, t] = m_g * im[f,t]   for g0 <= g < g0 + n_out
 * Consequences (finite W and H):
 *   G == 1: the output equals the input bit for bit (q / q == 1 and 1 / 1 == 1);
 *   two calls give identical bits (no atomics, no reduction across lanes: an element depends on its own operands only);
 *   the call for a window (g0, n_out) gives the bits of the matching slices of the full call (g0 = 0, n_out = G);
 *   an all-zero column of H gives (1.0f / G) * re and (1.0f / G) * im in every stem, re / G exactly where G is a power of two;
 *   a non-finite value in re / im [f,t] or in H[:,t] changes column t only, one in W[f,:] row f only.
 * MAUA_EINVAL, without a launch: a null pointer, F, T or K < 1, K > MAUA_NMF_MAX_K, G outside 1 .. MAUA_SEPARATE_MAX_GROUPS,
 * F * T >= 2^31, power not 1 or 2, g0 < 0, n_out < 1, g0 + n_out > G, a group[k] outside [0, G). */
#define MAUA_SEPARATE_MAX_GROUPS 32 /* = MAUA_NMF_MAX_K */
int maua_nmf_separate_f32(const float* re, const float* im /*[F, T]*/, const float* w /*[F, K]*/, const float* h /*[K, T]*/,
                          const int32_t* group /*HOST array [K]*/, int F, int T, int K, int G, int power /*1 or 2*/, int g0, int n_out,
                          float* out_re, float* out_im /*[n_out, F, T]*/, void* stream);

/* Structural segmentation (audioreactive laplacian_segmentation, ABI 6).  Every entry is deterministic run to run.
 * Tempogram: the onset envelope env[n_frames] padded by win/2 with a linear ramp to 0, framed with hop 1 (n_frames frames), each
 * frame times a periodic Hann window of win samples, autocorrelated over lags 0 .. win-1 (fp64), divided by its max |.| (unless
 * that is below FLT_MIN), averaged over frames -> tg[win].  2 <= win <= 1024; ws holds maua_tempogram_ws_doubles() doubles. */
int64_t maua_tempogram_ws_doubles(int n_frames, int win);
int maua_tempogram_f32(const float* env, int n_frames, int win, double* ws, float* tg, void* stream);
/* Beat tracking (librosa.beat's dynamic programme, tightness 100): onset[n_frames] is the normalised envelope; localscore =
 * onset convolved ('same', zero padding) with exp(-0.5 (j 32 / period)^2), j = -period..period; then, frame by frame,
 * cumscore[i] = localscore[i] + max over w = -2 period .. -round(period/2) of -100 log(-w/period)^2 (+ cumscore[i + w] when
 * i + w >= 0), first maximum; backlink[i] = i + w of that maximum, or -1 while no frame has yet reached 0.01 max(localscore).
 * 2 <= period <= 2000. */
int maua_beat_track_f64(const double* onset, int n_frames, int period, double* localscore, double* cumscore, int* backlink,
                        void* stream);
/* Beat-synchronous aggregation: out[r][s] = np.median (median = 1) or mean (median = 0) of x[r][bounds[s] .. bounds[s+1]) for
 * x[rows, n_frames]; bounds[n_spans + 1] increasing inside [0, n_frames] (clamped there: a bound outside [0, n_frames] is moved to
 * the nearer end, a bound below an earlier one is raised to it; an empty span gives NaN).  Spans of any length. */
int maua_beat_sync_f32(const float* x, int rows, int n_frames, const int* bounds, int n_spans, int median, float* out, void* stream);
/* k-nearest-neighbour links of the columns of x[d, s] (d <= 1024, 2 <= s <= 8192): row i links the k columns j with |i - j| >= width
 * of smallest fp32 Euclidean distance (ties to the lower j); links[i][j] = that distance on a link, -1 elsewhere.  The squares are summed
 * feature by feature, so the distance of (i, j) and of (j, i) are equal bit for bit. */
int maua_knn_links_f32(const float* x, int d, int s, int k, int width, float* links, void* stream);
/* Recurrence affinity from those links (4 <= s <= 8192): rec[i][j] = exp(-dist / bandwidth) where i links j and j links i, 0 elsewhere;
 * rec_filt = librosa timelag_filter(median_filter, size=(1, 7)) of rec: rec_filt[i][j] = median over s = -3..3 of rec[i - j + j'][j'],
 * j' = j + s reflected at the edges (d c b a | a b c d), 0 for a row outside [0, s). */
int maua_rec_affinity_f32(const float* links, int s, float bandwidth, float* rec, float* rec_filt, void* stream);

/* Recursive (IIR) filters (audioreactive filters: sosfilt, sosfiltfilt, bandpass, bands, envelope; csrc/iir.hip; additive: the ABI
 * version is unchanged).
 *
 * maua_sosfilt_f64: n_filters (F) filters in one call, each a cascade of n_sections second-order sections sos [F, n_sections, 6] in
 * scipy's layout [b0 b1 b2 a0 a1 a2]; a0 is taken as 1 and never read (the caller normalises).  Filter f runs over its own signal
 * x[f, 0 .. n) (n_signals == F) or all filters over one signal (n_signals == 1, the filter bank).  Exactly one of x_f32 / x_f64 is set
 * (a float sample is widened exactly); y_f64 and / or y_f32 [F, n] receive the result, y_f32 the round-to-nearest-even of the double that
 * y_f64 receives.  zi / zf [F, n_sections, 2] are the optional initial / final states (z1, z2) of every section; zi == NULL starts from 0.
 * Per sample, section by section (the input of section s + 1 is the y of section s), every operation in double, each line ONE rounding:
 *     y  = fma(b0, x, z1)
 *     z1 = fma(-a1, y, fma(b1, x, z2))
 *     z2 = fma(-a2, y, b2 * x)
 * which is scipy.signal.sosfilt's transposed direct form II  y = b0 x + z1;  z1 = b1 x - a1 y + z2;  z2 = b2 x - a2 y  with fused roundings.
 * Time is cut into nc = ceil(n / chunk) chunks of `chunk` samples (the last may be shorter); chunk == 0 selects
 * maua_sosfilt_default_chunk(n).  With D = 2 n_sections and the state vector (z1, z2 of section 0, z1, z2 of section 1, ...):
 *   1. A [D, D] per filter: column j is the state after `chunk` samples of zero input from the unit state e_j (the recurrence above);
 *   2. Z_c, c < nc - 1: the state after chunk c filtered from the zero state;
 *   3. S_0 = zi (or 0);  S_{c+1}[i] = acc + Z_c[i]  with  acc = 0;  acc = fma(A[i][j], S_c[j], acc)  for j ascending;
 *   4. chunk c is filtered again from S_c and y is written; zf is the state after the last sample.
 * Exact in exact arithmetic, whatever the chunk length; the order above is fixed, nothing is reduced across lanes and there are no
 * atomics, so two calls give identical bits (a result does depend on `chunk`, in its last bits).  A NaN in x[t] leaves every output before
 * t with the bits of the NaN-free call and, for a filter whose b0 are non-zero, makes every output from t on a NaN.
 * ws: maua_sosfilt_ws_doubles(F, n_sections, n, chunk) doubles of device memory (A, Z and S; -1 for arguments the entry refuses).  The
 * entry enqueues four launches on `stream` (two where nc == 1), never allocates, never synchronises and can be captured.  n == 0 is a
 * successful no-op that sets zf = zi (0 without zi).
 * maua_sosfilt_default_chunk(n): the smallest power of two p in [64, 4096] with MAUA_SOS_CHUNK_BALANCE p^2 >= n (4096 beyond): the
 * serial carry costs time per chunk, the passes per sample of a chunk, and their sum is least near chunk = sqrt(n / 4) as measured
 * (DESIGN.md 4.22); this is the power of two nearest to it in ratio: 64 up to 32 768 samples, 1024 for 2.1 M .. 8.4 M (a 240 s clip).
 * MAUA_EINVAL, without a launch: n_sections outside 1 .. MAUA_SOS_MAX_SECTIONS, F outside 1 .. MAUA_SOS_MAX_FILTERS, n_signals not 1 or F,
 * n < 0, chunk < 0 or > MAUA_SOS_MAX_CHUNK, both or neither of x_f32 / x_f64, neither y_f64 nor y_f32, a null sos or ws. */
#define MAUA_SOS_MAX_SECTIONS 16
#define MAUA_SOS_MAX_FILTERS 64
#define MAUA_SOS_MAX_CHUNK 65536
#define MAUA_SOS_CHUNK_BALANCE 8
int maua_sosfilt_default_chunk(int n);
int64_t maua_sosfilt_ws_doubles(int n_filters, int n_sections, int n, int chunk);
/* maua_sosfilt_plan: what a maua_sosfilt_f64 call with these shape arguments does, computed on the host from the entry's own constants
 * and checks; nothing is launched and no device is needed (the tests prove with it what their case lists reach).  MAUA_EINVAL where the
 * entry refuses the same four arguments (n_sections, F, n, chunk as listed above) and for a null out; else 0 and
 *   out[0] the chunk length used (maua_sosfilt_default_chunk(n) for chunk == 0);   out[1] nc = ceil(n / out[0]);
 *   out[2] launches: 4, 2 where nc == 1, and at n == 0 the one that sets zf (none where zf == NULL);
 *   out[3] workgroups per filter of the zero-state pass, ceil((nc - 1) / 64): a lane per chunk before the last (0: no such launch);
 *   out[4] workgroups per filter of the final pass, ceil(nc / 64);
 *   out[5] 16-sample tiles a lane walks through a full chunk, ceil(out[0] / 16);   out[6] samples in the last of them, 1 .. 16;
 *   out[7] length of the last chunk, 1 .. out[0] (0 at n == 0). */
int maua_sosfilt_plan(int n_filters, int n_sections, int n, int chunk, int32_t* out /*[8]*/);
int maua_sosfilt_f64(const double* sos /*[F, n_sections, 6]*/, int n_filters, int n_sections, const float* x_f32, const double* x_f64,
                     int n_signals /*1 or F*/, int n, int chunk, const double* zi, double* y_f64, float* y_f32, double* zf, double* ws,
                     void* stream);
/* maua_env_follow_f32: attack / release envelope follower over x [n_frames, n_cols] (frames outermost), one lane per column:
 *     d = x[t] - y[t-1];  k = x[t] > y[t-1] ? attack_coef : release_coef;  p = k * d;  y[t] = y[t-1] + p
 * three float32 operations — a subtraction, a product, a sum — each rounded to nearest once and never fused (the kernel is compiled
 * with `#pragma clang fp contract(off)`; the __fmul_rn / __fadd_rn intrinsics are not enough, the compiler fuses them into an fma), so a
 * numpy float32 restatement gives the same bits.  y[-1] = y0[col] where
 * y0 is given, else x[0][col] (so y[0] = x[0]).  A NaN in x[t] makes the comparison false: the release branch is taken and the NaN
 * stays in that column from t on (other columns keep their bits).  y must not overlap x.  n_frames == 0 is a successful no-op.
 * MAUA_EINVAL, without a launch: a null x or y, n_frames < 0, n_cols < 1, a coefficient outside [0, 1] or NaN. */
int maua_env_follow_f32(const float* x, const float* y0 /*[n_cols] or NULL*/, float* y, int n_frames, int n_cols, float attack_coef,
                        float release_coef, void* stream);

/* 3-D tileable Perlin noise (audioreactive/latent.py:188-246): grad [r0+1,r1+1,r2+1,3] -> out [n0,n1,n2]. */
int maua_perlin3d_f32(const float* grad, float* out, int n0, int n1, int n2, int r0, int r1, int r2, void* stream);

/* Looping latent sequences (additive to ABI 8; audioreactive/latent.py spline_loops, slerp_loops, loop_sections; csrc/latent_loops.hip).
 * A cubic-spline or great-circle loop through a set of keys is linear in the keys once the knot count and period (the leg angles) are
 * fixed, so a whole sectioned sequence is one gather-and-blend over a bank of keys:
 *   out[f, :] = sum_i weights[row_of_frame[f], i] * bank[key_idx[sec_of_frame[f], i], :]
 * bank [n_bank, feats], key_idx [n_sections, kmax] (int32 rows of bank), weights [n_rows, kmax] (columns a section does not use hold 0),
 * row_of_frame / sec_of_frame [n_frames] (int32), out [n_frames, feats].  Per element the sum is the chain acc = fmaf(w_i, key_i, acc) for
 * i ascending from acc = 0, in which a weight that is exactly 0 leaves acc as it is: a frame's bits depend on its weight row and its keys
 * alone, not on kmax, the tables around it, the tile or the launch.  16-byte loads and stores where feats % 4 == 0 and bank and out are
 * 16-byte aligned, element by element otherwise, with the same bits.  Indices found in the tables are clamped into their tables on the
 * device.  n_frames == 0 is a successful no-op; MAUA_EINVAL, without a launch, on a null pointer, a non-positive size or kmax >
 * MAUA_LOOP_MAX_KEYS. */
#define MAUA_LOOP_MAX_KEYS 32
int maua_keyframe_blend_f32(const float* bank, int n_bank, int feats, const int* key_idx, const float* weights, const int* row_of_frame,
                            const int* sec_of_frame, float* out, int n_frames, int n_sections, int n_rows, int kmax, void* stream);

/* Network-bending warp (audioreactive/bend.py:52-102): per-frame inverse affine map m[b] = {a00,a01,a02,a10,a11,a12}
 * (output pixel -> source pixel, in pixels), bilinear sampling of the reflect-padded source, zeros outside the padded
 * canvas (kornia warp_affine default padding_mode='zeros', align_corners as encoded by the host in m). */
int maua_affine_reflect_warp_f32(const float* x, const float* m, float* y, int batch, int channels, int h, int w,
                                 int pad_l, int pad_r, int pad_t, int pad_b, const float* add_noise, void* stream);
/* Same, for a canvas built by a CHAIN of ReflectionPad2d (audioreactive/bend.py:60-64 stacks three): pad_* are the total
 * paddings, xmap[w+pad_l+pad_r] / ymap[h+pad_t+pad_b] (int32, device, either may be NULL = single fold) give the source
 * column / row of every canvas column / row.  src != NULL: m is the map SEQUENCE of the whole render [n_frames, 6] and sample
 * b uses row src->frame0 + b (render.py:151-158 rebuilds the transform per batch; a captured graph reads it per replay). */
int maua_affine_reflect_warp_mapped_f32(const float* x, const float* m, float* y, int batch, int channels, int h, int w,
                                        int pad_l, int pad_r, int pad_t, int pad_b, const float* add_noise,
                                        const int* xmap, const int* ymap, const maua_frame_source_t* src, void* stream);

/* Point and morphological network bends (ABI 8; csrc/bend_ops.hip) — the transforms of Broad, Leymarie and Grierson, "Network Bending:
 * Expressive Manipulation of Deep Generative Models" (2020) that are not affine warps, each on a chosen subset of a layer's channels
 * (audioreactive/bend.py: Ablate, Invert, ScalarMultiply, BinaryThreshold, Erode, Dilate).  x, y [batch, channels, ...] fp32;
 * chan_mask[channels] (uint8, device): channel c is transformed where chan_mask[c] != 0 and copied through unchanged elsewhere; NULL = every
 * channel.  Per-frame parameter tables (`param` / `radius`, device, `rows` entries) work as the map sequence of
 * maua_affine_reflect_warp_mapped_f32: rows == 1: every sample uses row 0; src != NULL: sample b uses row src->frame0 + b, read on the
 * device (one captured launch serves every replay; the caller guarantees the table covers it); src == NULL: sample b uses row b, rows ==
 * batch.  batch <= 64, channels <= 65535, planes below 2 GiB; MAUA_EINVAL on null or non-positive arguments or an unknown op.
 *
 * Point ops on planes of hw elements:  op 0 ablate: 0;  1 invert: 1 - x;  2 scalar multiply: x * p;  3 binary threshold: x > p ? 1 : 0
 * (a NaN compares false).  param may be NULL for ops 0 and 1.  y == x is allowed. */
int maua_bend_point_f32(const float* x, float* y, int batch, int channels, int64_t hw, int op, const float* param, int param_rows,
                        const uint8_t* chan_mask, const maua_frame_source_t* src, void* stream);
/* Morphological ops:  op 0 erode / 1 dilate = minimum / maximum over the (2r + 1) x (2r + 1) window centred on the pixel, window positions
 * outside the map ignored: -max_pool2d(-x, 2r + 1, 1, r) / max_pool2d(x, 2r + 1, 1, r), bit for bit (-0 and +0 tie).  r = radius[row]
 * clamped on the device to 0 .. MAUA_BEND_MAX_RADIUS; r = 0 is the identity.  A NaN stays inside the windows that contain it.  Any
 * h, w >= 1.  The window is separable: one launch takes the extremum along rows, then along columns, on an LDS tile with a halo of
 * MAUA_BEND_MAX_RADIUS.  y == x is refused (MAUA_EINVAL). */
#define MAUA_BEND_MAX_RADIUS 16
int maua_bend_morph_f32(const float* x, float* y, int batch, int channels, int h, int w, int op, const int32_t* radius, int radius_rows,
                        const uint8_t* chan_mask, const maua_frame_source_t* src, void* stream);
/* Padding bend (additive to ABI 8; audioreactive/bend.py: Pad): y [batch, channels, h + pad_t + pad_b, w + pad_l + pad_r] =
 * torch.nn.functional.pad(x, (pad_l, pad_r, pad_t, pad_b), mode, value) + noise — the layer-0 transform that widens the 4 x 4 constant to
 * the 4 x 8 (8 x 4) one of a 1920 (1080) render.  mode 0 constant (filled with `value`), 1 replicate, 2 reflect (every pad < its axis),
 * 3 circular (every pad <= its axis); the four pads are independent and >= 0.  noise: NULL, or a static plane [noise_channels, padded h,
 * padded w] with noise_channels 1 (shared by the channels) or `channels`, added with one fp32 add: the result is bit-defined, a NaN or
 * an infinity of x or `value` is carried through.  Nothing is per frame, so there is no frame source: a captured launch is static.
 * 16-byte stores where the padded width is a multiple of 4 and y (and noise) are 16-byte aligned, element by element otherwise.
 * batch <= 64, channels <= 65535, planes below 2 GiB; y == x is refused.  MAUA_EINVAL on null or non-positive arguments, a negative pad, an
 * unknown mode, a reflect / circular pad beyond its limit, or a noise_channels other than 1 / channels. */
int maua_bend_pad_f32(const float* x, float* y, int batch, int channels, int h, int w, int pad_l, int pad_r, int pad_t, int pad_b,
                      int mode, float value, const float* noise, int noise_channels, void* stream);
/* Coordinate-remap bends (additive to ABI 8; csrc/bend_remap.hip; audioreactive/bend.py: Mirror, Kaleidoscope, Swirl, Ripple, Displace):
 * y[b, c, oy, ox] = x[b, c] sampled bilinearly at a source coordinate s(b, oy, ox) on the selected channels, the others copied through.
 * chan_mask, param_rows and src select channels and parameter rows exactly as in maua_bend_point_f32: param [param_rows,
 * MAUA_BEND_REMAP_PARAMS]; param_rows == 1: every sample uses row 0; src != NULL: sample b uses row src->frame0 + b, read on the device;
 * otherwise row b, param_rows == batch.
 *
 * Coordinates.  Output pixel o = (ox, oy), centre c = ((w - 1) / 2, (h - 1) / 2), d = o - c, r = |d|; angles in radians; row p[0..3]:
 *   op 0 mirror        n = (p0, p1) a unit normal (from the host), t = d . n - p2;  s = o - 2 t n where t < 0, s = o elsewhere
 *   op 1 kaleidoscope  N = clamp(rint(p0), 1, 64), ws = 2 pi / N;  a = atan2(dy, dx) - p1;  a -= ws floor(a / ws);  a = ws - a where
 *                      a > ws / 2;  a += p1 + p2;  s = c + r (cos a, sin a)
 *   op 2 swirl         phi = p0 exp(-r / p1);  s = c + (cos phi dx - sin phi dy, sin phi dx + cos phi dy)
 *   op 3 ripple        k = p0 sin(2 pi (r / p1 - p2));  s = o + k d / r  (s = o at r = 0)
 *   op 4 displace      s = o + p0 D(o, p1).  field [field_frames, 2, field_h, field_w] holds (dx, dy) planes of a looping bank, sampled
 *                      bilinearly at u = ox (field_w - 1) / (w - 1), v = oy (field_h - 1) / (h - 1) (0 along a map axis of length 1);
 *                      t = floor(p1), ft = p1 - t, t0 = t mod field_frames (non-negative), t1 = (t0 + 1) mod field_frames;
 *                      D = (1 - ft) field[t0] + ft field[t1]: a fractional loop position blends neighbouring frames.
 * Sampling.  s is folded per axis into [0, n - 1]: border 0 reflects without repeating the edge (period 2 (n - 1); an axis of length 1
 * gives 0), border 1 clamps; then x0 = floor(s), x1 = min(x0 + 1, n - 1) and the bilinear blend — grid_sample(mode="bilinear",
 * padding_mode="reflection" | "border", align_corners=True) on pixel coordinates.  The blend is held inside the range of its four taps,
 * so an output never leaves the range of its source plane; a NaN tap gives a NaN.
 * Bad rows.  A row with a NaN or an infinity among the parameters its op uses, or with p1 <= 0 for swirl or ripple, leaves its sample
 * unchanged (y = x, every channel).  Every finite row, however large, keeps every load inside x and field: the folded coordinate and
 * the integer taps are clamped.
 * The coordinate, the tap offsets and the weights are computed once per (sample, pixel) and reused over a chunk of channels.
 * batch <= 64, channels <= 65535, planes (of x and of field) below 2 GiB, any h, w >= 1; y == x is refused (a gather).  MAUA_EINVAL,
 * without a launch, on null or non-positive arguments, an unknown op or border, or op 4 without a field or with a non-positive field
 * size; field is ignored by ops 0 .. 3. */
#define MAUA_BEND_REMAP_PARAMS 4
int maua_bend_remap_f32(const float* x, float* y, int batch, int channels, int h, int w, int op, int border,
                        const float* param, int param_rows,                             /* [param_rows, 4] */
                        const float* field, int field_frames, int field_h, int field_w, /* op 4 only: [F, 2, fh, fw] (dx, dy planes) */
                        const uint8_t* chan_mask, const maua_frame_source_t* src, void* stream);

/* ------------------------------------------------------------------------------------------------ hipGraph runtime
 * Capture everything launched on `stream` between begin/end into a hipGraph and replay it (per-frame generator
 * forward, north_star "hipGraph-captured").  Handles are opaque. */
int maua_graph_begin_capture(void* stream);
int maua_graph_end_capture(void* stream, void** graph_exec_out);
int maua_graph_launch(void* graph_exec, void* stream);
int maua_graph_destroy(void* graph_exec);

/* HIP-event timing on an arbitrary stream (bench.py roofline leg; torch.cuda.Event only sees torch's stream). */
int maua_event_create(void** ev);
int maua_event_record(void* ev, void* stream);
int maua_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms);
int maua_event_destroy(void* ev);

#ifdef __cplusplus
}
#endif
#endif /* MAUA_HIP_H */
