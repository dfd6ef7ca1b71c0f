/*
 * trg_denoise.h -- first-hit guide buffers and an edge-avoiding a-trous denoiser for the low sample counts the renderer is used at
 * (Dammertz, Sewtz, Hanika, Lensch: "Edge-Avoiding A-Trous Wavelet Transform for fast Global Illumination Filtering", HPG 2010).
 * Part of libtoyraygun_hip.so; an addition beside trg.h (the reference has no denoiser).  Same conventions: plain pointers and sizes, TRG_OK
 * or a negative error code, trg_last_error() has the message.  Every image here is width*height float4, row 0 = the scene's bottom, like the
 * accumulation buffer.  `*_device` pointers are device memory of the context's device; everything is enqueued on the context's CURRENT
 * stream (trg_set_stream) and nothing waits for the device, unless a function says so.
 *
 * STATE.  The first call allocates per-context scratch (primary rays and hit records of the guide pass, two ping-pong images of the filter);
 * it is grow-only and lives until trg_denoise_release(ctx).  trg_destroy does NOT know about it: call trg_denoise_release BEFORE trg_destroy.
 */
#ifndef TRG_DENOISE_H
#define TRG_DENOISE_H

#include "trg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TRG_DENOISE_MAX_ITERATIONS 6

typedef struct trg_denoise_params {
    int32_t iterations;  /* 0 .. TRG_DENOISE_MAX_ITERATIONS; default 5 */
    float sigma_color;   /* default 4.0 */
    float sigma_normal;  /* default 128 */
    float sigma_depth;   /* default 1.0 */
    int32_t demodulate;  /* default 1 */
} trg_denoise_params;
TRG_API void trg_denoise_default_params(trg_denoise_params *p);

/* --- GUIDES: the first-hit features of the primary rays of ONE frame index -- exactly the rays trg_raygen produces for that index (mask 3,
 *     maxDistance infinite), nearest hit, by the strict or the shipped intersector as TRG_OPT_STRICT says, for a scene staged in LDS or
 *     traversed from HBM alike.  guides_device: TWO planes of width*height float4, G0 then G1:
 *       G0 = (shading normal xyz, hit distance)          distance < 0: the ray missed (then G0 = (0, 0, 0, -1))
 *       G1 = (albedo rgb, primitive index as int32 bits) index -1 and albedo 0 on a miss
 *     Normal and albedo are the vertex attributes interpolated as the shader's interpolateVertexAttribute does (Raytracing.metal:95-112):
 *     with c0, c1 = trg_isect.coordinates and c2 = 1 - c0 - c1, value = c0 * A0 + c1 * A1 + c2 * A2 in fp32, not normalised.  With textures
 *     loaded (trg_load_textures) the albedo of a MATERIAL_DEFAULT hit is multiplied by its texel; the albedo of an emissive primitive is (1, 1, 1).
 *     The guide rays go through the stage-level tracer (trg_trace's kernels), which does not count rays: trg_get_stats is unchanged. */
TRG_API int trg_guides_render(trg_ctx *ctx, uint32_t frameIndex, void *guides_device);

/* --- THE FILTER.  color_in_device, out_device: width*height float4 (they must not overlap); guides_device as above.
 *
 *  Notation: pixel p = (x, y); C(p) the rgb of the input, n_p = G0(p).xyz, z_p = G0(p).w, a_p = G1(p).rgb.  p is a MISS when z_p < 0 -- and,
 *  for the filter, also when its first hit is an EMITTER: G1(p).w names a primitive of the context's loaded scene whose material is
 *  TRG_MATERIAL_EMISSIVE (an index outside the scene, or no scene: not an emitter).  A light seen directly carries no noise, and next to the
 *  surface it is mounted on neither normal nor depth tells it apart, so it is kept out of the filter like the background: it copies its
 *  input and is nobody's tap.  Everywhere below "miss" means both, and z of such a pixel counts as negative.
 *
 *  iterations == 0: out = color_in, bit for bit.  Otherwise, with N = iterations:
 *   1. I_0(p) = C(p) / max(a_p, 1e-3) per channel when `demodulate` and p is not a miss, else C(p).
 *   2. For i = 0 .. N-1, with spacing s = 2^i:  a miss pixel copies: I_{i+1}(p) = I_i(p).  Any other pixel:
 *          I_{i+1}(p) = sum_q w(p,q) I_i(q) / sum_q w(p,q)      (if the sum of weights is not > 0: I_i(p))
 *      over the 25 taps q = p + s * (dx, dy), dx, dy in {-2 .. 2}, that lie INSIDE the image (taps outside are skipped, not clamped), with
 *          w(p,q) = h(dx) h(dy) * w_n * w_z * w_c * w_id,       h = (1/16, 1/4, 3/8, 1/4, 1/16) for offsets -2 .. 2  (B3 spline)
 *          w_id = 0 when q is a miss, else 1
 *          w_n  = 0 when n_p . n_q <= 0, else (n_p . n_q) ^ sigma_normal
 *          w_z  = exp(-|z_p - z_q| / (sigma_depth * (g_p * s * sqrt(dx^2 + dy^2) + 1e-6)))
 *                 g_p = sqrt(gx^2 + gy^2); gx = z(x+1, y) - z(x, y) if (x+1, y) is inside the image and not a miss, else z(x, y) - z(x-1, y)
 *                 if (x-1, y) is inside and not a miss, else 0; gy likewise along y
 *          w_c  = exp(-|I_i(p) - I_i(q)|^2 / (sigma_color^2 * (var_p + 1e-4)))         (squared distance over r, g, b)
 *                 var_p = (1/m) sum_r (L(r) - mean)^2, mean = (1/m) sum_r L(r), over the m pixels r of the 3 x 3 window around p (spacing 1,
 *                 whatever the iteration) that lie inside the image, misses included; L = 0.2126 r + 0.7152 g + 0.0722 b of I_i
 *   3. out(p).rgb = I_N(p) * max(a_p, 1e-3) when `demodulate` and p is not a miss, else I_N(p).   out(p).a = color_in(p).a for every pixel.
 *
 *  Arithmetic is fp32 without contraction in both settings.  TRG_OPT_STRICT 1: expf / powf / sqrtf of the math library; 0 (shipped): the
 *  hardware's exp2 / log2 (__expf, __powf).  The float64 reference of this definition: toyraygun_amd/denoise.py reference_denoise.
 *
 *  On the device: one launch per iteration over 16 x 16-pixel tiles of 256 threads.  Spacings 1 and 2 stage the tile and its halo (up to
 *  24 x 24 pixels of colour and G0) in LDS; from spacing 4 on the halo is larger than the tile and the taps are read through L2.
 *  Demodulation is part of the first launch (while staging) and remodulation of the last (before the store).  One streaming launch in front
 *  writes the filter's copy of G0 with the emitters marked as misses. */
TRG_API int trg_denoise(trg_ctx *ctx, const void *color_in_device, const void *guides_device, void *out_device, const trg_denoise_params *p /* NULL: defaults */);

/* --- trg_render(frameIndexBegin, spp, bounces) over the whole image, trg_guides_render(frameIndexBegin) into the state's own guide planes,
 *     trg_denoise from the context's accumulation buffer (as bound: trg_bind_accum) into out_device.  One stream; the accumulation buffer
 *     is only read, so progressive accumulation goes on from it as if nothing had happened.  With TRG_OPT_TIMING on, trg_render waits for
 *     its own kernels as always; the two passes behind it are only enqueued. */
TRG_API int trg_render_denoised(trg_ctx *ctx, uint32_t frameIndexBegin, uint32_t spp, uint32_t bounces, void *out_device, const trg_denoise_params *p);

/* --- for callers without device memory of their own (the engine plugin): guides of frameIndex, then the filter from the context's accumulation
 *     buffer (as bound) into an image the STATE owns; *out_device = that image (width*height float4, valid until the next call of this
 *     function or trg_denoise_release).  Only enqueues.  To tone-map it: trg_bind_accum(ctx, *out_device), trg_postprocess, bind back. */
TRG_API int trg_denoise_accum(trg_ctx *ctx, uint32_t frameIndex, const trg_denoise_params *p, void **out_device);

/* frees the context's denoise state (waits for the device first).  Harmless without one.  Call before trg_destroy. */
TRG_API int trg_denoise_release(trg_ctx *ctx);

/* --- the same three with HOST buffers (tests, scripts, the plugin's PNG path): temporary device copies on the context's stream, and they
 *     WAIT for the result.  guides_host: 2 * width*height*4 floats; colour and out: width*height*4 floats. */
TRG_API int trg_guides_read(trg_ctx *ctx, uint32_t frameIndex, float *guides_host);
TRG_API int trg_denoise_host(trg_ctx *ctx, const float *color_in_host, const float *guides_host, float *out_host, const trg_denoise_params *p);
TRG_API int trg_render_denoised_read(trg_ctx *ctx, uint32_t frameIndexBegin, uint32_t spp, uint32_t bounces, float *out_host, const trg_denoise_params *p);

#ifdef __cplusplus
}
#endif
#endif /* TRG_DENOISE_H */
