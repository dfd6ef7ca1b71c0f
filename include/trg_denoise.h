/*
 * trg_denoise.h -- first-hit guide buffers and an edge-avoiding a-trous denoiser for the low sample counts the renderer is used at
 * (Dammertz, Sewtz, Hanika, Lensch: "Edge-Avoiding A-Trous Wavelet Transform for fast Global Illumination Filtering", HPG 2010).
 * Part of libtoyraygun_hip.so; an addition beside trg.h (the reference has no denoiser).  Same conventions: plain pointers and sizes, TRG_OK
 * or a negative error code, trg_last_error() has the message.  Every image here is width*height float4, row 0 = the scene's bottom, like the
 * accumulation buffer.  `*_device` pointers are device memory of the context's device; everything is enqueued on the context's CURRENT
 * stream (trg_set_stream) and nothing waits for the device, unless a function says so.
 *
 * STATE.  The first call allocates per-context scratch (primary rays and hit records of the guide pass, two ping-pong images of the filter;
 * the half-sample images of the variance-guided path and the history planes of the temporal path on their first use); it is grow-only and
 * belongs to the context: trg_destroy frees it, and trg_denoise_release(ctx) remains for freeing it earlier.
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

/* frees the context's denoise state early (waits for the device first); trg_destroy frees it too.  Harmless without one. */
TRG_API int trg_denoise_release(trg_ctx *ctx);

/* --- the same three with HOST buffers (tests, scripts, the plugin's PNG path): temporary device copies on the context's stream, and they
 *     WAIT for the result.  guides_host: 2 * width*height*4 floats; colour and out: width*height*4 floats. */
TRG_API int trg_guides_read(trg_ctx *ctx, uint32_t frameIndex, float *guides_host);
TRG_API int trg_denoise_host(trg_ctx *ctx, const float *color_in_host, const float *guides_host, float *out_host, const trg_denoise_params *p);
TRG_API int trg_render_denoised_read(trg_ctx *ctx, uint32_t frameIndexBegin, uint32_t spp, uint32_t bounces, float *out_host, const trg_denoise_params *p);

/* =============================================================================================================================================
 * VARIANCE-GUIDED FILTERING FROM TWO HALF-SAMPLE BUFFERS (after SVGF: Schied et al., "Spatiotemporal Variance-Guided Filtering", HPG 2017).
 * The colour weight of trg_denoise is scaled by a SPATIAL variance, which cannot tell a shadow boundary from noise.  Here the frames of one
 * batch are rendered as two independent halves; their difference is an unbiased estimate of the variance of their mean, and the filter carries
 * that variance through its iterations, so it narrows as the noise goes down.
 * ============================================================================================================================================= */

/* --- HALVES.  n = spp must be even and >= 2 (and frameIndexBegin + n <= 2^32 - 1), else TRG_ERR_INVALID.  halves_device: TWO planes of
 *     width*height float4, H1 then H2; it must not overlap the bound accumulation buffer.  With b = frameIndexBegin:
 *       a zeroed image A of the state is bound (trg_bind_accum) and trg_render(b, n/2, bounces) runs over the whole image,
 *       a second zeroed image B is bound and trg_render(b + n/2, n/2, bounces) runs,
 *       the caller's binding is restored: the caller's accumulation buffer is never written.
 *     From a zeroed buffer the running average leaves (sum of the samples) / (b + n/2) in A and / (b + n) in B; one streaming kernel scales
 *       H1.rgb = A.rgb * f1,  f1 = fl((b + n/2) / (n/2))        H2.rgb = B.rgb * f2,  f2 = fl((b + n) / (n/2))
 *     (the quotient formed in double precision and rounded to fp32; ONE fp32 multiply per channel; for b = 0 the factors are 1 and 2 and the
 *     scaling is exact), alpha copied: H1, H2 = the means of the two halves' samples.
 *     Both renders are REAL renders on the context's current stream: trg_get_stats counts their rays (n frames in all), `renders` goes up by
 *     two, and with TRG_OPT_TIMING on each waits for its kernels as trg_render always does. */
TRG_API int trg_render_halves(trg_ctx *ctx, uint32_t frameIndexBegin, uint32_t spp, uint32_t bounces, void *halves_device);

typedef struct trg_denoise_var_params {
    int32_t iterations;  /* 0 .. TRG_DENOISE_MAX_ITERATIONS; default 5 */
    float sigma_lum;     /* default 4.0 */
    float sigma_normal;  /* default 128 */
    float sigma_depth;   /* default 1.0 */
    int32_t demodulate;  /* default 1 */
    int32_t prefilter;   /* default 1 */
} trg_denoise_var_params;
TRG_API void trg_denoise_var_default_params(trg_denoise_var_params *p);

/* --- THE VARIANCE-GUIDED FILTER.  halves_device: H1, H2 as above; guides_device as for trg_denoise; out_device: width*height float4, must not
 *     overlap the halves.  Notation, misses and emitters, the taps and h, w_n, w_z, w_id: exactly as for trg_denoise above.
 *
 *   Start.  D(X)(p) = X(p).rgb / max(a_p, 1e-3) per channel when `demodulate` and p is not a miss, else X(p).rgb.
 *          I_0(p) = 0.5 * (D(H1)(p) + D(H2)(p))
 *          V_0(p) = 0.25 * (L(D(H1)(p)) - L(D(H2)(p)))^2           a miss pixel has V_0 = 0
 *   Prefilter (when `prefilter`; one degree of freedom is too noisy an estimate on its own).  For p not a miss, V_0(p) is replaced by
 *          sum_q g(p,q) V_0(q) / sum_q g(p,q)                      (if the sum of g is not > 0: V_0(p) stays)
 *      over the 49 pixels q = p + (dx, dy), dx, dy in {-3 .. 3}, inside the image, with g = w_n * w_z * w_id at s = 1 (no B3 factor, no colour
 *      term; the V_0 on the right are all the un-prefiltered ones).
 *   Iteration i = 0 .. N-1, spacing s = 2^i.  A miss pixel copies I and V.  Any other pixel, over the 25 taps inside the image:
 *          w(p,q) = h(dx) h(dy) * w_n * w_z * w_l * w_id
 *          w_l = exp(-|L(I_i(p)) - L(I_i(q))| / (sigma_lum * sqrt(max(0, GV_i(p))) + 1e-3))
 *                GV_i(p) = sum_r b(r) V_i(r) / sum_r b(r) over the pixels r of the 3 x 3 window around p (spacing 1) that lie inside the image and
 *                are not misses, b = (1/4, 1/2, 1/4) along each axis
 *          I_{i+1}(p) = sum_q w I_i(q) / sum_q w          V_{i+1}(p) = sum_q w^2 V_i(q) / (sum_q w)^2      (sum of w not > 0: both copy)
 *      Every w of pixel p is taken times 2^-k, k = floor(log2 (n_p . n_p)^sigma_normal) kept within [-126, 126] (0 for a zero normal) -- formed as
 *      (h(dx) h(dy) w_n w_z * 2^-k) * w_l.  A power of two scales every sum exactly and cancels in both quotients, so the results are those of the
 *      unscaled w bit for bit wherever fp32 holds the unscaled sums; it is there because V squares a weight that w_n lets grow to 1e20 for
 *      normals of length 1.2 and shrink to 1e-25 for normals of length 0.8: unscaled, w^2 leaves fp32 and V_1 is not a number.
 *   End.   out(p).rgb = I_N(p) * max(a_p, 1e-3) when `demodulate` and p is not a miss, else I_N(p);  out(p).a = H1(p).a.
 *          iterations == 0: out.rgb = 0.5 * (H1 + H2), one fp32 add and one multiply per channel.
 *
 *  Arithmetic: fp32 without contraction; TRG_OPT_STRICT 1 uses expf / powf / sqrtf, 0 the hardware's exp2 / log2 / sqrt.  The float64
 *  reference: toyraygun_amd/denoise.py reference_denoise_variance.
 *
 *  On the device: V travels in the .w of the filter's ping-pong colour planes, so the LDS forms (spacings 1, 2) stage no extra bytes and a
 *  tap of the L2 form is still one global_load_dwordx4 per plane; GV is read from the staged tile in the LDS forms.  One streaming launch
 *  marks the emitters (as for trg_denoise), one combines H1, H2 into (I_0, V_0), the prefilter is one launch over 16 x 16 tiles with a
 *  22 x 22 halo of G0 and V in LDS, then one launch per iteration; remodulation and alpha are part of the last. */
TRG_API int trg_denoise_variance(trg_ctx *ctx, const void *halves_device, const void *guides_device, void *out_device, const trg_denoise_var_params *p /* NULL: defaults */);

/* --- trg_render_halves(frameIndexBegin, spp, bounces) into the state's own half planes, trg_guides_render(frameIndexBegin) into the state's own
 *     guide planes, trg_denoise_variance into out_device.  One stream.  The bound accumulation buffer is neither read nor written. */
TRG_API int trg_render_denoised_variance(trg_ctx *ctx, uint32_t frameIndexBegin, uint32_t spp, uint32_t bounces, void *out_device, const trg_denoise_var_params *p);

/* --- the same for callers without device memory of their own (the engine plugin): the result goes to the image the STATE owns (the one of
 *     trg_denoise_accum; valid until the next call of either function or trg_denoise_release).  Only enqueues (but see TRG_OPT_TIMING). */
TRG_API int trg_render_denoised_variance_own(trg_ctx *ctx, uint32_t frameIndexBegin, uint32_t spp, uint32_t bounces, const trg_denoise_var_params *p, void **out_device);

/* --- with HOST buffers; they WAIT for the result.  halves_host: 2 * width*height*4 floats.  var_host (may be NULL): width*height floats, V_N of
 *     the definition above -- the variance the filter carried to its end (V_0, prefiltered or not, when iterations == 0). */
TRG_API int trg_render_halves_read(trg_ctx *ctx, uint32_t frameIndexBegin, uint32_t spp, uint32_t bounces, float *halves_host);
TRG_API int trg_denoise_variance_host(trg_ctx *ctx, const float *halves_host, const float *guides_host, float *out_host, float *var_host, const trg_denoise_var_params *p);
TRG_API int trg_render_denoised_variance_read(trg_ctx *ctx, uint32_t frameIndexBegin, uint32_t spp, uint32_t bounces, float *out_host, const trg_denoise_var_params *p);

/* =============================================================================================================================================
 * TEMPORAL REPROJECTION AND ACCUMULATION (the other half of SVGF).  The result of the previous calls is reprojected through the guides into the
 * current frame, colour and the first two moments of luminance are accumulated over time, and the variance-guided iterations above are handed a
 * TEMPORAL variance: no second render, and a moving camera no longer starts from one sample per pixel.
 * ============================================================================================================================================= */

/* --- WORLD POSITIONS.  What trg_guides_render does (the same G0, G1, bit for bit), and one more plane X of width*height float4:
 *       X(p) = (o + z * d, 0)    o, d = origin and direction of the pixel's primary ray of that frame index (trg_raygen), z = G0(p).w;
 *                                per component one fp32 multiply and one fp32 add, not contracted
 *       X(p) = (0, 0, 0, 0)      on a miss */
TRG_API int trg_guides_render_pos(trg_ctx *ctx, uint32_t frameIndex, void *guides_device, void *pos_device);

/* --- THE CAMERA OF A FRAME, for the call that comes after it.  Host only; touches no context.  u->inv_view_proj is read as the matrix A with
 *     A[j][k] = m[j*4 + k] -- the way trg_raygen multiplies it: world_j = sum_k A[j][k] ndc_k.  vp16 = the inverse of A in the same layout,
 *     inverted in double precision and rounded to fp32; TRG_ERR_INVALID when A is singular or not finite (or a pointer is NULL).
 *     With clip_j = sum_k vp16[j*4 + k] (X, 1)_k a world point X lands at
 *       sx = (clip.x / clip.w * 0.5 + 0.5) * width,  sy = (clip.y / clip.w * 0.5 + 0.5) * height
 *     where pixel (x, y) has its centre at (x + 0.5, y + 0.5); row 0 is the bottom, nothing flips. */
TRG_API int trg_temporal_view_proj(const trg_uniforms *u, float vp16[16]);

typedef struct trg_temporal_params {
    int32_t iterations;   /* 0 .. TRG_DENOISE_MAX_ITERATIONS; default 5 */
    float sigma_lum;      /* default 4.0 */
    float sigma_normal;   /* default 128 */
    float sigma_depth;    /* default 1.0 */
    int32_t demodulate;   /* default 1 */
    float alpha;          /* in (0, 1]; default 0.2: the least weight of the new colour sample */
    float alpha_moments;  /* in (0, 1]; default 0.2: the same for the two moments */
    float plane_tol;      /* > 0; default 0.02: a tap's distance from the pixel's tangent plane, as a fraction of the hit distance */
    float normal_tol;     /* in [-1, 1]; default 0.9: the least cosine between the pixel's and a tap's normal */
    int32_t max_history;  /* >= 1; default 32: where the history length N stops growing */
} trg_temporal_params;
TRG_API void trg_temporal_default_params(trg_temporal_params *p);

/* --- HISTORY.  Four planes of width*height float4 per pixel, owned by the state (allocated on the first call, double-buffered, freed by
 *     trg_denoise_release):
 *       Hc = (I.rgb, N)      the accumulated (demodulated) colour and the history length
 *       Hm = (m1, m2, 0, 0)  the accumulated first and second moment of L(D)   (.z: A LONG HISTORY below, .w: PIXEL FOOTPRINTS below, while those settings are on)
 *       F  = the filter's G0 of that frame (normal | z), emitters marked as misses (z = -1)
 *       X  = the world positions of that frame
 *     A new state has no history, and trg_temporal_reset forgets it (and the view-projection trg_render_temporal remembered;
 *     it allocates nothing: harmless for a context that never denoised).
 *     THE LIBRARY DOES NOT NOTICE A CHANGED SCENE: after trg_load_scene or trg_load_textures the caller calls trg_temporal_reset
 *     -- or, for geometry that moved and kept its topology, trg_temporal_set_previous_scene (MOVING GEOMETRY below), which keeps the history.
 *     trg_temporal_history_read: Hc then Hm of the last call into 2 * width*height*4 floats; it WAITS for the result (TRG_ERR_INVALID while
 *     there is no history). */
TRG_API int trg_temporal_reset(trg_ctx *ctx);
TRG_API int trg_temporal_history_read(trg_ctx *ctx, float *hist_host);

/* --- ONE TEMPORAL STEP.  color_in_device, out_device: width*height float4; guides_device, pos_device: as trg_guides_render_pos writes them for
 *     THIS frame; prev_view_proj: trg_temporal_view_proj of the uniforms the PREVIOUS call's frame was rendered with (read during the call).  No two
 *     of the buffers may overlap and none may be NULL, else TRG_ERR_INVALID; so are parameters outside the ranges above -- refused before
 *     anything is enqueued or the history changes.
 *
 *  Notation, misses and emitters: as for trg_denoise ("miss" means both).  A prime marks the previous call's history planes.  For a vector n,
 *  nn(n) = n / sqrt(n.x^2 + n.y^2 + n.z^2); when that length is not > 0 every test n takes part in fails.  Sums of three products are formed
 *  left to right.  D(p) = C(p).rgb / max(a_p, 1e-3) per channel when `demodulate` and p is not a miss, else C(p).rgb;  l = L(D(p)).
 *
 *   Miss.  out(p) = color_in(p) bit for bit; history I = C(p).rgb, N = 0, m1 = m2 = 0; V_0 = 0.
 *   Reproject (p not a miss).  clip_j = vp[j*4] X(p).x + vp[j*4+1] X(p).y + vp[j*4+2] X(p).z + vp[j*4+3], left to right.
 *          NO HISTORY when there is none in the state, or clip.w is not > 0, or with
 *              fx = (clip.x / clip.w * 0.5 + 0.5) * width - 0.5,   fy = (clip.y / clip.w * 0.5 + 0.5) * height - 0.5
 *          not (-1 <= fx < width and -1 <= fy < height) (all four taps would lie outside).  Otherwise x0 = floor(fx), y0 = floor(fy),
 *          tx = fx - x0, ty = fy - y0, and the four taps q = (x0 + i, y0 + j), in the order (i, j) = (0,0), (1,0), (0,1), (1,1), have
 *              b = (i ? tx : 1 - tx) * (j ? ty : 1 - ty)
 *          A tap is VALID iff q is inside the image, F'(q).w >= 0,
 *              | nn(n_p) . (X'(q) - X(p)) | <= plane_tol * z_p      and      nn(n_p) . nn(F'(q).xyz) >= normal_tol
 *          W = sum of b over the valid taps.  W > 0: Ih, m1h, m2h, Nh = (sum of b * Hc'.rgb, Hm'.x, Hm'.y, Hc'.w over the valid taps) / W.
 *          W not > 0: no history.
 *   Accumulate.  No history: N = 1, I = D, m1 = l, m2 = l * l exactly.  Otherwise
 *              N = min(Nh + 1, max_history),  a = max(alpha, 1 / N),  am = max(alpha_moments, 1 / N)
 *              I = Ih + a (D - Ih),  m1 = m1h + am (l - m1h),  m2 = m2h + am (l * l - m2h)
 *          (I, N) and (m1, m2) become the history together with this frame's F and X.  The history holds UNFILTERED values: SVGF's feedback of
 *          the first filtered iteration is deliberately left out.
 *   Variance.  N >= 4: V_0 = max(0, m2 - m1 * m1).
 *          N < 4: with M1 = sum_q g m1(q) / sum_q g, M2 likewise with m2, over the 49 pixels q = p + (dx, dy), dx, dy in {-3 .. 3}, inside the
 *          image (rows outer, columns inner), g = w_n * w_z * w_id at s = 1 exactly as in the prefilter of trg_denoise_variance, m1, m2 THIS
 *          call's accumulated moments:  V_0 = max(0, M2 - M1 * M1) * 4 / N;  V_0 = 0 when the sum of g is not > 0.
 *   Filter.  (I, V_0) goes through iterations i = 0 .. iterations-1 of trg_denoise_variance exactly as defined there (no prefilter).
 *          out(p).rgb = I_N(p) * max(a_p, 1e-3) when `demodulate` and p is not a miss, else I_N(p);  out(p).a = color_in(p).a.
 *          iterations == 0: out.rgb = I remodulated in that way.
 *
 *  Arithmetic: fp32 without contraction; TRG_OPT_STRICT 1 uses expf / powf / sqrtf, 0 the hardware's exp2 / log2 / sqrt; the divisions are
 *  IEEE divisions in both.  The float64 reference: toyraygun_amd/denoise.py reference_temporal (+ reference_atrous_variance).
 *
 *  On the device: the emitter-marking launch of trg_denoise; ONE reprojection launch over 16 x 16 tiles of 256 threads, a pixel per thread: it
 *  reads the four current planes coalesced as float4, gathers 4 taps x 4 history planes through L2 (the target is arbitrary: nothing to stage)
 *  and writes the four new history planes and (I, V_0); ONE launch for the spatial estimate with a 22 x 22 halo of F and the moments in LDS,
 *  which a tile without a pixel of N < 4 leaves after one ballot per wave, before staging anything; then the launches of the
 *  variance-guided filter, unchanged. */
TRG_API int trg_temporal_denoise(trg_ctx *ctx, const void *color_in_device, const void *guides_device, const void *pos_device, const float prev_view_proj[16],
                                 void *out_device, const trg_temporal_params *p /* NULL: defaults */);

/* --- RENDER + TEMPORAL STEP on one stream.  spp >= 1 and frameIndexBegin + spp <= 2^32 - 1.  With b = frameIndexBegin, n = spp:
 *       1. a zeroed image of the state is bound, trg_render(b, n, bounces) runs over the whole image, the caller's binding is restored (the
 *          bound accumulation buffer is neither read nor written, as in trg_render_halves); a real render: its rays count, `renders` goes up by one;
 *       2. its rgb is multiplied by fl((b + n) / n) (the quotient in double precision, rounded to fp32): the mean of the samples;
 *       3. trg_guides_render_pos(b) with the context's current uniforms into planes of the state;
 *       4. trg_temporal_denoise against the view-projection the state remembered from its previous trg_render_temporal call; after a reset (or in
 *          a new state) there is none and the step runs without history;
 *       5. trg_temporal_view_proj of the current uniforms is remembered.
 *     out_device must not overlap the bound accumulation buffer (TRG_ERR_INVALID).
 *     _own: the result goes to the image the STATE owns (the one of trg_denoise_accum), for callers without device memory. */
TRG_API int trg_render_temporal(trg_ctx *ctx, uint32_t frameIndexBegin, uint32_t spp, uint32_t bounces, void *out_device, const trg_temporal_params *p);
TRG_API int trg_render_temporal_own(trg_ctx *ctx, uint32_t frameIndexBegin, uint32_t spp, uint32_t bounces, const trg_temporal_params *p, void **out_device);

/* --- with HOST buffers; they WAIT for the result.  pos_host: width*height*4 floats.  iv_host (may be NULL): width*height*4 floats, (I.rgb, V_0);
 *     var_host (may be NULL): width*height floats, V_N (V_0 when iterations == 0). */
TRG_API int trg_guides_pos_read(trg_ctx *ctx, uint32_t frameIndex, float *guides_host, float *pos_host);
TRG_API int trg_temporal_denoise_host(trg_ctx *ctx, const float *color_in_host, const float *guides_host, const float *pos_host, const float prev_view_proj[16],
                                      float *out_host, float *iv_host, float *var_host, const trg_temporal_params *p);
TRG_API int trg_render_temporal_read(trg_ctx *ctx, uint32_t frameIndexBegin, uint32_t spp, uint32_t bounces, float *out_host, const trg_temporal_params *p);

/* =============================================================================================================================================
 * MOVING GEOMETRY: PREVIOUS-POSITION PLANES (SVGF's motion vectors, in world space).  The step above follows a moving CAMERA: it looks for the
 * history of a pixel where the previous camera saw the hit's CURRENT world position.  A surface that moved was somewhere else then, so the
 * step either rejects good history (motion along the normal beyond plane_tol * z, a rotation beyond normal_tol) or accepts the history of
 * another surface point (a slide within the plane).  Here the caller says where every triangle was, and the step looks there.
 *
 * NOT COVERED.  Moving or changing EMITTERS: the history then holds stale lighting; `alpha` forgets it, and the gated lag correction (CHANGING
 * LIGHT below, off by default) removes what a 7 x 7 window can tell from noise -- a change of brightness almost at once, a moved shadow
 * hardly.  A changed TOPOLOGY (another
 * triangle count, or triangle k no longer the surface triangle k was): the caller calls trg_temporal_reset.  Device groups (trg_group_*).
 * Feeding filtered colour back into the history: as above, the history holds unfiltered values.  A float64 prototype of SVGF's feedback (the
 * first filtered iteration and its V_1 written back) on top of the variance of the mean was better on two of six sequences and worse on three
 * -- rmse 0.02277 against 0.02324 with the eye turning (8 calls x 2 spp), 0.03414 against 0.03375 at rest (24 x 1); the whole table stands
 * under A LONG HISTORY below.  Pixels whose footprint covers two surfaces: PIXEL FOOTPRINTS below (off by default) keeps them out of the
 * filter; misses and directly seen emitters still copy the call's one sample, as listed there.
 * ============================================================================================================================================= */

/* --- PREVIOUS GEOMETRY.  Call it AFTER trg_load_scene of the new geometry.  Triangle k here is the surface that triangle k of the loaded scene
 *     was at the previous call.  The layouts are trg_load_scene's: triangle k has the corners positions3[3 * indices[3k + c]], c = 0, 1, 2, and
 *     the normals normals3[3 * (3k + c)].  n_tris must be the loaded scene's triangle count, or 0: the previous scene is forgotten (no pointer
 *     is read, the state is disarmed).  TRG_ERR_INVALID when no scene is loaded, n_tris is neither, an index is >= n_verts, or positions3 or
 *     indices is NULL.  normals3 == NULL: the normals did not change (a pure translation); the previous normal of a hit is then its current one.
 *     Everything is copied into a grow-only device array of the state (freed by trg_denoise_release), one record of 80 bytes per ORIGINAL
 *     primitive index -- what the tracer reports, so no map is needed to find it -- of five float4:
 *       (P0.x P0.y P0.z P1.x) (P1.y P1.z P2.x P2.y) (P2.z N0.x N0.y N0.z) (N1.x N1.y N1.z N2.x) (N2.y N2.z 0 0)        N = 0 without normals3
 *     The call WAITS for the copy (the caller's arrays may be freed when it returns); a refused call changes nothing.
 *     ARMING.  A successful call with n_tris != 0 ARMS the state: the next successful trg_render_temporal / _own / _read uses the previous scene
 *     and disarms it.  One call describes ONE transition: a caller who stops animating sees no phantom motion.  trg_temporal_reset disarms
 *     too (the stored geometry stays).  While armed, trg_render_temporal* compares the stored triangle count with the loaded scene's and
 *     returns TRG_ERR_INVALID, before anything is enqueued or the history changes, when they differ (a trg_load_scene in between). */
TRG_API int trg_temporal_set_previous_scene(trg_ctx *ctx, const float *positions3, const float *normals3 /* may be NULL */, const uint32_t *indices,
                                            uint32_t n_verts, uint32_t n_tris);
/*     The same from buffers that are ALREADY ON THE DEVICE (the context's; the layouts above), e.g. the current pose of include/trg_pose.h before
 *     the next one is applied: the same records, written by one kernel on the context's stream, the same arming and the same refusals -- but
 *     nothing is copied and NOTHING IS WAITED FOR: the caller must not write the buffers before the stream has passed the call.  The caller vouches
 *     for the buffers; an index >= n_verts is not refused but clamped to the last vertex, so that nothing is read out of bounds. */
TRG_API int trg_temporal_set_previous_scene_device(trg_ctx *ctx, const void *positions3_dev, const void *normals3_dev /* may be NULL */,
                                                   const void *indices_dev, uint32_t n_verts, uint32_t n_tris);

/* --- MOTION PLANES.  G0, G1 and X are written as trg_guides_render_pos writes them, bit for bit.  motion_device: TWO planes of width*height
 *     float4, M0 then M1.  With c0, c1 = the hit's trg_isect.coordinates, c2 = 1 - c0 - c1 (as for the guides) and P0', P1', P2' / N0', N1', N2'
 *     the previous corners / normals of the hit primitive:
 *       M0(p) = ((c0 * P0' + c1 * P1') + c2 * P2', 1)      where the surface point under p WAS; every product and sum one fp32 operation, not
 *       M1(p) = ((c0 * N0' + c1 * N1') + c2 * N2', 0)      contracted.  Previous scene set with normals3 == NULL: M1 = (G0(p).xyz, 0) bit for bit
 *       M0(p) = M1(p) = (0, 0, 0, 0)                       on a miss
 *     M0.w > 0 says "a previous position is known": a caller who writes the planes from their own data (skinning) may clear it per pixel.
 *     TRG_ERR_INVALID without a previous scene of the loaded scene's triangle count (whether the state is armed plays no part), when a pointer
 *     is NULL or two of the buffers overlap.
 *     On the device: ONE launch behind the gather of the guides, a pixel per thread: it reads the pixel's hit record (one coalesced float4 of
 *     the guide pass' scratch) and the hit primitive's record above as float4 (the position rows alone without normals3, then G0(p) instead),
 *     and writes two coalesced float4.  No atomics, no scratch, no LDS. */
TRG_API int trg_guides_render_motion(trg_ctx *ctx, uint32_t frameIndex, void *guides_device, void *pos_device, void *motion_device);

/* --- THE STEP WITH MOTION.  trg_temporal_denoise exactly -- arguments, refusals, every formula --, with motion_device (as above; it must not be
 *     NULL nor overlap any other buffer) and three substitutions in Reproject:
 *       clip_j = vp[j*4] M0(p).x + vp[j*4+1] M0(p).y + vp[j*4+2] M0(p).z + vp[j*4+3]                  (M0(p).xyz in place of X(p))
 *       a tap's plane test:   | nn(M1(p).xyz) . (X'(q) - M0(p).xyz) | <= plane_tol * z_p               (z_p is still THIS frame's depth)
 *       a tap's normal test:  nn(M1(p).xyz) . nn(F'(q).xyz) >= normal_tol
 *     and NO HISTORY also when M0(p).w is not > 0 or nn(M1(p).xyz) has no length (the current normal n_p takes no part any more).
 *     Nothing else changes: the history that is written is this frame's F and X (not M), accumulation, V_0 and the filter are as above.
 *     So with M0 = (X.xyz, 1) and M1 = (G0.xyz, 0) every result -- out, the history, (I, V_0), V_N -- is trg_temporal_denoise's BIT FOR BIT.
 *     The float64 reference: reference_temporal(..., motion=(M0, M1)).
 *     On the device: the same launches; the reprojection kernel reads two more coalesced float4 per pixel. */
TRG_API int trg_temporal_denoise_motion(trg_ctx *ctx, const void *color_in_device, const void *guides_device, const void *pos_device, const void *motion_device,
                                        const float prev_view_proj[16], void *out_device, const trg_temporal_params *p /* NULL: defaults */);

/* --- trg_render_temporal / _own / _read WHILE ARMED: step 3 is trg_guides_render_motion into two more planes of the state (allocated on the first
 *     such call), step 4 is trg_temporal_denoise_motion; the call then disarms the state.  Unarmed they do what they did, bit for bit.
 *
 * --- with HOST buffers; they WAIT for the result.  motion_host: 2 * width*height*4 floats; the other buffers as for trg_guides_pos_read and
 *     trg_temporal_denoise_host. */
TRG_API int trg_guides_motion_read(trg_ctx *ctx, uint32_t frameIndex, float *guides_host, float *pos_host, float *motion_host);
TRG_API int trg_temporal_denoise_motion_host(trg_ctx *ctx, const float *color_in_host, const float *guides_host, const float *pos_host, const float *motion_host,
                                             const float prev_view_proj[16], float *out_host, float *iv_host, float *var_host, const trg_temporal_params *p);

/* =============================================================================================================================================
 * CHANGING LIGHT: GATED LAG CORRECTION.  When the lighting changes (trg_set_uniforms: the area light lives in trg_uniforms; or a moved box
 * whose shadow moves over a floor that did not), every surface still reprojects perfectly onto a history that is now wrong, and with
 * alpha = 0.2 a change leaves 0.8^m of the old picture after m calls.  The new samples know better: over a 7 x 7 window their mean differs from
 * the accumulated colour's by the LAG.  Where that difference is larger than the noise of the window mean explains, it is added to the accumulated
 * colour.  Off by default, switched on per context; with it off every entry point enqueues what it did and gives the same bits.
 * ============================================================================================================================================= */

/* --- THE CORRECTION sits between Accumulate and Variance of ONE TEMPORAL STEP.  Notation: trg_temporal_denoise's; p a pixel that is not a miss
 *     ("miss" includes emitters), D(q) this call's demodulated sample, I(q) the colour Accumulate produced for this call, F this call's filter G0.
 *     The window: the 49 pixels q = p + (dx, dy), dx, dy in {-3 .. 3}, inside the image, rows outer, columns inner, the centre included;
 *     g = w_n * w_z * w_id at s = 1 exactly as in the prefilter of trg_denoise_variance and in the spatial estimate, with the step's sigma_normal
 *     and sigma_depth -- times 2^-k, k = floor(log2 g(p,p)) kept within [-126, 126] (g(p,p), the centre's own weight, is (n_p . n_p)^sigma_normal; a zero normal has no tap at all):
 *     a power of two scales every sum exactly and cancels in every quotient below, so the results are those of the unscaled g bit for bit
 *     wherever fp32 holds the unscaled sums; it is there because G2 squares a weight that w_n lets grow to 1e20 for normals longer than 1.
 *     Per channel, every sum in window order, every product and sum one fp32 operation:
 *       G  = sum g                    G2 = sum g * g
 *       d  = (sum g * (D(q) - I(q))) / G
 *       A1 = sum g * t,   A2 = sum g * (t * t),   t = D(q) - D(p)          (centred on p: no cancellation on flat regions)
 *       se = sqrt(max(0, A2 / G - (A1 / G) * (A1 / G)) * G2) / G           the standard error of the window mean of D
 *       m  = |d| - gate * se
 *       Ic = max(I(p) + copysign(m, d), min(I(p), 0))   when m > 0         (soft threshold; never pushes a non-negative colour below 0)
 *       Ic = I(p) bit for bit                           when m is not > 0, or G is not > 0, or p is a miss
 *     Ic replaces I in the history plane Hc (N is untouched) and in (I, V_0), which is handed to the iterations and returned as iv_host.
 *     The moments, N and V_0 are NOT corrected: after a change of lighting the temporal variance is too large for a few calls (it holds the
 *     step between the old and the new level), and the filter is wider for as long.
 *     Three consequences:  where D = I on the whole window (a first call without history; a second call of the same constant colour) d = 0 and
 *     Ic = I bit for bit.  On a flat D, se = 0 and Ic = I + d: camera at rest, constant colour c0 and then c1, and every pixel whose window
 *     holds one history length has Ic = c1 up to rounding, whatever the gate.  Every operation is continuous in its inputs (at m = 0 both forms
 *     of Ic give I(p)); the one discrete decision, G > 0, is the spatial estimate's.
 *     Arithmetic: fp32 without contraction; TRG_OPT_STRICT 1 uses sqrtf, 0 the hardware's sqrt; the divisions are IEEE divisions in both.
 *     The float64 reference: toyraygun_amd/denoise.py reference_lag, reference_temporal(..., lag=gate).
 *
 *     On the device: ONE launch between the reprojection and the spatial estimate, and only while the correction is on: 16 x 16 tiles of 256
 *     threads, F, (D.rgb, E.r) and (E.g, E.b), E = D - I, of the tile and 3 pixels of halo in LDS (22 x 22 x 40 B = 19 KB; D is recomputed
 *     from the colour and G1 while staging; E(q) is the very fp32 difference the definition sums), 49 taps, eleven running sums.  It reads
 *     (I, V_0) as the reprojection wrote it, rewrites .rgb of the new Hc plane in place and writes the corrected (I, V_0) to the filter's other
 *     ping-pong image, so no tile reads what another one writes.  No atomics, no scratch. */
#define TRG_TEMPORAL_LAG_GATE_DEFAULT 3.0f
/* gate >= 0: on, for every later trg_temporal_denoise / _motion / _host and trg_render_temporal / _own / _read of this context; gate < 0: off
 * (the state of a new context); NaN: TRG_ERR_INVALID, nothing changes.  Host only: allocates nothing on the device, harmless for a context
 * that never denoised; survives trg_temporal_reset, ends with trg_denoise_release. */
TRG_API int trg_temporal_set_lag_correction(trg_ctx *ctx, float gate);
TRG_API int trg_temporal_lag_correction(trg_ctx *ctx, float *gate);   /* what is set; < 0 when off */
/* the correction alone on host buffers (stage-level, for tests; WAITS): colour, guides as for trg_temporal_denoise_host, hc_host = a plane
 * (I.rgb, N); out_hc_host = (Ic.rgb, N).  Emitters are marked from the context's loaded scene as everywhere.  gate must be >= 0, sigma_normal
 * >= 0 and sigma_depth > 0, else TRG_ERR_INVALID.  The context's own setting and history are neither read nor changed. */
TRG_API int trg_temporal_lag_correct_host(trg_ctx *ctx, const float *color_in_host, const float *guides_host, const float *hc_host, float gate,
                                          float sigma_normal, float sigma_depth, int32_t demodulate, float *out_hc_host);

/* =============================================================================================================================================
 * A LONG HISTORY: THE VARIANCE OF THE MEAN.  The step above hands the iterations the variance of ONE sample: from four frames on
 * V_0 = max(0, m2 - m1 * m1), a figure that does not shrink as the history grows, so a pixel with 24 frames behind it is filtered as widely as
 * one with four -- and the five default iterations then blur away what the accumulation had gained.  What the colour weight w_l wants is the
 * variance of the colour it compares, the ACCUMULATED one.  For independent samples an exponential average I = (1 - a) I' + a D has
 *       Var(I) = (1 - a)^2 Var(I') + a^2 Var(D)
 * and the history plane Hm = (m1, m2, 0, 0) has two unused channels: the variance travels there, at no extra bytes and no extra gathers.
 * Off by default, switched on per context; with it off every entry point enqueues what it did and gives the same bits.
 * ============================================================================================================================================= */

/* --- WITH THE SETTING ON, ONE TEMPORAL STEP (trg_temporal_denoise / _motion / _host, trg_render_temporal / _own / _read) differs in three places.
 *     Notation: trg_temporal_denoise's; a prime marks the previous call's history planes.
 *   History.   Hm = (m1, m2, Vc, 0): Vc = the variance estimate of L of the accumulated colour in Hc.  (Off: Hm.z stays 0.)
 *              trg_temporal_history_read returns the plane as it is.  A miss has Vc = 0.
 *   Reproject. Vh = (sum of b * Hm'.z over the valid taps) / W -- the taps, the order and the division of m1h.
 *   Variance.  S = the V_0 of trg_temporal_denoise exactly as defined there: max(0, m2 - m1 * m1) for N >= 4, the 7 x 7 spatial estimate times
 *              4 / N for N < 4.  a = max(alpha, 1 / N), the weight the colour was accumulated with.
 *                No history, or N < 4:   Vc = S
 *                otherwise:              Vc = ((1 - a) * (1 - a)) * Vh + (a * a) * S        every product and sum one fp32 operation, not contracted
 *              V_0 := Vc: it is what (I, V_0) carries, what the iterations get, what iv_host returns; and Hm.z = Vc.
 *     Everything else is the step as it stands: I, N, the moments, F, X, the motion substitutions (a step with M0 = (X.xyz, 1), M1 = (G0.xyz, 0)
 *     is still the step without motion planes bit for bit), the iterations and the remodulation.  The lag correction leaves Vc alone as it leaves
 *     the moments.  No new discrete decision: the choice of form is N against 4, which was there already.
 *     Three consequences.  A first call has Vc = S.  Vc <= max(Vh, S) wherever there is history (a in (0, 1] makes (1 - a)^2 + a^2 <= 1).  With
 *     the camera at rest, samples of constant variance S and a = 1 / N, Vc = S / N up to the error of S: the variance of an arithmetic mean.
 *     The history below four frames has Vc = S, the variance of one sample scaled by 4 / N, not S / N: the spatial estimate is already a guess
 *     made for want of history, and the recursion starts from it.
 *     The float64 reference: toyraygun_amd/denoise.py reference_temporal(..., track=True).
 *
 *     NOT COVERED.  SVGF also writes the first filtered iteration and its V_1 back into the history ("feedback").  On a float64 prototype
 *     (Cornell box 64 x 48, 3 bounces, rmse over the whole image against 512 spp at the last camera; plain / this setting / this setting with
 *     feedback) it was better on two sequences and worse on three:
 *       eye turning 1 degree per call, 8 calls x 2 spp, alpha 0.2:   0.02558 / 0.02324 / 0.02277
 *       the same, alpha 0.05:                                        0.02586 / 0.02377 / 0.02263
 *       at rest, 8 x 1, alpha 0.2:                                   0.03682 / 0.03548 / 0.03544
 *       at rest, 24 x 1, alpha 0.2:                                  0.03579 / 0.03375 / 0.03414
 *       at rest, 24 x 1, alpha 0.05:                                 0.03712 / 0.03454 / 0.03490
 *       turning, 16 x 1, alpha 0.2:                                  0.03878 / 0.03688 / 0.03737
 *     and it would put filtered values into a history that is defined to hold unfiltered ones: left out.  The light and the pixels on its edge,
 *     which the step copies unaccumulated, are part of those figures and stay as they are.
 *
 *     On the device: the same launches.  The reprojection kernel reads .z of the Hm' float4 it gathers anyway and writes Vc into Hm.z and
 *     (I, V_0).w; the spatial-estimate kernel writes its V_0 into (I, V_0).w as before and also into Hm.z of the pixels it owns.  It stages the
 *     moments of neighbouring tiles while other workgroups write their Vc: with the setting on it reads the 8 bytes (m1, m2) of a staged pixel
 *     and never the 4 bytes of Hm.z, so no byte is read by one workgroup and written by another.  No atomics, no scratch. */
/* on != 0: on, for every later temporal step of this context; 0: off (the state of a new context).  Host only: allocates nothing on the device,
 * harmless for a context that never denoised.  A call that CHANGES the setting also does what trg_temporal_reset does -- history written with
 * the setting off has no variance in it --; a call that repeats the current value changes nothing.  The setting survives trg_temporal_reset and
 * ends with trg_denoise_release. */
TRG_API int trg_temporal_set_variance_of_mean(trg_ctx *ctx, int on);
TRG_API int trg_temporal_variance_of_mean(trg_ctx *ctx, int *on);   /* what is set: 1 or 0 */

/* =============================================================================================================================================
 * PIXEL FOOTPRINTS: CENTRE GUIDES AND A COVERAGE HISTORY.  The guides above describe ONE ray, and trg_raygen jitters that ray inside the pixel:
 * a pixel whose footprint covers two surfaces is classified by whichever of them the ray of this frame index met.  Its class then changes from
 * call to call (the history alternates between the planes of two surfaces), the call's colour is demodulated by one surface's albedo whatever
 * its samples met, and its mixed colour is a full-weight tap for its neighbours.  Here the guides come from the ray through the pixel's CENTRE,
 * which no frame index moves; whether the jittered ray of the frame agrees with it is recorded per pixel; that agreement is accumulated over
 * time like the moments; and a pixel whose accumulated agreement is low is kept out of the filter as a miss is -- it shows its accumulated colour.
 * Off by default, switched on per context; with it off every entry point enqueues what it did and gives the same bits.
 * ============================================================================================================================================= */

/* --- CENTRE GUIDES.  The CENTRE RAY of pixel (x, y) is trg_raygen's arithmetic with r0 = r1 = 0.5 in place of the two Halton values, so the
 *     frame index plays no part in it.  Every operation is one fp32 operation, sums left to right:
 *       uvx = ((x + 0.5) / width) * 2 - 1,  uvy = ((y + 0.5) / height) * 2 - 1
 *       world_j = ((uvx * m[j*4] + uvy * m[j*4+1]) + 0 * m[j*4+2]) + 1 * m[j*4+3]          m = inv_view_proj, j = 0 .. 3
 *       t = (world_0 / world_3, world_1 / world_3, world_2 / world_3) - cam_pos,  direction = t * (1 / sqrt((t.x t.x + t.y t.y) + t.z t.z))
 *     origin = cam_pos, mask 3, maxDistance infinite, colour (1, 1, 1, 0).  The divisions are IEEE and the square root is the correctly rounded
 *     one in BOTH settings of TRG_OPT_STRICT: the setting decides the intersector only, as it does for the guides above.
 *     G0, G1 and X.xyz are what trg_guides_render_pos defines, from that ray's nearest hit.  X.w, which is 0 there and which no step reads
 *     without the setting below, is the AGREEMENT FLAG A(p):
 *       A(p) = 1  when the JITTERED primary ray of frameIndex (trg_raygen's, traced in the same pass) agrees with the centre hit,
 *       A(p) = 0  when it does not, and on a centre miss.
 *     The two AGREE iff both rays hit; both hits are emitters (material TRG_MATERIAL_EMISSIVE) or neither is; and, with n_c, X_c, z_c the centre
 *     hit's interpolated normal, position and distance and n_j, X_j = o + z d (one fp32 multiply and add per component) the jittered hit's,
 *       | nn(n_c) . (X_j - X_c) | <= plane_tol * z_c      and      nn(n_c) . nn(n_j) >= normal_tol
 *     (nn and the sums of three products as in trg_temporal_denoise; sqrtf and IEEE divisions in both settings).  These are the reprojection's
 *     two tap tests on purpose: agreement means "the history would accept it".  One jittered ray is tested, whatever the spp of the call.
 *     plane_tol must be > 0 and normal_tol in [-1, 1] (trg_temporal_params' ranges), no buffer NULL and no two overlapping: TRG_ERR_INVALID.
 *     _motion: M0, M1 as trg_guides_render_motion defines them, from the CENTRE hit's barycentrics.
 *     On the device: dn_centre_raygen_kernel (streaming; three float4 per thread) writes the centre rays; the library's raygen and trace run for
 *     the jittered rays into a second ray / hit scratch of the state, then the trace of the centre rays; the gather in its AGREE form also
 *     reads the jittered hit, its ray and the normal rows of its primitive's record.  No atomics, no LDS, no scratch memory. */
TRG_API int trg_guides_render_centre(trg_ctx *ctx, uint32_t frameIndex, float plane_tol, float normal_tol, void *guides_device, void *pos_device);
TRG_API int trg_guides_render_centre_motion(trg_ctx *ctx, uint32_t frameIndex, float plane_tol, float normal_tol, void *guides_device, void *pos_device,
                                            void *motion_device);
/* with HOST buffers; they WAIT for the result (sizes as for trg_guides_pos_read and trg_guides_motion_read) */
TRG_API int trg_guides_centre_read(trg_ctx *ctx, uint32_t frameIndex, float plane_tol, float normal_tol, float *guides_host, float *pos_host);
TRG_API int trg_guides_centre_motion_read(trg_ctx *ctx, uint32_t frameIndex, float plane_tol, float normal_tol, float *guides_host, float *pos_host,
                                          float *motion_host);

/* --- WITH THE SETTING ON, ONE TEMPORAL STEP (every entry point of the family) differs in these places.  Notation: trg_temporal_denoise's;
 *     A(p) = X(p).w of the position plane the step is given (trg_guides_render_centre writes it; a caller's own planes may carry any value in [0, 1]).
 *   Reproject.  covh = (sum of b * Hm'.w over the valid taps) / W -- the taps, the order and the division of m1h.
 *   Accumulate. No history: cov = A(p).  Otherwise cov = covh + am * (A(p) - covh).  A miss has cov = 0.  Hm = (m1, m2, Vc or 0, cov).
 *   Mixed.      p is MIXED iff it is not a miss and cov < cov_min.
 *   A mixed pixel counts as a MISS for everything behind the reprojection -- the spatial estimate, the lag correction and the iterations: it
 *               copies, and it is nobody's tap.  Its (I, V_0).rgb is I * max(a_p, 1e-3) when `demodulate` (else I), so the output of the step
 *               is its accumulated colour, remodulated once.  Its V_0 is the temporal form max(0, m2 - m1 * m1) whatever N (with the variance of
 *               the mean on: what the recursion gives, the same form below four frames), never the spatial estimate; nothing reads it.
 *   History.    The history plane F keeps the UNMARKED guide, so a later call still finds taps there.  Hc, the moments and N are untouched: the
 *               history always holds demodulated values, mixed or not.
 *     Consequences.  With A = 1 on every hit cov is exactly 1 and nobody is mixed (sum b / W over one order of summation is exactly 1, and
 *     1 + am * 0 is exactly 1): every output but Hm.w is then the step's with the setting off, BIT FOR BIT.  With A = 0 everywhere every hit is
 *     mixed from the first call on and the output is the remodulated accumulated colour.  The one new discrete decision is cov against cov_min;
 *     the reference marks it `near` within 1e-4, like the others.
 *     trg_render_temporal / _own / _read with the setting on: step 3 is trg_guides_render_centre(b, p.plane_tol, p.normal_tol) -- its motion
 *     form while armed --; everything else is unchanged.
 *     The float64 reference: toyraygun_amd/denoise.py reference_temporal(..., coverage=cov_min); reference_centre_rays, reference_agreement.
 *
 *     NOT COVERED.  Misses and directly seen emitters still copy the call's one sample: a pixel whose centre ray leaves the scene or meets the
 *     light, but whose footprint holds geometry, keeps its 1-spp noise (misses have no position to reproject; letting emitters accumulate made
 *     the whole image worse in a float64 prototype, 0.0295 against 0.0274, for a reason not yet understood).  Coverage for trg_denoise /
 *     trg_denoise_variance (one call, no history).  Device groups.  trg_guides_render, _pos and _motion return what they returned.
 *
 *     On the device: no new launch.  The COVER forms of the reprojection kernel read .w of the Hm' float4 they gather anyway and X.w of the float4
 *     they read anyway, and write Hm.w.  For a mixed pixel they write the remodulated (I, V_0) and set .w = -1 of THEIR OWN pixel of the filter's
 *     copy of G0 -- the emitters' mechanism; the kernel reads that plane at its own pixel only, and the launches that stage neighbours come
 *     after it, so no byte is read by one workgroup while another writes it.  No atomics, no scratch. */
#define TRG_TEMPORAL_COVERAGE_MIN_DEFAULT 0.9f
/* 0 <= cov_min < 1: on, for every later temporal step of this context; cov_min < 0: off (the state of a new context); NaN or cov_min >= 1:
 * TRG_ERR_INVALID, nothing changes (at rest covh comes out as 1 - 1 ulp on half the picture: a threshold of 1 would flag pixels by rounding alone).
 * cov_min = 0 is "centre guides, nobody mixed".  Host only: allocates nothing on the device, harmless for a context that never denoised.  A call
 * that CHANGES the value also does what trg_temporal_reset does -- history written under the other setting has no coverage in it and comes from
 * other guides --; a call that repeats the current value (or turns off what is off) changes nothing.  The setting survives trg_temporal_reset and
 * ends with trg_denoise_release. */
TRG_API int trg_temporal_set_coverage(trg_ctx *ctx, float cov_min);
TRG_API int trg_temporal_coverage(trg_ctx *ctx, float *cov_min);   /* what is set; < 0 when off */

#ifdef __cplusplus
}
#endif
#endif /* TRG_DENOISE_H */
