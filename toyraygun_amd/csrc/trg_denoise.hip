// trg_denoise.hip -- include/trg_denoise.h: first-hit guide buffers and the edge-avoiding a-trous filter.  A translation unit of its own beside
// the render kernels: it launches the library's stage-level raygen / trace kernels (both builds) and adds a gather kernel and the filter.
// Behind them the variance-guided form of the filter and the temporal reprojection / accumulation that feeds it.
// For geometry that moved: the previous scene, the motion planes and the MOTION form of the reprojection.
// For lighting that changed: the gated lag correction of the accumulated colour.
// For a long history: the variance of the accumulated colour, carried in Hm.z (the TRACK forms of the two temporal kernels).
// For pixels whose footprint covers two surfaces: guides from the pixel centres with an agreement flag, and its history in Hm.w (the COVER forms
// of the reprojection kernel).
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/trg_denoise.h"
#include "bvh_build.h"
#include "trg_ctx.h"
#include "trg_internal.h"
#include "trg_kernels.h"

// the definition in trg_denoise.h is evaluated as written in both settings: no fused multiply-adds anywhere in this file
#pragma clang fp contract(off)

using namespace trg;

namespace {

int fail(trg_ctx *c, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}
#define DN_HIPCHK(c, expr)                                                                                      \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) return fail((c), TRG_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// ---- the two launch shapes of this unit, on the context's stream; `who` names the entry point in the error text.  The arguments are converted to
// the kernel's parameter types here, so a call site writes nullptr and size_t as they come ----
template <typename... Params, typename... Args>
int launch(trg_ctx *c, const char *who, void (*kernel)(Params...), dim3 grid, Args... args) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, c->stream, static_cast<Params>(args)...);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? TRG_OK : fail(c, TRG_ERR_DEVICE, "%s: launch failed: %s", who, hipGetErrorString(e));
}
// one thread per element (pixel, leaf record) in blocks of 256
template <typename Kernel, typename... Args>
int launch_each(trg_ctx *c, const char *who, Kernel kernel, size_t n, Args... args) {
    return launch(c, who, kernel, dim3((uint32_t)((n + 255) / 256)), args...);
}
// one 16 x 16 tile of the image per block of 256
constexpr int kDnTile = 16;                      // = trg::kTileW x kTileH of the render kernels at 256 threads
template <typename Kernel, typename... Args>
int launch_tiles(trg_ctx *c, const char *who, Kernel kernel, Args... args) {
    return launch(c, who, kernel, dim3((c->w + kDnTile - 1) / kDnTile, (c->h + kDnTile - 1) / kDnTile), args...);
}
// the instantiation of a kernel template for the context's build setting (STRICT is its first parameter): the arguments are written once
#define DN_FOR_SETTING(c, kernel, ...) ((c)->opt_strict ? kernel<true, ##__VA_ARGS__> : kernel<false, ##__VA_ARGS__>)

}  // namespace

// ---- per-context state (grow-only device scratch): trg_ctx::denoise, created on first use, freed by denoise_state_free ----
struct trg::DenoiseState {
    size_t pixels = 0;             // what rays / isect / ping / pong / guides are sized for
    trg_ray *rays = nullptr;
    trg_isect *isect = nullptr;
    float4 *ping = nullptr, *pong = nullptr, *guides = nullptr;   // guides: the two planes trg_render_denoised fills
    float4 *result = nullptr;      // trg_denoise_accum's output image (allocated on its first call)
    float4 *fguide = nullptr;      // the filter's copy of G0: distance -1 where the first hit is an emitter (dn_exclude_emitters_kernel)
    uint32_t *rec_of_prim = nullptr;   // original primitive index -> leaf record of the HBM part of the scene blob
    size_t prims = 0;
    int *overflow = nullptr;       // traversal-stack levels beyond those kept in LDS (scenes traversed from HBM)
    size_t overflow_bytes = 0;
    // variance-guided path (allocated on its first use): the two zeroed images trg_render_halves renders into, and the half planes
    // trg_render_denoised_variance fills
    float4 *half_acc = nullptr, *halves = nullptr;
    // temporal path (allocated on its first use): two sets of the four history planes Hc, Hm, F, X -- hist[hist_cur] is what the last call
    // wrote, the next call writes the other --; the zeroed image, the position plane and the remembered view-projection of trg_render_temporal
    float4 *hist[2] = { nullptr, nullptr };
    int hist_cur = 0;
    bool hist_valid = false;
    float4 *timg = nullptr, *tpos = nullptr;
    float prev_vp[16] = {};
    bool have_prev_vp = false;
    // moving geometry (trg_temporal_set_previous_scene): kPrevRecord float4 per original primitive index (grow-only), how many are stored (0: no
    // previous scene), whether they hold normals, whether the next trg_render_temporal uses them; the two motion planes of trg_render_temporal
    float4 *prev_geo = nullptr;
    size_t prev_cap = 0;
    uint32_t prev_tris = 0;
    bool prev_normals = false, armed = false;
    float4 *tmotion = nullptr;
    // changing light (trg_temporal_set_lag_correction): the gate of the lag correction, < 0 = off.  Set on a state that may own nothing yet
    float lag_gate = -1.0f;
    // a long history (trg_temporal_set_variance_of_mean): the steps carry the variance of the accumulated colour in Hm.z.  Set like the gate
    bool track = false;
    // pixel footprints (trg_temporal_set_coverage): cov_min of the coverage history, < 0 = off.  Set like the gate.  The second ray / hit scratch
    // of the centre guides' jittered pass (allocated on its first use, for `pixels` rays)
    float cov_min = -1.0f;
    trg_ray *rays_j = nullptr;
    trg_isect *isect_j = nullptr;
};

namespace {

// every device buffer of a state, as f(pointer, bytes per pixel that state_of allocates with the state -- 0: the buffer is allocated on first use)
template <typename F>
void each_buffer(DenoiseState &s, F f) {
    f(s.rays, sizeof(trg_ray)); f(s.isect, sizeof(trg_isect)); f(s.ping, sizeof(float4)); f(s.pong, sizeof(float4)); f(s.guides, 2 * sizeof(float4));
    f(s.fguide, sizeof(float4));
    f(s.result, 0); f(s.rec_of_prim, 0); f(s.overflow, 0); f(s.half_acc, 0); f(s.halves, 0); f(s.hist[0], 0); f(s.hist[1], 0); f(s.timg, 0); f(s.tpos, 0);
    f(s.prev_geo, 0); f(s.tmotion, 0); f(s.rays_j, 0); f(s.isect_j, 0);
}

template <typename T>
int grow(trg_ctx *c, T *&mem, size_t &have, size_t need, size_t elem, const char *what) {
    if (need <= have && mem) return TRG_OK;
    if (mem) { (void)hipDeviceSynchronize(); (void)hipFree(mem); mem = nullptr; have = 0; }
    hipError_t e = hipMalloc((void **)&mem, need * elem);
    if (e != hipSuccess) return fail(c, TRG_ERR_NOMEM, "denoise: %s hipMalloc(%zu) failed: %s", what, need * elem, hipGetErrorString(e));
    have = need;
    return TRG_OK;
}

// the state of a context that owns no image yet (pixels == 0): what the setters need (a context is used by one host thread: trg.h)
DenoiseState &bare_state(trg_ctx *c) {
    if (!c->denoise) c->denoise = new DenoiseState;
    return *c->denoise;
}

// the state of a context, with the image-sized buffers allocated
int state_of(trg_ctx *c, DenoiseState *&out) {
    DenoiseState &s = bare_state(c);
    if (!s.pixels) {
        const size_t n = (size_t)c->w * c->h;
        hipError_t e = hipSuccess;
        each_buffer(s, [&](auto *&mem, size_t per_pixel) {
            if (per_pixel && e == hipSuccess) e = hipMalloc((void **)&mem, n * per_pixel);
        });
        if (e != hipSuccess) {
            denoise_state_free(c);   // (`s` is gone from here on, and with it what the setters had set: as it always was on this path)
            return fail(c, TRG_ERR_NOMEM, "denoise: hipMalloc of the scratch images failed: %s", hipGetErrorString(e));
        }
        s.pixels = n;
    }
    out = &s;
    return TRG_OK;
}

// an image-sized buffer of the state that only some entry points need: `planes` x width*height float4, allocated on first use
int lazy_planes(trg_ctx *c, DenoiseState &s, float4 *&mem, size_t planes, const char *what) {
    if (mem) return TRG_OK;
    const hipError_t e = hipMalloc((void **)&mem, planes * s.pixels * sizeof(float4));
    if (e != hipSuccess) { mem = nullptr; return fail(c, TRG_ERR_NOMEM, "denoise: hipMalloc of %s failed: %s", what, hipGetErrorString(e)); }
    return TRG_OK;
}

// the same for a buffer of one element of T per pixel
template <typename T>
int lazy_scratch(trg_ctx *c, DenoiseState &s, T *&mem, const char *what) {
    if (mem) return TRG_OK;
    const hipError_t e = hipMalloc((void **)&mem, s.pixels * sizeof(T));
    if (e != hipSuccess) { mem = nullptr; return fail(c, TRG_ERR_NOMEM, "denoise: hipMalloc of %s failed: %s", what, hipGetErrorString(e)); }
    return TRG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// Guides
// ---------------------------------------------------------------------------------------------------------------------------------------------
// Every scene has, in its blob, one 128-byte record per triangle in LEAF order (trg_kernels.h SceneDesc::off_fat: rows 0..2 = v0 | original
// index, e1 | material id, e2 | -; floats 12..20 the nine normal floats, 21..29 the nine colour floats) -- the one place where a scene too
// large for LDS keeps its attributes.  The tracer reports ORIGINAL indices, so: which record holds primitive k?
__global__ void dn_record_map_kernel(const float4 *recs, uint32_t n_rec, uint32_t n_prims, uint32_t *rec_of_prim) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rec) return;
    const uint32_t prim = (uint32_t)__float_as_int(recs[(size_t)r * 8u].w);
    if (prim < n_prims) rec_of_prim[prim] = r;
}

// POS: also the world-position plane X = (o + z d, 0) of trg_guides_render_pos, from the primary rays the hit records belong to (zero on a miss)
// AGREE (trg_guides_render_centre; needs POS): `isect` and `rays` are those of the CENTRE rays, and pos.w becomes the agreement flag A of the
// header -- 1 when the frame's jittered primary ray (ag.rays, its hit ag.isect) passes the reprojection's two tap tests against the centre hit
// and both hits are emitters or neither is.  Three more coalesced reads per pixel (one float4 of the hit, two of the ray) and the rows 1, 3, 4, 5
// of the jittered hit's record.  sqrtf and IEEE divisions whatever the build setting: the kernel has one form for both.
struct GatherAgree {
    const trg_isect *isect;
    const trg_ray *rays;
    float plane_tol, normal_tol;
};
template <bool POS, bool AGREE>
__device__ __forceinline__ void dn_gather_pixel(const trg_isect *isect, const uint32_t *rec_of_prim, const float4 *recs, uint32_t n_prims, const TexDesc &tex,
                                                float4 *g0, float4 *g1, uint32_t n, const trg_ray *rays, float4 *pos, const GatherAgree &ag) {
    static_assert(POS || !AGREE, "the agreement flag travels in the position plane");
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 is = reinterpret_cast<const float4 *>(isect)[i];   // distance, primitiveIndex, coordinates[2]
    const int prim = __float_as_int(is.y);
    if (!(is.x >= 0.0f) || prim < 0 || (uint32_t)prim >= n_prims) {
        g0[i] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        g1[i] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
        if (POS) pos[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    float4 X = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (POS) {
        const float4 *r = reinterpret_cast<const float4 *>(rays) + (size_t)i * 3u;   // origin | mask, direction | maxDistance, colour
        const float4 o = r[0], d = r[1];
        X = make_float4(o.x + is.x * d.x, o.y + is.x * d.y, o.z + is.x * d.z, 0.0f);
        if (!AGREE) pos[i] = X;
    }
    const float4 *rec = recs + (size_t)rec_of_prim[prim] * 8u;
    const uint32_t mat = (uint32_t)__float_as_int(rec[1].w);
    const float4 r3 = rec[3], r4 = rec[4], r5 = rec[5], r6 = rec[6], r7 = rec[7];
    const float c0 = is.z, c1 = is.w, c2 = 1.0f - c0 - c1;
    float4 n4, a4;
    n4.x = c0 * r3.x + c1 * r3.w + c2 * r4.z;
    n4.y = c0 * r3.y + c1 * r4.x + c2 * r4.w;
    n4.z = c0 * r3.z + c1 * r4.y + c2 * r5.x;
    n4.w = is.x;
    a4.x = c0 * r5.y + c1 * r6.x + c2 * r6.w;
    a4.y = c0 * r5.z + c1 * r6.y + c2 * r7.x;
    a4.z = c0 * r5.w + c1 * r6.z + c2 * r7.y;
    a4.w = __int_as_float(prim);
    if (mat == TRG_MATERIAL_EMISSIVE) {
        a4.x = 1.0f; a4.y = 1.0f; a4.z = 1.0f;
    } else if (tex.uv) {
        // trg_load_textures' lookup (trg.h): nearest texel, repeat
        const uint32_t id = tex.ids[prim];
        if (id != 0u) {
            const float *p = tex.uv + (size_t)prim * 6u;
            const float u = c0 * p[0] + c1 * p[2] + c2 * p[4], v = c0 * p[1] + c1 * p[3] + c2 * p[5];
            const uint32_t *t = tex.table + (id - 1u) * 4u;
            const uint32_t w = t[1], h = t[2];
            const float fu = u - floorf(u), fv = v - floorf(v);
            uint32_t x = (uint32_t)(fu * (float)w), y = (uint32_t)(fv * (float)h);
            x = x < w ? x : w - 1u; y = y < h ? y : h - 1u;
            const uint32_t texel = tex.texels[t[0] + y * w + x];
            a4.x = a4.x * ((float)(texel & 255u) / 255.0f);
            a4.y = a4.y * ((float)((texel >> 8) & 255u) / 255.0f);
            a4.z = a4.z * ((float)((texel >> 16) & 255u) / 255.0f);
        }
    }
    g0[i] = n4;
    g1[i] = a4;
    if (AGREE) {
        const float4 js = reinterpret_cast<const float4 *>(ag.isect)[i];
        const int jprim = __float_as_int(js.y);
        float A = 0.0f;
        if (js.x >= 0.0f && jprim >= 0 && (uint32_t)jprim < n_prims) {
            const float4 *jrec = recs + (size_t)rec_of_prim[jprim] * 8u;
            const bool same_kind = ((uint32_t)__float_as_int(jrec[1].w) == TRG_MATERIAL_EMISSIVE) == (mat == TRG_MATERIAL_EMISSIVE);
            const float4 j3 = jrec[3], j4 = jrec[4], j5 = jrec[5];
            const float d0 = js.z, d1 = js.w, d2 = 1.0f - d0 - d1;
            float jx = d0 * j3.x + d1 * j3.w + d2 * j4.z, jy = d0 * j3.y + d1 * j4.x + d2 * j4.w, jz = d0 * j3.z + d1 * j4.y + d2 * j5.x;
            const float4 *r = reinterpret_cast<const float4 *>(ag.rays) + (size_t)i * 3u;
            const float4 o = r[0], d = r[1];
            const float xj = o.x + js.x * d.x, yj = o.y + js.x * d.y, zj = o.z + js.x * d.z;
            float nx = n4.x, ny = n4.y, nz = n4.z;
            const float lc = sqrtf(nx * nx + ny * ny + nz * nz), lj = sqrtf(jx * jx + jy * jy + jz * jz);
            if (same_kind && lc > 0.0f && lj > 0.0f) {
                nx = nx / lc; ny = ny / lc; nz = nz / lc;
                jx = jx / lj; jy = jy / lj; jz = jz / lj;
                const float dist = nx * (xj - X.x) + ny * (yj - X.y) + nz * (zj - X.z);
                if (fabsf(dist) <= ag.plane_tol * is.x && nx * jx + ny * jy + nz * jz >= ag.normal_tol) A = 1.0f;
            }
        }
        X.w = A;
        pos[i] = X;
    }
}
template <bool POS>
__global__ void dn_gather_kernel(const trg_isect *isect, const uint32_t *rec_of_prim, const float4 *recs, uint32_t n_prims, const TexDesc tex,
                                 float4 *g0, float4 *g1, uint32_t n, const trg_ray *rays, float4 *pos) {
    dn_gather_pixel<POS, false>(isect, rec_of_prim, recs, n_prims, tex, g0, g1, n, rays, pos, GatherAgree{});
}
__global__ void dn_gather_agree_kernel(const trg_isect *isect, const uint32_t *rec_of_prim, const float4 *recs, uint32_t n_prims, const TexDesc tex,
                                       float4 *g0, float4 *g1, uint32_t n, const trg_ray *rays, float4 *pos, const GatherAgree ag) {
    dn_gather_pixel<true, true>(isect, rec_of_prim, recs, n_prims, tex, g0, g1, n, rays, pos, ag);
}

// The centre rays of trg_guides_render_centre: trg_raygen's arithmetic with 0.5 in place of the two Halton values, written out as the header
// writes it -- one fp32 operation each (no contraction in this file), IEEE divisions and sqrtf in both build settings.  One pixel per thread,
// a 48-byte trg_ray as three float4
__global__ void dn_centre_raygen_kernel(const trg_uniforms u, uint32_t w, uint32_t h, float4 *rays) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w * h) return;
    const uint32_t y = i / w, x = i - y * w;
    const float uvx = (((float)x + 0.5f) / (float)w) * 2.0f - 1.0f, uvy = (((float)y + 0.5f) / (float)h) * 2.0f - 1.0f;
    const float *m = u.inv_view_proj;
    float wd[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wd[j] = ((uvx * m[j * 4 + 0] + uvy * m[j * 4 + 1]) + 0.0f * m[j * 4 + 2]) + 1.0f * m[j * 4 + 3];
    const float tx = wd[0] / wd[3] - u.cam_pos[0], ty = wd[1] / wd[3] - u.cam_pos[1], tz = wd[2] / wd[3] - u.cam_pos[2];
    const float inv = 1.0f / sqrtf((tx * tx + ty * ty) + tz * tz);
    float4 *r = rays + (size_t)i * 3u;
    r[0] = make_float4(u.cam_pos[0], u.cam_pos[1], u.cam_pos[2], __uint_as_float(3u));
    r[1] = make_float4(tx * inv, ty * inv, tz * inv, __builtin_inff());
    r[2] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
}

inline uint32_t align16(uint32_t v) { return (v + 15u) & ~15u; }

// LDS layout of the stage-level tracer for this context's scene: what trg_trace plans (trg_capi.cpp plan_lds: the frame-serial plan)
struct TracePlan { bool lds_scene; uint32_t stack_off, total, klds, overflow_levels; };
bool plan_trace_as(const trg_ctx *c, TracePlan &p, bool lds_scene) {
    p.lds_scene = lds_scene;
    uint32_t levels;
    if (lds_scene) {
        levels = c->bvh_depth + 2;
        p.klds = levels;
    } else {
        levels = TRG_WIDE8 ? 2 * c->bvh_depth4 + 4 : wide_stack_levels(c->bvh_depth4);
        p.klds = levels < (uint32_t)c->opt_stack_levels ? levels : (uint32_t)c->opt_stack_levels;
    }
    p.overflow_levels = levels - p.klds;
    p.stack_off = lds_scene ? align16(c->sc.lds_stage_bytes) : 0u;
    const uint32_t red_off = p.stack_off + p.klds * (uint32_t)kBlock * 4u;
    p.total = align16(red_off + 4u * 8u * 4u);
    if (!lds_scene) p.total += (uint32_t)kBlock * 40u;
    return p.total <= 64u * 1024u;
}
int plan_trace(trg_ctx *c, TracePlan &p) {
    const bool want_lds = !c->opt_force_global && c->sc.lds_stage_bytes != 0 && c->sc.lds_stage_bytes <= kMaxLdsScene;
    if (want_lds && plan_trace_as(c, p, true)) return TRG_OK;
    if (plan_trace_as(c, p, false)) return TRG_OK;
    return fail(c, TRG_ERR_RANGE, "denoise: BVH depth %u needs %u B of LDS per workgroup", c->bvh_depth, p.total);
}

// enqueues the map original primitive index -> leaf record of the loaded scene.  Rebuilt per call (one 4-byte read per record): a scene may
// have been reloaded into the same allocation since
int record_map(trg_ctx *c, DenoiseState &s, const char *who) {
    const SceneDesc &sc = c->sc;
    if (int rc = grow(c, s.rec_of_prim, s.prims, (size_t)sc.n_tris, sizeof(uint32_t), "record map")) return rc;
    DN_HIPCHK(c, hipMemsetAsync(s.rec_of_prim, 0, (size_t)sc.n_tris * sizeof(uint32_t), c->stream));
    return launch_each(c, who, dn_record_map_kernel, sc.n_fat, reinterpret_cast<const float4 *>(c->blob + sc.off_fat), sc.n_fat, sc.n_tris, s.rec_of_prim);
}

// ---- moving geometry: the previous scene and the motion planes (trg_denoise.h, MOVING GEOMETRY) ----
// One record per ORIGINAL primitive index, five float4: (P0.xyz P1.x) (P1.yz P2.xy) (P2.z N0.xyz) (N1.xyz N2.x) (N2.yz 0 0)
constexpr uint32_t kPrevRecord = 5;

// the records from buffers that are on the device already (trg_temporal_set_previous_scene_device), one thread per triangle.  An index out of range is
// CLAMPED to the last vertex, as the refit unit clamps it: nothing is read out of bounds
__global__ void dn_prev_pack_kernel(const float *pos, const float *nrm, const uint32_t *idx, uint32_t n_verts, uint32_t n_tris, float4 *prev) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tris) return;
    float r[20];
    for (int corner = 0; corner < 3; ++corner) {
        uint32_t i = idx[(size_t)t * 3u + corner];
        if (i >= n_verts) i = n_verts - 1u;
        for (int k = 0; k < 3; ++k) {
            r[corner * 3 + k] = pos[(size_t)i * 3u + k];
            r[9 + corner * 3 + k] = nrm ? nrm[((size_t)t * 3u + corner) * 3u + k] : 0.0f;
        }
    }
    r[18] = r[19] = 0.0f;
    float4 *rec = prev + (size_t)t * kPrevRecord;
    for (int q = 0; q < 5; ++q) rec[q] = make_float4(r[4 * q], r[4 * q + 1], r[4 * q + 2], r[4 * q + 3]);
}

// M0 = (the hit's barycentrics over the previous corners, 1), M1 = (the same over the previous normals, 0); zero on a miss -- the gather's test.
// NORMALS = false: the previous scene came without normals, M1 = (G0.xyz, 0) and the two normal rows of the record are not read.
template <bool NORMALS>
__global__ void dn_motion_kernel(const trg_isect *isect, const float4 *prev, uint32_t n_prims, const float4 *g0, float4 *m0, float4 *m1, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 is = reinterpret_cast<const float4 *>(isect)[i];   // distance, primitiveIndex, coordinates[2]
    const int prim = __float_as_int(is.y);
    if (!(is.x >= 0.0f) || prim < 0 || (uint32_t)prim >= n_prims) {
        m0[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        m1[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float4 *rec = prev + (size_t)prim * kPrevRecord;
    const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
    const float c0 = is.z, c1 = is.w, c2 = 1.0f - c0 - c1;
    m0[i] = make_float4((c0 * r0.x + c1 * r0.w) + c2 * r1.z, (c0 * r0.y + c1 * r1.x) + c2 * r1.w, (c0 * r0.z + c1 * r1.y) + c2 * r2.x, 1.0f);
    if (NORMALS) {
        const float4 r3 = rec[3], r4 = rec[4];
        m1[i] = make_float4((c0 * r2.y + c1 * r3.x) + c2 * r3.w, (c0 * r2.z + c1 * r3.y) + c2 * r4.x, (c0 * r2.w + c1 * r3.z) + c2 * r4.y, 0.0f);
    } else {
        const float4 g = g0[i];
        m1[i] = make_float4(g.x, g.y, g.z, 0.0f);
    }
}

// is there a previous scene for the scene that is loaded?
bool have_previous_scene(const trg_ctx *c, const DenoiseState &s) { return c->scene_loaded && s.prev_tris != 0 && s.prev_tris == c->sc.n_tris; }

// pos (may be null): the world-position plane of trg_guides_render_pos; motion (may be null, needs pos): behind it the two motion planes of
// trg_guides_render_motion (the caller has checked have_previous_scene).  centre (may be null, needs pos): the tolerances of
// trg_guides_render_centre -- the guides come from the rays through the pixel centres and pos.w is the agreement flag
struct CentreTol { float plane_tol, normal_tol; };
int guides_render(trg_ctx *c, DenoiseState &s, uint32_t frameIndex, float4 *guides, float4 *pos = nullptr, float4 *motion = nullptr, const CentreTol *centre = nullptr) {
    if (!c->scene_loaded) return fail(c, TRG_ERR_INVALID, "trg_guides_render: no scene loaded");
    if (!c->have_uniforms || !c->have_offsets) return fail(c, TRG_ERR_INVALID, "trg_guides_render: uniforms / pixel offsets not set");
    const size_t n = (size_t)c->w * c->h;
    if (n > 0x7FFFFFFFull) return fail(c, TRG_ERR_RANGE, "trg_guides_render: image too large");
    const SceneDesc &sc = c->sc;
    if (sc.n_tris == 0 || sc.n_fat == 0) return fail(c, TRG_ERR_INVALID, "trg_guides_render: empty scene");
    TracePlan plan;
    if (int rc = plan_trace(c, plan)) return rc;
    TraceParams tp{};
    tp.sc = sc; tp.rays = s.rays; tp.out = s.isect; tp.n = (uint32_t)n; tp.stack_off = plan.stack_off;
    tp.stack.klds = plan.klds; tp.stack.overflow = nullptr;
    if (plan.overflow_levels) {
        const size_t grid_threads = ((n + kBlock - 1) / kBlock) * kBlock;
        if (int rc = grow(c, s.overflow, s.overflow_bytes, (size_t)plan.overflow_levels * grid_threads * sizeof(int), 1, "stack scratch")) return rc;
        tp.stack.overflow = s.overflow;
    }
    hipStream_t st = c->stream;
    trg_uniforms u = c->u;
    u.frameIndex = frameIndex;
    if (centre) {
        if (int rc = lazy_scratch(c, s, s.rays_j, "the jittered rays")) return rc;
        if (int rc = lazy_scratch(c, s, s.isect_j, "the jittered hit records")) return rc;
    }
    // the frame's jittered rays: the guides' own, or with `centre` the ones the agreement flag tests, into the second scratch
    trg_ray *const jrays = centre ? s.rays_j : s.rays;
    tp.rays = jrays; tp.out = centre ? s.isect_j : s.isect;
    hipError_t e = (c->opt_strict ? launch_raygen_strict : launch_raygen_fast)(u, c->offsets, jrays, st);
    if (e != hipSuccess) return fail(c, TRG_ERR_DEVICE, "trg_guides_render: raygen launch failed: %s", hipGetErrorString(e));
    e = (c->opt_strict ? launch_trace_strict : launch_trace_fast)(tp, plan.lds_scene, false, plan.total, st);
    if (e != hipSuccess) return fail(c, TRG_ERR_DEVICE, "trg_guides_render: trace launch failed: %s", hipGetErrorString(e));
    if (centre) {
        // the centre rays and, LAST, their trace: s.isect holds the centre hits for the gather and the motion kernel
        if (int rc = launch_each(c, "trg_guides_render_centre", dn_centre_raygen_kernel, n, u, c->w, c->h, reinterpret_cast<float4 *>(s.rays))) return rc;
        tp.rays = s.rays; tp.out = s.isect;
        e = (c->opt_strict ? launch_trace_strict : launch_trace_fast)(tp, plan.lds_scene, false, plan.total, st);
        if (e != hipSuccess) return fail(c, TRG_ERR_DEVICE, "trg_guides_render_centre: trace launch failed: %s", hipGetErrorString(e));
    }
    if (int rc = record_map(c, s, "trg_guides_render")) return rc;
    if (centre) {
        if (int rc = launch_each(c, "trg_guides_render_centre", dn_gather_agree_kernel, n, s.isect, s.rec_of_prim, reinterpret_cast<const float4 *>(c->blob + sc.off_fat),
                                 sc.n_tris, c->tex, guides, guides + n, n, s.rays, pos, GatherAgree{ s.isect_j, s.rays_j, centre->plane_tol, centre->normal_tol }))
            return rc;
    } else
    if (int rc = launch_each(c, "trg_guides_render", pos ? dn_gather_kernel<true> : dn_gather_kernel<false>, n, s.isect, s.rec_of_prim,
                             reinterpret_cast<const float4 *>(c->blob + sc.off_fat), sc.n_tris, c->tex, guides, guides + n, n, pos ? s.rays : nullptr, pos))
        return rc;
    if (!motion) return TRG_OK;
    return launch_each(c, "trg_guides_render_motion", s.prev_normals ? dn_motion_kernel<true> : dn_motion_kernel<false>, n, s.isect, s.prev_geo, s.prev_tris, guides,
                       motion, motion + n, n);
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// The filter (trg_denoise.h has the definition)
// ---------------------------------------------------------------------------------------------------------------------------------------------
// The filter's own copy of G0: a pixel whose first hit is an EMITTER of the loaded scene (G1.w names a primitive of material
// TRG_MATERIAL_EMISSIVE) gets distance -1, i.e. the filter treats it exactly like a miss -- it copies its input and is nobody's tap.
// n_prims == 0 (no scene): a plain copy.
__global__ void dn_exclude_emitters_kernel(const float4 *g0, const float4 *g1, const uint32_t *rec_of_prim, const float4 *recs, uint32_t n_prims,
                                           float4 *fguide, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float4 g = g0[i];
    const int prim = __float_as_int(g1[i].w);
    if (g.w >= 0.0f && prim >= 0 && (uint32_t)prim < n_prims &&
        (uint32_t)__float_as_int(recs[(size_t)rec_of_prim[prim] * 8u + 1u].w) == TRG_MATERIAL_EMISSIVE)
        g.w = -1.0f;
    fguide[i] = g;
}

struct AtrousParams {
    const float4 *in, *g0, *g1;
    float4 *out;
    int w, h, spacing;
    int demod_in, remod_out;   // first / last launch of a demodulated run
    float sigma_color, sigma_normal, sigma_depth;   // (variance-guided form: sigma_color holds sigma_lum)
    // variance-guided form only: the last launch takes alpha from H1 and, when asked, writes the variance it carried to a plane of floats
    int last;
    const float4 *alpha;
    float *var_out;
};
constexpr int kDnLdsMaxSpacing = 2;              // spacings 1, 2: tile + halo of 2 * spacing pixels in LDS
constexpr int kDnLdsSide = kDnTile + 4 * kDnLdsMaxSpacing;   // 24
static_assert(kTileW == kDnTile && kTileH == kDnTile && kBlock == 256, "the filter's tiles are the render kernels' 16 x 16 tiles");

template <bool STRICT> __device__ __forceinline__ float dn_exp(float x) { return STRICT ? expf(x) : __expf(x); }
template <bool STRICT> __device__ __forceinline__ float dn_pow(float x, float y) { return STRICT ? powf(x, y) : __powf(x, y); }
template <bool STRICT> __device__ __forceinline__ float dn_sqrt(float x) { return STRICT ? sqrtf(x) : __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float dn_lum(const float4 c) { return 0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z; }
// c.rgb / max(albedo, 1e-3) and c.rgb * max(albedo, 1e-3) of the header
__device__ __forceinline__ float4 dn_demodulate(const float4 c, const float4 a) { return make_float4(c.x / fmaxf(a.x, 1e-3f), c.y / fmaxf(a.y, 1e-3f), c.z / fmaxf(a.z, 1e-3f), c.w); }
__device__ __forceinline__ float4 dn_remodulate(const float4 c, const float4 a) { return make_float4(c.x * fmaxf(a.x, 1e-3f), c.y * fmaxf(a.y, 1e-3f), c.z * fmaxf(a.z, 1e-3f), c.w); }

// g_p of the header: forward differences of the depth, backward where the forward neighbour is outside the image or a miss
template <typename Guide>
__device__ __forceinline__ float dn_depth_gradient(const Guide &guide, int x, int y, int w, int h, float zp) {
    float gx = 0.0f, gy = 0.0f;
    float z1 = -1.0f;
    if (x + 1 < w) z1 = guide(x + 1, y).w;
    if (z1 >= 0.0f) gx = z1 - zp;
    else if (x >= 1) { z1 = guide(x - 1, y).w; if (z1 >= 0.0f) gx = zp - z1; }
    z1 = -1.0f;
    if (y + 1 < h) z1 = guide(x, y + 1).w;
    if (z1 >= 0.0f) gy = z1 - zp;
    else if (y >= 1) { z1 = guide(x, y - 1).w; if (z1 >= 0.0f) gy = zp - z1; }
    return sqrtf(gx * gx + gy * gy);
}

// k w_n w_z of the header, multiplied in that order, for the tap q = p + s (dx, dy) with n_p . n_q = dn > 0 and the depths zp, zq
template <bool STRICT>
__device__ __forceinline__ float dn_geometry_weight(float k, float dn, float zp, float zq, float grad, float s, int dx, int dy, float sigma_normal, float sigma_depth) {
    const float wn = dn_pow<STRICT>(dn, sigma_normal);
    const float dist = sqrtf((float)(dx * dx + dy * dy));
    const float wz = dn_exp<STRICT>(-(fabsf(zp - zq) / (sigma_depth * (grad * s * dist + 1e-6f))));
    return k * wn * wz;
}

// VAR = true: the variance-guided form (trg_denoise_variance): the .w of the colour plane is V_i, the colour weight is w_l, scaled by the 3 x 3
// binomial of V around p, and V_{i+1} is written beside I_{i+1}.
// LDS = true: colour (already demodulated) and G0 of the tile + halo sit in LDS as [row][x] float4 -- a wavefront's four rows of 16 lanes read
// 16 consecutive float4 each; false: every tap is a global_load_dwordx4 per plane (neighbouring lanes' taps fall on the same 128-byte lines).
template <bool STRICT, bool LDS, bool VAR>
__global__ __launch_bounds__(256) void dn_atrous_kernel(const AtrousParams p) {
    __shared__ float4 s_col[LDS ? kDnLdsSide * kDnLdsSide : 1];
    __shared__ float4 s_g0[LDS ? kDnLdsSide * kDnLdsSide : 1];
    const int s = p.spacing, halo = 2 * s, side = kDnTile + 2 * halo;   // side <= kDnLdsSide when LDS
    const int x0 = (int)blockIdx.x * kDnTile, y0 = (int)blockIdx.y * kDnTile;
    if (LDS) {
        for (int k = (int)threadIdx.x; k < side * side; k += 256) {
            const int ly = k / side, lx = k - ly * side;
            const int gx = x0 - halo + lx, gy = y0 - halo + ly;
            float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
            if (gx >= 0 && gx < p.w && gy >= 0 && gy < p.h) {
                const size_t q = (size_t)gy * (size_t)p.w + (size_t)gx;
                c = p.in[q];
                g = p.g0[q];
                if (p.demod_in && g.w >= 0.0f) c = dn_demodulate(c, p.g1[q]);
            }
            s_col[k] = c;
            s_g0[k] = g;
        }
        __syncthreads();
    }
    const int x = x0 + ((int)threadIdx.x & 15), y = y0 + ((int)threadIdx.x >> 4);
    if (x >= p.w || y >= p.h) return;
    // (callers pass coordinates inside the image only)
    auto colour = [&](int qx, int qy) -> float4 { return LDS ? s_col[(qy - y0 + halo) * side + (qx - x0 + halo)] : p.in[(size_t)qy * (size_t)p.w + (size_t)qx]; };
    auto guide = [&](int qx, int qy) -> float4 { return LDS ? s_g0[(qy - y0 + halo) * side + (qx - x0 + halo)] : p.g0[(size_t)qy * (size_t)p.w + (size_t)qx]; };
    const size_t pix = (size_t)y * (size_t)p.w + (size_t)x;
    const float4 cp = colour(x, y), gp = guide(x, y);
    if (gp.w < 0.0f) {   // a miss copies its input
        float4 o = cp;
        if (VAR && p.last) {
            if (p.var_out) p.var_out[pix] = cp.w;
            o.w = p.alpha[pix].w;
        }
        p.out[pix] = o;
        return;
    }
    float var = 0.0f;
    if (VAR) {
        // GV(p): the 3 x 3 binomial of V over the pixels inside the image that are not misses, renormalised (p itself is one of them)
        const float bk[3] = { 0.25f, 0.5f, 0.25f };
        float vs = 0.0f, bs = 0.0f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int qx = x + k % 3 - 1, qy = y + k / 3 - 1;
            if (qx < 0 || qx >= p.w || qy < 0 || qy >= p.h) continue;
            if (guide(qx, qy).w < 0.0f) continue;
            const float b = bk[k % 3] * bk[k / 3];
            vs += b * colour(qx, qy).w;
            bs += b;
        }
        var = vs / bs;
    } else {
        // variance of luminance over the 3 x 3 window (two passes: mean, then squared deviations)
        float lum[9];
        int m = 0;
        float mean = 0.0f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int qx = x + k % 3 - 1, qy = y + k / 3 - 1;
            const bool in = qx >= 0 && qx < p.w && qy >= 0 && qy < p.h;
            lum[k] = in ? dn_lum(colour(qx, qy)) : 0.0f;
            mean += lum[k];
            m += in ? 1 : 0;
        }
        mean = mean / (float)m;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int qx = x + k % 3 - 1, qy = y + k / 3 - 1;
            const bool in = qx >= 0 && qx < p.w && qy >= 0 && qy < p.h;
            const float d = lum[k] - mean;
            var += in ? d * d : 0.0f;
        }
        var = var / (float)m;
    }
    const float grad = dn_depth_gradient(guide, x, y, p.w, p.h, gp.w);
    // the denominator of the colour term: w_c's sigma_color^2 (var + 1e-4), w_l's sigma_lum sqrt(max(0, GV)) + 1e-3
    const float cden = VAR ? p.sigma_color * dn_sqrt<STRICT>(fmaxf(0.0f, var)) + 1e-3f : p.sigma_color * p.sigma_color * (var + 1e-4f);
    const float lp = VAR ? dn_lum(cp) : 0.0f;
    // VAR squares a weight that w_n lets grow to 1e20 for normals longer than 1 (and shrink to 1e-25 for shorter ones): every weight times 2^-k,
    // k = the exponent of the centre's own w_n within [-126, 126], as the lag correction does -- exact, and it cancels in both quotients
    float scale = 1.0f;
    if (VAR) {
        const float nn = gp.x * gp.x + gp.y * gp.y + gp.z * gp.z;
        const float own = nn > 0.0f ? dn_pow<STRICT>(nn, p.sigma_normal) : 1.0f;
        int k2 = (int)((__float_as_uint(own) >> 23) & 255u) - 127;
        k2 = k2 < -126 ? -126 : (k2 > 126 ? 126 : k2);
        scale = __uint_as_float((uint32_t)(127 - k2) << 23);
    }
    const float hk[5] = { 1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f };
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, av = 0.0f, wsum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * s, qy = y + dy * s;
            if (qx < 0 || qx >= p.w || qy < 0 || qy >= p.h) continue;
            const float4 gq = guide(qx, qy);
            if (gq.w < 0.0f) continue;
            const float dn = gp.x * gq.x + gp.y * gq.y + gp.z * gq.z;
            if (!(dn > 0.0f)) continue;
            const float4 cq = colour(qx, qy);
            const float wg = dn_geometry_weight<STRICT>(hk[dx + 2] * hk[dy + 2], dn, gp.w, gq.w, grad, (float)s, dx, dy, p.sigma_normal, p.sigma_depth);
            float wc;
            if (VAR) {
                wc = dn_exp<STRICT>(-(fabsf(lp - dn_lum(cq)) / cden));
            } else {
                const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
                wc = dn_exp<STRICT>(-((dr * dr + dg * dg + db * db) / cden));
            }
            const float wgt = VAR ? (wg * scale) * wc : wg * wc;
            ar += wgt * cq.x; ag += wgt * cq.y; ab += wgt * cq.z;
            if (VAR) av += wgt * wgt * cq.w;
            wsum += wgt;
        }
    }
    float4 o = cp;
    if (wsum > 0.0f) {
        o.x = ar / wsum; o.y = ag / wsum; o.z = ab / wsum;
        if (VAR) o.w = av / (wsum * wsum);
    }
    if (VAR && p.last) {
        if (p.var_out) p.var_out[pix] = o.w;
        o.w = p.alpha[pix].w;
    }
    if (p.remod_out) o = dn_remodulate(o, p.g1[pix]);
    p.out[pix] = o;
}

bool overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    return (const char *)a < (const char *)b + b_bytes && (const char *)b < (const char *)a + a_bytes;
}
// are these buffers pairwise disjoint?  (a null pointer is a buffer the call does not have)
struct Span { const void *mem; size_t bytes; };
bool disjoint(std::initializer_list<Span> spans) {
    for (const Span *a = spans.begin(); a != spans.end(); ++a)
        for (const Span *b = a + 1; b != spans.end(); ++b)
            if (a->mem && b->mem && overlap(a->mem, a->bytes, b->mem, b->bytes)) return false;
    return true;
}

// the leading fields that the three parameter structures share (sigma_color of the plain filter, sigma_lum of the other two)
bool valid_filter(int iterations, float sigma_color, float sigma_normal, float sigma_depth) {
    return iterations >= 0 && iterations <= TRG_DENOISE_MAX_ITERATIONS && sigma_color > 0.0f && sigma_normal >= 0.0f && sigma_depth > 0.0f;
}
bool valid_params(const trg_denoise_params &q) { return valid_filter(q.iterations, q.sigma_color, q.sigma_normal, q.sigma_depth); }

// enqueues the filter's copy of G0 (s.fguide) with the emitters of the loaded scene marked as misses
int exclude_emitters(trg_ctx *c, DenoiseState &s, const float4 *guides, const char *who) {
    const size_t n = (size_t)c->w * c->h;
    const bool scene = c->scene_loaded && c->sc.n_tris != 0 && c->sc.n_fat != 0;
    if (scene)
        if (int rc = record_map(c, s, who)) return rc;
    return launch_each(c, who, dn_exclude_emitters_kernel, n, guides, guides + n, s.rec_of_prim,
                       scene ? reinterpret_cast<const float4 *>(c->blob + c->sc.off_fat) : nullptr, scene ? c->sc.n_tris : 0u, s.fguide, n);
}

// what the launches of one run of the filter share
AtrousParams atrous_params(const trg_ctx *c, const DenoiseState &s, const float4 *guides, float sigma_color, float sigma_normal, float sigma_depth) {
    AtrousParams p{};
    p.g0 = s.fguide; p.g1 = guides + (size_t)c->w * c->h;
    p.w = (int)c->w; p.h = (int)c->h;
    p.sigma_color = sigma_color; p.sigma_normal = sigma_normal; p.sigma_depth = sigma_depth;
    return p;
}
// The filter's iterations 0 .. N-1 from `src` to `out`, spacing 2^i: every launch but the last writes whichever of the state's ping / pong is not
// its source; the first launch demodulates and the last one remodulates when asked.  VAR: the variance-guided form, p.alpha and p.var_out set
template <bool VAR>
int atrous_run(trg_ctx *c, DenoiseState &s, const char *who, AtrousParams p, const float4 *src, float4 *out, int iterations, bool demod_first, bool remod_last) {
    for (int i = 0; i < iterations; ++i) {
        const bool last = i + 1 == iterations;
        p.in = src;
        p.out = last ? out : (src == s.ping ? s.pong : s.ping);
        p.spacing = 1 << i;
        p.demod_in = (demod_first && i == 0) ? 1 : 0;
        p.remod_out = (remod_last && last) ? 1 : 0;
        p.last = last ? 1 : 0;
        const auto kernel = p.spacing <= kDnLdsMaxSpacing ? DN_FOR_SETTING(c, dn_atrous_kernel, true, VAR) : DN_FOR_SETTING(c, dn_atrous_kernel, false, VAR);
        if (int rc = launch_tiles(c, who, kernel, p)) return rc;
        src = p.out;
    }
    return TRG_OK;
}

int denoise(trg_ctx *c, DenoiseState &s, const float4 *in, const float4 *guides, float4 *out, const trg_denoise_params *pp) {
    trg_denoise_params q;
    trg_denoise_default_params(&q);
    if (pp) q = *pp;
    if (!valid_params(q)) return fail(c, TRG_ERR_INVALID, "trg_denoise: iterations must be 0..%d and the sigmas positive", TRG_DENOISE_MAX_ITERATIONS);
    const size_t n = (size_t)c->w * c->h, bytes = n * sizeof(float4);
    if (overlap(out, bytes, in, bytes)) return fail(c, TRG_ERR_INVALID, "trg_denoise: out_device overlaps color_in_device");
    if (q.iterations == 0) {
        DN_HIPCHK(c, hipMemcpyAsync(out, in, bytes, hipMemcpyDeviceToDevice, c->stream));
        return TRG_OK;
    }
    if (int rc = exclude_emitters(c, s, guides, "trg_denoise")) return rc;
    return atrous_run<false>(c, s, "trg_denoise", atrous_params(c, s, guides, q.sigma_color, q.sigma_normal, q.sigma_depth), in, out, q.iterations, q.demodulate != 0,
                             q.demodulate != 0);
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// The variance-guided filter from two half-sample buffers (trg_denoise.h has the definition)
// ---------------------------------------------------------------------------------------------------------------------------------------------
// H1.rgb = A.rgb * f1, H2.rgb = B.rgb * f2, alpha copied: the running averages trg_render left in two zeroed images, as means of their halves
__global__ void dn_scale_halves_kernel(const float4 *a, const float4 *b, float4 *h1, float4 *h2, float f1, float f2, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float4 u = a[i], v = b[i];
    u.x = u.x * f1; u.y = u.y * f1; u.z = u.z * f1;
    v.x = v.x * f2; v.y = v.y * f2; v.z = v.z * f2;
    h1[i] = u;
    h2[i] = v;
}

// (I_0, V_0) of the header into one float4 plane.  plain: iterations == 0, out = (0.5 (H1 + H2), H1.a)
__global__ void dn_var_combine_kernel(const float4 *h1, const float4 *h2, const float4 *fguide, const float4 *g1, float4 *out, int demod, int plain,
                                      uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float4 a = h1[i], b = h2[i];
    if (plain) {
        out[i] = make_float4(0.5f * (a.x + b.x), 0.5f * (a.y + b.y), 0.5f * (a.z + b.z), a.w);
        return;
    }
    const bool miss = fguide[i].w < 0.0f;
    if (demod && !miss) {
        const float4 al = g1[i];
        a = dn_demodulate(a, al);
        b = dn_demodulate(b, al);
    }
    const float d = dn_lum(a) - dn_lum(b);
    out[i] = make_float4(0.5f * (a.x + b.x), 0.5f * (a.y + b.y), 0.5f * (a.z + b.z), miss ? 0.0f : 0.25f * (d * d));
}

__global__ void dn_var_extract_kernel(const float4 *in, float *var, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) var[i] = in[i].w;
}

// The 7 x 7 geometry window at spacing 1, g = w_n w_z w_id, of the prefilter of V_0, of the temporal step's spatial estimate and of the lag
// correction: the one place that stages, tests and walks it.  A user's payload is a structure `Planes` -- one array of kDnPreArea per staged plane
// ([row][x] like s_g0 here: a wavefront's four rows of 16 lanes read 16 consecutive elements each), a `Pixel` (zeros: a pixel outside the image)
// and put / get of a pixel at a slot -- and three pieces:
//   load(q, g)                  the payload of pixel q, whose (filter's) G0 is g; by the whole workgroup, for the tile + 3 pixels of halo;
//   centre(pixel, own_weight)   once, by a thread with `active` set (a pixel inside the image) whose pixel is no miss: its own payload, and
//                               own_weight() = the weight of the centre tap (1 for a zero normal, which has no tap); returns the factor on every g;
//   tap(pixel, g)               for each tap that counts -- inside the image, no miss, n_p . n_q > 0 --, rows outer, columns inner.
// True for the threads that walked the window.
constexpr int kDnPreR = 3;
constexpr int kDnPreSide = kDnTile + 2 * kDnPreR;   // 22
constexpr int kDnPreArea = kDnPreSide * kDnPreSide;
template <int NP> struct alignas(4 * NP) DnPayload { float v[NP]; };
template <bool STRICT, typename Planes, typename Load, typename Centre, typename Tap>
__device__ __forceinline__ bool dn_window7(const float4 *g0, int w, int h, float sigma_normal, float sigma_depth, bool active, const Load load, const Centre centre,
                                           const Tap tap) {
    __shared__ float4 s_g0[kDnPreArea];
    __shared__ Planes s_p;
    const int x0 = (int)blockIdx.x * kDnTile, y0 = (int)blockIdx.y * kDnTile;
    for (int k = (int)threadIdx.x; k < kDnPreArea; k += 256) {
        const int ly = k / kDnPreSide, lx = k - ly * kDnPreSide;
        const int gx = x0 - kDnPreR + lx, gy = y0 - kDnPreR + ly;
        float4 g = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        typename Planes::Pixel v{};
        if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
            const size_t q = (size_t)gy * (size_t)w + (size_t)gx;
            g = g0[q];
            v = load(q, g);
        }
        s_g0[k] = g;
        s_p.put(k, v);
    }
    __syncthreads();
    if (!active) return false;
    const int x = x0 + ((int)threadIdx.x & 15), y = y0 + ((int)threadIdx.x >> 4);
    auto slot = [&](int qx, int qy) -> int { return (qy - y0 + kDnPreR) * kDnPreSide + (qx - x0 + kDnPreR); };
    auto guide = [&](int qx, int qy) -> float4 { return s_g0[(qy - y0 + kDnPreR) * kDnPreSide + (qx - x0 + kDnPreR)]; };   // (through slot() it costs the linear users three VGPRs)
    const float4 gp = guide(x, y);
    if (gp.w < 0.0f) return false;
    const float grad = dn_depth_gradient(guide, x, y, w, h, gp.w);
    const float scale = centre(s_p.get(slot(x, y)), [&]() -> float {
        const float nn = gp.x * gp.x + gp.y * gp.y + gp.z * gp.z;
        return nn > 0.0f ? dn_geometry_weight<STRICT>(1.0f, nn, gp.w, gp.w, grad, 1.0f, 0, 0, sigma_normal, sigma_depth) : 1.0f;
    });
#pragma unroll
    for (int dy = -kDnPreR; dy <= kDnPreR; ++dy) {
#pragma unroll
        for (int dx = -kDnPreR; dx <= kDnPreR; ++dx) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
            const float4 gq = guide(qx, qy);
            if (gq.w < 0.0f) continue;
            const float dn = gp.x * gq.x + gp.y * gq.y + gp.z * gq.z;
            if (!(dn > 0.0f)) continue;
            const float g = dn_geometry_weight<STRICT>(1.0f, dn, gp.w, gq.w, grad, 1.0f, dx, dy, sigma_normal, sigma_depth) * scale;
            tap(s_p.get(slot(qx, qy)), g);
        }
    }
    return true;
}
// The window whose sums are linear in a payload of NP floats per pixel, read by `load(q)` (an absent pixel holds zeros): sum[k] = the g-weighted
// sum of payload k, gs = the sum of g
template <bool STRICT, int NP, typename Load>
__device__ __forceinline__ bool dn_window7_sums(const float4 *g0, const Load load, int w, int h, float sigma_normal, float sigma_depth, bool active, float (&sum)[NP],
                                                float &gs) {
    struct Planes {
        using Pixel = DnPayload<NP>;
        Pixel v[kDnPreArea];
        __device__ void put(int k, const Pixel &p) { v[k] = p; }
        __device__ Pixel get(int k) const { return v[k]; }
    };
    return dn_window7<STRICT, Planes>(
        g0, w, h, sigma_normal, sigma_depth, active, [&](size_t q, const float4 &) { return load(q); },
        [&](const DnPayload<NP> &, const auto &) {
            gs = 0.0f;
            for (int j = 0; j < NP; ++j) sum[j] = 0.0f;
            return 1.0f;
        },
        [&](const DnPayload<NP> &v, float g) {
            for (int j = 0; j < NP; ++j) sum[j] += g * v.v[j];
            gs += g;
        });
}

// The prefilter of V_0: the payload is V; the colour passes through, and a miss keeps V_0 = 0
template <bool STRICT>
__global__ __launch_bounds__(256) void dn_var_prefilter_kernel(const float4 *in, const float4 *g0, float4 *out, int w, int h, float sigma_normal,
                                                               float sigma_depth) {
    const int x = (int)blockIdx.x * kDnTile + ((int)threadIdx.x & 15), y = (int)blockIdx.y * kDnTile + ((int)threadIdx.x >> 4);
    const bool inside = x < w && y < h;
    float vs[1], gs;
    const bool hit = dn_window7_sums<STRICT, 1>(g0, [&](size_t q) { return DnPayload<1>{ { in[q].w } }; }, w, h, sigma_normal, sigma_depth, inside, vs, gs);
    if (!inside) return;
    const size_t pix = (size_t)y * (size_t)w + (size_t)x;
    float4 o = in[pix];
    if (hit && gs > 0.0f) o.w = vs[0] / gs;
    out[pix] = o;
}

bool valid_var_params(const trg_denoise_var_params &q) { return valid_filter(q.iterations, q.sigma_lum, q.sigma_normal, q.sigma_depth); }

// var_out (may be null): a plane of width*height floats for V_N
int denoise_variance(trg_ctx *c, DenoiseState &s, const float4 *halves, const float4 *guides, float4 *out, float *var_out, const trg_denoise_var_params *pp) {
    const char *const who = "trg_denoise_variance";
    trg_denoise_var_params q;
    trg_denoise_var_default_params(&q);
    if (pp) q = *pp;
    if (!valid_var_params(q)) return fail(c, TRG_ERR_INVALID, "trg_denoise_variance: iterations must be 0..%d and the sigmas positive", TRG_DENOISE_MAX_ITERATIONS);
    const size_t n = (size_t)c->w * c->h, bytes = n * sizeof(float4);
    if (overlap(out, bytes, halves, 2 * bytes)) return fail(c, TRG_ERR_INVALID, "trg_denoise_variance: out_device overlaps halves_device");
    const float4 *h1 = halves, *h2 = halves + n;
    if (q.iterations == 0 && !var_out) return launch_each(c, who, dn_var_combine_kernel, n, h1, h2, nullptr, nullptr, out, 0, 1, n);
    if (int rc = exclude_emitters(c, s, guides, who)) return rc;
    if (int rc = launch_each(c, who, dn_var_combine_kernel, n, h1, h2, s.fguide, guides + n, s.ping, q.demodulate ? 1 : 0, 0, n)) return rc;
    const float4 *src = s.ping;
    if (q.prefilter) {
        if (int rc = launch_tiles(c, who, DN_FOR_SETTING(c, dn_var_prefilter_kernel), src, s.fguide, s.pong, c->w, c->h, q.sigma_normal, q.sigma_depth)) return rc;
        src = s.pong;
    }
    if (q.iterations == 0) {   // only the variance was asked for beside the plain mean
        if (int rc = launch_each(c, who, dn_var_extract_kernel, n, src, var_out, n)) return rc;
        return launch_each(c, who, dn_var_combine_kernel, n, h1, h2, nullptr, nullptr, out, 0, 1, n);
    }
    AtrousParams p = atrous_params(c, s, guides, q.sigma_lum, q.sigma_normal, q.sigma_depth);
    p.alpha = h1; p.var_out = var_out;
    return atrous_run<true>(c, s, who, p, src, out, q.iterations, false, q.demodulate != 0);   // (the combine kernel demodulated)
}

// trg_render of `parts` consecutive runs of n frames from b on, run k into plane k of `img`, an image of the state that is zeroed first.  The
// caller's accumulation buffer stays bound afterwards, also on failure
int render_zeroed(trg_ctx *c, float4 *img, uint32_t parts, uint32_t b, uint32_t n, uint32_t bounces) {
    const size_t npix = (size_t)c->w * c->h;
    DN_HIPCHK(c, hipMemsetAsync(img, 0, parts * npix * sizeof(float4), c->stream));
    float *const bound = c->accum;
    const bool own = bound == c->accum_own;
    int rc = TRG_OK;
    for (uint32_t k = 0; k < parts && rc == TRG_OK; ++k) {
        rc = trg_bind_accum(c, img + k * npix);
        if (rc == TRG_OK) rc = trg_render(c, b + k * n, n, bounces, 0, c->h);
    }
    (void)trg_bind_accum(c, own ? nullptr : bound);   // (cannot fail: the pointer was bound before)
    return rc;
}

int render_halves(trg_ctx *c, DenoiseState &s, uint32_t b, uint32_t n, uint32_t bounces, float4 *halves, const char *who) {
    if (n < 2u || (n & 1u)) return fail(c, TRG_ERR_INVALID, "%s: spp must be even and at least 2 (got %u): the samples are rendered as two equal halves", who, n);
    if ((uint64_t)b + n > 0xFFFFFFFFull) return fail(c, TRG_ERR_INVALID, "%s: frame range [%u, %u + %u) exceeds 32 bits", who, b, b, n);
    const size_t npix = (size_t)c->w * c->h, bytes = npix * sizeof(float4);
    if (overlap(halves, 2 * bytes, c->accum, bytes)) return fail(c, TRG_ERR_INVALID, "%s: halves_device overlaps the bound accumulation buffer", who);
    if (int rc = lazy_planes(c, s, s.half_acc, 2, "the half-sample images")) return rc;
    const uint32_t half = n / 2u;
    if (int rc = render_zeroed(c, s.half_acc, 2, b, half, bounces)) return rc;
    const float f1 = (float)((double)((uint64_t)b + half) / (double)half), f2 = (float)((double)((uint64_t)b + n) / (double)half);
    return launch_each(c, who, dn_scale_halves_kernel, npix, s.half_acc, s.half_acc + npix, halves, halves + npix, f1, f2, npix);
}

int render_denoised_variance(trg_ctx *c, DenoiseState &s, uint32_t b, uint32_t n, uint32_t bounces, float4 *out, const trg_denoise_var_params *p, const char *who) {
    if (p && !valid_var_params(*p)) return fail(c, TRG_ERR_INVALID, "%s: bad parameters", who);
    if (int rc = lazy_planes(c, s, s.halves, 2, "the half planes")) return rc;
    if (int rc = render_halves(c, s, b, n, bounces, s.halves, who)) return rc;
    if (int rc = guides_render(c, s, b, s.guides)) return rc;
    return denoise_variance(c, s, s.halves, s.guides, out, nullptr, p);
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// Temporal reprojection and accumulation (trg_denoise.h has the definition)
// ---------------------------------------------------------------------------------------------------------------------------------------------
bool valid_temporal_params(const trg_temporal_params &q) {
    return valid_filter(q.iterations, q.sigma_lum, q.sigma_normal, q.sigma_depth) && q.alpha > 0.0f && q.alpha <= 1.0f && q.alpha_moments > 0.0f &&
           q.alpha_moments <= 1.0f && q.plane_tol > 0.0f && q.normal_tol >= -1.0f && q.normal_tol <= 1.0f && q.max_history >= 1;
}

struct ReprojectParams {
    const float4 *color, *fguide, *g1, *pos;          // this frame: C, F, G1, X
    const float4 *hc, *hm, *hf, *hx;                  // the previous call's history planes (null: no history)
    float4 *oc, *om, *of, *ox, *iv;                   // the new history planes and (I, V_0)
    int w, h, demod;
    float vp[16];
    float alpha, alpha_moments, plane_tol, normal_tol, max_history;
    const float4 *m0, *m1;                            // MOTION: the previous-position planes M0, M1 (last: the other fields keep their offsets)
    float4 *fmark;                                    // COVER: the filter's G0 again (= fguide), writable: a mixed pixel marks its own .w
    float cov_min;
};

// n / |n| into (x, y, z); false when the length is not > 0
template <bool STRICT>
__device__ __forceinline__ bool dn_unit(float &x, float &y, float &z) {
    const float len = dn_sqrt<STRICT>(x * x + y * y + z * z);
    if (!(len > 0.0f)) return false;
    x = x / len; y = y / len; z = z / len;
    return true;
}

// One pixel per thread over 16 x 16 tiles.  The four planes of this frame are read coalesced (a wavefront = four rows of 16 consecutive float4);
// the four taps of the four history planes land wherever the camera moved the surface to, neighbouring lanes mostly on the same 128-byte lines
// of L2.
// MOTION (trg_temporal_denoise_motion): the history is looked for where the surface WAS -- M0.xyz takes X's place in the projection and in the
// plane test, M1.xyz the current normal's in both tests -- and only where M0.w > 0; two more coalesced float4 per pixel.
// TRACK (trg_temporal_set_variance_of_mean): Hm'.z of the float4 that is gathered anyway is the variance of the accumulated colour; it goes
// through the taps like the moments, through the recursion of the header from four frames on, and out into Hm.z and (I, V_0).w.
// COVER (trg_temporal_set_coverage): Hm'.w of the same float4 is the accumulated agreement; it goes through the taps like the moments and is blended
// with X.w, this call's agreement flag, at the moments' rate.  A hit whose result is below cov_min is MIXED: its (I, V_0) carries the remodulated
// colour and the .w of ITS OWN pixel of the filter's G0 is set to -1, so every launch behind this one treats it as a miss (the history keeps
// the unmarked guide, written before).
template <bool STRICT, bool MOTION, bool TRACK, bool COVER>
__global__ __launch_bounds__(256) void dn_temporal_reproject_kernel(const ReprojectParams p) {
    const int x = (int)blockIdx.x * kDnTile + ((int)threadIdx.x & 15), y = (int)blockIdx.y * kDnTile + ((int)threadIdx.x >> 4);
    if (x >= p.w || y >= p.h) return;
    const size_t pix = (size_t)y * (size_t)p.w + (size_t)x;
    const float4 c = p.color[pix], f = p.fguide[pix], X = p.pos[pix];
    const float4 R = MOTION ? p.m0[pix] : X;            // where the hit was when the history was written
    const float agree = COVER ? p.pos[pix].w : 0.0f;    // COVER: A(p) (read beside X: taking X apart leaves a dead copy of it in LDS)
    p.of[pix] = f;
    p.ox[pix] = X;
    if (f.w < 0.0f) {   // a miss: nothing to accumulate
        p.oc[pix] = make_float4(c.x, c.y, c.z, 0.0f);
        p.om[pix] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        p.iv[pix] = make_float4(c.x, c.y, c.z, 0.0f);
        return;
    }
    float dr = c.x, dg = c.y, db = c.z;
    if (p.demod) { const float4 d = dn_demodulate(c, p.g1[pix]); dr = d.x; dg = d.y; db = d.z; }
    const float l = dn_lum(make_float4(dr, dg, db, 0.0f));
    float ir = 0.0f, ig = 0.0f, ib = 0.0f, m1 = 0.0f, m2 = 0.0f, nh = 0.0f, W = 0.0f;
    float vh = 0.0f;                                    // TRACK: Vh
    float cov = 0.0f;                                   // COVER: covh
    float nx = f.x, ny = f.y, nz = f.z;
    if (MOTION) { const float4 pn = p.m1[pix]; nx = pn.x; ny = pn.y; nz = pn.z; }
    if (p.hc && (!MOTION || R.w > 0.0f) && dn_unit<STRICT>(nx, ny, nz)) {
        const float *m = p.vp;
        const float cx = m[0] * R.x + m[1] * R.y + m[2] * R.z + m[3];
        const float cy = m[4] * R.x + m[5] * R.y + m[6] * R.z + m[7];
        const float cw = m[12] * R.x + m[13] * R.y + m[14] * R.z + m[15];
        if (cw > 0.0f) {
            const float fx = (cx / cw * 0.5f + 0.5f) * (float)p.w - 0.5f, fy = (cy / cw * 0.5f + 0.5f) * (float)p.h - 0.5f;
            if (fx >= -1.0f && fx < (float)p.w && fy >= -1.0f && fy < (float)p.h) {   // (false for NaN)
                const float flx = floorf(fx), fly = floorf(fy);
                const int x0 = (int)flx, y0 = (int)fly;
                const float tx = fx - flx, ty = fy - fly;
                const float tol = p.plane_tol * f.w;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int i = k & 1, j = k >> 1;
                    const int qx = x0 + i, qy = y0 + j;
                    if (qx < 0 || qx >= p.w || qy < 0 || qy >= p.h) continue;
                    const size_t q = (size_t)qy * (size_t)p.w + (size_t)qx;
                    const float4 fq = p.hf[q];
                    if (!(fq.w >= 0.0f)) continue;
                    const float4 xq = p.hx[q];
                    const float dist = nx * (xq.x - R.x) + ny * (xq.y - R.y) + nz * (xq.z - R.z);
                    if (!(fabsf(dist) <= tol)) continue;
                    float qnx = fq.x, qny = fq.y, qnz = fq.z;
                    if (!dn_unit<STRICT>(qnx, qny, qnz)) continue;
                    if (!(nx * qnx + ny * qny + nz * qnz >= p.normal_tol)) continue;
                    const float b = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
                    const float4 hc = p.hc[q], hm = p.hm[q];
                    ir += b * hc.x; ig += b * hc.y; ib += b * hc.z; nh += b * hc.w;
                    m1 += b * hm.x; m2 += b * hm.y;
                    if (TRACK) vh += b * hm.z;
                    if (COVER) cov += b * hm.w;
                    W += b;
                }
            }
        }
    }
    float N = 1.0f, v0, ac = 1.0f;
    if (W > 0.0f) {
        ir = ir / W; ig = ig / W; ib = ib / W; nh = nh / W; m1 = m1 / W; m2 = m2 / W;
        if (TRACK) vh = vh / W;
        N = fminf(nh + 1.0f, p.max_history);
        const float a = fmaxf(p.alpha, 1.0f / N), am = fmaxf(p.alpha_moments, 1.0f / N);
        if (TRACK) ac = a;
        if (COVER) { cov = cov / W; cov = cov + am * (agree - cov); }
        ir = ir + a * (dr - ir); ig = ig + a * (dg - ig); ib = ib + a * (db - ib);
        m1 = m1 + am * (l - m1);
        m2 = m2 + am * (l * l - m2);
    } else {
        ir = dr; ig = dg; ib = db; m1 = l; m2 = l * l;
        if (COVER) cov = agree;
    }
    v0 = fmaxf(0.0f, m2 - m1 * m1);   // (N < 4: replaced by the spatial estimate of the next launch)
    // TRACK: Vc of the header from four frames on (without history N = 1); below, the next launch writes the spatial estimate here and into Hm.z
    if (TRACK && N >= 4.0f) v0 = ((1.0f - ac) * (1.0f - ac)) * vh + (ac * ac) * v0;
    p.oc[pix] = make_float4(ir, ig, ib, N);
    p.om[pix] = make_float4(m1, m2, TRACK ? v0 : 0.0f, COVER ? cov : 0.0f);
    if (COVER && cov < p.cov_min) {   // mixed: the remodulated colour (dn_remodulate's products), and a miss from here on
        if (p.demod) {
            const float4 a = p.g1[pix];
            ir = ir * fmaxf(a.x, 1e-3f); ig = ig * fmaxf(a.y, 1e-3f); ib = ib * fmaxf(a.z, 1e-3f);
        }
        p.fmark[pix].w = -1.0f;
    }
    p.iv[pix] = make_float4(ir, ig, ib, v0);
}

// V_0 of the pixels whose history is shorter than four frames: the variance of the moments over the 7 x 7 window, with the prefilter's weights
// (dn_window7, the payload is the two moments).  A tile in which no pixel needs it -- the usual case once the camera has stood still for four
// frames -- leaves before staging anything: one ballot per wave, four flags in LDS.
// TRACK (trg_temporal_set_variance_of_mean): V_0 also goes to Hm.z of the pixel (the one form that writes `hm`).  Other workgroups stage this
// pixel's moments at the same time, so with TRACK the staging reads the 8 bytes (m1, m2) of a pixel as a float2 and never its .z: no byte of
// the plane is read by one workgroup and written by another, and the 4-byte store lies inside one aligned dword, which a store cannot tear.
template <bool STRICT, bool TRACK>
__global__ __launch_bounds__(256) void dn_temporal_spatial_kernel(const float4 *hc, float4 *hm, const float4 *g0, float4 *iv, int w, int h,
                                                                  float sigma_normal, float sigma_depth) {
    __shared__ int s_need[4];
    const int x = (int)blockIdx.x * kDnTile + ((int)threadIdx.x & 15), y = (int)blockIdx.y * kDnTile + ((int)threadIdx.x >> 4);
    const bool inside = x < w && y < h;
    const size_t pix = inside ? (size_t)y * (size_t)w + (size_t)x : 0;
    float N = 0.0f;
    bool need = false;
    if (inside) {
        N = hc[pix].w;
        need = g0[pix].w >= 0.0f && N < 4.0f;
    }
    const unsigned long long any = __ballot(need);
    if ((threadIdx.x & 63u) == 0u) s_need[threadIdx.x >> 6] = any != 0ull ? 1 : 0;
    __syncthreads();
    if (!(s_need[0] | s_need[1] | s_need[2] | s_need[3])) return;   // (uniform over the workgroup)
    float sm[2], gs;
    const auto moments = [&](size_t q) {
        if (TRACK) { const float2 mm = *reinterpret_cast<const float2 *>(hm + q); return DnPayload<2>{ { mm.x, mm.y } }; }
        const float4 mm = hm[q];
        return DnPayload<2>{ { mm.x, mm.y } };
    };
    if (!dn_window7_sums<STRICT, 2>(g0, moments, w, h, sigma_normal, sigma_depth, need, sm, gs)) return;
    float v0 = 0.0f;
    if (gs > 0.0f) {
        const float M1 = sm[0] / gs, M2 = sm[1] / gs;
        v0 = fmaxf(0.0f, M2 - M1 * M1) * 4.0f / N;
    }
    iv[pix].w = v0;
    if (TRACK) hm[pix].z = v0;
}

// The gated lag correction of the accumulated colour (trg_denoise.h, CHANGING LIGHT) over the 7 x 7 geometry window of dn_window7; a tap needs
// the centre's D and the sums are not all linear in the payload, so the tap body is its own.  Staged per pixel: 24 bytes of payload as one float4
// (D.rgb, E.r) and one DnPayload<2> (E.g, E.b), E = D - I -- the rows read as the window's float4 and DnPayload<2> rows do, no worse on the
// banks.  I comes from (I, V_0) as the reprojection wrote it and is not written here: the corrected colour goes to .rgb of the new Hc plane and,
// with V_0, to `iv_out`, another image.
struct LagParams {
    const float4 *color, *g0, *g1, *iv_in;   // this frame: C, F, G1; (I, V_0)
    float4 *hc, *iv_out;
    int w, h, demod;
    float gate, sigma_normal, sigma_depth;
};
// one channel: I, the window sums of g E, g t and g t^2 (t = D(q) - D(p)), G and G2 -> Ic
template <bool STRICT>
__device__ __forceinline__ float dn_lag_channel(float I, float ds, float a1, float a2, float G, float G2, float gate) {
    const float d = ds / G, m1 = a1 / G;
    const float se = dn_sqrt<STRICT>(fmaxf(0.0f, a2 / G - m1 * m1) * G2) / G;
    const float m = fabsf(d) - gate * se;
    if (!(m > 0.0f)) return I;
    return fmaxf(I + copysignf(m, d), fminf(I, 0.0f));
}
template <bool STRICT>
__global__ __launch_bounds__(256) void dn_temporal_lag_kernel(const LagParams p) {
    struct Planes {
        struct Pixel { float4 d; DnPayload<2> e; };
        float4 d[kDnPreArea];
        DnPayload<2> e[kDnPreArea];
        __device__ void put(int k, const Pixel &p) { d[k] = p.d; e[k] = p.e; }
        __device__ Pixel get(int k) const { return Pixel{ d[k], e[k] }; }
    };
    const int x = (int)blockIdx.x * kDnTile + ((int)threadIdx.x & 15), y = (int)blockIdx.y * kDnTile + ((int)threadIdx.x >> 4);
    const bool inside = x < p.w && y < p.h;
    const auto load = [&](size_t q, const float4 &g) {
        float4 c = p.color[q];
        const float4 i = p.iv_in[q];
        if (p.demod && g.w >= 0.0f) c = dn_demodulate(c, p.g1[q]);
        return typename Planes::Pixel{ make_float4(c.x, c.y, c.z, c.x - i.x), { { c.y - i.y, c.z - i.z } } };
    };
    float4 dp;
    const auto centre = [&](const typename Planes::Pixel &own, const auto &own_weight) -> float {
        dp = own.d;
        // 2^-k, k = the exponent of the centre's own weight within [-126, 126]: an exact scaling that keeps g * g inside fp32
        int k2 = (int)((__float_as_uint(own_weight()) >> 23) & 255u) - 127;
        k2 = k2 < -126 ? -126 : (k2 > 126 ? 126 : k2);
        return __uint_as_float((uint32_t)(127 - k2) << 23);
    };
    float G = 0.0f, G2 = 0.0f, er = 0.0f, eg = 0.0f, eb = 0.0f, a1r = 0.0f, a1g = 0.0f, a1b = 0.0f, a2r = 0.0f, a2g = 0.0f, a2b = 0.0f;
    const auto tap = [&](const typename Planes::Pixel &q, float g) {
        const float4 dq = q.d;
        const DnPayload<2> eq = q.e;
        const float tr = dq.x - dp.x, tg = dq.y - dp.y, tb = dq.z - dp.z;
        G += g; G2 += g * g;
        er += g * dq.w; eg += g * eq.v[0]; eb += g * eq.v[1];
        a1r += g * tr; a1g += g * tg; a1b += g * tb;
        a2r += g * (tr * tr); a2g += g * (tg * tg); a2b += g * (tb * tb);
    };
    const bool hit = dn_window7<STRICT, Planes>(p.g0, p.w, p.h, p.sigma_normal, p.sigma_depth, inside, load, centre, tap);
    if (!inside) return;
    const size_t pix = (size_t)y * (size_t)p.w + (size_t)x;
    float4 iv = p.iv_in[pix];
    if (hit && G > 0.0f) {   // (a miss keeps its colour: its Hc is the reprojection's)
        iv.x = dn_lag_channel<STRICT>(iv.x, er, a1r, a2r, G, G2, p.gate);
        iv.y = dn_lag_channel<STRICT>(iv.y, eg, a1g, a2g, G, G2, p.gate);
        iv.z = dn_lag_channel<STRICT>(iv.z, eb, a1b, a2b, G, G2, p.gate);
        p.hc[pix] = make_float4(iv.x, iv.y, iv.z, p.hc[pix].w);
    }
    p.iv_out[pix] = iv;
}
// enqueues the correction: I from `iv_in`, Ic into .rgb of `hc` and, beside iv_in's .w, into `iv_out` (neither may be iv_in)
int lag_correct(trg_ctx *c, DenoiseState &s, const char *who, const float4 *color, const float4 *guides, const float4 *iv_in, float4 *hc, float4 *iv_out, float gate,
                float sigma_normal, float sigma_depth, bool demod) {
    LagParams l{};
    l.color = color; l.g0 = s.fguide; l.g1 = guides + (size_t)c->w * c->h; l.iv_in = iv_in;
    l.hc = hc; l.iv_out = iv_out;
    l.w = (int)c->w; l.h = (int)c->h; l.demod = demod ? 1 : 0;
    l.gate = gate; l.sigma_normal = sigma_normal; l.sigma_depth = sigma_depth;
    return launch_tiles(c, who, DN_FOR_SETTING(c, dn_temporal_lag_kernel), l);
}

// iterations == 0: out.rgb = I remodulated, out.a = the input's alpha; var (may be null) = V_0
__global__ void dn_temporal_finish_kernel(const float4 *iv, const float4 *color, const float4 *fguide, const float4 *g1, float4 *out, float *var, int demod,
                                          uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float4 o = iv[i];
    if (var) var[i] = o.w;
    if (demod && !(fguide[i].w < 0.0f)) o = dn_remodulate(o, g1[i]);
    o.w = color[i].w;
    out[i] = o;
}

// rgb *= f in place: the running average trg_render left in a zeroed image, as the mean of its samples
__global__ void dn_scale_kernel(float4 *a, float f, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float4 u = a[i];
    u.x = u.x * f; u.y = u.y * f; u.z = u.z * f;
    a[i] = u;
}

// inverse of the 4 x 4 matrix a (row-major) in double precision, Gauss-Jordan with partial pivoting; false when a is singular or not finite
bool invert4(const float *a, float *out) {
    double m[4][8];
    double big = 0.0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const double v = (double)a[i * 4 + j];
            if (!(v - v == 0.0)) return false;   // inf or NaN
            m[i][j] = v;
            m[i][4 + j] = i == j ? 1.0 : 0.0;
            if (fabs(v) > big) big = fabs(v);
        }
    if (!(big > 0.0)) return false;
    for (int col = 0; col < 4; ++col) {
        int piv = col;
        for (int r = col + 1; r < 4; ++r)
            if (fabs(m[r][col]) > fabs(m[piv][col])) piv = r;
        // entries are fp32 values: a pivot this far under the largest of them is the rounding residue of a singular matrix
        if (!(fabs(m[piv][col]) > 1e-13 * big)) return false;
        if (piv != col)
            for (int j = 0; j < 8; ++j) { const double t = m[piv][j]; m[piv][j] = m[col][j]; m[col][j] = t; }
        const double d = m[col][col];
        for (int j = 0; j < 8; ++j) m[col][j] /= d;
        for (int r = 0; r < 4; ++r) {
            if (r == col) continue;
            const double f = m[r][col];
            if (f == 0.0) continue;
            for (int j = 0; j < 8; ++j) m[r][j] -= f * m[col][j];
        }
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const float v = (float)m[i][4 + j];
            if (!(v - v == 0.0f)) return false;
            out[i * 4 + j] = v;
        }
    return true;
}

// use_history = false: the step runs as after a reset (trg_render_temporal without a remembered view-projection).  iv_out (may be null): a plane
// of width*height float4 for (I, V_0); var_out (may be null): a plane of floats for V_N; motion (may be null): the planes M0, M1 of
// trg_temporal_denoise_motion
int temporal_denoise(trg_ctx *c, DenoiseState &s, const float4 *color, const float4 *guides, const float4 *pos, const float *vp, bool use_history,
                     float4 *out, float4 *iv_out, float *var_out, const trg_temporal_params *pp, const char *who, const float4 *motion = nullptr) {
    trg_temporal_params q;
    trg_temporal_default_params(&q);
    if (pp) q = *pp;
    if (!valid_temporal_params(q))
        return fail(c, TRG_ERR_INVALID, "%s: iterations must be 0..%d, the sigmas and plane_tol positive, alpha and alpha_moments in (0, 1], normal_tol in [-1, 1], max_history >= 1",
                    who, TRG_DENOISE_MAX_ITERATIONS);
    const size_t n = (size_t)c->w * c->h, bytes = n * sizeof(float4);
    if (!disjoint({ { out, bytes }, { color, bytes }, { guides, 2 * bytes }, { pos, bytes } })) return fail(c, TRG_ERR_INVALID, "%s: the buffers overlap", who);
    if (!disjoint({ { motion, 2 * bytes }, { out, bytes }, { color, bytes }, { guides, 2 * bytes }, { pos, bytes } }))   // (the last four are disjoint)
        return fail(c, TRG_ERR_INVALID, "%s: motion_device overlaps another buffer", who);
    for (int k = 0; k < 16; ++k)
        if (!(vp[k] - vp[k] == 0.0f)) return fail(c, TRG_ERR_INVALID, "%s: prev_view_proj is not finite", who);
    if (int rc = lazy_planes(c, s, s.hist[0], 4, "the history planes")) return rc;
    if (int rc = lazy_planes(c, s, s.hist[1], 4, "the history planes")) return rc;
    if (int rc = exclude_emitters(c, s, guides, who)) return rc;
    const float4 *prev = s.hist[s.hist_cur];
    float4 *next = s.hist[s.hist_cur ^ 1];
    ReprojectParams r{};
    r.color = color; r.fguide = s.fguide; r.g1 = guides + n; r.pos = pos;
    if (s.hist_valid && use_history) { r.hc = prev; r.hm = prev + n; r.hf = prev + 2 * n; r.hx = prev + 3 * n; }
    r.oc = next; r.om = next + n; r.of = next + 2 * n; r.ox = next + 3 * n; r.iv = s.ping;
    r.w = (int)c->w; r.h = (int)c->h; r.demod = q.demodulate ? 1 : 0;
    for (int k = 0; k < 16; ++k) r.vp[k] = vp[k];
    r.alpha = q.alpha; r.alpha_moments = q.alpha_moments; r.plane_tol = q.plane_tol; r.normal_tol = q.normal_tol; r.max_history = (float)q.max_history;
    if (motion) { r.m0 = motion; r.m1 = motion + n; }
    const bool cover = s.cov_min >= 0.0f;
    if (cover) { r.fmark = s.fguide; r.cov_min = s.cov_min; }
    // the kernel's form, [MOTION][TRACK][COVER]
#define DN_REPROJECT(M, T, C) DN_FOR_SETTING(c, dn_temporal_reproject_kernel, M, T, C)
    void (*const forms[2][2][2])(ReprojectParams) = {
        { { DN_REPROJECT(false, false, false), DN_REPROJECT(false, false, true) }, { DN_REPROJECT(false, true, false), DN_REPROJECT(false, true, true) } },
        { { DN_REPROJECT(true, false, false), DN_REPROJECT(true, false, true) }, { DN_REPROJECT(true, true, false), DN_REPROJECT(true, true, true) } } };
#undef DN_REPROJECT
    const auto reproject = forms[motion ? 1 : 0][s.track ? 1 : 0][cover ? 1 : 0];
    if (int rc = launch_tiles(c, who, reproject, r)) return rc;
    s.hist_cur ^= 1;          // (enqueued: from here on the new planes are the history, also if a later launch fails)
    s.hist_valid = true;
    // the lag correction, while it is on: (I, V_0) moves to the other ping-pong image, everything behind it starts from there
    float4 *iv = s.ping;
    if (s.lag_gate >= 0.0f) {
        if (int rc = lag_correct(c, s, who, color, guides, s.ping, r.oc, s.pong, s.lag_gate, q.sigma_normal, q.sigma_depth, q.demodulate != 0)) return rc;
        iv = s.pong;
    }
    if (int rc = launch_tiles(c, who, s.track ? DN_FOR_SETTING(c, dn_temporal_spatial_kernel, true) : DN_FOR_SETTING(c, dn_temporal_spatial_kernel, false), r.oc, r.om,
                              s.fguide, iv, c->w, c->h, q.sigma_normal, q.sigma_depth))
        return rc;
    if (iv_out) DN_HIPCHK(c, hipMemcpyAsync(iv_out, iv, bytes, hipMemcpyDeviceToDevice, c->stream));
    if (q.iterations == 0) return launch_each(c, who, dn_temporal_finish_kernel, n, iv, color, s.fguide, guides + n, out, var_out, q.demodulate ? 1 : 0, n);
    AtrousParams p = atrous_params(c, s, guides, q.sigma_lum, q.sigma_normal, q.sigma_depth);
    p.alpha = color; p.var_out = var_out;
    return atrous_run<true>(c, s, who, p, iv, out, q.iterations, false, q.demodulate != 0);   // (the reprojection kernel demodulated)
}

int render_temporal(trg_ctx *c, DenoiseState &s, uint32_t b, uint32_t n, uint32_t bounces, float4 *out, const trg_temporal_params *p, const char *who) {
    if (p && !valid_temporal_params(*p)) return fail(c, TRG_ERR_INVALID, "%s: bad parameters", who);
    if (n < 1u) return fail(c, TRG_ERR_INVALID, "%s: spp must be at least 1", who);
    if ((uint64_t)b + n > 0xFFFFFFFFull) return fail(c, TRG_ERR_INVALID, "%s: frame range [%u, %u + %u) exceeds 32 bits", who, b, b, n);
    if (!c->have_uniforms) return fail(c, TRG_ERR_INVALID, "%s: uniforms not set", who);
    float vp_now[16];
    if (!invert4(c->u.inv_view_proj, vp_now)) return fail(c, TRG_ERR_INVALID, "%s: the uniforms' inverse view-projection is singular or not finite", who);
    const size_t npix = (size_t)c->w * c->h, bytes = npix * sizeof(float4);
    if (overlap(out, bytes, c->accum, bytes)) return fail(c, TRG_ERR_INVALID, "%s: out_device overlaps the bound accumulation buffer", who);
    // armed (trg_temporal_set_previous_scene): this call looks for the history where the geometry was, and consumes the arming
    const bool armed = s.armed;
    if (armed && !have_previous_scene(c, s))
        return fail(c, TRG_ERR_INVALID, "%s: the previous scene has %u triangles, the loaded scene %u: call trg_temporal_set_previous_scene again, or trg_temporal_reset",
                    who, s.prev_tris, c->scene_loaded ? c->sc.n_tris : 0u);
    if (int rc = lazy_planes(c, s, s.timg, 1, "the temporal path's image")) return rc;
    if (int rc = lazy_planes(c, s, s.tpos, 1, "the position plane")) return rc;
    if (armed)
        if (int rc = lazy_planes(c, s, s.tmotion, 2, "the motion planes")) return rc;
    if (int rc = render_zeroed(c, s.timg, 1, b, n, bounces)) return rc;
    const float f = (float)((double)((uint64_t)b + n) / (double)n);
    if (int rc = launch_each(c, who, dn_scale_kernel, npix, s.timg, f, npix)) return rc;
    // with the coverage history on the guides come from the pixel centres, under the step's own two tolerances
    trg_temporal_params q;
    trg_temporal_default_params(&q);
    if (p) q = *p;
    const CentreTol tol{ q.plane_tol, q.normal_tol };
    if (int rc = guides_render(c, s, b, s.guides, s.tpos, armed ? s.tmotion : nullptr, s.cov_min >= 0.0f ? &tol : nullptr)) return rc;
    const float zero[16] = {};
    const int rc = temporal_denoise(c, s, s.timg, s.guides, s.tpos, s.have_prev_vp ? s.prev_vp : zero, s.have_prev_vp, out, nullptr, nullptr, p, who,
                                    armed ? s.tmotion : nullptr);
    if (rc != TRG_OK) return rc;
    for (int k = 0; k < 16; ++k) s.prev_vp[k] = vp_now[k];
    s.have_prev_vp = true;
    s.armed = false;
    return TRG_OK;
}

// The round trip of an entry point that works on host memory: device temporaries, uploads, the run (while rc is TRG_OK), downloads.  finish()
// waits for the stream also after an error -- only then does the destructor free the temporaries -- and returns the first error.
struct HostTrip {
    trg_ctx *c;
    const char *who;
    int rc = TRG_OK;
    struct { void *dev, *host; size_t bytes; } temp[8] = {};   // (trg_temporal_denoise_motion_host has seven)
    int n = 0;
    HostTrip(trg_ctx *c_, const char *who_) : c(c_), who(who_) {}
    HostTrip(const HostTrip &) = delete;
    ~HostTrip() { for (int k = 0; k < n; ++k) (void)hipFree(temp[k].dev); }
    // a temporary of `bytes` that finish() copies to `host` (may be null: none); null after a failure
    void *alloc(size_t bytes, void *host) {
        if (rc != TRG_OK) return nullptr;
        const hipError_t e = hipMalloc(&temp[n].dev, bytes ? bytes : 16);
        if (e != hipSuccess) { rc = fail(c, TRG_ERR_DEVICE, "%s: hipMalloc(%zu) failed: %s", who, bytes, hipGetErrorString(e)); return nullptr; }
        temp[n].host = host; temp[n].bytes = bytes;
        return temp[n++].dev;
    }
    // a temporary with a copy of `host`
    const float4 *upload(const float *host, size_t bytes) {
        void *dev = alloc(bytes, nullptr);
        if (dev) {
            const hipError_t e = hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, c->stream);
            if (e != hipSuccess) rc = fail(c, TRG_ERR_DEVICE, "%s: copy failed: %s", who, hipGetErrorString(e));
        }
        return static_cast<const float4 *>(dev);
    }
    // a temporary for a result that goes to `host`; null when host is (an output nobody asked for)
    template <typename T = float4>
    T *result(float *host, size_t bytes) { return host ? static_cast<T *>(alloc(bytes, host)) : nullptr; }
    int finish() {
        for (int k = 0; k < n && rc == TRG_OK; ++k) {
            if (!temp[k].host) continue;
            const hipError_t e = hipMemcpyAsync(temp[k].host, temp[k].dev, temp[k].bytes, hipMemcpyDeviceToHost, c->stream);
            if (e != hipSuccess) rc = fail(c, TRG_ERR_DEVICE, "%s: copy failed: %s", who, hipGetErrorString(e));
        }
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (rc == TRG_OK && e != hipSuccess) rc = fail(c, TRG_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
        return rc;
    }
};

// the state's result image of the _own entry points (allocated on first use); refused while the caller has bound it as the accumulation buffer
int own_result(trg_ctx *c, DenoiseState &s, const char *who) {
    if (int rc = lazy_planes(c, s, s.result, 1, "the result image")) return rc;
    if (c->accum == reinterpret_cast<float *>(s.result)) return fail(c, TRG_ERR_INVALID, "%s: the state's image is bound as the accumulation buffer", who);
    return TRG_OK;
}

int enter(trg_ctx *c, DenoiseState *&s, const char *who) {
    if (!c) return TRG_ERR_INVALID;
    DN_HIPCHK(c, hipSetDevice(c->device));
    return state_of(c, s);
}

// ---- the bodies that families of entry points share; `who` is the entry point's own name ----
// _own: run(state, image) into the state's result image, whose address is handed out
template <typename Run>
int run_own(trg_ctx *c, const char *who, void **out_device, const Run run) {
    DenoiseState *s;
    if (int rc = enter(c, s, who)) return rc;
    if (!out_device) return fail(c, TRG_ERR_INVALID, "%s: out_device is NULL", who);
    if (int rc = own_result(c, *s, who)) return rc;
    if (int rc = run(*s, s->result)) return rc;
    *out_device = s->result;
    return TRG_OK;
}
// _read: run(state, images) into a temporary of `planes` images that goes to `host`, the argument the entry point calls `what`
template <typename Run>
int run_read(trg_ctx *c, const char *who, float *host, const char *what, size_t planes, const Run run) {
    DenoiseState *s;
    if (int rc = enter(c, s, who)) return rc;
    if (!host) return fail(c, TRG_ERR_INVALID, "%s: %s is NULL", who, what);
    HostTrip t(c, who);
    float4 *res = t.result(host, planes * s->pixels * sizeof(float4));
    if (t.rc == TRG_OK) t.rc = run(*s, res);
    return t.finish();
}
// trg_guides_render_pos and, moving, trg_guides_render_motion
bool valid_centre(const CentreTol *t) { return !t || (t->plane_tol > 0.0f && t->normal_tol >= -1.0f && t->normal_tol <= 1.0f); }
int guides_pos_device(trg_ctx *c, const char *who, uint32_t frameIndex, void *guides, void *pos, bool moving, void *motion, const CentreTol *centre = nullptr) {
    DenoiseState *s;
    if (int rc = enter(c, s, who)) return rc;
    if (!valid_centre(centre)) return fail(c, TRG_ERR_INVALID, "%s: plane_tol must be positive and normal_tol in [-1, 1]", who);
    if (!guides || !pos || (moving && !motion)) return fail(c, TRG_ERR_INVALID, "%s: NULL buffer", who);
    const size_t bytes = (size_t)c->w * c->h * sizeof(float4);
    if (!disjoint({ { guides, 2 * bytes }, { pos, bytes }, { motion, 2 * bytes } }))
        return fail(c, TRG_ERR_INVALID, moving ? "%s: the buffers overlap" : "%s: pos_device overlaps guides_device", who);
    if (moving && !have_previous_scene(c, *s))
        return fail(c, TRG_ERR_INVALID, "%s: no previous scene of the loaded scene's triangle count (trg_temporal_set_previous_scene)", who);
    return guides_render(c, *s, frameIndex, static_cast<float4 *>(guides), static_cast<float4 *>(pos), static_cast<float4 *>(motion), centre);
}
// trg_guides_pos_read and, moving, trg_guides_motion_read
int guides_pos_host(trg_ctx *c, const char *who, uint32_t frameIndex, float *guides, float *pos, bool moving, float *motion, const CentreTol *centre = nullptr) {
    DenoiseState *s;
    if (int rc = enter(c, s, who)) return rc;
    if (!valid_centre(centre)) return fail(c, TRG_ERR_INVALID, "%s: plane_tol must be positive and normal_tol in [-1, 1]", who);
    if (!guides || !pos || (moving && !motion)) return fail(c, TRG_ERR_INVALID, "%s: NULL buffer", who);
    if (moving && !have_previous_scene(c, *s))
        return fail(c, TRG_ERR_INVALID, "%s: no previous scene of the loaded scene's triangle count (trg_temporal_set_previous_scene)", who);
    const size_t bytes = s->pixels * sizeof(float4);
    HostTrip t(c, who);
    float4 *g = t.result(guides, 2 * bytes), *x = t.result(pos, bytes), *m = t.result(motion, 2 * bytes);
    if (t.rc == TRG_OK) t.rc = guides_render(c, *s, frameIndex, g, x, m, centre);
    return t.finish();
}
// trg_temporal_denoise and, moving, trg_temporal_denoise_motion
int temporal_device(trg_ctx *c, const char *who, const void *color, const void *guides, const void *pos, bool moving, const void *motion, const float *prev_view_proj,
                    void *out, const trg_temporal_params *p) {
    DenoiseState *s;
    if (int rc = enter(c, s, who)) return rc;
    if (!color || !guides || !pos || (moving && !motion) || !prev_view_proj || !out) return fail(c, TRG_ERR_INVALID, "%s: NULL buffer", who);
    return temporal_denoise(c, *s, static_cast<const float4 *>(color), static_cast<const float4 *>(guides), static_cast<const float4 *>(pos), prev_view_proj, true,
                            static_cast<float4 *>(out), nullptr, nullptr, p, who, static_cast<const float4 *>(motion));
}
// trg_temporal_denoise_host and, moving, trg_temporal_denoise_motion_host
int temporal_host(trg_ctx *c, const char *who, const float *color, const float *guides, const float *pos, bool moving, const float *motion, const float *prev_view_proj,
                  float *out_host, float *iv_host, float *var_host, const trg_temporal_params *p) {
    DenoiseState *s;
    if (int rc = enter(c, s, who)) return rc;
    if (!color || !guides || !pos || (moving && !motion) || !prev_view_proj || !out_host) return fail(c, TRG_ERR_INVALID, "%s: NULL buffer", who);
    const size_t bytes = s->pixels * sizeof(float4);
    HostTrip t(c, who);
    const float4 *in = t.upload(color, bytes), *g = t.upload(guides, 2 * bytes), *x = t.upload(pos, bytes), *m = moving ? t.upload(motion, 2 * bytes) : nullptr;
    float4 *out = t.result(out_host, bytes), *iv = t.result(iv_host, bytes);
    float *var = t.result<float>(var_host, s->pixels * sizeof(float));
    if (t.rc == TRG_OK) t.rc = temporal_denoise(c, *s, in, g, x, prev_view_proj, true, out, iv, var, p, who, m);
    return t.finish();
}

}  // namespace

void trg::denoise_state_free(trg_ctx *c) {
    if (!c->denoise) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    each_buffer(*c->denoise, [](auto *mem, size_t) { (void)hipFree(mem); });
    delete c->denoise;
    c->denoise = nullptr;
}

extern "C" {

void trg_denoise_default_params(trg_denoise_params *p) {
    if (!p) return;
    p->iterations = 5; p->sigma_color = 4.0f; p->sigma_normal = 128.0f; p->sigma_depth = 1.0f; p->demodulate = 1;
}

int trg_guides_render(trg_ctx *c, uint32_t frameIndex, void *guides_device) {
    DenoiseState *s;
    if (int rc = enter(c, s, "trg_guides_render")) return rc;
    if (!guides_device) return fail(c, TRG_ERR_INVALID, "trg_guides_render: guides_device is NULL");
    return guides_render(c, *s, frameIndex, static_cast<float4 *>(guides_device));
}

int trg_denoise(trg_ctx *c, const void *color_in_device, const void *guides_device, void *out_device, const trg_denoise_params *p) {
    DenoiseState *s;
    if (int rc = enter(c, s, "trg_denoise")) return rc;
    if (!color_in_device || !guides_device || !out_device) return fail(c, TRG_ERR_INVALID, "trg_denoise: NULL buffer");
    return denoise(c, *s, static_cast<const float4 *>(color_in_device), static_cast<const float4 *>(guides_device), static_cast<float4 *>(out_device), p);
}

int trg_render_denoised(trg_ctx *c, uint32_t frameIndexBegin, uint32_t spp, uint32_t bounces, void *out_device, const trg_denoise_params *p) {
    DenoiseState *s;
    if (int rc = enter(c, s, "trg_render_denoised")) return rc;
    if (!out_device) return fail(c, TRG_ERR_INVALID, "trg_render_denoised: out_device is NULL");
    if (p && !valid_params(*p)) return fail(c, TRG_ERR_INVALID, "trg_render_denoised: bad parameters");
    if (int rc = trg_render(c, frameIndexBegin, spp, bounces, 0, c->h)) return rc;
    if (int rc = guides_render(c, *s, frameIndexBegin, s->guides)) return rc;
    return denoise(c, *s, reinterpret_cast<const float4 *>(c->accum), s->guides, static_cast<float4 *>(out_device), p);
}

int trg_denoise_accum(trg_ctx *c, uint32_t frameIndex, const trg_denoise_params *p, void **out_device) {
    return run_own(c, "trg_denoise_accum", out_device, [&](DenoiseState &s, float4 *out) {
        if (int rc = guides_render(c, s, frameIndex, s.guides)) return rc;
        return denoise(c, s, reinterpret_cast<const float4 *>(c->accum), s.guides, out, p);
    });
}

int trg_denoise_release(trg_ctx *c) {
    if (!c) return TRG_ERR_INVALID;
    denoise_state_free(c);
    return TRG_OK;
}

int trg_guides_read(trg_ctx *c, uint32_t frameIndex, float *guides_host) {
    return run_read(c, "trg_guides_read", guides_host, "guides_host", 2, [&](DenoiseState &s, float4 *g) { return guides_render(c, s, frameIndex, g); });
}

int trg_denoise_host(trg_ctx *c, const float *color_in_host, const float *guides_host, float *out_host, const trg_denoise_params *p) {
    DenoiseState *s;
    if (int rc = enter(c, s, "trg_denoise_host")) return rc;
    if (!color_in_host || !guides_host || !out_host) return fail(c, TRG_ERR_INVALID, "trg_denoise_host: NULL buffer");
    const size_t bytes = s->pixels * sizeof(float4);
    HostTrip t(c, "trg_denoise_host");
    const float4 *in = t.upload(color_in_host, bytes), *g = t.upload(guides_host, 2 * bytes);
    float4 *out = t.result(out_host, bytes);
    if (t.rc == TRG_OK) t.rc = denoise(c, *s, in, g, out, p);
    return t.finish();
}

int trg_render_denoised_read(trg_ctx *c, uint32_t frameIndexBegin, uint32_t spp, uint32_t bounces, float *out_host, const trg_denoise_params *p) {
    return run_read(c, "trg_render_denoised_read", out_host, "out_host", 1,
                    [&](DenoiseState &, float4 *out) { return trg_render_denoised(c, frameIndexBegin, spp, bounces, out, p); });
}

void trg_denoise_var_default_params(trg_denoise_var_params *p) {
    if (!p) return;
    p->iterations = 5; p->sigma_lum = 4.0f; p->sigma_normal = 128.0f; p->sigma_depth = 1.0f; p->demodulate = 1; p->prefilter = 1;
}

int trg_render_halves(trg_ctx *c, uint32_t frameIndexBegin, uint32_t spp, uint32_t bounces, void *halves_device) {
    DenoiseState *s;
    if (int rc = enter(c, s, "trg_render_halves")) return rc;
    if (!halves_device) return fail(c, TRG_ERR_INVALID, "trg_render_halves: halves_device is NULL");
    return render_halves(c, *s, frameIndexBegin, spp, bounces, static_cast<float4 *>(halves_device), "trg_render_halves");
}

int trg_denoise_variance(trg_ctx *c, const void *halves_device, const void *guides_device, void *out_device, const trg_denoise_var_params *p) {
    DenoiseState *s;
    if (int rc = enter(c, s, "trg_denoise_variance")) return rc;
    if (!halves_device || !guides_device || !out_device) return fail(c, TRG_ERR_INVALID, "trg_denoise_variance: NULL buffer");
    return denoise_variance(c, *s, static_cast<const float4 *>(halves_device), static_cast<const float4 *>(guides_device), static_cast<float4 *>(out_device), nullptr, p);
}

int trg_render_denoised_variance(trg_ctx *c, uint32_t frameIndexBegin, uint32_t spp, uint32_t bounces, void *out_device, const trg_denoise_var_params *p) {
    DenoiseState *s;
    if (int rc = enter(c, s, "trg_render_denoised_variance")) return rc;
    if (!out_device) return fail(c, TRG_ERR_INVALID, "trg_render_denoised_variance: out_device is NULL");
    return render_denoised_variance(c, *s, frameIndexBegin, spp, bounces, static_cast<float4 *>(out_device), p, "trg_render_denoised_variance");
}

int trg_render_denoised_variance_own(trg_ctx *c, uint32_t frameIndexBegin, uint32_t spp, uint32_t bounces, const trg_denoise_var_params *p, void **out_device) {
    const char *const who = "trg_render_denoised_variance_own";
    return run_own(c, who, out_device, [&](DenoiseState &s, float4 *out) { return render_denoised_variance(c, s, frameIndexBegin, spp, bounces, out, p, who); });
}

int trg_render_halves_read(trg_ctx *c, uint32_t frameIndexBegin, uint32_t spp, uint32_t bounces, float *halves_host) {
    const char *const who = "trg_render_halves_read";
    return run_read(c, who, halves_host, "halves_host", 2, [&](DenoiseState &s, float4 *hv) { return render_halves(c, s, frameIndexBegin, spp, bounces, hv, who); });
}

int trg_denoise_variance_host(trg_ctx *c, const float *halves_host, const float *guides_host, float *out_host, float *var_host, const trg_denoise_var_params *p) {
    DenoiseState *s;
    if (int rc = enter(c, s, "trg_denoise_variance_host")) return rc;
    if (!halves_host || !guides_host || !out_host) return fail(c, TRG_ERR_INVALID, "trg_denoise_variance_host: NULL buffer");
    const size_t bytes = s->pixels * sizeof(float4);
    HostTrip t(c, "trg_denoise_variance_host");
    const float4 *in = t.upload(halves_host, 2 * bytes), *g = t.upload(guides_host, 2 * bytes);
    float4 *out = t.result(out_host, bytes);
    float *var = t.result<float>(var_host, s->pixels * sizeof(float));
    if (t.rc == TRG_OK) t.rc = denoise_variance(c, *s, in, g, out, var, p);
    return t.finish();
}

int trg_render_denoised_variance_read(trg_ctx *c, uint32_t frameIndexBegin, uint32_t spp, uint32_t bounces, float *out_host, const trg_denoise_var_params *p) {
    const char *const who = "trg_render_denoised_variance_read";
    return run_read(c, who, out_host, "out_host", 1, [&](DenoiseState &s, float4 *out) { return render_denoised_variance(c, s, frameIndexBegin, spp, bounces, out, p, who); });
}

void trg_temporal_default_params(trg_temporal_params *p) {
    if (!p) return;
    p->iterations = 5; p->sigma_lum = 4.0f; p->sigma_normal = 128.0f; p->sigma_depth = 1.0f; p->demodulate = 1;
    p->alpha = 0.2f; p->alpha_moments = 0.2f; p->plane_tol = 0.02f; p->normal_tol = 0.9f; p->max_history = 32;
}

int trg_temporal_view_proj(const trg_uniforms *u, float vp16[16]) {
    if (!u || !vp16) return TRG_ERR_INVALID;
    return invert4(u->inv_view_proj, vp16) ? TRG_OK : TRG_ERR_INVALID;
}

int trg_guides_render_pos(trg_ctx *c, uint32_t frameIndex, void *guides_device, void *pos_device) {
    return guides_pos_device(c, "trg_guides_render_pos", frameIndex, guides_device, pos_device, false, nullptr);
}

int trg_temporal_reset(trg_ctx *c) {
    if (!c) return TRG_ERR_INVALID;
    // allocates nothing: a context that never denoised has no state, and a new state starts without history anyway
    if (!c->denoise) return TRG_OK;
    c->denoise->hist_valid = false;
    c->denoise->have_prev_vp = false;
    c->denoise->armed = false;
    return TRG_OK;
}

int trg_temporal_history_read(trg_ctx *c, float *hist_host) {
    DenoiseState *s;
    if (int rc = enter(c, s, "trg_temporal_history_read")) return rc;
    if (!hist_host) return fail(c, TRG_ERR_INVALID, "trg_temporal_history_read: hist_host is NULL");
    if (!s->hist_valid) return fail(c, TRG_ERR_INVALID, "trg_temporal_history_read: there is no history");
    DN_HIPCHK(c, hipMemcpyAsync(hist_host, s->hist[s->hist_cur], 2 * s->pixels * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    DN_HIPCHK(c, hipStreamSynchronize(c->stream));
    return TRG_OK;
}

int trg_temporal_denoise(trg_ctx *c, const void *color_in_device, const void *guides_device, const void *pos_device, const float prev_view_proj[16], void *out_device,
                         const trg_temporal_params *p) {
    return temporal_device(c, "trg_temporal_denoise", color_in_device, guides_device, pos_device, false, nullptr, prev_view_proj, out_device, p);
}

int trg_render_temporal(trg_ctx *c, uint32_t frameIndexBegin, uint32_t spp, uint32_t bounces, void *out_device, const trg_temporal_params *p) {
    DenoiseState *s;
    if (int rc = enter(c, s, "trg_render_temporal")) return rc;
    if (!out_device) return fail(c, TRG_ERR_INVALID, "trg_render_temporal: out_device is NULL");
    return render_temporal(c, *s, frameIndexBegin, spp, bounces, static_cast<float4 *>(out_device), p, "trg_render_temporal");
}

int trg_render_temporal_own(trg_ctx *c, uint32_t frameIndexBegin, uint32_t spp, uint32_t bounces, const trg_temporal_params *p, void **out_device) {
    const char *const who = "trg_render_temporal_own";
    return run_own(c, who, out_device, [&](DenoiseState &s, float4 *out) { return render_temporal(c, s, frameIndexBegin, spp, bounces, out, p, who); });
}

int trg_guides_pos_read(trg_ctx *c, uint32_t frameIndex, float *guides_host, float *pos_host) {
    return guides_pos_host(c, "trg_guides_pos_read", frameIndex, guides_host, pos_host, false, nullptr);
}

int trg_temporal_denoise_host(trg_ctx *c, const float *color_in_host, const float *guides_host, const float *pos_host, const float prev_view_proj[16], float *out_host,
                              float *iv_host, float *var_host, const trg_temporal_params *p) {
    return temporal_host(c, "trg_temporal_denoise_host", color_in_host, guides_host, pos_host, false, nullptr, prev_view_proj, out_host, iv_host, var_host, p);
}

int trg_render_temporal_read(trg_ctx *c, uint32_t frameIndexBegin, uint32_t spp, uint32_t bounces, float *out_host, const trg_temporal_params *p) {
    const char *const who = "trg_render_temporal_read";
    return run_read(c, who, out_host, "out_host", 1, [&](DenoiseState &s, float4 *out) { return render_temporal(c, s, frameIndexBegin, spp, bounces, out, p, who); });
}

int trg_temporal_set_previous_scene(trg_ctx *c, const float *positions3, const float *normals3, const uint32_t *indices, uint32_t n_verts, uint32_t n_tris) {
    const char *const who = "trg_temporal_set_previous_scene";
    if (!c) return TRG_ERR_INVALID;
    if (n_tris != 0 && (!positions3 || !indices)) return fail(c, TRG_ERR_INVALID, "%s: positions3 / indices is NULL", who);
    DenoiseState *s;
    if (int rc = enter(c, s, who)) return rc;
    if (!c->scene_loaded) return fail(c, TRG_ERR_INVALID, "%s: no scene loaded", who);
    if (n_tris == 0) {
        s->prev_tris = 0;
        s->armed = false;
        return TRG_OK;
    }
    if (n_tris != c->sc.n_tris) return fail(c, TRG_ERR_INVALID, "%s: %u triangles, the loaded scene has %u", who, n_tris, c->sc.n_tris);
    for (size_t k = 0; k < (size_t)n_tris * 3u; ++k)
        if (indices[k] >= n_verts) return fail(c, TRG_ERR_INVALID, "%s: index %u of triangle %zu is outside the %u vertices", who, indices[k], k / 3u, n_verts);
    std::vector<float> rec((size_t)n_tris * kPrevRecord * 4u, 0.0f);
    for (size_t t = 0; t < n_tris; ++t) {
        float *r = rec.data() + t * kPrevRecord * 4u;
        for (int corner = 0; corner < 3; ++corner)
            for (int k = 0; k < 3; ++k) {
                r[corner * 3 + k] = positions3[(size_t)indices[t * 3u + corner] * 3u + k];
                if (normals3) r[9 + corner * 3 + k] = normals3[(t * 3u + corner) * 3u + k];
            }
    }
    if (int rc = grow(c, s->prev_geo, s->prev_cap, (size_t)n_tris * kPrevRecord, sizeof(float4), "previous scene")) {
        s->prev_tris = 0;   // (the old array is gone)
        s->armed = false;
        return rc;
    }
    // the running launches of an earlier call may still read the array: the copy is ordered behind them on the context's stream
    DN_HIPCHK(c, hipMemcpyAsync(s->prev_geo, rec.data(), rec.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    DN_HIPCHK(c, hipStreamSynchronize(c->stream));
    s->prev_tris = n_tris;
    s->prev_normals = normals3 != nullptr;
    s->armed = true;
    return TRG_OK;
}

int trg_temporal_set_previous_scene_device(trg_ctx *c, const void *positions3_dev, const void *normals3_dev, const void *indices_dev, uint32_t n_verts, uint32_t n_tris) {
    const char *const who = "trg_temporal_set_previous_scene_device";
    if (!c) return TRG_ERR_INVALID;
    if (n_tris != 0 && (!positions3_dev || !indices_dev)) return fail(c, TRG_ERR_INVALID, "%s: positions3 / indices is NULL", who);
    DenoiseState *s;
    if (int rc = enter(c, s, who)) return rc;
    if (!c->scene_loaded) return fail(c, TRG_ERR_INVALID, "%s: no scene loaded", who);
    if (n_tris == 0) {
        s->prev_tris = 0;
        s->armed = false;
        return TRG_OK;
    }
    if (n_tris != c->sc.n_tris) return fail(c, TRG_ERR_INVALID, "%s: %u triangles, the loaded scene has %u", who, n_tris, c->sc.n_tris);
    if (n_verts == 0) return fail(c, TRG_ERR_INVALID, "%s: %u triangles and no vertices", who, n_tris);
    if (int rc = grow(c, s->prev_geo, s->prev_cap, (size_t)n_tris * kPrevRecord, sizeof(float4), "previous scene")) {
        s->prev_tris = 0;   // (the old array is gone)
        s->armed = false;
        return rc;
    }
    // ordered on the context's stream behind the launches that still read the array and in front of those that will; nothing is waited for
    if (int rc = launch_each(c, who, dn_prev_pack_kernel, n_tris, positions3_dev, normals3_dev, indices_dev, n_verts, n_tris, s->prev_geo)) return rc;
    s->prev_tris = n_tris;
    s->prev_normals = normals3_dev != nullptr;
    s->armed = true;
    return TRG_OK;
}

int trg_guides_render_motion(trg_ctx *c, uint32_t frameIndex, void *guides_device, void *pos_device, void *motion_device) {
    return guides_pos_device(c, "trg_guides_render_motion", frameIndex, guides_device, pos_device, true, motion_device);
}

int trg_temporal_denoise_motion(trg_ctx *c, const void *color_in_device, const void *guides_device, const void *pos_device, const void *motion_device,
                                const float prev_view_proj[16], void *out_device, const trg_temporal_params *p) {
    return temporal_device(c, "trg_temporal_denoise_motion", color_in_device, guides_device, pos_device, true, motion_device, prev_view_proj, out_device, p);
}

int trg_guides_motion_read(trg_ctx *c, uint32_t frameIndex, float *guides_host, float *pos_host, float *motion_host) {
    return guides_pos_host(c, "trg_guides_motion_read", frameIndex, guides_host, pos_host, true, motion_host);
}

int trg_temporal_denoise_motion_host(trg_ctx *c, const float *color_in_host, const float *guides_host, const float *pos_host, const float *motion_host,
                                     const float prev_view_proj[16], float *out_host, float *iv_host, float *var_host, const trg_temporal_params *p) {
    return temporal_host(c, "trg_temporal_denoise_motion_host", color_in_host, guides_host, pos_host, true, motion_host, prev_view_proj, out_host, iv_host, var_host, p);
}

int trg_temporal_set_lag_correction(trg_ctx *c, float gate) {
    if (!c) return TRG_ERR_INVALID;
    if (gate != gate) return fail(c, TRG_ERR_INVALID, "trg_temporal_set_lag_correction: gate is NaN");
    // allocates nothing: a state created here owns no image yet (pixels == 0), and state_of fills it in on the first call that denoises
    DenoiseState &s = bare_state(c);
    s.lag_gate = gate;
    return TRG_OK;
}

int trg_temporal_lag_correction(trg_ctx *c, float *gate) {
    if (!c) return TRG_ERR_INVALID;
    if (!gate) return fail(c, TRG_ERR_INVALID, "trg_temporal_lag_correction: gate is NULL");
    *gate = c->denoise ? c->denoise->lag_gate : -1.0f;
    return TRG_OK;
}

int trg_temporal_set_variance_of_mean(trg_ctx *c, int on) {
    if (!c) return TRG_ERR_INVALID;
    // allocates nothing, like the gate above
    DenoiseState &s = bare_state(c);
    if (s.track == (on != 0)) return TRG_OK;
    s.track = on != 0;
    // a change is a reset: a history written with the setting off has no variance in it (and one written with it on has, where 0 is promised)
    s.hist_valid = false;
    s.have_prev_vp = false;
    s.armed = false;
    return TRG_OK;
}

int trg_temporal_variance_of_mean(trg_ctx *c, int *on) {
    if (!c) return TRG_ERR_INVALID;
    if (!on) return fail(c, TRG_ERR_INVALID, "trg_temporal_variance_of_mean: on is NULL");
    *on = c->denoise && c->denoise->track ? 1 : 0;
    return TRG_OK;
}

int trg_guides_render_centre(trg_ctx *c, uint32_t frameIndex, float plane_tol, float normal_tol, void *guides_device, void *pos_device) {
    const CentreTol tol{ plane_tol, normal_tol };
    return guides_pos_device(c, "trg_guides_render_centre", frameIndex, guides_device, pos_device, false, nullptr, &tol);
}

int trg_guides_render_centre_motion(trg_ctx *c, uint32_t frameIndex, float plane_tol, float normal_tol, void *guides_device, void *pos_device, void *motion_device) {
    const CentreTol tol{ plane_tol, normal_tol };
    return guides_pos_device(c, "trg_guides_render_centre_motion", frameIndex, guides_device, pos_device, true, motion_device, &tol);
}

int trg_guides_centre_read(trg_ctx *c, uint32_t frameIndex, float plane_tol, float normal_tol, float *guides_host, float *pos_host) {
    const CentreTol tol{ plane_tol, normal_tol };
    return guides_pos_host(c, "trg_guides_centre_read", frameIndex, guides_host, pos_host, false, nullptr, &tol);
}

int trg_guides_centre_motion_read(trg_ctx *c, uint32_t frameIndex, float plane_tol, float normal_tol, float *guides_host, float *pos_host, float *motion_host) {
    const CentreTol tol{ plane_tol, normal_tol };
    return guides_pos_host(c, "trg_guides_centre_motion_read", frameIndex, guides_host, pos_host, true, motion_host, &tol);
}

int trg_temporal_set_coverage(trg_ctx *c, float cov_min) {
    if (!c) return TRG_ERR_INVALID;
    if (!(cov_min < 1.0f)) return fail(c, TRG_ERR_INVALID, "trg_temporal_set_coverage: cov_min must be below 1 (negative: off)");   // (NaN too)
    // allocates nothing, like the gate above
    DenoiseState &s = bare_state(c);
    if (s.cov_min == cov_min || (s.cov_min < 0.0f && cov_min < 0.0f)) return TRG_OK;
    s.cov_min = cov_min;
    // a change is a reset: a history written with the setting off has no coverage in it and comes from other guides
    s.hist_valid = false;
    s.have_prev_vp = false;
    s.armed = false;
    return TRG_OK;
}

int trg_temporal_coverage(trg_ctx *c, float *cov_min) {
    if (!c) return TRG_ERR_INVALID;
    if (!cov_min) return fail(c, TRG_ERR_INVALID, "trg_temporal_coverage: cov_min is NULL");
    *cov_min = c->denoise ? c->denoise->cov_min : -1.0f;
    return TRG_OK;
}

int trg_temporal_lag_correct_host(trg_ctx *c, const float *color_in_host, const float *guides_host, const float *hc_host, float gate, float sigma_normal,
                                  float sigma_depth, int32_t demodulate, float *out_hc_host) {
    const char *const who = "trg_temporal_lag_correct_host";
    DenoiseState *s;
    if (int rc = enter(c, s, who)) return rc;
    if (!color_in_host || !guides_host || !hc_host || !out_hc_host) return fail(c, TRG_ERR_INVALID, "%s: NULL buffer", who);
    if (!(gate >= 0.0f) || !(sigma_normal >= 0.0f) || !(sigma_depth > 0.0f)) return fail(c, TRG_ERR_INVALID, "%s: gate and sigma_normal must be >= 0 and sigma_depth > 0", who);
    const size_t bytes = s->pixels * sizeof(float4);
    HostTrip t(c, who);
    const float4 *in = t.upload(color_in_host, bytes), *g = t.upload(guides_host, 2 * bytes), *hc = t.upload(hc_host, bytes);
    float4 *res = t.result(out_hc_host, bytes);
    if (t.rc == TRG_OK) {
        const hipError_t e = hipMemcpyAsync(res, hc, bytes, hipMemcpyDeviceToDevice, c->stream);   // the plane whose .rgb is rewritten; N stays
        if (e != hipSuccess) t.rc = fail(c, TRG_ERR_DEVICE, "%s: copy failed: %s", who, hipGetErrorString(e));
    }
    if (t.rc == TRG_OK) t.rc = exclude_emitters(c, *s, g, who);
    if (t.rc == TRG_OK) t.rc = lag_correct(c, *s, who, in, g, hc, res, s->pong, gate, sigma_normal, sigma_depth, demodulate != 0);
    return t.finish();
}

}  // extern "C"
