// trg_refit.hip -- include/trg_refit.h: refit a loaded scene from new vertex positions.  A translation unit of its own beside the render path.
// The arithmetic per record, per box and per node is trg_refit_math.h (host + device: the CPU tests evaluate the same functions); this file is the
// kernels that apply it, the order they run in, and the small-scene path through the host builder.  include/trg_pose.h lives here too: it shares
// refit_device and the context's RefitState -- the same refit from buffers already on the device, and the per-object poses that feed it
// (arithmetic: trg_pose_math.h).  So does include/trg_skin.h: blended bone matrices per vertex in front of the same refit (trg_skin_math.h).
// And include/trg_morph.h: blend shapes in front of that skin (trg_morph_math.h).  The three keep one binding protocol: RefitState::Binding.
// And include/trg_rig.h: a keyframed joint forest evaluated into the bones those two read (trg_rig_math.h) -- RefitState::Rig, which is no Binding.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/trg_morph.h"
#include "../../include/trg_pose.h"
#include "../../include/trg_skin.h"
#include "../../include/trg_refit.h"
#include "../../include/trg_rig.h"
#include "trg_ctx.h"
#include "trg_internal.h"
#include "trg_kernels.h"
#include "trg_morph_math.h"
#include "trg_pose_math.h"
#include "trg_skin_math.h"
#include "trg_refit_math.h"
#include "trg_rig_math.h"

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
#define RF_HIPCHK(c, expr)                                                                                      \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) return fail((c), TRG_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// ---- what the device reports back: the flag words and the bounds, read by the host in the call's one wait ----
enum { kFlagIndex = 0, kFlagFinite = 1, kFlagQuad = 2, kFlagBox = 3, kFlagNode = 4, kCountQuads = 5 };
struct Hdr {
    uint32_t flag[8];            // kFlag*: the smallest offending triangle (node for kFlagNode), ~0u = none; kCountQuads: a count
    float lo[3], hi[3], center[3], pad;
    double area[4];              // plain array as it is / refitted, box flavour as it is / refitted
};
constexpr uint32_t kNone = ~0u;
constexpr int kT = 256;
constexpr uint32_t kMaxPartials = 1024;

// ---- step 2a: indices, finiteness, bounds of the indexed vertices (per-block partial results; no atomics on floats) ----
__global__ void rf_bounds_kernel(refit::Geo g, const float *nrm, float *partial, uint32_t *flag) {
    __shared__ float sh[6][kT];
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (uint32_t t = blockIdx.x * kT + threadIdx.x; t < g.n_tris; t += gridDim.x * kT) {
        bool bad_index = false, bad_value = false;
        for (int j = 0; j < 3; ++j) {
            const uint32_t i = g.idx[(size_t)t * 3 + j];
            if (i >= g.n_verts) { bad_index = true; continue; }
            const float *p = g.pos + (size_t)i * 3;
            for (int a = 0; a < 3; ++a) { bad_value = bad_value || !isfinite(p[a]); lo[a] = fminf(lo[a], p[a]); hi[a] = fmaxf(hi[a], p[a]); }
        }
        if (nrm)
            for (int k = 0; k < 9; ++k) bad_value = bad_value || !isfinite(nrm[(size_t)t * 9 + k]);
        if (bad_index) atomicMin(&flag[kFlagIndex], t);
        if (bad_value) atomicMin(&flag[kFlagFinite], t);
    }
    for (int a = 0; a < 3; ++a) { sh[a][threadIdx.x] = lo[a]; sh[3 + a][threadIdx.x] = hi[a]; }
    __syncthreads();
    for (int s = kT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int a = 0; a < 3; ++a) {
                sh[a][threadIdx.x] = fminf(sh[a][threadIdx.x], sh[a][threadIdx.x + s]);
                sh[3 + a][threadIdx.x] = fmaxf(sh[3 + a][threadIdx.x], sh[3 + a][threadIdx.x + s]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 6) partial[blockIdx.x * 6 + threadIdx.x] = sh[threadIdx.x][0];
}
// ... and the one block that finishes them: bounds, centre and padding as trg_load_scene computes them
__global__ void rf_bounds_final_kernel(const float *partial, uint32_t n_partials, Hdr *hdr) {
    __shared__ float sh[6][kT];
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (uint32_t b = threadIdx.x; b < n_partials; b += kT)
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], partial[b * 6 + a]); hi[a] = fmaxf(hi[a], partial[b * 6 + 3 + a]); }
    for (int a = 0; a < 3; ++a) { sh[a][threadIdx.x] = lo[a]; sh[3 + a][threadIdx.x] = hi[a]; }
    __syncthreads();
    for (int s = kT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int a = 0; a < 3; ++a) {
                sh[a][threadIdx.x] = fminf(sh[a][threadIdx.x], sh[a][threadIdx.x + s]);
                sh[3 + a][threadIdx.x] = fmaxf(sh[3 + a][threadIdx.x], sh[3 + a][threadIdx.x + s]);
            }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        for (int a = 0; a < 3; ++a) { lo[a] = sh[a][0]; hi[a] = sh[3 + a][0]; hdr->lo[a] = lo[a]; hdr->hi[a] = hi[a]; }
        refit::scene_center(lo, hi, hdr->center);
        hdr->pad = refit::scene_pad(lo, hi);
    }
}

// the loaded scene as the kernels of this unit see it
struct View {
    unsigned char *blob;
    uint32_t off_fat, off_fat_planes, off_boxrec, n_fat, n_boxrec, n_tris;
};
__device__ inline uint32_t rec_prim(const View &v, uint32_t r) { return reinterpret_cast<const uint32_t *>(v.blob + v.off_fat + (size_t)r * kFatRecBytes)[3]; }
__device__ inline const uint32_t *box_row3(const View &v, uint32_t b) { return reinterpret_cast<const uint32_t *>(v.blob + v.off_boxrec + (size_t)b * kFatRecBytes) + 12; }
__device__ inline bool padding_node(const uint32_t *nd) { return (nd[12] | nd[13] | nd[14] | nd[15]) == 0u; }   // (zeroed bytes behind an odd number of nodes: no node has child 0)

// ---- steps 2b + 5a, one thread per node of one node array: the unpadded box of every LEAF child from the moved triangles, their union, and --
//      quadx != nullptr, the plain array -- the quad rule for every quad leaf and the mark on its X record ----
__global__ void rf_leaf_kernel(refit::Geo g, View v, uint32_t off_nodes, uint32_t n_nodes, float *childbox, float *leafbox, unsigned char *quadx, uint32_t *flag) {
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i >= n_nodes) return;
    const uint32_t *nd = reinterpret_cast<const uint32_t *>(v.blob + off_nodes + (size_t)i * kQ4NodeBytes);
    float L[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };
    const bool padding = padding_node(nd);
    for (int k = 0; k < 4; ++k) {
        float b[6] = { INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY };
        const int32_t c = (int32_t)nd[12 + k];
        if (!padding && c < 0 && c != kQ4Empty) {
            const uint32_t code = (uint32_t)~c, kind = code & 7u;
            uint32_t first = code >> 3, count = 0;
            if (kind == refit::kCodeBox) {
                const uint32_t bx = first - v.n_fat;
                if (first >= v.n_fat && bx < v.n_boxrec) { const uint32_t *row3 = box_row3(v, bx); first = row3[0]; count = (row3[3] >> 31) ? 2u : 12u; }
            } else {
                count = refit::code_records(code);
            }
            if (count == 0u || (uint64_t)first + count > v.n_fat) { atomicMin(&flag[kFlagNode], i); count = 0; }
            for (uint32_t r = first; r < first + count; ++r) {
                const uint32_t prim = rec_prim(v, r);
                if (prim >= v.n_tris) { atomicMin(&flag[kFlagNode], i); continue; }
                refit::grow_tri(g, prim, b, b + 3);
            }
            if (quadx && kind == refit::kCodeQuad && count == 2u) {
                const uint32_t x = rec_prim(v, first), y = rec_prim(v, first + 1u);
                if (x < v.n_tris && y < v.n_tris && !refit::quad_still(g, x, y)) atomicMin(&flag[kFlagQuad], x);
                quadx[first] = 1;
                atomicAdd(&flag[kCountQuads], 1u);
            }
        }
        for (int a = 0; a < 6; ++a) childbox[((size_t)i * 4 + k) * 6 + a] = b[a];
        for (int a = 0; a < 3; ++a) { L[a] = fminf(L[a], b[a]); L[3 + a] = fmaxf(L[3 + a], b[3 + a]); }
    }
    for (int a = 0; a < 6; ++a) leafbox[(size_t)i * 6 + a] = L[a];
}

// ---- step 5b, one bottom-up pass: a node's box = its leaf children's union and the boxes its inner children had after the pass before.
//      changed != nullptr: the pass only CHECKS that nothing moves any more (the tree was deeper than the passes run) ----
__global__ void rf_pass_kernel(const unsigned char *nodes, uint32_t n_nodes, const float *leafbox, const float *src, float *dst, uint32_t *changed) {
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i >= n_nodes) return;
    const uint32_t *nd = reinterpret_cast<const uint32_t *>(nodes + (size_t)i * kQ4NodeBytes);
    float b[6];
    for (int a = 0; a < 6; ++a) b[a] = leafbox[(size_t)i * 6 + a];
    if (!padding_node(nd))
        for (int k = 0; k < 4; ++k) {
            const int32_t c = (int32_t)nd[12 + k];
            if (c < 0 || (uint32_t)c >= n_nodes) continue;
            for (int a = 0; a < 3; ++a) { b[a] = fminf(b[a], src[(size_t)c * 6 + a]); b[3 + a] = fmaxf(b[3 + a], src[(size_t)c * 6 + 3 + a]); }
        }
    if (changed) {
        bool same = true;
        for (int a = 0; a < 6; ++a) same = same && b[a] == src[(size_t)i * 6 + a];
        if (!same) atomicMin(changed, i);
        return;
    }
    for (int a = 0; a < 6; ++a) dst[(size_t)i * 6 + a] = b[a];
}

// ---- step 5c: pad and quantise every node (q4node.h) into scratch; child codes and unused slots as they are ----
__global__ void rf_quantize_kernel(const unsigned char *nodes, uint32_t n_nodes, const float *childbox, const float *nodebox, const Hdr *hdr, uint32_t *out, uint32_t *flag) {
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i >= n_nodes) return;
    const uint32_t *nd = reinterpret_cast<const uint32_t *>(nodes + (size_t)i * kQ4NodeBytes);
    uint32_t *o = out + (size_t)i * 16;
    if (padding_node(nd)) { for (int k = 0; k < 16; ++k) o[k] = nd[k]; return; }
    float cb[24], f32[32];
    uint32_t child[4];
    for (int k = 0; k < 4; ++k) {
        child[k] = nd[12 + k];
        const int32_t c = (int32_t)child[k];
        const float *b = childbox + ((size_t)i * 4 + k) * 6;
        if (c >= 0) {
            if ((uint32_t)c >= n_nodes || (uint32_t)c <= i) { atomicMin(&flag[kFlagNode], i); b = nodebox + (size_t)i * 6; }
            else b = nodebox + (size_t)c * 6;
        }
        for (int a = 0; a < 6; ++a) cb[k * 6 + a] = b[a];
        if (c != kQ4Empty && !(b[0] <= b[3] && b[1] <= b[4] && b[2] <= b[5])) atomicMin(&flag[kFlagNode], i);
    }
    refit::node_floats(cb, child, hdr->pad, f32);
    quantize_node4(f32, o);
}

// ---- the node-area figure of trg_refit_info: per-block partial sums in a fixed order, then one thread adds them in order ----
__global__ void rf_area_kernel(const unsigned char *nodes, uint32_t n_nodes, double *partial) {
    __shared__ double sh[kT];
    double sum = 0.0;
    for (uint32_t i = blockIdx.x * kT + threadIdx.x; i < n_nodes; i += gridDim.x * kT) {
        const uint32_t *nd = reinterpret_cast<const uint32_t *>(nodes + (size_t)i * kQ4NodeBytes);
        if (!padding_node(nd)) sum += refit::node_half_area(nd);
    }
    sh[threadIdx.x] = sum;
    __syncthreads();
    for (int s = kT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}
__global__ void rf_area_final_kernel(const double *partial, uint32_t n_partials, double *out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double sum = 0.0;
    for (uint32_t b = 0; b < n_partials; ++b) sum += partial[b];
    *out = sum;
}

// ---- steps 2c + 4, one thread per box record: the frame from the box's twelve moved triangles (a lone quad dressed as a box: from its quad), checked
//      by the builder's rule and against the face table the record keeps; the rows go to scratch ----
__global__ void rf_box_kernel(refit::Geo g, View v, const Hdr *hdr, float *boxrows, uint32_t *flag) {
    const uint32_t b = blockIdx.x * kT + threadIdx.x;
    if (b >= v.n_boxrec) return;
    const uint32_t *row3 = box_row3(v, b);
    const uint32_t first = row3[0];
    const bool lone = (row3[3] >> 31) != 0u;
    const uint32_t count = lone ? 2u : 12u;
    if ((uint64_t)first + count > v.n_fat) { atomicMin(&flag[kFlagNode], 0u); return; }
    uint32_t prim[12], k0 = kNone;
    for (uint32_t r = 0; r < count; ++r) {
        prim[r] = rec_prim(v, first + r);
        if (prim[r] >= v.n_tris) { atomicMin(&flag[kFlagNode], 0u); return; }
        k0 = prim[r] < k0 ? prim[r] : k0;
    }
    refit::Frame fr;
    bool ok;
    if (lone) {
        float xr[12], yr[12];
        refit::tri_rows(g, prim[0], xr); refit::tri_rows(g, prim[1], yr);
        ok = refit::lone_quad_frame(xr, yr + 8, fr);
    } else {
        uint32_t face_quad[6] = { 0, 0, 0, 0, 0, 0 };
        ok = refit::box_group_pos(g, k0, fr, face_quad);
        for (int f = 0; f < 6 && ok; ++f) {   // the face table of the loaded record must still name the quads the frame assigns
            const uint32_t off = (row3[2 + f / 4] >> (7 * (f % 4))) & 15u;
            if (off + 1u >= 12u) { ok = false; break; }
            const uint32_t px = prim[off], py = prim[off + 1u];
            ok = ((px < py ? px : py) - k0) / 2u == face_quad[f];
        }
    }
    if (!ok) { atomicMin(&flag[kFlagBox], k0); return; }
    refit::frame_rows(fr, hdr->center, boxrows + (size_t)b * 12);
}
__global__ void rf_box_write_kernel(View v, const float *boxrows) {
    const uint32_t t = blockIdx.x * kT + threadIdx.x;
    if (t >= v.n_boxrec * 12u) return;
    reinterpret_cast<float *>(v.blob + v.off_boxrec + (size_t)(t / 12u) * kFatRecBytes)[t % 12u] = boxrows[t];
}

// ---- step 3, one thread per leaf record: both 128-byte forms from the true vertices of the record's triangle ----
__global__ void rf_records_kernel(refit::Geo g, const float *nrm, View v, float cx, float cy, float cz, const unsigned char *quadx) {
    const uint32_t r = blockIdx.x * kT + threadIdx.x;
    if (r >= v.n_fat) return;
    float *mt = reinterpret_cast<float *>(v.blob + v.off_fat + (size_t)r * kFatRecBytes);
    float *pl = reinterpret_cast<float *>(v.blob + v.off_fat_planes + (size_t)r * kFatRecBytes);
    const uint32_t prim = refit::f2u(mt[3]);
    if (prim >= v.n_tris) return;
    float rows[12], yrows[12], planes[12];
    refit::tri_rows(g, prim, rows);
    const float *e2row = rows + 8;
    if (quadx[r] && r + 1u < v.n_fat) {   // the X of a quad: the parallelogram's second edge is its Y's
        const uint32_t py = rec_prim(v, r + 1u);
        if (py < v.n_tris) { refit::tri_rows(g, py, yrows); e2row = yrows + 8; }
    }
    const float center[3] = { cx, cy, cz };
    refit::plane_rows(rows, e2row, center, planes);
    for (int k = 0; k < 3; ++k) { mt[k] = rows[k]; mt[4 + k] = rows[4 + k]; mt[8 + k] = rows[8 + k]; }
    for (int k = 0; k < 12; ++k) pl[k] = planes[k];
    if (nrm)
        for (int k = 0; k < 9; ++k) { const float n = nrm[(size_t)prim * 9 + k]; mt[12 + k] = n; pl[14 + k] = n; }
}

// ---- include/trg_pose.h: one thread per vertex, then -- from the next whole block on, nrm_out != nullptr -- one per corner normal.  A thread
//      reads its map word, its object's 12 floats and 12 bytes, and writes 12 bytes; as three dword accesses each: a vertex is only 4-byte aligned,
//      and a wave's 64 lanes together still cover one contiguous 768-byte span, every cache line of it used whole ----
__global__ void rf_pose_kernel(const float *rest_pos, const uint32_t *vtx_obj, uint32_t n_verts, const float *rest_nrm, const uint32_t *tri_obj, uint32_t n_corners,
                               const float *xforms, float *pos_out, float *nrm_out) {
    const uint32_t vertex_blocks = (n_verts + kT - 1) / kT;
    if (blockIdx.x < vertex_blocks) {
        const uint32_t v = blockIdx.x * kT + threadIdx.x;
        if (v >= n_verts) return;
        const uint32_t o = vtx_obj[v];
        const float p[3] = { rest_pos[(size_t)v * 3], rest_pos[(size_t)v * 3 + 1], rest_pos[(size_t)v * 3 + 2] };
        float q[3] = { p[0], p[1], p[2] };
        if (o != pose::kNoObject) {
            float m[12];
            for (int k = 0; k < 12; ++k) m[k] = xforms[(size_t)o * 12 + k];
            pose::point(m, p, q);
        }
        for (int k = 0; k < 3; ++k) pos_out[(size_t)v * 3 + k] = q[k];
        return;
    }
    const uint32_t k = (blockIdx.x - vertex_blocks) * kT + threadIdx.x;
    if (!nrm_out || k >= n_corners) return;
    const uint32_t o = tri_obj[k / 3u];
    float m[12];
    for (int j = 0; j < 12; ++j) m[j] = xforms[(size_t)o * 12 + j];
    const float n[3] = { rest_nrm[(size_t)k * 3], rest_nrm[(size_t)k * 3 + 1], rest_nrm[(size_t)k * 3 + 2] };
    float q[3];
    pose::normal(m, n, q);
    for (int j = 0; j < 3; ++j) nrm_out[(size_t)k * 3 + j] = q[j];
}

// ---- include/trg_skin.h: one thread per vertex, then -- from the next whole block on, nrm_out != nullptr -- one per corner normal.  A thread reads
//      its ids and weights as one 16-byte record each, blends bone by bone (a bone is three 16-byte rows; twelve accumulators and one bone are live),
//      and moves 12 bytes in and 12 out as the pose kernel does.  A corner thread reads its index first and blends its vertex's matrix again: no
//      scratch, no second launch, and the same operations on the same inputs give the same bits ----
__device__ inline void rf_skin_matrix(const float4 *bones, const uint4 id, const float4 w, float *M) {
    const uint32_t ids[4] = { id.x, id.y, id.z, id.w };
    const float ws[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 *b = bones + (size_t)ids[j] * 3;
        const float4 r0 = b[0], r1 = b[1], r2 = b[2];
        const float bone[12] = { r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w };
        if (j == 0) skin::blend_first(bone, ws[0], M);
        else skin::blend_next(bone, ws[j], M);
    }
}
__global__ void rf_skin_kernel(const float *rest_pos, const uint4 *ids, const float4 *weights, uint32_t n_verts, const float *rest_nrm, const uint32_t *idx,
                               uint32_t n_corners, const float4 *bones, float *pos_out, float *nrm_out) {
    const uint32_t vertex_blocks = (n_verts + kT - 1) / kT;
    float M[12], q[3];
    if (blockIdx.x < vertex_blocks) {
        const uint32_t v = blockIdx.x * kT + threadIdx.x;
        if (v >= n_verts) return;
        const float p[3] = { rest_pos[(size_t)v * 3], rest_pos[(size_t)v * 3 + 1], rest_pos[(size_t)v * 3 + 2] };
        rf_skin_matrix(bones, ids[v], weights[v], M);
        pose::point(M, p, q);
        for (int k = 0; k < 3; ++k) pos_out[(size_t)v * 3 + k] = q[k];
        return;
    }
    const uint32_t k = (blockIdx.x - vertex_blocks) * kT + threadIdx.x;
    if (!nrm_out || k >= n_corners) return;
    const uint32_t v = idx[k];   // (< n_verts: trg_skin_bind checked the indices it uploaded)
    const float n[3] = { rest_nrm[(size_t)k * 3], rest_nrm[(size_t)k * 3 + 1], rest_nrm[(size_t)k * 3 + 2] };
    rf_skin_matrix(bones, ids[v], weights[v], M);
    pose::normal(M, n, q);
    for (int j = 0; j < 3; ++j) nrm_out[(size_t)k * 3 + j] = q[j];
}

// ---- include/trg_morph.h: the launch shape of the skin kernel -- one thread per vertex, then, from the next whole block on and only when a corner
//      can change, one per corner normal.  A vertex thread reads the two ends of its range and walks its records, 16 bytes each and one load each;
//      the weight comes from the n_targets-float table the apply uploaded, and a zero weight leaves the sum alone.  A corner thread reads its index and
//      walks that vertex's NORMAL records; under bones both blend their vertex's matrix as the skin kernel does (no scratch, one launch).  The trip
//      count differs per lane: the loop is NOT unrolled -- one record and three accumulators are live, nothing else grows with it ----
__device__ inline bool rf_morph_walk(const float4 *recs, const uint32_t *vfirst, const float *tw, uint32_t v, float *acc) {
    const uint32_t e0 = vfirst[v], e1 = vfirst[v + 1];
    bool touched = false;
#pragma unroll 1
    for (uint32_t e = e0; e < e1; ++e) {
        const float4 r = recs[e];
        const float w = tw[__float_as_uint(r.w)];
        // the skip as a SELECT: the whole record stays one 16-byte load issued before the weight is known (a branch lets the compiler sink the
        // delta's load behind the weight's: three dependent loads per entry), and an inactive target still leaves the accumulator's bits alone
        const bool on = w != 0.f;
        const float d[3] = { r.x, r.y, r.z };
        float sum[3] = { acc[0], acc[1], acc[2] };
        morph::add(w, d, sum);
        for (int a = 0; a < 3; ++a) acc[a] = on ? sum[a] : acc[a];
        touched = touched || on;
    }
    return touched;
}
template <bool kBones, bool kNormalDeltas>
__global__ void rf_morph_kernel(const float *rest_pos, const uint32_t *vfirst, const float4 *pos_recs, const float4 *nrm_recs, const float *tw, uint32_t n_verts,
                                const float *rest_nrm, const uint32_t *idx, uint32_t n_corners, const uint4 *ids, const float4 *weights, const float4 *bones,
                                float *pos_out, float *nrm_out) {
    const uint32_t vertex_blocks = (n_verts + kT - 1) / kT;
    float M[12], q[3];
    if (blockIdx.x < vertex_blocks) {
        const uint32_t v = blockIdx.x * kT + threadIdx.x;
        if (v >= n_verts) return;
        float p[3] = { rest_pos[(size_t)v * 3], rest_pos[(size_t)v * 3 + 1], rest_pos[(size_t)v * 3 + 2] };
        rf_morph_walk(pos_recs, vfirst, tw, v, p);
        if (kBones) {
            rf_skin_matrix(bones, ids[v], weights[v], M);
            pose::point(M, p, q);
        } else {
            for (int k = 0; k < 3; ++k) q[k] = p[k];
        }
        for (int k = 0; k < 3; ++k) pos_out[(size_t)v * 3 + k] = q[k];
        return;
    }
    const uint32_t k = (blockIdx.x - vertex_blocks) * kT + threadIdx.x;
    if (!nrm_out || k >= n_corners) return;
    const uint32_t v = idx[k];   // (< n_verts: trg_morph_bind checked the indices it uploaded)
    const float rest[3] = { rest_nrm[(size_t)k * 3], rest_nrm[(size_t)k * 3 + 1], rest_nrm[(size_t)k * 3 + 2] };
    float n1[3] = { rest[0], rest[1], rest[2] };
    if (kNormalDeltas) {
        float n[3] = { rest[0], rest[1], rest[2] };
        const bool touched = rf_morph_walk(nrm_recs, vfirst, tw, v, n);
        morph::finish_normal(rest, n, touched, n1);
    }
    if (kBones) {
        rf_skin_matrix(bones, ids[v], weights[v], M);
        pose::normal(M, n1, q);
    } else {
        for (int j = 0; j < 3; ++j) q[j] = n1[j];
    }
    for (int j = 0; j < 3; ++j) nrm_out[(size_t)k * 3 + j] = q[j];
}

// ---- include/trg_rig.h: one launch per LEVEL of the joint forest, one thread per joint of that level, reached through `order` (the level table of
//      trg_rig_math.h).  A thread finds its key pair (the search reads only the times), loads the two records as three 16-byte rows each, samples,
//      builds its local matrix, reads its parent's world rows -- which the launch BEFORE this one wrote: no thread ever waits on another thread's
//      store, the order between levels is the stream's --, composes, writes its world rows, composes with its inverse bind and writes its bone rows.
//      kRoot: the level is level 0 and nobody has a parent; kInv: there are inverse binds.  No LDS, no atomics, no grid stride ----
__device__ inline void rf_rows_get(const float4 *src, float *m) {
    const float4 r0 = src[0], r1 = src[1], r2 = src[2];
    m[0] = r0.x; m[1] = r0.y; m[2] = r0.z; m[3] = r0.w; m[4] = r1.x; m[5] = r1.y; m[6] = r1.z; m[7] = r1.w; m[8] = r2.x; m[9] = r2.y; m[10] = r2.z; m[11] = r2.w;
}
__device__ inline void rf_rows_put(float4 *dst, const float *m) {
    dst[0] = make_float4(m[0], m[1], m[2], m[3]);
    dst[1] = make_float4(m[4], m[5], m[6], m[7]);
    dst[2] = make_float4(m[8], m[9], m[10], m[11]);
}
template <bool kRoot, bool kInv>
__global__ void rf_rig_level_kernel(const uint32_t *order, uint32_t first, uint32_t count, const uint32_t *parent, const uint32_t *kfirst, const float4 *keys,
                                    const uint32_t *clock_of, const float *clocks, const float4 *inv_bind, float4 *world, float4 *bones) {
    const uint32_t k = blockIdx.x * kT + threadIdx.x;
    if (k >= count) return;
    const uint32_t j = order[first + k];
    const float t = clocks[clock_of[j]];
    uint32_t ia, ib;
    rig::key_pair(reinterpret_cast<const float *>(keys), kfirst[j], kfirst[j + 1] - 1u, t, &ia, &ib);
    float ka[12], kb[12], T[3], R[4], S[3], L[12], W[12];
    rf_rows_get(keys + (size_t)ia * 3, ka);
    rf_rows_get(keys + (size_t)ib * 3, kb);
    rig::sample(ka, kb, ia == ib, t, T, R, S);
    rig::local(T, R, S, L);
    if (kRoot) {
        for (int e = 0; e < 12; ++e) W[e] = L[e];
    } else {
        float P[12];
        rf_rows_get(world + (size_t)parent[j] * 3, P);
        rig::compose(P, L, W);
    }
    rf_rows_put(world + (size_t)j * 3, W);
    if (kInv) {
        float I[12], B[12];
        rf_rows_get(inv_bind + (size_t)j * 3, I);
        rig::compose(W, I, B);
        rf_rows_put(bones + (size_t)j * 3, B);
    } else {
        rf_rows_put(bones + (size_t)j * 3, W);
    }
}

// ---- per-context scratch (grow-only): trg_ctx::refit, created on first use, freed by refit_state_free ----
struct Buf {
    void *p = nullptr;
    size_t bytes = 0;
    template <typename T> T *as() const { return static_cast<T *>(p); }
};
}  // namespace

struct trg::RefitState {
    Buf pos, idx, nrm, childbox, leafbox, ping, pong, qplain, qbox, quadx, boxrows, partial, hdr;
    Hdr host{};                    // what the host sends and reads back
    trg_refit_info last{};
    const void *area_blob = nullptr;   // the blob whose as-loaded areas are remembered, and what its arrays summed to after this unit's last write
    double loaded_area[2] = { 0.0, 0.0 }, written_area[2] = { 0.0, 0.0 };
    // ---- THE BINDING PROTOCOL, once, for include/trg_pose.h, trg_skin.h and trg_morph.h (a unit adds its own inputs and its kernel) ----
    // bind     validates on the host FIRST -- a refusal there leaves an earlier binding as it was -- then marks the unit unbound, uploads the rest
    //          geometry and the indices, sets all three copies to the rest pose, waits, remembers the scene and marks the unit bound.  A failure
    //          while allocating or copying leaves it unbound.
    // apply    poses into posed[spare()], refits the loaded scene from that copy (apply_finish) and only then rotates: posed[cur] is the current
    //          pose, posed[prev] the one before.  A refused apply or refit has written the spare copy alone: current, previous and scene stay.
    // read / buffers  the current copy to the host / the addresses of current and previous.  release frees one unit's buffers.
    // The three bindings of a context are independent: bound together, each with its own current and previous pose; the loaded scene is the last
    // apply's.  The scene a binding was made for is known by a HEURISTIC (trg_ctx.h has no load counter and stays as it is): its memory, its layout
    // and -- a reload of as many bytes is usually handed the same address -- the time its build took, which every trg_load_scene measures anew.
    struct Binding {
        Buf rest_pos, rest_nrm, idx, posed[3], posed_nrm[3];
        uint32_t n_verts = 0, n_tris = 0, cur = 0, prev = 1;
        bool bound = false, has_nrm = false;
        const void *blob = nullptr;
        double build_ms = 0.0;
        uint32_t blob_bytes = 0, n_nodes4 = 0, n_fat = 0, off_fat = 0;
        bool same_scene(const trg_ctx *c) const {
            return c->scene_loaded && blob == (const void *)c->blob && n_tris == c->sc.n_tris && build_ms == c->last_build_ms && blob_bytes == c->sc.blob_bytes &&
                   n_nodes4 == c->sc.n_nodes4 && n_fat == c->sc.n_fat && off_fat == c->sc.off_fat;
        }
        void remember_scene(const trg_ctx *c) {
            blob = c->blob; build_ms = c->last_build_ms; blob_bytes = c->sc.blob_bytes; n_nodes4 = c->sc.n_nodes4; n_fat = c->sc.n_fat; off_fat = c->sc.off_fat;
        }
        uint32_t spare() const { return 3u - cur - prev; }
        void rotate() { const uint32_t s = spare(); prev = cur; cur = s; }
        float *pos_of(uint32_t k) const { return posed[k].as<float>(); }
        float *nrm_of(uint32_t k) const { return has_nrm ? posed_nrm[k].as<float>() : nullptr; }
        // vertex blocks, then -- corners -- corner blocks: the grid of every apply kernel
        uint32_t blocks(bool corners) const { return (uint32_t)(((size_t)n_verts + kT - 1) / kT + (corners ? ((size_t)n_tris * 3 + kT - 1) / kT : 0)); }
        template <typename F> void each_shared(F f) { for (Buf *b : { &rest_pos, &rest_nrm, &idx, &posed[0], &posed[1], &posed[2], &posed_nrm[0], &posed_nrm[1], &posed_nrm[2] }) f(*b); }
    };
    // what each unit adds: its own buffers, listed once (each_own), and their counts
    struct Pose : Binding {
        Buf vtx_obj, tri_obj, xforms;
        uint32_t n_objects = 0;
        template <typename F> void each_own(F f) { for (Buf *b : { &vtx_obj, &tri_obj, &xforms }) f(*b); }
    } pose;
    // ids and weights are 16-byte records per vertex, bones 48 bytes each
    struct Skin : Binding {
        Buf ids, weights, bones;
        uint32_t n_bones = 0;
        template <typename F> void each_own(F f) { for (Buf *b : { &ids, &weights, &bones }) f(*b); }
    } skin;
    // vfirst is n_verts + 1 words; pos_recs and (has_dnrm) nrm_recs 16-byte records; tw the n_targets weights of the last apply; ids, weights, bones as
    // the skin binding's, only with has_bones
    struct Morph : Binding {
        Buf vfirst, pos_recs, nrm_recs, tw, ids, weights, bones;
        uint32_t n_targets = 0, n_bones = 0;
        bool has_dnrm = false, has_bones = false;
        template <typename F> void each_own(F f) { for (Buf *b : { &vfirst, &pos_recs, &nrm_recs, &tw, &ids, &weights, &bones }) f(*b); }
    } morph;
    // include/trg_rig.h.  NOT a Binding: it holds no geometry, knows no scene and survives trg_load_scene.  keys are 48-byte records, world and bones
    // 48 bytes per joint (hipMalloc aligns them far beyond the 16 bytes their float4 rows need); the level table stays on the host, which launches
    // level by level.  evaluated: world and bones hold an evaluation
    struct Rig {
        Buf parent, order, keys, kfirst, clock_of, inv_bind, clocks, world, bones;
        uint32_t n_joints = 0, n_keys = 0, n_clocks = 0, n_levels = 0;
        uint32_t level_first[rig::kMaxLevels + 1] = {};
        bool bound = false, has_inv = false, evaluated = false;
        template <typename F> void each_own(F f) { for (Buf *b : { &parent, &order, &keys, &kfirst, &clock_of, &inv_bind, &clocks, &world, &bones }) f(*b); }
    } rig;
};

namespace {

template <typename B, typename F>
void each_binding_buffer(B &b, F f) {
    b.each_shared(f);
    b.each_own(f);
}
template <typename F>
void each_buffer(RefitState &s, F f) {
    for (Buf *b : { &s.pos, &s.idx, &s.nrm, &s.childbox, &s.leafbox, &s.ping, &s.pong, &s.qplain, &s.qbox, &s.quadx, &s.boxrows, &s.partial, &s.hdr }) f(*b);
    each_binding_buffer(s.pose, f);
    each_binding_buffer(s.skin, f);
    each_binding_buffer(s.morph, f);
    s.rig.each_own(f);
}
int grow(trg_ctx *c, Buf &b, size_t need, const char *what) {
    if (need <= b.bytes && b.p) return TRG_OK;
    if (b.p) { (void)hipStreamSynchronize(c->stream); (void)hipFree(b.p); b.p = nullptr; b.bytes = 0; }
    const size_t want = need + need / 8 + 256;
    const hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) { b.p = nullptr; return fail(c, TRG_ERR_NOMEM, "trg_refit_scene: %s hipMalloc(%zu) failed: %s", what, want, hipGetErrorString(e)); }
    b.bytes = want;
    return TRG_OK;
}
RefitState &state_of(trg_ctx *c) {
    if (!c->refit) c->refit = new RefitState;
    return *c->refit;
}

inline dim3 blocks_for(size_t n) { return dim3((uint32_t)((n + kT - 1) / kT)); }
#define RF_LAUNCH(c, kernel, grid, ...)                                                                                                 \
    do {                                                                                                                                \
        hipLaunchKernelGGL(kernel, grid, dim3(kT), 0, (c)->stream, __VA_ARGS__);                                                        \
        const hipError_t e_ = hipGetLastError();                                                                                        \
        if (e_ != hipSuccess) return fail((c), TRG_ERR_DEVICE, "trg_refit_scene: launch of %s failed: %s", #kernel, hipGetErrorString(e_)); \
    } while (0)

// one node array: leaf boxes, the bottom-up passes, the check that they settled, the quantised nodes into `q`, and the area sums before / after
int refit_node_array(trg_ctx *c, RefitState &s, const refit::Geo &g, const View &v, uint32_t off_nodes, uint32_t n_nodes, uint32_t passes, Buf &q, bool plain,
                     double *area_before, double *area_after) {
    Hdr *hdr = s.hdr.as<Hdr>();
    const unsigned char *nodes = v.blob + off_nodes;
    RF_LAUNCH(c, rf_leaf_kernel, blocks_for(n_nodes), g, v, off_nodes, n_nodes, s.childbox.as<float>(), s.leafbox.as<float>(), plain ? s.quadx.as<unsigned char>() : nullptr, hdr->flag);
    RF_HIPCHK(c, hipMemcpyAsync(s.ping.p, s.leafbox.p, (size_t)n_nodes * 24, hipMemcpyDeviceToDevice, c->stream));
    float *src = s.ping.as<float>(), *dst = s.pong.as<float>();
    for (uint32_t p = 0; p < passes; ++p) {
        RF_LAUNCH(c, rf_pass_kernel, blocks_for(n_nodes), nodes, n_nodes, s.leafbox.as<float>(), src, dst, nullptr);
        std::swap(src, dst);
    }
    RF_LAUNCH(c, rf_pass_kernel, blocks_for(n_nodes), nodes, n_nodes, s.leafbox.as<float>(), src, dst, &hdr->flag[kFlagNode]);
    RF_LAUNCH(c, rf_quantize_kernel, blocks_for(n_nodes), nodes, n_nodes, s.childbox.as<float>(), src, hdr, q.as<uint32_t>(), hdr->flag);
    const uint32_t nb = std::min<uint32_t>(kMaxPartials, (n_nodes + kT - 1) / kT);
    RF_LAUNCH(c, rf_area_kernel, dim3(nb), nodes, n_nodes, s.partial.as<double>());
    RF_LAUNCH(c, rf_area_final_kernel, dim3(1), s.partial.as<double>(), nb, area_before);
    RF_LAUNCH(c, rf_area_kernel, dim3(nb), q.as<unsigned char>(), n_nodes, s.partial.as<double>());
    RF_LAUNCH(c, rf_area_final_kernel, dim3(1), s.partial.as<double>(), nb, area_after);
    return TRG_OK;
}

// on_device: pos, nrm and idx are device memory of the context's device, read where they are; else host arrays, uploaded into scratch first.  That
// upload is the only difference between the two.
int refit_device(trg_ctx *c, const float *pos, const float *nrm, const uint32_t *idx, uint32_t n_verts, uint32_t n_tris, bool on_device) {
    const auto t0 = std::chrono::steady_clock::now();
    RefitState &s = state_of(c);
    const SceneDesc sc = c->sc;
    const uint32_t n4 = sc.n_nodes4;
    const bool has_box = sc.off_nodes4_box != sc.off_nodes4 && sc.off_fat > sc.off_nodes4_box;
    const uint32_t n4b = has_box ? (sc.off_fat - sc.off_nodes4_box) / kQ4NodeBytes : 0u;   // (may count one zeroed line half of padding: padding_node)
    const uint32_t nmax = std::max(n4, n4b);
    if (n4 == 0 || sc.n_fat == 0) return fail(c, TRG_ERR_INVALID, "trg_refit_scene: the loaded scene has no node array to refit");
    // the blob's sections must lie where this unit expects them before a kernel is handed their offsets
    if ((uint64_t)sc.off_nodes4 + (uint64_t)n4 * kQ4NodeBytes > sc.blob_bytes || (uint64_t)sc.off_fat_planes + (uint64_t)sc.n_fat * kFatRecBytes > sc.blob_bytes ||
        (uint64_t)sc.off_fat + (uint64_t)sc.n_fat * kFatRecBytes > sc.off_fat_planes || (uint64_t)sc.off_boxrec + (uint64_t)sc.n_boxrec * kFatRecBytes > sc.blob_bytes)
        return fail(c, TRG_ERR_INVALID, "trg_refit_scene: the loaded scene's layout is not the one this unit knows");

    int rc = TRG_OK;
    if ((!on_device && ((rc = grow(c, s.pos, (size_t)n_verts * 12, "positions")) || (rc = grow(c, s.idx, (size_t)n_tris * 12, "indices")) ||
                        (nrm && (rc = grow(c, s.nrm, (size_t)n_tris * 36, "normals"))))) || (rc = grow(c, s.childbox, (size_t)nmax * 96, "child boxes")) ||
        (rc = grow(c, s.leafbox, (size_t)nmax * 24, "leaf boxes")) || (rc = grow(c, s.ping, (size_t)nmax * 24, "node boxes")) ||
        (rc = grow(c, s.pong, (size_t)nmax * 24, "node boxes")) || (rc = grow(c, s.qplain, (size_t)n4 * kQ4NodeBytes, "nodes")) ||
        (has_box && (rc = grow(c, s.qbox, (size_t)n4b * kQ4NodeBytes, "box-flavour nodes"))) || (rc = grow(c, s.quadx, (size_t)sc.n_fat, "quad marks")) ||
        (sc.n_boxrec && (rc = grow(c, s.boxrows, (size_t)sc.n_boxrec * 48, "box frames"))) || (rc = grow(c, s.partial, (size_t)kMaxPartials * 48, "partial results")) ||
        (rc = grow(c, s.hdr, sizeof(Hdr), "flags")))
        return rc;

    // step 1: upload
    if (!on_device) {
        RF_HIPCHK(c, hipMemcpyAsync(s.pos.p, pos, (size_t)n_verts * 12, hipMemcpyHostToDevice, c->stream));
        RF_HIPCHK(c, hipMemcpyAsync(s.idx.p, idx, (size_t)n_tris * 12, hipMemcpyHostToDevice, c->stream));
        if (nrm) RF_HIPCHK(c, hipMemcpyAsync(s.nrm.p, nrm, (size_t)n_tris * 36, hipMemcpyHostToDevice, c->stream));
    }
    s.host = Hdr{};
    for (int k = 0; k < 5; ++k) s.host.flag[k] = kNone;
    RF_HIPCHK(c, hipMemcpyAsync(s.hdr.p, &s.host, sizeof(Hdr), hipMemcpyHostToDevice, c->stream));
    RF_HIPCHK(c, hipMemsetAsync(s.quadx.p, 0, sc.n_fat, c->stream));

    // step 2 (and everything that only READS the scene): bounds, checks, node boxes, quantised nodes and box frames into scratch
    Hdr *hdr = s.hdr.as<Hdr>();
    const refit::Geo g{ on_device ? pos : s.pos.as<float>(), on_device ? idx : s.idx.as<uint32_t>(), n_verts, n_tris };
    const float *d_nrm = !nrm ? nullptr : on_device ? nrm : s.nrm.as<float>();
    const View v{ c->blob, sc.off_fat, sc.off_fat_planes, sc.off_boxrec, sc.n_fat, has_box ? sc.n_boxrec : 0u, n_tris };
    const uint32_t nb = std::min<uint32_t>(kMaxPartials, (n_tris + kT - 1) / kT);
    RF_LAUNCH(c, rf_bounds_kernel, dim3(nb), g, d_nrm, s.partial.as<float>(), hdr->flag);
    RF_LAUNCH(c, rf_bounds_final_kernel, dim3(1), s.partial.as<float>(), nb, hdr);
    const uint32_t passes = std::max(c->bvh_depth4, 1u);
    if ((rc = refit_node_array(c, s, g, v, sc.off_nodes4, n4, passes, s.qplain, true, &hdr->area[0], &hdr->area[1]))) return rc;
    if (has_box && (rc = refit_node_array(c, s, g, v, sc.off_nodes4_box, n4b, passes, s.qbox, false, &hdr->area[2], &hdr->area[3]))) return rc;
    if (v.n_boxrec) RF_LAUNCH(c, rf_box_kernel, blocks_for(v.n_boxrec), g, v, hdr, s.boxrows.as<float>(), hdr->flag);

    // the call's one wait: the bounds and the flag words
    RF_HIPCHK(c, hipMemcpyAsync(&s.host, s.hdr.p, sizeof(Hdr), hipMemcpyDeviceToHost, c->stream));
    RF_HIPCHK(c, hipStreamSynchronize(c->stream));
    const Hdr &h = s.host;
    if (h.flag[kFlagIndex] != kNone) return fail(c, TRG_ERR_INVALID, "trg_refit_scene: triangle %u has an index out of range (%u vertices)", h.flag[kFlagIndex], n_verts);
    if (h.flag[kFlagFinite] != kNone) return fail(c, TRG_ERR_INVALID, "trg_refit_scene: triangle %u has a coordinate that is not finite", h.flag[kFlagFinite]);
    if (h.flag[kFlagQuad] != kNone)
        return fail(c, TRG_ERR_RANGE, "trg_refit_scene: triangle %u and its neighbour are a quad leaf of the loaded tree and no longer a parallelogram (reload the scene)", h.flag[kFlagQuad]);
    if (h.flag[kFlagBox] != kNone)
        return fail(c, TRG_ERR_RANGE, "trg_refit_scene: the box leaf that begins at triangle %u is no longer a parallelepiped to 1e-5 (reload the scene)", h.flag[kFlagBox]);
    if (h.flag[kFlagNode] != kNone)
        return fail(c, TRG_ERR_RANGE, "trg_refit_scene: node %u of the loaded tree could not be refitted (%u passes)", h.flag[kFlagNode], passes);

    // steps 3 - 5: write
    RF_LAUNCH(c, rf_records_kernel, blocks_for(sc.n_fat), g, d_nrm, v, h.center[0], h.center[1], h.center[2], s.quadx.as<unsigned char>());
    if (v.n_boxrec) RF_LAUNCH(c, rf_box_write_kernel, blocks_for((size_t)v.n_boxrec * 12), v, s.boxrows.as<float>());
    RF_HIPCHK(c, hipMemcpyAsync(c->blob + sc.off_nodes4, s.qplain.p, (size_t)n4 * kQ4NodeBytes, hipMemcpyDeviceToDevice, c->stream));
    if (has_box) RF_HIPCHK(c, hipMemcpyAsync(c->blob + sc.off_nodes4_box, s.qbox.p, (size_t)n4b * kQ4NodeBytes, hipMemcpyDeviceToDevice, c->stream));
    for (int a = 0; a < 3; ++a) { c->sc.center[a] = h.center[a]; c->scene_lo[a] = h.lo[a]; c->scene_hi[a] = h.hi[a]; }

    // the tree "as loaded": the sums this blob's arrays had when this unit first saw them -- or saw them changed by somebody else
    const bool ours = s.area_blob == (const void *)c->blob && s.written_area[0] == h.area[0] && s.written_area[1] == h.area[2];
    if (!ours) { s.area_blob = c->blob; s.loaded_area[0] = h.area[0]; s.loaded_area[1] = h.area[2]; }
    s.written_area[0] = h.area[1]; s.written_area[1] = h.area[3];
    trg_refit_info &o = s.last;
    o = trg_refit_info{};
    o.path = TRG_REFIT_DEVICE;
    o.n_records = sc.n_fat; o.n_quads = h.flag[kCountQuads]; o.n_boxes = v.n_boxrec; o.n_nodes = n4; o.n_nodes_box = n4b; o.passes = passes;
    for (int a = 0; a < 3; ++a) { o.lo[a] = h.lo[a]; o.hi[a] = h.hi[a]; }
    o.pad = h.pad;
    o.area_ratio = s.loaded_area[0] > 0.0 ? h.area[1] / s.loaded_area[0] : 0.0;
    o.area_ratio_box = (has_box && s.loaded_area[1] > 0.0) ? h.area[3] / s.loaded_area[1] : 0.0;
    o.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return TRG_OK;
}

// the small-scene path: the host builder again, with the colours and material ids the blob holds; the textures stay
int refit_rebuild(trg_ctx *c, const float *pos, const float *nrm, const uint32_t *idx, uint32_t n_verts, uint32_t n_tris) {
    const auto t0 = std::chrono::steady_clock::now();
    RefitState &s = state_of(c);
    const SceneDesc sc = c->sc;
    for (uint32_t t = 0; t < n_tris; ++t)
        for (int j = 0; j < 3; ++j) {
            const uint32_t i = idx[(size_t)t * 3 + j];
            if (i >= n_verts) return fail(c, TRG_ERR_INVALID, "trg_refit_scene: triangle %u has an index out of range (%u vertices)", t, n_verts);
            bool finite = std::isfinite(pos[(size_t)i * 3]) && std::isfinite(pos[(size_t)i * 3 + 1]) && std::isfinite(pos[(size_t)i * 3 + 2]);
            for (int k = 0; nrm && k < 3; ++k) finite = finite && std::isfinite(nrm[((size_t)t * 3 + j) * 3 + k]);
            if (!finite) return fail(c, TRG_ERR_INVALID, "trg_refit_scene: triangle %u has a coordinate that is not finite", t);
        }
    std::vector<float> col((size_t)n_tris * 9), own_nrm;
    std::vector<uint32_t> mat(n_tris);
    RF_HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_tris) {
        RF_HIPCHK(c, hipMemcpy(col.data(), c->blob + sc.off_colors, (size_t)n_tris * 36, hipMemcpyDeviceToHost));
        RF_HIPCHK(c, hipMemcpy(mat.data(), c->blob + sc.off_mats, (size_t)n_tris * 4, hipMemcpyDeviceToHost));
        if (!nrm) {
            own_nrm.resize((size_t)n_tris * 9);
            RF_HIPCHK(c, hipMemcpy(own_nrm.data(), c->blob + sc.off_normals, (size_t)n_tris * 36, hipMemcpyDeviceToHost));
            nrm = own_nrm.data();
        }
    }
    HostScene *hs = nullptr;
    if (int rc = host_scene_build(c, pos, nrm, col.data(), idx, mat.data(), n_verts, n_tris, &hs)) return rc;
    // host_scene_upload drops the textures of the scene it replaces; this scene is the same one, moved: they are kept out of its sight
    unsigned char *tex_mem = c->tex_mem;
    const TexDesc tex = c->tex;
    c->tex_mem = nullptr;
    const int rc = host_scene_upload(c, hs);
    c->tex_mem = tex_mem; c->tex = tex;
    trg_refit_info &o = s.last;
    if (rc == TRG_OK) {
        o = trg_refit_info{};
        o.path = TRG_REFIT_REBUILD;
        o.n_records = c->sc.n_fat; o.n_quads = c->bvh_quads; o.n_boxes = c->bvh_boxes; o.n_nodes = c->sc.n_nodes4;
        for (int a = 0; a < 3; ++a) { o.lo[a] = c->scene_lo[a]; o.hi[a] = c->scene_hi[a]; }
        o.pad = n_tris ? refit::scene_pad(o.lo, o.hi) : 0.f;
        o.area_ratio = 1.0;   // a tree of its own: nothing has grown loose
        o.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    host_scene_free(hs);
    return rc;
}

// what both entry points check before they look at a buffer
int refit_arguments(trg_ctx *c, const void *positions3, const void *indices, uint32_t n_verts, uint32_t n_tris) {
#if TRG_WIDE8
    return fail(c, TRG_ERR_INVALID, "trg_refit_scene: an 8-wide experiments build has no refit (reload the scene)");
#endif
    if (!c->scene_loaded || !c->blob) return fail(c, TRG_ERR_INVALID, "trg_refit_scene: no scene loaded");
    if (n_tris != c->sc.n_tris) return fail(c, TRG_ERR_INVALID, "trg_refit_scene: %u triangles, the loaded scene has %u (a changed topology is a reload)", n_tris, c->sc.n_tris);
    if (n_tris && (!positions3 || !indices || n_verts == 0)) return fail(c, TRG_ERR_INVALID, "trg_refit_scene: null buffer");
    RF_HIPCHK(c, hipSetDevice(c->device));
    return TRG_OK;
}

// ---- include/trg_pose.h: trg_refit_scene_device ----
// `need` bytes from p on: device memory of the context's device, by the runtime's own records; nothing is enqueued
int device_span(trg_ctx *c, const void *p, size_t need, const char *what, const char *who = "trg_refit_scene_device") {
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, TRG_ERR_INVALID, "%s: %s: %p is not memory the device runtime knows", who, what, p);
    }
    if (attr.type != hipMemoryTypeDevice || attr.device != c->device)
        return fail(c, TRG_ERR_INVALID, "%s: %s: %p is not device memory of device %d", who, what, p, c->device);
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(p)) != hipSuccess || !base) {
        (void)hipGetLastError();
        return fail(c, TRG_ERR_INVALID, "%s: %s: no allocation holds %p", who, what, p);
    }
    const size_t at = (size_t)(static_cast<const char *>(p) - static_cast<const char *>(base));
    if (at > size || size - at < need)
        return fail(c, TRG_ERR_INVALID, "%s: %s: the allocation holds %zu bytes from %p on, the call reads %zu", who, what, at > size ? (size_t)0 : size - at, p, need);
    return TRG_OK;
}

// buffers on the context's device (vouched for by the caller: device_span, or a binding's own): the device path reads them in place, a scene
// of the LDS tier is rebuilt from a download of them
int refit_from_device(trg_ctx *c, const float *pos, const float *nrm, const uint32_t *idx, uint32_t n_verts, uint32_t n_tris) {
    if (c->sc.n_nodes == 0 && n_tris != 0) return refit_device(c, pos, nrm, idx, n_verts, n_tris, true);
    std::vector<float> h_pos((size_t)n_verts * 3), h_nrm(nrm ? (size_t)n_tris * 9 : 0);
    std::vector<uint32_t> h_idx((size_t)n_tris * 3);
    if (n_tris) {
        RF_HIPCHK(c, hipMemcpyAsync(h_pos.data(), pos, h_pos.size() * 4, hipMemcpyDeviceToHost, c->stream));
        RF_HIPCHK(c, hipMemcpyAsync(h_idx.data(), idx, h_idx.size() * 4, hipMemcpyDeviceToHost, c->stream));
        if (nrm) RF_HIPCHK(c, hipMemcpyAsync(h_nrm.data(), nrm, h_nrm.size() * 4, hipMemcpyDeviceToHost, c->stream));
        RF_HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return refit_rebuild(c, h_pos.data(), nrm ? h_nrm.data() : nullptr, h_idx.data(), n_verts, n_tris);
}

// ---- the binding protocol (RefitState::Binding), `who` the entry point named in the texts ----
// the context's binding `unit`, or why there is none to use
template <typename B>
int binding_of(trg_ctx *c, const char *who, B RefitState::*unit, const char *bind_name, B **out) {
    if (!c) return TRG_ERR_INVALID;
    if (!c->refit || !(c->refit->*unit).bound) return fail(c, TRG_ERR_INVALID, "%s: nothing bound (%s first)", who, bind_name);
    B &b = c->refit->*unit;
    if (!b.same_scene(c))
        return fail(c, TRG_ERR_INVALID, "%s: the binding was made for a scene that has been replaced since (bind again)", who);
    RF_HIPCHK(c, hipSetDevice(c->device));
    *out = &b;
    return TRG_OK;
}

template <typename B>
int binding_release(trg_ctx *c, B RefitState::*unit) {
    if (!c) return TRG_ERR_INVALID;
    if (!c->refit) return TRG_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    B &b = c->refit->*unit;
    each_binding_buffer(b, [](Buf &buf) { if (buf.p) (void)hipFree(buf.p); buf.p = nullptr; buf.bytes = 0; });
    b.bound = false;
    b.blob = nullptr;
    return TRG_OK;
}

// what a bind checks of the geometry, in three pieces: every bind reports its first offence in an order of its own
int scene_check(trg_ctx *c, const char *who, uint32_t n_tris, bool null_or_empty) {
    if (!c->scene_loaded || !c->blob) return fail(c, TRG_ERR_INVALID, "%s: no scene loaded", who);
    if (n_tris != c->sc.n_tris) return fail(c, TRG_ERR_INVALID, "%s: %u triangles, the loaded scene has %u", who, n_tris, c->sc.n_tris);
    if (null_or_empty) return fail(c, TRG_ERR_INVALID, "%s: null or empty buffer", who);
    return TRG_OK;
}
int indices_check(trg_ctx *c, const char *who, const uint32_t *indices, uint32_t n_verts, uint32_t n_tris) {
    for (size_t k = 0; k < (size_t)n_tris * 3; ++k)
        if (indices[k] >= n_verts) return fail(c, TRG_ERR_INVALID, "%s: triangle %u has an index out of range (%u vertices)", who, (uint32_t)(k / 3), n_verts);
    return TRG_OK;
}
int finite_check(trg_ctx *c, const char *who, const float *positions3, const float *normals3, uint32_t n_verts, uint32_t n_tris) {
    for (uint32_t v = 0; v < n_verts; ++v)
        if (!(std::isfinite(positions3[(size_t)v * 3]) && std::isfinite(positions3[(size_t)v * 3 + 1]) && std::isfinite(positions3[(size_t)v * 3 + 2])))
            return fail(c, TRG_ERR_INVALID, "%s: vertex %u has a coordinate that is not finite", who, v);
    for (size_t k = 0; normals3 && k < (size_t)n_tris * 9; ++k)
        if (!std::isfinite(normals3[k])) return fail(c, TRG_ERR_INVALID, "%s: triangle %u has a normal that is not finite", who, (uint32_t)(k / 9));
    return TRG_OK;
}
// the skin unit's rules for ids and weights (trg_skin_math.h), for the binds that take them
int skin_check(trg_ctx *c, const char *who, const uint32_t *bone_ids4, const float *weights4, uint32_t n_verts, uint32_t n_bones) {
    uint32_t vert = 0, slot = 0;
    if (skin::ids_check(bone_ids4, n_verts, n_bones, &vert, &slot) != skin::kSkinOk)
        return fail(c, TRG_ERR_INVALID, "%s: vertex %u names bone %u (id %u of its four), there are %u bones", who, vert, bone_ids4[(size_t)vert * 4 + slot], slot, n_bones);
    switch (skin::weights_check(weights4, n_verts, &vert, &slot)) {
    case skin::kSkinWeight: return fail(c, TRG_ERR_INVALID, "%s: vertex %u has a weight (%u of its four) that is negative or not finite", who, vert, slot);
    case skin::kSkinSum: {
        const float *w = weights4 + (size_t)vert * 4;
        return fail(c, TRG_ERR_INVALID, "%s: vertex %u has weights that sum to %.9g, not to 1 within 1e-4 (weights are not normalised here)", who, vert,
                    (double)w[0] + (double)w[1] + (double)w[2] + (double)w[3]);
    }
    default: return TRG_OK;
    }
}
int bones_finite(trg_ctx *c, const char *who, const float *bones12, uint32_t n_bones) {
    for (size_t k = 0; k < (size_t)n_bones * 12; ++k)
        if (!std::isfinite(bones12[k])) return fail(c, TRG_ERR_INVALID, "%s: bone %u is not finite", who, (uint32_t)(k / 12));
    return TRG_OK;
}

// bind, after validation: the unit is unbound from here on; rest geometry and indices to the device, the three copies set to the rest pose
// (enqueued: the unit adds its own uploads, and bind_finish waits)
int copies_bind(trg_ctx *c, RefitState::Binding &g, const float *positions3, const float *normals3, const uint32_t *indices, uint32_t n_verts, uint32_t n_tris) {
    RF_HIPCHK(c, hipSetDevice(c->device));
    g.bound = false;
    const size_t pos_bytes = (size_t)n_verts * 12, idx_bytes = (size_t)n_tris * 12, nrm_bytes = (size_t)n_tris * 36;
    int rc = TRG_OK;
    if ((rc = grow(c, g.rest_pos, pos_bytes, "rest positions")) || (rc = grow(c, g.idx, idx_bytes, "bound indices")) ||
        (normals3 && (rc = grow(c, g.rest_nrm, nrm_bytes, "rest normals"))))
        return rc;
    for (int k = 0; k < 3; ++k)
        if ((rc = grow(c, g.posed[k], pos_bytes, "posed positions")) || (normals3 && (rc = grow(c, g.posed_nrm[k], nrm_bytes, "posed normals")))) return rc;
    RF_HIPCHK(c, hipMemcpyAsync(g.rest_pos.p, positions3, pos_bytes, hipMemcpyHostToDevice, c->stream));
    RF_HIPCHK(c, hipMemcpyAsync(g.idx.p, indices, idx_bytes, hipMemcpyHostToDevice, c->stream));
    if (normals3) RF_HIPCHK(c, hipMemcpyAsync(g.rest_nrm.p, normals3, nrm_bytes, hipMemcpyHostToDevice, c->stream));
    for (int k = 0; k < 3; ++k) {
        RF_HIPCHK(c, hipMemcpyAsync(g.posed[k].p, g.rest_pos.p, pos_bytes, hipMemcpyDeviceToDevice, c->stream));
        if (normals3) RF_HIPCHK(c, hipMemcpyAsync(g.posed_nrm[k].p, g.rest_nrm.p, nrm_bytes, hipMemcpyDeviceToDevice, c->stream));
    }
    g.n_verts = n_verts;
    g.cur = 0; g.prev = 1;
    g.has_nrm = normals3 != nullptr;
    return TRG_OK;
}
int bind_finish(trg_ctx *c, RefitState::Binding &g, uint32_t n_tris) {
    RF_HIPCHK(c, hipStreamSynchronize(c->stream));   // (the caller's arrays, and the bind's own, are free again on return)
    g.n_tris = n_tris;
    g.remember_scene(c);
    g.bound = true;
    return TRG_OK;
}
// apply, after the unit's kernel wrote the spare copy: the loaded scene from it, and only then is it the current pose
int apply_finish(trg_ctx *c, RefitState::Binding &g) {
    const uint32_t spare = g.spare();
    if (int rc = refit_from_device(c, g.pos_of(spare), g.nrm_of(spare), g.idx.as<uint32_t>(), g.n_verts, g.n_tris)) return rc;   // (current and previous are untouched)
    g.rotate();
    g.remember_scene(c);   // (the small-scene path gives the same scene new memory, and builds it)
    return TRG_OK;
}
template <typename B>
int binding_read(trg_ctx *c, const char *who, B RefitState::*unit, const char *bind_name, float *positions3_host, float *normals3_host) {
    B *g = nullptr;
    if (int rc = binding_of(c, who, unit, bind_name, &g)) return rc;
    if (!positions3_host) return fail(c, TRG_ERR_INVALID, "%s: null buffer", who);
    if (normals3_host && !g->has_nrm) return fail(c, TRG_ERR_INVALID, "%s: bound without normals", who);
    RF_HIPCHK(c, hipMemcpyAsync(positions3_host, g->posed[g->cur].p, (size_t)g->n_verts * 12, hipMemcpyDeviceToHost, c->stream));
    if (normals3_host) RF_HIPCHK(c, hipMemcpyAsync(normals3_host, g->posed_nrm[g->cur].p, (size_t)g->n_tris * 36, hipMemcpyDeviceToHost, c->stream));
    RF_HIPCHK(c, hipStreamSynchronize(c->stream));
    return TRG_OK;
}
template <typename B>
int binding_buffers(trg_ctx *c, const char *who, B RefitState::*unit, const char *bind_name, void **pos_dev, void **nrm_dev, void **idx_dev, void **prev_pos_dev,
                    void **prev_nrm_dev) {
    B *g = nullptr;
    if (int rc = binding_of(c, who, unit, bind_name, &g)) return rc;
    if (pos_dev) *pos_dev = g->posed[g->cur].p;
    if (nrm_dev) *nrm_dev = g->nrm_of(g->cur);
    if (idx_dev) *idx_dev = g->idx.p;
    if (prev_pos_dev) *prev_pos_dev = g->posed[g->prev].p;
    if (prev_nrm_dev) *prev_nrm_dev = g->nrm_of(g->prev);
    return TRG_OK;
}

// a call on every context of a group in turn, after the group's wait; the first refusal ends it
template <typename Call>
int group_each(trg_group *g, Call call) {
    if (!g) return TRG_ERR_INVALID;
    const int n = trg_group_size(g);
    if (n <= 0) return TRG_ERR_INVALID;
    if (int rc = trg_group_sync(g)) return rc;
    for (int r = 0; r < n; ++r) {
        trg_ctx *c = trg_group_ctx(g, r);
        if (!c) return TRG_ERR_INVALID;
        if (int rc = call(c)) return rc;
    }
    return TRG_OK;
}

template <bool kBones, bool kNormalDeltas>
int morph_launch(trg_ctx *c, RefitState::Morph &m, uint32_t blocks, float *pos_out, float *nrm_out) {
    RF_LAUNCH(c, (rf_morph_kernel<kBones, kNormalDeltas>), dim3(blocks), m.rest_pos.as<float>(), m.vfirst.as<uint32_t>(), m.pos_recs.as<float4>(),
              m.nrm_recs.as<float4>(), m.tw.as<float>(), m.n_verts, m.rest_nrm.as<float>(), m.idx.as<uint32_t>(), m.n_tris * 3u, m.ids.as<uint4>(),
              m.weights.as<float4>(), m.bones.as<float4>(), pos_out, nrm_out);
    return TRG_OK;
}

// ---- the second half of an apply of the skin and the morph unit: the binding's `bones` buffer (and the morph's weights) hold this call's values
//      -- uploaded by trg_skin_apply / trg_morph_apply, copied device to device by include/trg_rig.h's calls --; launch, refit, rotate ----
int skin_run(trg_ctx *c, RefitState::Skin &p) {
    RF_LAUNCH(c, rf_skin_kernel, dim3(p.blocks(p.has_nrm)), p.rest_pos.as<float>(), p.ids.as<uint4>(), p.weights.as<float4>(), p.n_verts, p.rest_nrm.as<float>(),
              p.idx.as<uint32_t>(), p.n_tris * 3u, p.bones.as<float4>(), p.pos_of(p.spare()), p.nrm_of(p.spare()));
    return apply_finish(c, p);
}
int morph_run(trg_ctx *c, RefitState::Morph &m) {
    float *pos_out = m.pos_of(m.spare()), *nrm_out = m.nrm_of(m.spare());
    // no corner can change without normal deltas and without bones: that copy holds the rest normals since bind, and the range is left out
    const uint32_t blocks = m.blocks(m.has_nrm && (m.has_dnrm || m.has_bones));
    int rc = TRG_OK;
    if (m.has_bones) rc = m.has_dnrm ? morph_launch<true, true>(c, m, blocks, pos_out, nrm_out) : morph_launch<true, false>(c, m, blocks, pos_out, nrm_out);
    else rc = m.has_dnrm ? morph_launch<false, true>(c, m, blocks, pos_out, nrm_out) : morph_launch<false, false>(c, m, blocks, pos_out, nrm_out);
    if (rc) return rc;
    return apply_finish(c, m);
}
// what trg_morph_apply checks of its weights
int morph_weights(trg_ctx *c, const char *who, const RefitState::Morph &m, const float *target_weights) {
    if (!target_weights) return fail(c, TRG_ERR_INVALID, "%s: null target weights", who);
    for (uint32_t k = 0; k < m.n_targets; ++k)
        if (!std::isfinite(target_weights[k])) return fail(c, TRG_ERR_INVALID, "%s: the weight of target %u is not finite", who, k);
    return TRG_OK;
}

// ---- include/trg_rig.h ----
// the context's rig, or why there is none to use
int rig_of(trg_ctx *c, const char *who, RefitState::Rig **out) {
    if (!c) return TRG_ERR_INVALID;
#if TRG_WIDE8
    return fail(c, TRG_ERR_INVALID, "%s: an 8-wide experiments build has no rigs", who);
#endif
    if (!c->refit || !c->refit->rig.bound) return fail(c, TRG_ERR_INVALID, "%s: no rig bound (trg_rig_bind first)", who);
    RF_HIPCHK(c, hipSetDevice(c->device));
    *out = &c->refit->rig;
    return TRG_OK;
}
int clocks_finite(trg_ctx *c, const char *who, const RefitState::Rig &r, const float *clocks) {
    if (!clocks) return fail(c, TRG_ERR_INVALID, "%s: null clocks", who);
    for (uint32_t k = 0; k < r.n_clocks; ++k)
        if (!std::isfinite(clocks[k])) return fail(c, TRG_ERR_INVALID, "%s: clock %u is not finite", who, k);
    return TRG_OK;
}
template <bool kRoot>
int rig_level(trg_ctx *c, RefitState::Rig &r, uint32_t first, uint32_t count) {
    if (r.has_inv)
        RF_LAUNCH(c, (rf_rig_level_kernel<kRoot, true>), blocks_for(count), r.order.as<uint32_t>(), first, count, r.parent.as<uint32_t>(), r.kfirst.as<uint32_t>(),
                  r.keys.as<float4>(), r.clock_of.as<uint32_t>(), r.clocks.as<float>(), r.inv_bind.as<float4>(), r.world.as<float4>(), r.bones.as<float4>());
    else
        RF_LAUNCH(c, (rf_rig_level_kernel<kRoot, false>), blocks_for(count), r.order.as<uint32_t>(), first, count, r.parent.as<uint32_t>(), r.kfirst.as<uint32_t>(),
                  r.keys.as<float4>(), r.clock_of.as<uint32_t>(), r.clocks.as<float>(), nullptr, r.world.as<float4>(), r.bones.as<float4>());
    return TRG_OK;
}
// the clocks (checked by the caller) to the device and one launch per level, enqueued; nobody waits
int rig_evaluate(trg_ctx *c, RefitState::Rig &r, const float *clocks) {
    RF_HIPCHK(c, hipMemcpyAsync(r.clocks.p, clocks, (size_t)r.n_clocks * 4, hipMemcpyHostToDevice, c->stream));
    for (uint32_t l = 0; l < r.n_levels; ++l) {
        const uint32_t first = r.level_first[l], count = r.level_first[l + 1] - first;
        if (int rc = l == 0 ? rig_level<true>(c, r, first, count) : rig_level<false>(c, r, first, count)) return rc;
    }
    r.evaluated = true;
    return TRG_OK;
}
// the rig and the binding of an apply from the rig's bones: both bound, the binding's scene still loaded, as many joints as bones
template <typename B>
int rig_target(trg_ctx *c, const char *who, B RefitState::*unit, const char *bind_name, RefitState::Rig **r, B **b) {
    int rc = TRG_OK;
    if ((rc = rig_of(c, who, r)) || (rc = binding_of(c, who, unit, bind_name, b))) return rc;
    return TRG_OK;
}
int rig_counts(trg_ctx *c, const char *who, const RefitState::Rig &r, uint32_t n_bones) {
    if (r.n_joints != n_bones) return fail(c, TRG_ERR_INVALID, "%s: the rig has %u joints, the binding %u bones (joint j is bone j)", who, r.n_joints, n_bones);
    return TRG_OK;
}
int morph_has_bones(trg_ctx *c, const char *who, const RefitState::Morph &m) {
    if (!m.has_bones) return fail(c, TRG_ERR_INVALID, "%s: the morph binding has no bones (trg_morph_bind with bone ids and weights)", who);
    return TRG_OK;
}
// the 8-wide refusal and the binding of the _device forms, which need no rig
template <typename B>
int device_target(trg_ctx *c, const char *who, B RefitState::*unit, const char *bind_name, B **b) {
    if (!c) return TRG_ERR_INVALID;
#if TRG_WIDE8
    return fail(c, TRG_ERR_INVALID, "%s: an 8-wide experiments build has no rigs", who);
#endif
    return binding_of(c, who, unit, bind_name, b);
}

}  // namespace

void trg::refit_state_free(trg_ctx *c) {
    if (!c->refit) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    each_buffer(*c->refit, [](Buf &b) { if (b.p) (void)hipFree(b.p); });
    delete c->refit;
    c->refit = nullptr;
}

extern "C" {

int trg_refit_scene(trg_ctx *c, const float *positions3, const float *normals3, const uint32_t *indices, uint32_t n_verts, uint32_t n_tris) {
    if (!c) return TRG_ERR_INVALID;
    if (int rc = refit_arguments(c, positions3, indices, n_verts, n_tris)) return rc;
    if (c->sc.n_nodes != 0 || n_tris == 0) return refit_rebuild(c, positions3, normals3, indices, n_verts, n_tris);
    return refit_device(c, positions3, normals3, indices, n_verts, n_tris, false);
}

int trg_refit_scene_device(trg_ctx *c, const void *positions3_dev, const void *normals3_dev, const void *indices_dev, uint32_t n_verts, uint32_t n_tris) {
    if (!c) return TRG_ERR_INVALID;
    if (int rc = refit_arguments(c, positions3_dev, indices_dev, n_verts, n_tris)) return rc;
    if (n_tris) {
        int rc = TRG_OK;
        if ((rc = device_span(c, positions3_dev, (size_t)n_verts * 12, "positions")) || (rc = device_span(c, indices_dev, (size_t)n_tris * 12, "indices")) ||
            (normals3_dev && (rc = device_span(c, normals3_dev, (size_t)n_tris * 36, "normals"))))
            return rc;
    }
    return refit_from_device(c, static_cast<const float *>(positions3_dev), static_cast<const float *>(normals3_dev), static_cast<const uint32_t *>(indices_dev), n_verts, n_tris);
}

int trg_pose_bind(trg_ctx *c, const float *positions3, const float *normals3, const uint32_t *indices, uint32_t n_verts, uint32_t n_tris,
                  const uint32_t *object_first_tri, uint32_t n_objects) {
    if (!c) return TRG_ERR_INVALID;
#if TRG_WIDE8
    return fail(c, TRG_ERR_INVALID, "trg_pose_bind: an 8-wide experiments build has no poses");
#endif
    const char *who = "trg_pose_bind";
    if (int rc = scene_check(c, who, n_tris, !positions3 || !indices || !object_first_tri || n_verts == 0 || n_tris == 0 || n_objects == 0)) return rc;
    uint32_t obj = 0, tri = 0, vert = 0;
    switch (pose::table_check(object_first_tri, n_objects, n_tris, &obj)) {
    case pose::kTableFirst: return fail(c, TRG_ERR_INVALID, "trg_pose_bind: object 0 begins at triangle %u, not at 0", object_first_tri[0]);
    case pose::kTableOrder: return fail(c, TRG_ERR_INVALID, "trg_pose_bind: object %u begins at triangle %u and ends at %u: the table is not strictly ascending", obj, object_first_tri[obj], object_first_tri[obj + 1]);
    case pose::kTableEnd: return fail(c, TRG_ERR_INVALID, "trg_pose_bind: object %u ends at triangle %u, the scene has %u", obj, object_first_tri[n_objects], n_tris);
    default: break;
    }
    std::vector<uint32_t> tri_obj(n_tris), vtx_obj(n_verts);
    pose::triangle_objects(object_first_tri, n_objects, tri_obj.data());
    switch (pose::vertex_objects(indices, n_verts, n_tris, tri_obj.data(), vtx_obj.data(), &tri, &vert)) {   // (which finds an index out of range)
    case pose::kVertsIndex: return fail(c, TRG_ERR_INVALID, "trg_pose_bind: triangle %u has an index out of range (%u vertices)", tri, n_verts);
    case pose::kVertsShared: return fail(c, TRG_ERR_INVALID, "trg_pose_bind: vertex %u is named by triangle %u of object %u and by object %u: a vertex belongs to one object", vert, tri, tri_obj[tri], vtx_obj[vert]);
    default: break;
    }
    if (int rc = finite_check(c, who, positions3, normals3, n_verts, n_tris)) return rc;

    RefitState::Pose &p = state_of(c).pose;
    int rc = TRG_OK;
    if ((rc = copies_bind(c, p, positions3, normals3, indices, n_verts, n_tris)) || (rc = grow(c, p.vtx_obj, (size_t)n_verts * 4, "vertex map")) ||
        (rc = grow(c, p.tri_obj, (size_t)n_tris * 4, "triangle map")) || (rc = grow(c, p.xforms, (size_t)n_objects * 48, "transforms")))
        return rc;
    RF_HIPCHK(c, hipMemcpyAsync(p.vtx_obj.p, vtx_obj.data(), (size_t)n_verts * 4, hipMemcpyHostToDevice, c->stream));
    RF_HIPCHK(c, hipMemcpyAsync(p.tri_obj.p, tri_obj.data(), (size_t)n_tris * 4, hipMemcpyHostToDevice, c->stream));
    p.n_objects = n_objects;
    return bind_finish(c, p, n_tris);
}

int trg_pose_apply(trg_ctx *c, const float *xforms12) {
    RefitState::Pose *pp = nullptr;
    if (int rc = binding_of(c, "trg_pose_apply", &RefitState::pose, "trg_pose_bind", &pp)) return rc;
    RefitState::Pose &p = *pp;
    if (!xforms12) return fail(c, TRG_ERR_INVALID, "trg_pose_apply: null transforms");
    for (size_t k = 0; k < (size_t)p.n_objects * 12; ++k)
        if (!std::isfinite(xforms12[k])) return fail(c, TRG_ERR_INVALID, "trg_pose_apply: the transform of object %u is not finite", (uint32_t)(k / 12));
    RF_HIPCHK(c, hipMemcpyAsync(p.xforms.p, xforms12, (size_t)p.n_objects * 48, hipMemcpyHostToDevice, c->stream));
    RF_LAUNCH(c, rf_pose_kernel, dim3(p.blocks(p.has_nrm)), p.rest_pos.as<float>(), p.vtx_obj.as<uint32_t>(), p.n_verts, p.rest_nrm.as<float>(), p.tri_obj.as<uint32_t>(),
              p.n_tris * 3u, p.xforms.as<float>(), p.pos_of(p.spare()), p.nrm_of(p.spare()));
    return apply_finish(c, p);
}

int trg_pose_read(trg_ctx *c, float *positions3_host, float *normals3_host) {
    return binding_read(c, "trg_pose_read", &RefitState::pose, "trg_pose_bind", positions3_host, normals3_host);
}

int trg_pose_buffers(trg_ctx *c, void **pos_dev, void **nrm_dev, void **idx_dev, void **prev_pos_dev, void **prev_nrm_dev) {
    return binding_buffers(c, "trg_pose_buffers", &RefitState::pose, "trg_pose_bind", pos_dev, nrm_dev, idx_dev, prev_pos_dev, prev_nrm_dev);
}

int trg_pose_release(trg_ctx *c) { return binding_release(c, &RefitState::pose); }

int trg_group_pose_bind(trg_group *g, const float *positions3, const float *normals3, const uint32_t *indices, uint32_t n_verts, uint32_t n_tris,
                        const uint32_t *object_first_tri, uint32_t n_objects) {
    return group_each(g, [&](trg_ctx *c) { return trg_pose_bind(c, positions3, normals3, indices, n_verts, n_tris, object_first_tri, n_objects); });
}

int trg_group_pose_apply(trg_group *g, const float *xforms12) {
    return group_each(g, [&](trg_ctx *c) { return trg_pose_apply(c, xforms12); });
}

int trg_skin_bind(trg_ctx *c, const float *positions3, const float *normals3, const uint32_t *indices, uint32_t n_verts, uint32_t n_tris,
                  const uint32_t *bone_ids4, const float *weights4, uint32_t n_bones) {
    if (!c) return TRG_ERR_INVALID;
#if TRG_WIDE8
    return fail(c, TRG_ERR_INVALID, "trg_skin_bind: an 8-wide experiments build has no skinning");
#endif
    const char *who = "trg_skin_bind";
    int rc = TRG_OK;
    if ((rc = scene_check(c, who, n_tris, !positions3 || !indices || !bone_ids4 || !weights4 || n_verts == 0 || n_tris == 0 || n_bones == 0)) ||
        (rc = indices_check(c, who, indices, n_verts, n_tris)) || (rc = skin_check(c, who, bone_ids4, weights4, n_verts, n_bones)) ||
        (rc = finite_check(c, who, positions3, normals3, n_verts, n_tris)))
        return rc;

    RefitState::Skin &p = state_of(c).skin;
    const size_t rec_bytes = (size_t)n_verts * 16;
    if ((rc = copies_bind(c, p, positions3, normals3, indices, n_verts, n_tris)) || (rc = grow(c, p.ids, rec_bytes, "bone ids")) ||
        (rc = grow(c, p.weights, rec_bytes, "bone weights")) || (rc = grow(c, p.bones, (size_t)n_bones * 48, "bones")))
        return rc;
    RF_HIPCHK(c, hipMemcpyAsync(p.ids.p, bone_ids4, rec_bytes, hipMemcpyHostToDevice, c->stream));
    RF_HIPCHK(c, hipMemcpyAsync(p.weights.p, weights4, rec_bytes, hipMemcpyHostToDevice, c->stream));
    p.n_bones = n_bones;
    return bind_finish(c, p, n_tris);
}

int trg_skin_apply(trg_ctx *c, const float *bones12) {
    RefitState::Skin *pp = nullptr;
    if (int rc = binding_of(c, "trg_skin_apply", &RefitState::skin, "trg_skin_bind", &pp)) return rc;
    RefitState::Skin &p = *pp;
    if (!bones12) return fail(c, TRG_ERR_INVALID, "trg_skin_apply: null bones");
    if (int rc = bones_finite(c, "trg_skin_apply", bones12, p.n_bones)) return rc;
    RF_HIPCHK(c, hipMemcpyAsync(p.bones.p, bones12, (size_t)p.n_bones * 48, hipMemcpyHostToDevice, c->stream));
    return skin_run(c, p);
}

int trg_skin_read(trg_ctx *c, float *positions3_host, float *normals3_host) {
    return binding_read(c, "trg_skin_read", &RefitState::skin, "trg_skin_bind", positions3_host, normals3_host);
}

int trg_skin_buffers(trg_ctx *c, void **pos_dev, void **nrm_dev, void **idx_dev, void **prev_pos_dev, void **prev_nrm_dev) {
    return binding_buffers(c, "trg_skin_buffers", &RefitState::skin, "trg_skin_bind", pos_dev, nrm_dev, idx_dev, prev_pos_dev, prev_nrm_dev);
}

int trg_skin_release(trg_ctx *c) { return binding_release(c, &RefitState::skin); }

int trg_group_skin_bind(trg_group *g, const float *positions3, const float *normals3, const uint32_t *indices, uint32_t n_verts, uint32_t n_tris,
                        const uint32_t *bone_ids4, const float *weights4, uint32_t n_bones) {
    return group_each(g, [&](trg_ctx *c) { return trg_skin_bind(c, positions3, normals3, indices, n_verts, n_tris, bone_ids4, weights4, n_bones); });
}

int trg_group_skin_apply(trg_group *g, const float *bones12) {
    return group_each(g, [&](trg_ctx *c) { return trg_skin_apply(c, bones12); });
}

int trg_morph_bind(trg_ctx *c, const float *positions3, const float *normals3, const uint32_t *indices, uint32_t n_verts, uint32_t n_tris, uint32_t n_targets,
                   const uint32_t *target_first, uint32_t n_entries, const uint32_t *entry_vertex, const float *entry_dpos3, const float *entry_dnrm3, const uint32_t *bone_ids4,
                   const float *bone_weights4, uint32_t n_bones) {
    if (!c) return TRG_ERR_INVALID;
#if TRG_WIDE8
    return fail(c, TRG_ERR_INVALID, "trg_morph_bind: an 8-wide experiments build has no blend shapes");
#endif
    const char *who = "trg_morph_bind";
    int rc = TRG_OK;
    if ((rc = scene_check(c, who, n_tris, !positions3 || !indices || n_verts == 0 || n_tris == 0)) || (rc = indices_check(c, who, indices, n_verts, n_tris)) ||
        (rc = finite_check(c, who, positions3, normals3, n_verts, n_tris)))
        return rc;
    if (n_targets == 0 || !target_first) return fail(c, TRG_ERR_INVALID, "trg_morph_bind: no targets (at least one is needed, and its table)");
    uint32_t target = 0, entry = 0;
    switch (morph::targets_check(target_first, n_targets, n_entries, &target)) {
    case morph::kTargetsFirst: return fail(c, TRG_ERR_INVALID, "trg_morph_bind: target 0 begins at entry %u, not at 0", target_first[0]);
    case morph::kTargetsOrder: return fail(c, TRG_ERR_INVALID, "trg_morph_bind: target %u begins at entry %u and ends at %u: the table is descending", target, target_first[target], target_first[target + 1]);
    case morph::kTargetsEnd: return fail(c, TRG_ERR_INVALID, "trg_morph_bind: target %u ends at entry %u, there are %u entries", target, target_first[n_targets], n_entries);
    default: break;
    }
    if (n_entries && (!entry_vertex || !entry_dpos3)) return fail(c, TRG_ERR_INVALID, "trg_morph_bind: %u entries, and a null entry list", n_entries);
    switch (morph::entries_check(target_first, n_targets, entry_vertex, n_verts, entry_dpos3, entry_dnrm3, &target, &entry)) {
    case morph::kEntriesVertex: return fail(c, TRG_ERR_INVALID, "trg_morph_bind: entry %u of target %u names vertex %u, there are %u vertices", entry, target, entry_vertex[entry], n_verts);
    case morph::kEntriesOrder: return fail(c, TRG_ERR_INVALID, "trg_morph_bind: entry %u of target %u names vertex %u after vertex %u: a target's vertices are strictly ascending", entry, target, entry_vertex[entry], entry_vertex[entry - 1]);
    case morph::kEntriesDelta: return fail(c, TRG_ERR_INVALID, "trg_morph_bind: entry %u of target %u has a position delta that is not finite", entry, target);
    case morph::kEntriesNormalDelta: return fail(c, TRG_ERR_INVALID, "trg_morph_bind: entry %u of target %u has a normal delta that is not finite", entry, target);
    default: break;
    }
    if (entry_dnrm3 && !normals3) return fail(c, TRG_ERR_INVALID, "trg_morph_bind: normal deltas given without normals");
    const bool has_bones = bone_ids4 && bone_weights4 && n_bones;
    if (!has_bones && (bone_ids4 || bone_weights4 || n_bones))
        return fail(c, TRG_ERR_INVALID, "trg_morph_bind: bone ids, bone weights and the number of bones are given all three or none (ids %s, weights %s, %u bones)",
                    bone_ids4 ? "given" : "null", bone_weights4 ? "given" : "null", n_bones);
    if (has_bones && (rc = skin_check(c, who, bone_ids4, bone_weights4, n_verts, n_bones))) return rc;
    // by-target lists -> per-vertex records.  (At least one record is allocated: a binding whose targets are all empty is legal.)
    std::vector<uint32_t> vfirst((size_t)n_verts + 1), cursor(n_verts);
    std::vector<morph::Rec> pos_recs(n_entries), nrm_recs(entry_dnrm3 ? n_entries : 0);
    morph::transpose(target_first, n_targets, entry_vertex, entry_dpos3, entry_dnrm3, n_verts, vfirst.data(), cursor.data(), pos_recs.data(), entry_dnrm3 ? nrm_recs.data() : nullptr);

    RefitState::Morph &m = state_of(c).morph;
    const size_t rec_bytes = (size_t)n_entries * sizeof(morph::Rec), skin_bytes = (size_t)n_verts * 16;
    if ((rc = copies_bind(c, m, positions3, normals3, indices, n_verts, n_tris)) || (rc = grow(c, m.vfirst, vfirst.size() * 4, "entry ranges")) ||
        (rc = grow(c, m.pos_recs, rec_bytes + 16, "position deltas")) || (entry_dnrm3 && (rc = grow(c, m.nrm_recs, rec_bytes + 16, "normal deltas"))) ||
        (rc = grow(c, m.tw, (size_t)n_targets * 4, "target weights")) ||
        (has_bones && ((rc = grow(c, m.ids, skin_bytes, "bone ids")) || (rc = grow(c, m.weights, skin_bytes, "bone weights")) || (rc = grow(c, m.bones, (size_t)n_bones * 48, "bones")))))
        return rc;
    RF_HIPCHK(c, hipMemcpyAsync(m.vfirst.p, vfirst.data(), vfirst.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (rec_bytes) RF_HIPCHK(c, hipMemcpyAsync(m.pos_recs.p, pos_recs.data(), rec_bytes, hipMemcpyHostToDevice, c->stream));
    if (rec_bytes && entry_dnrm3) RF_HIPCHK(c, hipMemcpyAsync(m.nrm_recs.p, nrm_recs.data(), rec_bytes, hipMemcpyHostToDevice, c->stream));
    if (has_bones) {
        RF_HIPCHK(c, hipMemcpyAsync(m.ids.p, bone_ids4, skin_bytes, hipMemcpyHostToDevice, c->stream));
        RF_HIPCHK(c, hipMemcpyAsync(m.weights.p, bone_weights4, skin_bytes, hipMemcpyHostToDevice, c->stream));
    }
    m.n_targets = n_targets; m.n_bones = has_bones ? n_bones : 0u;
    m.has_dnrm = entry_dnrm3 != nullptr;
    m.has_bones = has_bones;
    return bind_finish(c, m, n_tris);
}

int trg_morph_apply(trg_ctx *c, const float *target_weights, const float *bones12) {
    RefitState::Morph *mp = nullptr;
    if (int rc = binding_of(c, "trg_morph_apply", &RefitState::morph, "trg_morph_bind", &mp)) return rc;
    RefitState::Morph &m = *mp;
    if (int rc = morph_weights(c, "trg_morph_apply", m, target_weights)) return rc;
    if (m.has_bones && !bones12) return fail(c, TRG_ERR_INVALID, "trg_morph_apply: null bones, the binding has %u", m.n_bones);
    if (!m.has_bones && bones12) return fail(c, TRG_ERR_INVALID, "trg_morph_apply: bones given, the binding has none");
    if (int rc = bones_finite(c, "trg_morph_apply", bones12, m.n_bones)) return rc;
    RF_HIPCHK(c, hipMemcpyAsync(m.tw.p, target_weights, (size_t)m.n_targets * 4, hipMemcpyHostToDevice, c->stream));
    if (m.has_bones) RF_HIPCHK(c, hipMemcpyAsync(m.bones.p, bones12, (size_t)m.n_bones * 48, hipMemcpyHostToDevice, c->stream));
    return morph_run(c, m);
}

int trg_morph_read(trg_ctx *c, float *positions3_host, float *normals3_host) {
    return binding_read(c, "trg_morph_read", &RefitState::morph, "trg_morph_bind", positions3_host, normals3_host);
}

int trg_morph_buffers(trg_ctx *c, void **pos_dev, void **nrm_dev, void **idx_dev, void **prev_pos_dev, void **prev_nrm_dev) {
    return binding_buffers(c, "trg_morph_buffers", &RefitState::morph, "trg_morph_bind", pos_dev, nrm_dev, idx_dev, prev_pos_dev, prev_nrm_dev);
}

int trg_morph_release(trg_ctx *c) { return binding_release(c, &RefitState::morph); }

int trg_group_morph_bind(trg_group *g, const float *positions3, const float *normals3, const uint32_t *indices, uint32_t n_verts, uint32_t n_tris, uint32_t n_targets,
                         const uint32_t *target_first, uint32_t n_entries, const uint32_t *entry_vertex, const float *entry_dpos3, const float *entry_dnrm3, const uint32_t *bone_ids4,
                         const float *bone_weights4, uint32_t n_bones) {
    return group_each(g, [&](trg_ctx *c) {
        return trg_morph_bind(c, positions3, normals3, indices, n_verts, n_tris, n_targets, target_first, n_entries, entry_vertex, entry_dpos3, entry_dnrm3, bone_ids4, bone_weights4, n_bones);
    });
}

int trg_group_morph_apply(trg_group *g, const float *target_weights, const float *bones12) {
    return group_each(g, [&](trg_ctx *c) { return trg_morph_apply(c, target_weights, bones12); });
}

int trg_rig_bind(trg_ctx *c, const uint32_t *parent, uint32_t n_joints, const uint32_t *key_first, const float *keys12, uint32_t n_keys, const uint32_t *clock_of,
                 uint32_t n_clocks, const float *inv_bind12) {
    if (!c) return TRG_ERR_INVALID;
#if TRG_WIDE8
    return fail(c, TRG_ERR_INVALID, "trg_rig_bind: an 8-wide experiments build has no rigs");
#endif
    uint32_t j = 0, k = 0;
    const bool counts = n_joints != 0 && n_keys != 0 && n_clocks != 0;
    if (counts && (!parent || !key_first || !keys12 || !clock_of)) return fail(c, TRG_ERR_INVALID, "trg_rig_bind: null table");
    const int what = !counts ? (int)rig::kRigCounts : rig::check(parent, n_joints, key_first, keys12, n_keys, clock_of, n_clocks, inv_bind12, &j, &k);
    switch (what) {
    case rig::kRigCounts: return fail(c, TRG_ERR_INVALID, "trg_rig_bind: %u joints, %u keys, %u clocks: none of them may be zero", n_joints, n_keys, n_clocks);
    case rig::kRigParent: return fail(c, TRG_ERR_INVALID, "trg_rig_bind: joint %u names parent %u: a parent comes before its children (or is 0xFFFFFFFF, a root)", j, parent[j]);
    case rig::kRigTableFirst: return fail(c, TRG_ERR_INVALID, "trg_rig_bind: joint 0 begins at key %u, not at 0", key_first[0]);
    case rig::kRigTableOrder: return fail(c, TRG_ERR_INVALID, "trg_rig_bind: joint %u begins at key %u and ends at %u: every joint has a key and the table is strictly ascending", j, key_first[j], key_first[j + 1]);
    case rig::kRigTableEnd: return fail(c, TRG_ERR_INVALID, "trg_rig_bind: joint %u ends at key %u, there are %u keys", j, key_first[n_joints], n_keys);
    case rig::kRigTime: return fail(c, TRG_ERR_INVALID, "trg_rig_bind: key %u of joint %u has a time that is not finite or not after the key before it", k, j);
    case rig::kRigTS: return fail(c, TRG_ERR_INVALID, "trg_rig_bind: key %u of joint %u has a translation or a scale that is not finite", k, j);
    case rig::kRigQuat: return fail(c, TRG_ERR_INVALID, "trg_rig_bind: key %u of joint %u has a rotation that is not finite or not of unit length within 1e-3", k, j);
    case rig::kRigClock: return fail(c, TRG_ERR_INVALID, "trg_rig_bind: joint %u names clock %u, there are %u clocks", j, clock_of[j], n_clocks);
    case rig::kRigInvBind: return fail(c, TRG_ERR_INVALID, "trg_rig_bind: the inverse bind matrix of joint %u is not finite", j);
    default: break;
    }
    std::vector<uint32_t> depth(n_joints), order(n_joints);
    uint32_t level_first[rig::kMaxLevels + 1], n_levels = 0;
    if (rig::levels(parent, n_joints, depth.data(), order.data(), level_first, &n_levels, &j) != rig::kRigOk)
        return fail(c, TRG_ERR_RANGE, "trg_rig_bind: joint %u lies deeper than %u levels (TRG_RIG_MAX_LEVELS)", j, (uint32_t)TRG_RIG_MAX_LEVELS);

    RF_HIPCHK(c, hipSetDevice(c->device));
    RefitState::Rig &r = state_of(c).rig;
    r.bound = false; r.evaluated = false;
    const size_t words = (size_t)n_joints * 4, mats = (size_t)n_joints * 48;
    int rc = TRG_OK;
    if ((rc = grow(c, r.parent, words, "rig parents")) || (rc = grow(c, r.order, words, "rig order")) || (rc = grow(c, r.keys, (size_t)n_keys * 48, "rig keys")) ||
        (rc = grow(c, r.kfirst, words + 4, "rig key ranges")) || (rc = grow(c, r.clock_of, words, "rig clock ids")) || (inv_bind12 && (rc = grow(c, r.inv_bind, mats, "inverse binds"))) ||
        (rc = grow(c, r.clocks, (size_t)n_clocks * 4, "rig clocks")) || (rc = grow(c, r.world, mats, "world matrices")) || (rc = grow(c, r.bones, mats, "rig bones")))
        return rc;
    RF_HIPCHK(c, hipMemcpyAsync(r.parent.p, parent, words, hipMemcpyHostToDevice, c->stream));
    RF_HIPCHK(c, hipMemcpyAsync(r.order.p, order.data(), words, hipMemcpyHostToDevice, c->stream));
    RF_HIPCHK(c, hipMemcpyAsync(r.keys.p, keys12, (size_t)n_keys * 48, hipMemcpyHostToDevice, c->stream));
    RF_HIPCHK(c, hipMemcpyAsync(r.kfirst.p, key_first, words + 4, hipMemcpyHostToDevice, c->stream));
    RF_HIPCHK(c, hipMemcpyAsync(r.clock_of.p, clock_of, words, hipMemcpyHostToDevice, c->stream));
    if (inv_bind12) RF_HIPCHK(c, hipMemcpyAsync(r.inv_bind.p, inv_bind12, mats, hipMemcpyHostToDevice, c->stream));
    RF_HIPCHK(c, hipStreamSynchronize(c->stream));   // (the caller's arrays, and the bind's own, are free again on return)
    r.n_joints = n_joints; r.n_keys = n_keys; r.n_clocks = n_clocks; r.n_levels = n_levels;
    for (uint32_t l = 0; l <= rig::kMaxLevels; ++l) r.level_first[l] = level_first[l];
    r.has_inv = inv_bind12 != nullptr;
    r.bound = true;
    return TRG_OK;
}

int trg_rig_evaluate(trg_ctx *c, const float *clocks) {
    RefitState::Rig *r = nullptr;
    int rc = TRG_OK;
    if ((rc = rig_of(c, "trg_rig_evaluate", &r)) || (rc = clocks_finite(c, "trg_rig_evaluate", *r, clocks))) return rc;
    return rig_evaluate(c, *r, clocks);
}

int trg_rig_read(trg_ctx *c, float *bones12_host, float *world12_host) {
    RefitState::Rig *r = nullptr;
    if (int rc = rig_of(c, "trg_rig_read", &r)) return rc;
    if (!r->evaluated) return fail(c, TRG_ERR_INVALID, "trg_rig_read: the rig has not been evaluated since it was bound");
    const size_t mats = (size_t)r->n_joints * 48;
    if (bones12_host) RF_HIPCHK(c, hipMemcpyAsync(bones12_host, r->bones.p, mats, hipMemcpyDeviceToHost, c->stream));
    if (world12_host) RF_HIPCHK(c, hipMemcpyAsync(world12_host, r->world.p, mats, hipMemcpyDeviceToHost, c->stream));
    RF_HIPCHK(c, hipStreamSynchronize(c->stream));
    return TRG_OK;
}

int trg_rig_buffers(trg_ctx *c, void **bones_dev, void **world_dev) {
    RefitState::Rig *r = nullptr;
    if (int rc = rig_of(c, "trg_rig_buffers", &r)) return rc;
    if (bones_dev) *bones_dev = r->bones.p;
    if (world_dev) *world_dev = r->world.p;
    return TRG_OK;
}

int trg_rig_release(trg_ctx *c) {
    if (!c) return TRG_ERR_INVALID;
    if (!c->refit) return TRG_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    RefitState::Rig &r = c->refit->rig;
    r.each_own([](Buf &buf) { if (buf.p) (void)hipFree(buf.p); buf.p = nullptr; buf.bytes = 0; });
    r.bound = false; r.evaluated = false;
    return TRG_OK;
}

int trg_rig_skin_apply(trg_ctx *c, const float *clocks) {
    const char *who = "trg_rig_skin_apply";
    RefitState::Rig *r = nullptr;
    RefitState::Skin *p = nullptr;
    int rc = TRG_OK;
    if ((rc = rig_target(c, who, &RefitState::skin, "trg_skin_bind", &r, &p)) || (rc = rig_counts(c, who, *r, p->n_bones)) || (rc = clocks_finite(c, who, *r, clocks)) ||
        (rc = rig_evaluate(c, *r, clocks)))
        return rc;
    RF_HIPCHK(c, hipMemcpyAsync(p->bones.p, r->bones.p, (size_t)p->n_bones * 48, hipMemcpyDeviceToDevice, c->stream));
    return skin_run(c, *p);
}

int trg_rig_morph_apply(trg_ctx *c, const float *target_weights, const float *clocks) {
    const char *who = "trg_rig_morph_apply";
    RefitState::Rig *r = nullptr;
    RefitState::Morph *m = nullptr;
    int rc = TRG_OK;
    if ((rc = rig_target(c, who, &RefitState::morph, "trg_morph_bind", &r, &m)) || (rc = morph_has_bones(c, who, *m)) || (rc = rig_counts(c, who, *r, m->n_bones)) ||
        (rc = morph_weights(c, who, *m, target_weights)) || (rc = clocks_finite(c, who, *r, clocks)) || (rc = rig_evaluate(c, *r, clocks)))
        return rc;
    RF_HIPCHK(c, hipMemcpyAsync(m->tw.p, target_weights, (size_t)m->n_targets * 4, hipMemcpyHostToDevice, c->stream));
    RF_HIPCHK(c, hipMemcpyAsync(m->bones.p, r->bones.p, (size_t)m->n_bones * 48, hipMemcpyDeviceToDevice, c->stream));
    return morph_run(c, *m);
}

int trg_rig_skin_apply_device(trg_ctx *c, const void *bones12_dev) {
    const char *who = "trg_rig_skin_apply_device";
    RefitState::Skin *p = nullptr;
    if (int rc = device_target(c, who, &RefitState::skin, "trg_skin_bind", &p)) return rc;
    if (!bones12_dev) return fail(c, TRG_ERR_INVALID, "%s: null bones", who);
    if (int rc = device_span(c, bones12_dev, (size_t)p->n_bones * 48, "bones", who)) return rc;
    RF_HIPCHK(c, hipMemcpyAsync(p->bones.p, bones12_dev, (size_t)p->n_bones * 48, hipMemcpyDeviceToDevice, c->stream));
    return skin_run(c, *p);
}

int trg_rig_morph_apply_device(trg_ctx *c, const float *target_weights, const void *bones12_dev) {
    const char *who = "trg_rig_morph_apply_device";
    RefitState::Morph *m = nullptr;
    int rc = TRG_OK;
    if ((rc = device_target(c, who, &RefitState::morph, "trg_morph_bind", &m)) || (rc = morph_has_bones(c, who, *m)) || (rc = morph_weights(c, who, *m, target_weights))) return rc;
    if (!bones12_dev) return fail(c, TRG_ERR_INVALID, "%s: null bones", who);
    if ((rc = device_span(c, bones12_dev, (size_t)m->n_bones * 48, "bones", who))) return rc;
    RF_HIPCHK(c, hipMemcpyAsync(m->tw.p, target_weights, (size_t)m->n_targets * 4, hipMemcpyHostToDevice, c->stream));
    RF_HIPCHK(c, hipMemcpyAsync(m->bones.p, bones12_dev, (size_t)m->n_bones * 48, hipMemcpyDeviceToDevice, c->stream));
    return morph_run(c, *m);
}

int trg_group_rig_bind(trg_group *g, const uint32_t *parent, uint32_t n_joints, const uint32_t *key_first, const float *keys12, uint32_t n_keys, const uint32_t *clock_of,
                       uint32_t n_clocks, const float *inv_bind12) {
    return group_each(g, [&](trg_ctx *c) { return trg_rig_bind(c, parent, n_joints, key_first, keys12, n_keys, clock_of, n_clocks, inv_bind12); });
}

int trg_group_rig_skin_apply(trg_group *g, const float *clocks) {
    return group_each(g, [&](trg_ctx *c) { return trg_rig_skin_apply(c, clocks); });
}

int trg_group_rig_morph_apply(trg_group *g, const float *target_weights, const float *clocks) {
    return group_each(g, [&](trg_ctx *c) { return trg_rig_morph_apply(c, target_weights, clocks); });
}

int trg_refit_last(trg_ctx *c, trg_refit_info *out) {
    if (!c || !out) return TRG_ERR_INVALID;
    *out = c->refit ? c->refit->last : trg_refit_info{};
    return TRG_OK;
}

int trg_refit_release(trg_ctx *c) {
    if (!c) return TRG_ERR_INVALID;
    refit_state_free(c);
    return TRG_OK;
}

int trg_group_refit_scene(trg_group *g, const float *positions3, const float *normals3, const uint32_t *indices, uint32_t n_verts, uint32_t n_tris) {
    return group_each(g, [&](trg_ctx *c) { return trg_refit_scene(c, positions3, normals3, indices, n_verts, n_tris); });
}

}  // extern "C"
