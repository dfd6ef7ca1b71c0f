// trg_refit_math.h -- the arithmetic of a refit (include/trg_refit.h), host and device: what trg_refit.hip's kernels evaluate per leaf record, per
// box record and per node, written once so that a CPU-only machine can check it against the builders (tests/helpers/refit_check.cpp).
// Every function here repeats a rule of the builders, named at its head; none of them allocates or touches anything but its arguments.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "q4node.h"

#if defined(__HIPCC__)
#define TRG_RF_HD __host__ __device__
#else
#define TRG_RF_HD
#endif

// the builders' double arithmetic is evaluated as written: no fused multiply-adds in this header's functions, host or device
// (a compiler that does not know the pragma is given -ffp-contract=off by whoever builds with it)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace trg {
namespace refit {

// the caller's buffers; an index out of range is reported by the bounds pass and CLAMPED by everyone else, so that no pass reads out of bounds
struct Geo { const float *pos; const uint32_t *idx; uint32_t n_verts, n_tris; };
TRG_RF_HD inline const float *vtx(const Geo &g, uint32_t t, int j) {
    uint32_t i = g.idx[(size_t)t * 3 + j];
    if (i >= g.n_verts) i = g.n_verts - 1u;
    return g.pos + (size_t)i * 3;
}
TRG_RF_HD inline bool same3(const float *p, const float *q) { return p[0] == q[0] && p[1] == q[1] && p[2] == q[2]; }
TRG_RF_HD inline float max2(float a, float b) { return a < b ? b : a; }   // (std::max's order of arguments: NaN in b is dropped, as there)
TRG_RF_HD inline uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// ---- bvh_build.cpp put_rec: the xyz of the three rows (v0, e1, e2) of triangle `prim`; the .w words (index, mask, 0) are not touched ----
TRG_RF_HD inline void tri_rows(const Geo &g, uint32_t prim, float *rows12) {
    const float *a = vtx(g, prim, 0), *b = vtx(g, prim, 1), *c = vtx(g, prim, 2);
    for (int k = 0; k < 3; ++k) { rows12[k] = a[k]; rows12[4 + k] = b[k] - a[k]; rows12[8 + k] = c[k] - a[k]; }
}

// ---- bounds of a triangle's three vertices (Box::grow) ----
TRG_RF_HD inline void grow_tri(const Geo &g, uint32_t prim, float *lo, float *hi) {
    for (int j = 0; j < 3; ++j) {
        const float *p = vtx(g, prim, j);
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], p[a]); hi[a] = fmaxf(hi[a], p[a]); }
    }
}

// ---- the builders' padding and the scene centre from the bounds of the triangles (bvh_build.cpp build_bvh, trg_capi.cpp host_scene_build) ----
TRG_RF_HD inline float scene_pad(const float *lo, const float *hi) {
    const float diag = max2(max2(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
    float maxabs = 0.f;
    for (int a = 0; a < 3; ++a) maxabs = max2(max2(maxabs, fabsf(lo[a])), fabsf(hi[a]));
    return max2(2e-5f * max2(diag, 1e-3f), 4e-6f * maxabs);
}
TRG_RF_HD inline void scene_center(const float *lo, const float *hi, float *center) {
    for (int a = 0; a < 3; ++a) center[a] = 0.5f * (lo[a] + hi[a]);
}

// ---- bvh_build.cpp quad_pair without the material ids (they do not move): are triangles k and k + 1 the halves of a parallelogram, and which
//      is X?  A pair the loaded tree holds as a quad leaf must give true and the same (x, y). ----
TRG_RF_HD inline bool quad_pair_pos(const Geo &g, uint32_t k, uint32_t &x, uint32_t &y) {
    if (k + 1u >= g.n_tris || !same3(vtx(g, k, 0), vtx(g, k + 1u, 0))) return false;
    const float *a = vtx(g, k, 0), *p1, *dg, *p3;
    if (same3(vtx(g, k, 2), vtx(g, k + 1u, 1))) { x = k; y = k + 1u; p1 = vtx(g, k, 1); dg = vtx(g, k, 2); p3 = vtx(g, k + 1u, 2); }
    else if (same3(vtx(g, k, 1), vtx(g, k + 1u, 2))) { x = k + 1u; y = k; p1 = vtx(g, k + 1u, 1); dg = vtx(g, k, 1); p3 = vtx(g, k, 2); }
    else return false;
    float big = 0.f;
    for (int c = 0; c < 3; ++c) big = max2(max2(max2(max2(big, fabsf(a[c])), fabsf(p1[c])), fabsf(p3[c])), fabsf(dg[c]));
    for (int c = 0; c < 3; ++c)
        if (!(fabsf((p1[c] - a[c]) + (p3[c] - a[c]) - (dg[c] - a[c])) <= 4e-6f * big)) return false;
    const float e1[3] = { p1[0] - a[0], p1[1] - a[1], p1[2] - a[2] }, e2[3] = { p3[0] - a[0], p3[1] - a[1], p3[2] - a[2] };
    const float n[3] = { e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0] };
    const float area2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    return area2 > 0.f && isfinite(area2);
}
// the pair (x, y) of a quad leaf of the loaded tree under the moved vertices
TRG_RF_HD inline bool quad_still(const Geo &g, uint32_t x, uint32_t y) {
    uint32_t nx = 0, ny = 0;
    const uint32_t k = x < y ? x : y;
    return (x > y ? x - y : y - x) == 1u && quad_pair_pos(g, k, nx, ny) && nx == x && ny == y;
}

// ---- trg_capi.cpp fill_plane_record: the three planes of (v0, e1, e2) relative to `center`, in double; `e2row` = the row whose xyz is the second
//      edge -- the record's own row 2, or row 2 of the Y record when this record is the X of a quad ----
TRG_RF_HD inline void plane_rows(const float *rows12, const float *e2row, const float *center, float *out12) {
    const double v0[3] = { (double)rows12[0] - center[0], (double)rows12[1] - center[1], (double)rows12[2] - center[2] };
    const double e1[3] = { rows12[4], rows12[5], rows12[6] }, e2[3] = { e2row[0], e2row[1], e2row[2] };
    double n[3] = { e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0] };
    const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    const float never[12] = { 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, -1.f, 0.f, 0.f, 0.f, -1.f };
    for (int k = 0; k < 12; ++k) out12[k] = never[k];
    if (!(len > 0.0) || !isfinite(len)) return;
    for (int k = 0; k < 3; ++k) n[k] /= len;
    double a1[3] = { e2[1] * n[2] - e2[2] * n[1], e2[2] * n[0] - e2[0] * n[2], e2[0] * n[1] - e2[1] * n[0] };
    double a2[3] = { n[1] * e1[2] - n[2] * e1[1], n[2] * e1[0] - n[0] * e1[2], n[0] * e1[1] - n[1] * e1[0] };
    const double s1 = e1[0] * a1[0] + e1[1] * a1[1] + e1[2] * a1[2], s2 = e2[0] * a2[0] + e2[1] * a2[1] + e2[2] * a2[2];
    if (s1 == 0.0 || s2 == 0.0) return;
    for (int k = 0; k < 3; ++k) { a1[k] /= s1; a2[k] /= s2; }
    const double d0 = n[0] * v0[0] + n[1] * v0[1] + n[2] * v0[2], d1 = -(a1[0] * v0[0] + a1[1] * v0[1] + a1[2] * v0[2]),
                 d2 = -(a2[0] * v0[0] + a2[1] * v0[1] + a2[2] * v0[2]);
    const float r[12] = { (float)n[0], (float)n[1], (float)n[2], (float)d0, (float)a1[0], (float)a1[1], (float)a1[2], (float)d1,
                          (float)a2[0], (float)a2[1], (float)a2[2], (float)d2 };
    bool ok = true;
    for (int k = 0; k < 12; ++k) ok = ok && isfinite(r[k]);
    if (ok) for (int k = 0; k < 12; ++k) out12[k] = r[k];
}

// ---- a box's own frame as the builder keeps it (bvh_build.h BoxLeaf: fp32 centre and rows) ----
struct Frame { float center[3]; float axis[3][3]; };
// trg_capi.cpp box_frame_rows: (a_k, d_k), l_k = a_k . (P - scene centre) + d_k
TRG_RF_HD inline void frame_rows(const Frame &f, const float *scene_center, float *rows12) {
    for (int k = 0; k < 3; ++k) {
        double dk = 0.0;
        for (int a = 0; a < 3; ++a) { rows12[k * 4 + a] = f.axis[k][a]; dk -= (double)f.axis[k][a] * ((double)f.center[a] - (double)scene_center[a]); }
        rows12[k * 4 + 3] = (float)dk;
    }
}

// ---- bvh_build.cpp box_group without the material ids: triangles k .. k + 11 as six quads that bound a parallelepiped; the corner test at 1e-5.
//      face_quad[f]: which of the six quads (index order) is face f = 2 axis + (l > 0) ----
TRG_RF_HD inline bool box_group_pos(const Geo &g, uint32_t k, Frame &out, uint32_t *face_quad) {
    if (k + 12u > g.n_tris) return false;
    double corner[6][4][3], fc[6][3], C[3] = { 0, 0, 0 };
    for (uint32_t q = 0; q < 6; ++q) {
        uint32_t x = 0, y = 0;
        if (!quad_pair_pos(g, k + 2u * q, x, y)) return false;
        const float *p[4] = { vtx(g, x, 0), vtx(g, x, 1), vtx(g, x, 2), vtx(g, y, 2) };
        for (int a = 0; a < 3; ++a) {
            fc[q][a] = 0;
            for (int j = 0; j < 4; ++j) { corner[q][j][a] = p[j][a]; fc[q][a] += 0.25 * p[j][a]; }
            C[a] += fc[q][a] / 6.0;
        }
    }
    int opp[6] = { -1, -1, -1, -1, -1, -1 };
    double scale = 0;
    for (int q = 0; q < 6; ++q) for (int a = 0; a < 3; ++a) { const double d = fabs(fc[q][a] - C[a]); scale = scale < d ? d : scale; }
    if (!(scale > 0) || !isfinite(scale)) return false;
    for (int q = 0; q < 6; ++q) {
        double best = 1e300; int bq = -1;
        for (int r = 0; r < 6; ++r) {
            if (r == q) continue;
            double e = 0;
            for (int a = 0; a < 3; ++a) { const double d = fabs(fc[q][a] + fc[r][a] - 2 * C[a]); e = e < d ? d : e; }
            if (e < best) { best = e; bq = r; }
        }
        if (bq < 0 || best > 1e-5 * scale) return false;
        opp[q] = bq;
    }
    double h[3][3], A[3][3];
    int axis_of[6], nax = 0;
    for (int q = 0; q < 6; ++q) axis_of[q] = -1;
    for (int q = 0; q < 6; ++q) {
        if (opp[opp[q]] != q) return false;
        if (axis_of[q] >= 0) continue;
        if (nax == 3) return false;
        for (int a = 0; a < 3; ++a) h[nax][a] = 0.5 * (fc[q][a] - fc[opp[q]][a]);
        axis_of[q] = axis_of[opp[q]] = nax;
        face_quad[2 * nax + 1] = (uint32_t)q; face_quad[2 * nax] = (uint32_t)opp[q];
        ++nax;
    }
    if (nax != 3) return false;
    const double c12[3] = { h[1][1] * h[2][2] - h[1][2] * h[2][1], h[1][2] * h[2][0] - h[1][0] * h[2][2], h[1][0] * h[2][1] - h[1][1] * h[2][0] };
    const double c20[3] = { h[2][1] * h[0][2] - h[2][2] * h[0][1], h[2][2] * h[0][0] - h[2][0] * h[0][2], h[2][0] * h[0][1] - h[2][1] * h[0][0] };
    const double c01[3] = { h[0][1] * h[1][2] - h[0][2] * h[1][1], h[0][2] * h[1][0] - h[0][0] * h[1][2], h[0][0] * h[1][1] - h[0][1] * h[1][0] };
    const double det = h[0][0] * c12[0] + h[0][1] * c12[1] + h[0][2] * c12[2];
    if (!(fabs(det) > 1e-12 * scale * scale * scale) || !isfinite(det)) return false;
    for (int a = 0; a < 3; ++a) { A[0][a] = c12[a] / det; A[1][a] = c20[a] / det; A[2][a] = c01[a] / det; }
    for (int q = 0; q < 6; ++q) {
        const int kx = axis_of[q];
        const double side = face_quad[2 * kx + 1] == (uint32_t)q ? 1.0 : -1.0;
        double sum[3] = { 0, 0, 0 };
        for (int j = 0; j < 4; ++j)
            for (int ax = 0; ax < 3; ++ax) {
                double l = 0;
                for (int a = 0; a < 3; ++a) l += A[ax][a] * (corner[q][j][a] - C[a]);
                if (!(fabs(fabs(l) - 1.0) <= 1e-5)) return false;
                if (ax == kx && l * side < 0) return false;
                sum[ax] += l;
            }
        for (int ax = 0; ax < 3; ++ax)
            if (ax != kx && fabs(sum[ax]) > 1e-3) return false;
    }
    for (int a = 0; a < 3; ++a) { out.center[a] = (float)C[a]; for (int r = 0; r < 3; ++r) out.axis[r][a] = (float)A[r][a]; }
    return true;
}

// ---- bvh_build.cpp, "a LONE QUAD is a box too": the frame of a quad of no thickness from its X rows and the e2 row of its Y ----
TRG_RF_HD inline bool lone_quad_frame(const float *xrows12, const float *y_e2row, Frame &out) {
    const double p0[3] = { xrows12[0], xrows12[1], xrows12[2] }, e1[3] = { xrows12[4], xrows12[5], xrows12[6] }, e2[3] = { y_e2row[0], y_e2row[1], y_e2row[2] };
    double nn[3] = { e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0] };
    const double d11 = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2], d22 = e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2];
    const double len = sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]), size = sqrt(d11 < d22 ? d22 : d11);
    if (!(len > 0.0) || !isfinite(len) || !(size > 0.0)) return false;
    for (int a = 0; a < 3; ++a) nn[a] /= len;
    const double c1[3] = { e2[1] * nn[2] - e2[2] * nn[1], e2[2] * nn[0] - e2[0] * nn[2], e2[0] * nn[1] - e2[1] * nn[0] };
    const double c2[3] = { nn[1] * e1[2] - nn[2] * e1[1], nn[2] * e1[0] - nn[0] * e1[2], nn[0] * e1[1] - nn[1] * e1[0] };
    const double s1 = e1[0] * c1[0] + e1[1] * c1[1] + e1[2] * c1[2], s2 = e2[0] * c2[0] + e2[1] * c2[1] + e2[2] * c2[2], eh = size * (1.0 / 1073741824.0);
    if (s1 == 0.0 || s2 == 0.0) return false;
    bool finite = true;
    for (int a = 0; a < 3; ++a) {
        out.center[a] = (float)(p0[a] + 0.5 * (e1[a] + e2[a]));
        out.axis[0][a] = (float)(2.0 * c1[a] / s1); out.axis[1][a] = (float)(2.0 * c2[a] / s2); out.axis[2][a] = (float)(nn[a] / eh);
        finite = finite && isfinite(out.axis[0][a]) && isfinite(out.axis[1][a]) && isfinite(out.axis[2][a]);
    }
    return finite;
}

// ---- leaf codes (bvh_build.h) ----
constexpr uint32_t kCodeQuad = 7u, kCodeBox = 6u;
TRG_RF_HD inline uint32_t code_records(uint32_t code) { return (code & 7u) == kCodeQuad ? 2u : (code & 7u) + 1u; }   // (not for a box code)

// ---- one node: the float form quantize_node4 takes (lo.x[4] hi.x[4] lo.y[4] hi.y[4] lo.z[4] hi.z[4] child[4] pad[4]) from the UNPADDED boxes of its
//      children (6 floats each: lo, hi) and its child words, padded as the builders pad (lo - pad, hi + pad; an unused slot: zeros) ----
TRG_RF_HD inline void node_floats(const float *child_boxes24, const uint32_t *child4, float pad, float *out32) {
    for (int k = 0; k < 4; ++k) {
        const bool e = (int32_t)child4[k] == kQ4Empty;
        for (int a = 0; a < 3; ++a) {
            out32[a * 8 + k] = e ? 0.f : child_boxes24[k * 6 + a] - pad;
            out32[a * 8 + 4 + k] = e ? 0.f : child_boxes24[k * 6 + 3 + a] + pad;
        }
        memcpy(&out32[24 + k], &child4[k], 4);
        out32[28 + k] = 0.f;
    }
}

// the decoded box of child k of a quantised node, in double (exact: origin + q * power of two)
TRG_RF_HD inline void decode_child(const uint32_t *node16, int k, double *lo, double *hi) {
    float o[3], s[3];
    memcpy(&o[0], &node16[0], 4); memcpy(&o[1], &node16[1], 4); memcpy(&o[2], &node16[2], 4);
    memcpy(&s[0], &node16[3], 4); memcpy(&s[1], &node16[10], 4); memcpy(&s[2], &node16[11], 4);
    const uint32_t ql[3] = { node16[4], node16[6], node16[8] }, qh[3] = { node16[5], node16[7], node16[9] };
    for (int a = 0; a < 3; ++a) {
        lo[a] = (double)o[a] + (double)((ql[a] >> (8 * k)) & 255u) * (double)s[a];
        hi[a] = (double)o[a] + (double)((qh[a] >> (8 * k)) & 255u) * (double)s[a];
    }
}
// sum of the half areas of the decoded boxes of a node's used children
TRG_RF_HD inline double node_half_area(const uint32_t *node16) {
    double sum = 0.0;
    for (int k = 0; k < 4; ++k) {
        if ((int32_t)node16[12 + k] == kQ4Empty) continue;
        double lo[3], hi[3];
        decode_child(node16, k, lo, hi);
        const double d[3] = { hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2] };
        sum += d[0] * d[1] + d[1] * d[2] + d[2] * d[0];
    }
    return sum;
}

}  // namespace refit
}  // namespace trg
