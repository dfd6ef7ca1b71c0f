// trg_pose_math.h -- the arithmetic of a pose (include/trg_pose.h), host and device: what trg_refit.hip's pose kernel evaluates per vertex and per
// corner normal, and the two maps trg_pose_bind derives on the host, written once so that a CPU-only machine can run them
// (tests/helpers/pose_check.cpp).  None of these functions allocates or touches anything but its arguments.
//
// A transform is 12 floats, row-major M = [A | t]: m[4 i + j] = a_ij, m[4 i + 3] = t_i.  Every operation below is ONE fp32 operation, in the order
// written; nothing is fused (toyraygun_amd/pose.py pose_reference restates this text in numpy float32 and must agree to the bit).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TRG_PM_HD __host__ __device__
#else
#define TRG_PM_HD
#endif

// (a compiler that does not know the pragma is given -ffp-contract=off by whoever builds with it)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace trg {
namespace pose {

constexpr uint32_t kNoObject = ~0u;   // the map word of a vertex that no triangle names: it never moves

// x' = ((m0 x + m1 y) + m2 z) + m3, per row
TRG_PM_HD inline void point(const float *m, const float *p, float *out) {
    for (int i = 0; i < 3; ++i) {
        const float *r = m + 4 * i;
        const float a = r[0] * p[0], b = r[1] * p[1], c = r[2] * p[2];
        out[i] = ((a + b) + c) + r[3];
    }
}

// the cofactors C_ij of A, each p q - r s (two products, one difference), and det = (a00 C00 + a01 C01) + a02 C02
TRG_PM_HD inline float cofactors(const float *m, float *C9) {
    const float a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[4], a11 = m[5], a12 = m[6], a20 = m[8], a21 = m[9], a22 = m[10];
    const float pq[9] = { a11 * a22, a12 * a20, a10 * a21, a02 * a21, a00 * a22, a01 * a20, a01 * a12, a02 * a10, a00 * a11 };
    const float rs[9] = { a12 * a21, a10 * a22, a11 * a20, a01 * a22, a02 * a20, a00 * a21, a02 * a11, a00 * a12, a01 * a10 };
    for (int k = 0; k < 9; ++k) C9[k] = pq[k] - rs[k];
    const float d0 = a00 * C9[0], d1 = a01 * C9[1], d2 = a02 * C9[2];
    return (d0 + d1) + d2;
}

// n' = s ((C_i0 nx + C_i1 ny) + C_i2 nz), s = -1 for a mirroring A; the posed normal is n' / |n'| by IEEE division, or the rest normal when |n'| is
// zero or not finite (a matrix of rank 1 or less, an overflow)
TRG_PM_HD inline void normal(const float *m, const float *n, float *out) {
    float C[9];
    const float det = cofactors(m, C);
    const float s = det < 0.f ? -1.f : 1.f;
    float v[3];
    for (int i = 0; i < 3; ++i) {
        const float a = C[3 * i] * n[0], b = C[3 * i + 1] * n[1], c = C[3 * i + 2] * n[2];
        v[i] = s * ((a + b) + c);
    }
    const float xx = v[0] * v[0], yy = v[1] * v[1], zz = v[2] * v[2];
    const float len = sqrtf((xx + yy) + zz);
    const bool ok = len > 0.f && isfinite(len);
    for (int i = 0; i < 3; ++i) out[i] = ok ? v[i] / len : n[i];
}

// ---- the maps of trg_pose_bind (host) ----
enum { kTableOk = 0, kTableFirst = 1, kTableOrder = 2, kTableEnd = 3 };
// object j is triangles [first[j], first[j + 1]): first[0] = 0, strictly ascending, first[n_objects] = n_tris.  *offender: the first object at fault
inline int table_check(const uint32_t *first, uint32_t n_objects, uint32_t n_tris, uint32_t *offender) {
    *offender = 0;
    if (first[0] != 0u) return kTableFirst;
    for (uint32_t j = 0; j < n_objects; ++j)
        if (!(first[j] < first[j + 1])) { *offender = j; return kTableOrder; }
    if (first[n_objects] != n_tris) { *offender = n_objects - 1u; return kTableEnd; }
    return kTableOk;
}
// (of a table that passed table_check)
inline void triangle_objects(const uint32_t *first, uint32_t n_objects, uint32_t *tri_obj) {
    for (uint32_t j = 0; j < n_objects; ++j)
        for (uint32_t t = first[j]; t < first[j + 1]; ++t) tri_obj[t] = j;
}
enum { kVertsOk = 0, kVertsIndex = 1, kVertsShared = 2 };
// every vertex belongs to the one object whose triangles name it, or to none.  *tri, *vert: the first triangle (in index order) at fault and the
// vertex it names
inline int vertex_objects(const uint32_t *idx, uint32_t n_verts, uint32_t n_tris, const uint32_t *tri_obj, uint32_t *vtx_obj, uint32_t *tri, uint32_t *vert) {
    for (uint32_t v = 0; v < n_verts; ++v) vtx_obj[v] = kNoObject;
    for (uint32_t t = 0; t < n_tris; ++t)
        for (int j = 0; j < 3; ++j) {
            const uint32_t i = idx[(size_t)t * 3 + j];
            *tri = t; *vert = i;
            if (i >= n_verts) return kVertsIndex;
            if (vtx_obj[i] == kNoObject) vtx_obj[i] = tri_obj[t];
            else if (vtx_obj[i] != tri_obj[t]) return kVertsShared;
        }
    *tri = *vert = 0;
    return kVertsOk;
}

}  // namespace pose
}  // namespace trg
