// trg_skin_math.h -- the arithmetic of linear-blend skinning (include/trg_skin.h), host and device: what trg_refit.hip's skin kernel evaluates per
// vertex and per corner normal, and the checks trg_skin_bind makes on the host, written once so that a CPU-only machine can run them
// (tests/helpers/skin_check.cpp).  None of these functions allocates or touches anything but its arguments.
//
// A bone is 12 floats, row-major B = [A | t], like a pose transform (trg_pose_math.h).  Vertex v has four bone ids b0..b3 and four weights w0..w3.
// Its blended matrix is, for k = 0..11,
//     M[k] = ((w0 B_b0[k] + w1 B_b1[k]) + w2 B_b2[k]) + w3 B_b3[k]
// every product and every sum ONE fp32 operation, in that order; nothing is fused (toyraygun_amd/skin.py skin_reference restates this text in numpy
// float32 and must agree to the bit).  The skinned position is pose::point(M, p).  Corner c of triangle t belongs to vertex indices[3 t + c]: its
// normal is pose::normal(M of that vertex, n) -- the cofactor matrix of M's linear part, the sign of its determinant, an IEEE division by the
// length; the rest normal is kept when that length is zero or not finite.
//
// What follows from it:
//   - equal inputs give equal outputs: the copies of a shared corner stay bitwise equal;
//   - a vertex with weights (1, 0, 0, 0) and finite bones gets M == B_b0 (1 x is x, 0 x is a zero, x + 0 is x; a -0 entry becomes +0), so its
//     position and normals are equal under == to trg_pose_apply's with that bone as its object's matrix; only the sign of a zero may differ;
//   - the weights are used AS GIVEN: the library does not normalise them.  weights_check refuses a sum further than 1e-4 from 1; within that, a sum
//     that is not exactly 1 scales the vertex about the origin by that much.
#pragma once
#include "trg_pose_math.h"

namespace trg {
namespace skin {

// M += w B, or M = w B for the first bone: one product (and one sum) per entry.  The kernel calls this once per bone, so that twelve accumulators
// and one bone are live, not four bones
TRG_PM_HD inline void blend_first(const float *bone, float w, float *M) {
    for (int k = 0; k < 12; ++k) M[k] = w * bone[k];
}
TRG_PM_HD inline void blend_next(const float *bone, float w, float *M) {
    for (int k = 0; k < 12; ++k) { const float t = w * bone[k]; M[k] = M[k] + t; }
}
// the blended matrix of one vertex: ids4 / weights4 are that vertex's records, bones the table
TRG_PM_HD inline void blend(const float *bones, const uint32_t *ids4, const float *weights4, float *M) {
    blend_first(bones + (size_t)ids4[0] * 12, weights4[0], M);
    for (int j = 1; j < 4; ++j) blend_next(bones + (size_t)ids4[j] * 12, weights4[j], M);
}

// ---- the checks of trg_skin_bind (host) ----
enum { kSkinOk = 0, kSkinId = 1, kSkinWeight = 2, kSkinSum = 3 };
// every id < n_bones -- also the id of a zero weight: the kernel reads that bone.  *vert: the first vertex at fault, *slot: which of its four
inline int ids_check(const uint32_t *ids4, uint32_t n_verts, uint32_t n_bones, uint32_t *vert, uint32_t *slot) {
    *vert = *slot = 0;
    for (uint32_t v = 0; v < n_verts; ++v)
        for (uint32_t j = 0; j < 4; ++j)
            if (ids4[(size_t)v * 4 + j] >= n_bones) { *vert = v; *slot = j; return kSkinId; }
    return kSkinOk;
}
// every weight finite and >= 0, and |w0 + w1 + w2 + w3 - 1| <= 1e-4 with the sum formed in double.  Vertex by vertex: the first vertex at fault
// is named, whichever rule it breaks
inline int weights_check(const float *weights4, uint32_t n_verts, uint32_t *vert, uint32_t *slot) {
    *vert = *slot = 0;
    for (uint32_t v = 0; v < n_verts; ++v) {
        const float *w = weights4 + (size_t)v * 4;
        double sum = 0.0;
        for (uint32_t j = 0; j < 4; ++j) {
            if (!(isfinite(w[j]) && w[j] >= 0.f)) { *vert = v; *slot = j; return kSkinWeight; }
            sum += (double)w[j];
        }
        if (!(fabs(sum - 1.0) <= 1e-4)) { *vert = v; return kSkinSum; }
    }
    return kSkinOk;
}

}  // namespace skin
}  // namespace trg
