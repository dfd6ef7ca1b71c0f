// trg_morph_math.h -- the arithmetic of blend shapes in front of the skin (include/trg_morph.h), host and device: what trg_refit.hip's morph kernel
// evaluates per vertex and per corner normal, and what trg_morph_bind does on the host -- the checks of the target table and of the entries, and
// the transposition of the caller's by-target lists into per-vertex records --, written once so that a CPU-only machine can run them
// (tests/helpers/morph_check.cpp).  None of these functions allocates or touches anything but its arguments.
//
// An apply has one weight w[k] per target.  Target k is ACTIVE iff w[k] != 0 (so -0 is inactive); an inactive target is SKIPPED, not multiplied
// through.  Every operation below is ONE fp32 operation, in the order written; nothing is fused (toyraygun_amd/morph.py morph_reference restates
// this text in numpy float32 and must agree to the bit).
//
// Position of vertex v: p = rest; for every active target that holds an entry for v, in ascending target order, per component
//     t = w[k] * d;  p = p + t
// Without bones the result is p.  With bones it is pose::point(M, p), M = skin::blend(...) of v (trg_skin_math.h).
//
// Normal of corner c of triangle t, v = indices[3 t + c]: n = the corner's rest normal; if the binding has normal deltas, they are accumulated by
// the same loop over v's entries.  The corner is TOUCHED iff at least one active entry was applied.  An untouched corner keeps the rest normal's
// bits.  A touched corner becomes n / len, len = sqrtf((nx nx + ny ny) + nz nz), by IEEE division -- or the rest normal when len is zero or not
// finite.  Call that n1.  Without bones the result is n1; with bones it is pose::normal(M, n1), M the blended matrix of v.
//
// What follows from it:
//   - equal inputs give equal outputs: the copies of a shared corner stay bitwise equal;
//   - all-zero weights without bones return the rest pose BIT FOR BIT, a -0.0 coordinate included;
//   - all-zero weights with bones equal trg_skin_apply bit for bit;
//   - the fused form equals skin_reference applied to the bone-free result, bit for bit, by construction.  The one extra normalisation of a
//     touched corner under bones is the price of that identity: a few ALU operations in a kernel that waits for memory.
#pragma once
#include "trg_skin_math.h"

namespace trg {
namespace morph {

// one entry of one vertex as the device keeps it: 16 bytes, one load.  Position records and -- only when normal deltas were bound -- a parallel
// array of normal records; vertex v's are [vfirst[v], vfirst[v + 1]) of both, in ascending target order
struct Rec {
    float d[3];
    uint32_t target;
};

// p += w d: one product and one sum per component
TRG_PM_HD inline void add(float w, const float *d, float *p) {
    for (int a = 0; a < 3; ++a) { const float t = w * d[a]; p[a] = p[a] + t; }
}
// the records [first, last) under the weights tw, onto acc; returns whether any was active
TRG_PM_HD inline bool accumulate(const Rec *recs, size_t first, size_t last, const float *tw, float *acc) {
    bool touched = false;
    for (size_t e = first; e < last; ++e) {
        const float w = tw[recs[e].target];
        if (w != 0.f) { add(w, recs[e].d, acc); touched = true; }
    }
    return touched;
}
// n1 of a corner: rest if untouched; n / |n| if touched, rest again when |n| is zero or not finite
TRG_PM_HD inline void finish_normal(const float *rest, const float *n, bool touched, float *out) {
    const float xx = n[0] * n[0], yy = n[1] * n[1], zz = n[2] * n[2];
    const float len = sqrtf((xx + yy) + zz);
    const bool ok = touched && len > 0.f && isfinite(len);
    for (int a = 0; a < 3; ++a) out[a] = ok ? n[a] / len : rest[a];
}

// vertex v, whole: ids4 / weights4 / bones are the skin's (bones == nullptr: a binding without bones)
TRG_PM_HD inline void vertex(const float *rest3, const uint32_t *vfirst, const Rec *recs, const float *tw, uint32_t v, const uint32_t *ids4, const float *weights4,
                             const float *bones, float *out) {
    float p[3] = { rest3[0], rest3[1], rest3[2] };
    accumulate(recs, vfirst[v], vfirst[v + 1], tw, p);
    if (bones) {
        float M[12];
        skin::blend(bones, ids4, weights4, M);
        pose::point(M, p, out);
    } else {
        for (int a = 0; a < 3; ++a) out[a] = p[a];
    }
}
// one corner of vertex v, whole: nrm_recs == nullptr: a binding without normal deltas
TRG_PM_HD inline void corner(const float *rest3, const uint32_t *vfirst, const Rec *nrm_recs, const float *tw, uint32_t v, const uint32_t *ids4, const float *weights4,
                             const float *bones, float *out) {
    float n[3] = { rest3[0], rest3[1], rest3[2] }, n1[3];
    const bool touched = nrm_recs && accumulate(nrm_recs, vfirst[v], vfirst[v + 1], tw, n);
    finish_normal(rest3, n, touched, n1);
    if (bones) {
        float M[12];
        skin::blend(bones, ids4, weights4, M);
        pose::normal(M, n1, out);
    } else {
        for (int a = 0; a < 3; ++a) out[a] = n1[a];
    }
}

// ---- the checks of trg_morph_bind (host) ----
enum { kTargetsOk = 0, kTargetsFirst = 1, kTargetsOrder = 2, kTargetsEnd = 3 };
// target k is entries [first[k], first[k + 1]): first[0] = 0, NON-decreasing (an empty target is legal), first[n_targets] = n_entries.
// *offender: the first target at fault
inline int targets_check(const uint32_t *first, uint32_t n_targets, uint32_t n_entries, uint32_t *offender) {
    *offender = 0;
    if (first[0] != 0u) return kTargetsFirst;
    for (uint32_t k = 0; k < n_targets; ++k)
        if (first[k] > first[k + 1]) { *offender = k; return kTargetsOrder; }
    if (first[n_targets] != n_entries) { *offender = n_targets - 1u; return kTargetsEnd; }
    return kTargetsOk;
}
enum { kEntriesOk = 0, kEntriesVertex = 1, kEntriesOrder = 2, kEntriesDelta = 3, kEntriesNormalDelta = 4 };
// (of a table that passed targets_check)  every entry's vertex < n_verts and strictly ascending within its target -- all of them first --, then
// every delta finite.  *target, *entry: the first entry at fault (its number in the whole list) and the target that owns it.  dnrm3 may be null
inline int entries_check(const uint32_t *first, uint32_t n_targets, const uint32_t *entry_vertex, uint32_t n_verts, const float *dpos3, const float *dnrm3,
                         uint32_t *target, uint32_t *entry) {
    for (uint32_t k = 0; k < n_targets; ++k)
        for (size_t e = first[k]; e < first[k + 1]; ++e) {
            *target = k; *entry = (uint32_t)e;
            if (entry_vertex[e] >= n_verts) return kEntriesVertex;
            if (e > first[k] && !(entry_vertex[e - 1] < entry_vertex[e])) return kEntriesOrder;
        }
    for (uint32_t k = 0; k < n_targets; ++k)
        for (size_t e = first[k]; e < first[k + 1]; ++e) {
            *target = k; *entry = (uint32_t)e;
            for (int a = 0; a < 3; ++a) {
                if (!isfinite(dpos3[e * 3 + a])) return kEntriesDelta;
                if (dnrm3 && !isfinite(dnrm3[e * 3 + a])) return kEntriesNormalDelta;
            }
        }
    *target = *entry = 0;
    return kEntriesOk;
}

// ---- the transposition of trg_morph_bind (host): by-target lists -> per-vertex records (of lists that passed both checks) ----
// vfirst[n_verts + 1]: vertex v's records are [vfirst[v], vfirst[v + 1]), in ascending target order; pos_recs[n_entries], and nrm_recs[n_entries]
// when dnrm3 is given (both null or both not).  cursor[n_verts] is scratch.  A counting sort: count, prefix sums, then the targets in ascending
// order each append to their vertices' ranges
inline void transpose(const uint32_t *first, uint32_t n_targets, const uint32_t *entry_vertex, const float *dpos3, const float *dnrm3, uint32_t n_verts,
                      uint32_t *vfirst, uint32_t *cursor, Rec *pos_recs, Rec *nrm_recs) {
    const size_t n_entries = first[n_targets];
    for (uint32_t v = 0; v <= n_verts; ++v) vfirst[v] = 0;
    for (size_t e = 0; e < n_entries; ++e) ++vfirst[(size_t)entry_vertex[e] + 1];
    for (uint32_t v = 0; v < n_verts; ++v) { vfirst[v + 1] += vfirst[v]; cursor[v] = vfirst[v]; }
    for (uint32_t k = 0; k < n_targets; ++k)
        for (size_t e = first[k]; e < first[k + 1]; ++e) {
            const size_t at = cursor[entry_vertex[e]]++;
            for (int a = 0; a < 3; ++a) pos_recs[at].d[a] = dpos3[e * 3 + a];
            pos_recs[at].target = k;
            if (dnrm3) {
                for (int a = 0; a < 3; ++a) nrm_recs[at].d[a] = dnrm3[e * 3 + a];
                nrm_recs[at].target = k;
            }
        }
}

}  // namespace morph
}  // namespace trg
