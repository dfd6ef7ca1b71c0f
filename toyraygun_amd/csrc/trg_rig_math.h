// trg_rig_math.h -- the arithmetic of a rig (include/trg_rig.h), host and device: what trg_refit.hip's rig kernel evaluates per joint, and the
// checks and the level table trg_rig_bind makes on the host, written once so that a CPU-only machine can run them (tests/helpers/rig_check.cpp).
// None of these functions allocates or touches anything but its arguments.
//
// DATA.  n_joints joints; joint j is bone j.  parent[j] is kNoParent (a root; several are legal: a forest) or < j.  Joint j's keys are the records
// kfirst[j] .. kfirst[j + 1] - 1 of `keys`, each 12 floats = three 16-byte rows
//     { time, Tx, Ty, Tz | Rx, Ry, Rz, Rw | Sx, Sy, Sz, 0 }
// at least one per joint, times strictly ascending within a joint.  clock_of[j] < n_clocks names the clock joint j is sampled at.  inv_bind is
// n_joints x 12 floats, row-major [A | t] like a bone (trg_pose_math.h), or absent.
//
// Every product, sum, difference, quotient and square root below is ONE fp32 operation, in the order written; nothing is fused
// (toyraygun_amd/rig.py rig_reference restates this text in numpy float32 and must agree to the bit).
//
// SAMPLE joint j at t = clocks[clock_of[j]], first / last its first and last key:
//     t <= time[first]: the first key's T, R, S, bit for bit.          t >= time[last]: the last key's, bit for bit.
//     otherwise i = the largest index with time[i] <= t (any search finds the same one), a = key i, b = key i + 1,
//         u = (t - time_a) / (time_b - time_a)
//         T = a.T + u * (b.T - a.T)         S = a.S + u * (b.S - a.S)                      per component
//         d = ((ax bx + ay by) + az bz) + aw bw           of the rotations; if d < 0, b's rotation is negated (the short path)
//         q = a.R + u * (b.R - a.R)                                                        per component
//         len = sqrtf(((qx qx + qy qy) + qz qz) + qw qw)
//         R = q / len by IEEE division -- or a.R when len is zero or not finite.
// This is the normalised lerp.  SPHERICAL interpolation is out of scope: sinf and acosf are correctly rounded neither on the host nor on the
// device, so a slerp's bits could not be pinned, and a unit whose bits cannot be pinned cannot be tested the way refit, pose, skin and morph are.
//
// LOCAL matrix of (T, R = (x, y, z, w), S), row-major [A | t]:
//     xx = x x, yy = y y, zz = z z, xy = x y, xz = x z, yz = y z, wx = w x, wy = w y, wz = w z
//     r00 = 1 - 2 (yy + zz)    r01 = 2 (xy - wz)        r02 = 2 (xz + wy)
//     r10 = 2 (xy + wz)        r11 = 1 - 2 (xx + zz)    r12 = 2 (yz - wx)
//     r20 = 2 (xz - wy)        r21 = 2 (yz + wx)        r22 = 1 - 2 (xx + yy)           (the sum or difference, then the doubling, then 1 - .)
//     a_ik = r_ik * S[k]       t_i = T[i]
//
// COMPOSE P o L of two such matrices:
//     a_ik = (p_i0 l_0k + p_i1 l_1k) + p_i2 l_2k          t_i = ((p_i0 lt_0 + p_i1 lt_1) + p_i2 lt_2) + pt_i
// world[j] = world[parent[j]] o local[j]; a ROOT's world is its local, bits and all (it is not multiplied by an identity).
// bone[j] = world[j] o inv_bind[j]; without inverse binds, the world's bits.
#pragma once
#include "trg_skin_math.h"

namespace trg {
namespace rig {

constexpr uint32_t kNoParent = 0xFFFFFFFFu;
constexpr uint32_t kMaxLevels = 64;   // TRG_RIG_MAX_LEVELS: the kernel is launched once per level

// ---- sampling ----
// the key pair of a clock: *ia == *ib (the first or the last key) when t is not strictly inside the track.  time(i) is float 0 of record i
TRG_PM_HD inline void key_pair(const float *keys12, uint32_t first, uint32_t last, float t, uint32_t *ia, uint32_t *ib) {
    if (t <= keys12[(size_t)first * 12]) { *ia = *ib = first; return; }
    if (t >= keys12[(size_t)last * 12]) { *ia = *ib = last; return; }
    uint32_t lo = first, hi = last;   // time[lo] <= t < time[hi] (a clock that is not a number keeps lo = first: nothing is read out of range)
#if defined(__clang__)
#pragma unroll 1
#endif
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (keys12[(size_t)mid * 12] <= t) lo = mid;
        else hi = mid;
    }
    *ia = lo; *ib = lo + 1u;
}
// the rotation between a and b (4 floats each) at u
TRG_PM_HD inline void nlerp(const float *a, const float *b, float u, float *out) {
    const float p0 = a[0] * b[0], p1 = a[1] * b[1], p2 = a[2] * b[2], p3 = a[3] * b[3];
    const float d = ((p0 + p1) + p2) + p3;
    float q[4];
    for (int k = 0; k < 4; ++k) {
        const float bk = d < 0.f ? -b[k] : b[k];
        const float diff = bk - a[k];
        const float step = u * diff;
        q[k] = a[k] + step;
    }
    const float xx = q[0] * q[0], yy = q[1] * q[1], zz = q[2] * q[2], ww = q[3] * q[3];
    const float len = sqrtf(((xx + yy) + zz) + ww);
    const bool ok = len > 0.f && isfinite(len);
    for (int k = 0; k < 4; ++k) out[k] = ok ? q[k] / len : a[k];
}
// T (3), R (4), S (3) of the records ka, kb (12 floats each) at t; same: ka is the key to take as it is
TRG_PM_HD inline void sample(const float *ka, const float *kb, bool same, float t, float *T, float *R, float *S) {
    if (same) {
        for (int k = 0; k < 3; ++k) { T[k] = ka[1 + k]; S[k] = ka[8 + k]; }
        for (int k = 0; k < 4; ++k) R[k] = ka[4 + k];
        return;
    }
    const float num = t - ka[0], den = kb[0] - ka[0];
    const float u = num / den;
    for (int k = 0; k < 3; ++k) {
        const float dt = kb[1 + k] - ka[1 + k], ds = kb[8 + k] - ka[8 + k];
        const float st = u * dt, ss = u * ds;
        T[k] = ka[1 + k] + st;
        S[k] = ka[8 + k] + ss;
    }
    nlerp(ka + 4, kb + 4, u, R);
}

// ---- matrices ----
TRG_PM_HD inline void local(const float *T, const float *R, const float *S, float *L) {
    const float x = R[0], y = R[1], z = R[2], w = R[3];
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    const float s0 = yy + zz, s1 = xx + zz, s2 = xx + yy;
    const float d0 = 2.f * s0, d1 = 2.f * s1, d2 = 2.f * s2;
    const float e01 = xy - wz, e02 = xz + wy, e10 = xy + wz, e12 = yz - wx, e20 = xz - wy, e21 = yz + wx;
    const float r[9] = { 1.f - d0, 2.f * e01, 2.f * e02, 2.f * e10, 1.f - d1, 2.f * e12, 2.f * e20, 2.f * e21, 1.f - d2 };
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 3; ++k) L[4 * i + k] = r[3 * i + k] * S[k];
        L[4 * i + 3] = T[i];
    }
}
TRG_PM_HD inline void compose(const float *P, const float *L, float *out) {
    for (int i = 0; i < 3; ++i) {
        const float *p = P + 4 * i;
        for (int k = 0; k < 3; ++k) {
            const float a = p[0] * L[k], b = p[1] * L[4 + k], c = p[2] * L[8 + k];
            out[4 * i + k] = (a + b) + c;
        }
        const float a = p[0] * L[3], b = p[1] * L[7], c = p[2] * L[11];
        out[4 * i + 3] = ((a + b) + c) + p[3];
    }
}
// joint j's local matrix at its clock
TRG_PM_HD inline void joint_local(const float *keys12, const uint32_t *kfirst, const uint32_t *clock_of, const float *clocks, uint32_t j, float *L) {
    const float t = clocks[clock_of[j]];
    uint32_t ia, ib;
    key_pair(keys12, kfirst[j], kfirst[j + 1] - 1u, t, &ia, &ib);
    float T[3], R[4], S[3];
    sample(keys12 + (size_t)ia * 12, keys12 + (size_t)ib * 12, ia == ib, t, T, R, S);
    local(T, R, S, L);
}

// ---- the checks of trg_rig_bind (host), in the order they are made; *joint and *key name the first offender ----
enum { kRigOk = 0, kRigCounts, kRigParent, kRigTableFirst, kRigTableOrder, kRigTableEnd, kRigTime, kRigTS, kRigQuat, kRigClock, kRigInvBind, kRigDepth };
inline int check(const uint32_t *parent, uint32_t n_joints, const uint32_t *kfirst, const float *keys12, uint32_t n_keys, const uint32_t *clock_of, uint32_t n_clocks,
                 const float *inv_bind12, uint32_t *joint, uint32_t *key) {
    *joint = *key = 0;
    if (n_joints == 0 || n_keys == 0 || n_clocks == 0) return kRigCounts;
    for (uint32_t j = 0; j < n_joints; ++j)
        if (parent[j] != kNoParent && parent[j] >= j) { *joint = j; return kRigParent; }
    if (kfirst[0] != 0u) return kRigTableFirst;
    for (uint32_t j = 0; j < n_joints; ++j)
        if (!(kfirst[j] < kfirst[j + 1])) { *joint = j; return kRigTableOrder; }
    if (kfirst[n_joints] != n_keys) { *joint = n_joints - 1u; return kRigTableEnd; }
    for (uint32_t j = 0; j < n_joints; ++j)
        for (uint32_t i = kfirst[j]; i < kfirst[j + 1]; ++i) {
            const float time = keys12[(size_t)i * 12];
            if (!isfinite(time) || (i > kfirst[j] && !(keys12[(size_t)(i - 1) * 12] < time))) { *joint = j; *key = i; return kRigTime; }
        }
    for (uint32_t j = 0; j < n_joints; ++j)
        for (uint32_t i = kfirst[j]; i < kfirst[j + 1]; ++i) {
            const float *k = keys12 + (size_t)i * 12;
            if (!(isfinite(k[1]) && isfinite(k[2]) && isfinite(k[3]) && isfinite(k[8]) && isfinite(k[9]) && isfinite(k[10]))) { *joint = j; *key = i; return kRigTS; }
        }
    for (uint32_t j = 0; j < n_joints; ++j)
        for (uint32_t i = kfirst[j]; i < kfirst[j + 1]; ++i) {
            const float *q = keys12 + (size_t)i * 12 + 4;
            const double len2 = (double)q[0] * q[0] + (double)q[1] * q[1] + (double)q[2] * q[2] + (double)q[3] * q[3];
            if (!(isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]) && isfinite(q[3]) && fabs(len2 - 1.0) <= 1e-3)) { *joint = j; *key = i; return kRigQuat; }
        }
    for (uint32_t j = 0; j < n_joints; ++j)
        if (clock_of[j] >= n_clocks) { *joint = j; return kRigClock; }
    for (size_t k = 0; inv_bind12 && k < (size_t)n_joints * 12; ++k)
        if (!isfinite(inv_bind12[k])) { *joint = (uint32_t)(k / 12); return kRigInvBind; }
    return kRigOk;
}

// ---- the level table: a counting sort of the joints by depth, ascending joint index within a level.  depth and order hold n_joints words,
//      level_first kMaxLevels + 1; level l is order[level_first[l]] .. order[level_first[l + 1] - 1].  Of parents that passed check.  A forest
//      deeper than kMaxLevels: kRigDepth, *joint the first joint that deep ----
inline int levels(const uint32_t *parent, uint32_t n_joints, uint32_t *depth, uint32_t *order, uint32_t *level_first, uint32_t *n_levels, uint32_t *joint) {
    *joint = 0; *n_levels = 0;
    for (uint32_t l = 0; l <= kMaxLevels; ++l) level_first[l] = 0;
    for (uint32_t j = 0; j < n_joints; ++j) {
        depth[j] = parent[j] == kNoParent ? 0u : depth[parent[j]] + 1u;
        if (depth[j] >= kMaxLevels) { *joint = j; return kRigDepth; }
        ++level_first[depth[j] + 1u];
        if (depth[j] + 1u > *n_levels) *n_levels = depth[j] + 1u;
    }
    for (uint32_t l = 0; l < kMaxLevels; ++l) level_first[l + 1] += level_first[l];
    uint32_t cursor[kMaxLevels];
    for (uint32_t l = 0; l < kMaxLevels; ++l) cursor[l] = level_first[l];
    for (uint32_t j = 0; j < n_joints; ++j) order[cursor[depth[j]]++] = j;
    return kRigOk;
}

// ---- the whole evaluation on the host, level by level through the table as the kernel's launches go: world and bones, n_joints x 12 floats ----
inline void evaluate(const uint32_t *parent, const uint32_t *kfirst, const float *keys12, const uint32_t *clock_of, const float *inv_bind12, const float *clocks,
                     const uint32_t *order, const uint32_t *level_first, uint32_t n_levels, float *world, float *bones) {
    for (uint32_t l = 0; l < n_levels; ++l)
        for (uint32_t k = level_first[l]; k < level_first[l + 1]; ++k) {
            const uint32_t j = order[k];
            float L[12];
            joint_local(keys12, kfirst, clock_of, clocks, j, L);
            float *W = world + (size_t)j * 12, *B = bones + (size_t)j * 12;
            if (parent[j] == kNoParent) { for (int e = 0; e < 12; ++e) W[e] = L[e]; }
            else compose(world + (size_t)parent[j] * 12, L, W);
            if (inv_bind12) compose(W, inv_bind12 + (size_t)j * 12, B);
            else for (int e = 0; e < 12; ++e) B[e] = W[e];
        }
}

}  // namespace rig
}  // namespace trg
