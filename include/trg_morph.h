/* trg_morph.h -- morph a loaded scene on the device: blend shapes (morph targets), in front of the skin.
 *
 * trg_skin_* (trg_skin.h) bends a mesh by bones.  A face, a muscle bulge, a corrective shape on a bent elbow are not bones: they are TARGETS, each a
 * list of per-vertex deltas, mixed by one weight each -- and every asset format applies them first and skins the result.  Per call the information
 * is 4 bytes per target (and 48 per bone); the targets, and optionally the skin's ids and weights, are bound once.  A unit of its own beside the
 * render path (include/trg.h names none of it), with trg_skin.h's semantics wherever they apply:
 *
 *  bind     the REST geometry -- the arrays trg_load_scene was given --, the targets, and optionally a skin.  Target k owns the entries
 *           [target_first[k], target_first[k + 1]); entry e names vertex entry_vertex[e] and carries the position delta entry_dpos3[3 e ..] and,
 *           with entry_dnrm3, a normal delta for EVERY corner whose index names that vertex.  The sparse form assets ship; a dense target is one
 *           with n_verts entries.  Checked on the host, in this order, the first offender named in trg_last_error (TRG_ERR_INVALID, nothing is
 *           written to the device): the geometry as trg_skin_bind checks it; n_targets >= 1; target_first[0] == 0, non-decreasing,
 *           target_first[n_targets] == n_entries (an EMPTY target is legal); every entry_vertex < n_verts and strictly ascending within its
 *           target (a vertex appears in a target at most once); every delta finite; entry_dnrm3 without normals3 is refused; bone_ids4,
 *           bone_weights4 and n_bones are given all three or none (NULL, NULL, 0), and if given pass trg_skin_bind's checks with its texts.
 *           The device keeps the rest positions and normals, the indices, the targets transposed into per-vertex records, and three posed copies:
 *           CURRENT, PREVIOUS and a spare, all the rest pose at first.  Bind does not refit and does not touch the scene.
 *  apply    n_targets weights, finite, of any sign and size -- nothing is clamped --, and n_bones x 12 floats exactly when the binding has bones
 *           (NULL otherwise); else TRG_ERR_INVALID, nothing enqueued.  Always from the REST geometry, never from the current pose.  One streaming
 *           kernel writes every vertex and every corner normal that can change into the spare copy, and trg_refit_scene_device's path runs on it.
 *           On success the copies rotate: current becomes previous.  A refused refit (TRG_ERR_RANGE: a quad or a box of the loaded tree that the
 *           morphed vertices no longer form) leaves the scene, the current and the previous pose and trg_refit_last bit for bit what they were.
 *           EVERY vertex is processed, also one that no triangle names.
 *  read / buffers / release / group   as trg_skin_read, trg_skin_buffers, trg_skin_release, trg_group_skin_*.
 *
 * A target whose weight is zero (either zero) is SKIPPED, not multiplied through: all-zero weights without bones give the rest pose back bit for
 * bit, and with bones what trg_skin_apply gives, bit for bit.  The arithmetic, operation by operation, is toyraygun_amd/csrc/trg_morph_math.h.
 * Equal inputs give equal outputs: the copies of a shared corner stay bitwise equal.
 *
 * A scene of the LDS tier takes the REBUILD path, as for poses and skins, and keeps its textures.  A binding is stale after a trg_load_scene --
 * and, for a scene of the LDS tier, after any rebuild this binding did not make --: every call then returns TRG_ERR_INVALID ("bind again"),
 * detected by the HEURISTIC of trg_pose.h: bind after every load.  A morph binding, a skin binding and a pose binding of one context are
 * independent: each keeps its own rest geometry and copies, and the last apply defines the scene.
 *
 * Out of scope: targets or weights that live on the device; tangents; more than one normal delta per vertex and target; compaction of the active
 * targets (with 50 dense targets of which 3 are active the kernel still reads all 50 records of every vertex); dual-quaternion skinning; changed
 * topology; the 8-wide experiments build, which refuses these calls.
 */
#ifndef TRG_MORPH_H
#define TRG_MORPH_H

#include "trg_refit.h"

#ifdef __cplusplus
extern "C" {
#endif

TRG_API int trg_morph_bind(trg_ctx *ctx, const float *positions3, const float *normals3, const uint32_t *indices, uint32_t n_verts, uint32_t n_tris,
                           uint32_t n_targets, const uint32_t *target_first, uint32_t n_entries, const uint32_t *entry_vertex, const float *entry_dpos3,
                           const float *entry_dnrm3, const uint32_t *bone_ids4, const float *bone_weights4, uint32_t n_bones);
TRG_API int trg_morph_apply(trg_ctx *ctx, const float *target_weights, const float *bones12);
/* the current pose, n_verts x 3 and (bound with normals) n_tris x 9 floats; waits */
TRG_API int trg_morph_read(trg_ctx *ctx, float *positions3_host, float *normals3_host);
/* the unit's device buffers: current positions / normals, indices, previous positions / normals (normals NULL when bound without).  Any out pointer
 * may be NULL.  They stay valid, and change roles, until the next apply, bind or release. */
TRG_API int trg_morph_buffers(trg_ctx *ctx, void **pos_dev, void **nrm_dev, void **idx_dev, void **prev_pos_dev, void **prev_nrm_dev);
/* frees the binding only (trg_refit_release and trg_destroy free it too) */
TRG_API int trg_morph_release(trg_ctx *ctx);
/* every context of the group binds / morphs its own copy; the first failure is returned (trg_last_error of that context has the text) */
TRG_API int trg_group_morph_bind(trg_group *g, const float *positions3, const float *normals3, const uint32_t *indices, uint32_t n_verts, uint32_t n_tris,
                                 uint32_t n_targets, const uint32_t *target_first, uint32_t n_entries, const uint32_t *entry_vertex, const float *entry_dpos3,
                                 const float *entry_dnrm3, const uint32_t *bone_ids4, const float *bone_weights4, uint32_t n_bones);
TRG_API int trg_group_morph_apply(trg_group *g, const float *target_weights, const float *bones12);

#ifdef __cplusplus
}
#endif
#endif /* TRG_MORPH_H */
