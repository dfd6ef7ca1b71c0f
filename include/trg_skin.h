/* trg_skin.h -- skin a loaded scene on the device: linear-blend skinning, four bones per vertex.
 *
 * trg_pose_* (trg_pose.h) moves whole objects by one matrix each.  A mesh that BENDS belongs to no single object: each vertex follows a weighted
 * blend of bone matrices.  The per-call information is again 48 bytes per bone; the per-vertex part -- four bone ids, four weights -- is bound once.
 * A unit of its own beside the render path (include/trg.h names none of it), with trg_pose.h's semantics wherever they apply:
 *
 *  bind     the REST geometry -- the arrays trg_load_scene was given --, and per vertex four bone ids (uint32) and four weights (float).  Checked on
 *           the host: indices in range, finite positions and normals, every id < n_bones (also the id of a zero weight), every weight finite and
 *           >= 0, |w0 + w1 + w2 + w3 - 1| <= 1e-4 with the sum formed in double.  TRG_ERR_INVALID names the first offending vertex in
 *           trg_last_error.  THE LIBRARY DOES NOT NORMALISE WEIGHTS: they are used as given.  The device keeps the rest positions and normals, the
 *           ids and weights, the indices and three posed copies: CURRENT, PREVIOUS and a spare, all the rest pose at first.  Bind does not refit
 *           and does not touch the scene.  With normals3 == NULL normals are not skinned: the loaded ones stay.
 *  apply    n_bones x 12 floats on the host, row-major [A | t] per bone, finite (else TRG_ERR_INVALID, nothing enqueued).  48 bytes per bone are
 *           uploaded, one streaming kernel writes every vertex and every corner normal of the spare copy, and trg_refit_scene_device's path runs on
 *           it.  On success the copies rotate: current becomes previous.  A refused refit (TRG_ERR_RANGE: a quad or a box of the loaded tree that
 *           the skinned vertices no longer form) leaves the scene, the current and the previous pose bit for bit what they were.
 *           EVERY vertex is skinned, also one that no triangle names -- unlike trg_pose_*, where such a vertex belongs to no object and never
 *           moves: here it has ids and weights of its own like any other.
 *           Corner c of triangle t is skinned with the blended matrix of vertex indices[3 t + c].
 *  read / buffers / release / group   as trg_pose_read, trg_pose_buffers, trg_pose_release, trg_group_pose_*.
 *
 * A scene of the LDS tier takes the REBUILD path, as for poses.  A binding is stale after a trg_load_scene -- and, for a scene of the LDS tier,
 * after any rebuild this binding did not make --: every call then returns TRG_ERR_INVALID ("bind again").  As in trg_pose.h this is detected by a
 * HEURISTIC, the same one (memory, triangle count, layout and measured build time of the scene): bind after every load.
 *
 * A skin binding and a pose binding of one context are independent: each keeps its own rest geometry and copies, neither reads the other's, and
 * the last apply defines the scene.  (In the LDS tier an apply of one rebuilds the scene, which makes the other stale as any rebuild does.)
 *
 * The arithmetic, operation by operation, is toyraygun_amd/csrc/trg_skin_math.h.  Equal inputs give equal outputs: the copies of a shared corner
 * stay bitwise equal.  A vertex with weights (1, 0, 0, 0) gets values equal under == to trg_pose_apply's with that bone as its object's matrix.
 *
 * Out of scope: dual-quaternion blending; more than four bones per vertex; bones that live on the device (trg_rig.h has them: a keyframed joint forest, or the caller's device memory); blend shapes (trg_morph.h has them, in front of this skin); changed topology; the
 * 8-wide experiments build, which refuses these calls.
 */
#ifndef TRG_SKIN_H
#define TRG_SKIN_H

#include "trg_refit.h"

#ifdef __cplusplus
extern "C" {
#endif

TRG_API int trg_skin_bind(trg_ctx *ctx, const float *positions3, const float *normals3, const uint32_t *indices, uint32_t n_verts, uint32_t n_tris,
                          const uint32_t *bone_ids4, const float *weights4, uint32_t n_bones);
TRG_API int trg_skin_apply(trg_ctx *ctx, const float *bones12);
/* the current pose, n_verts x 3 and (bound with normals) n_tris x 9 floats; waits */
TRG_API int trg_skin_read(trg_ctx *ctx, float *positions3_host, float *normals3_host);
/* the unit's device buffers: current positions / normals, indices, previous positions / normals (normals NULL when bound without).  Any out pointer
 * may be NULL.  They stay valid, and change roles, until the next apply, bind or release. */
TRG_API int trg_skin_buffers(trg_ctx *ctx, void **pos_dev, void **nrm_dev, void **idx_dev, void **prev_pos_dev, void **prev_nrm_dev);
/* frees the binding only (trg_refit_release and trg_destroy free it too) */
TRG_API int trg_skin_release(trg_ctx *ctx);
/* every context of the group binds / skins its own copy; the first failure is returned (trg_last_error of that context has the text) */
TRG_API int trg_group_skin_bind(trg_group *g, const float *positions3, const float *normals3, const uint32_t *indices, uint32_t n_verts, uint32_t n_tris,
                                const uint32_t *bone_ids4, const float *weights4, uint32_t n_bones);
TRG_API int trg_group_skin_apply(trg_group *g, const float *bones12);

#ifdef __cplusplus
}
#endif
#endif /* TRG_SKIN_H */
