/* trg_pose.h -- pose a loaded scene on the device: refit from buffers that are already there, and per-object transforms.
 *
 * trg_refit_scene (trg_refit.h) takes host arrays and uploads them: 12 bytes per vertex, 12 + 36 per triangle, every call.  What moves in the
 * scenes this backend renders is mostly rigid or affine PER OBJECT -- 48 bytes of information, not 36 per vertex.  Two entry families, a unit of its
 * own beside the render path (include/trg.h names none of it):
 *
 *  trg_refit_scene_device   trg_refit_scene with the three buffers read where they are: device memory of the context's device, on the context's
 *                           stream, nothing copied.  Same checks, same refusals and texts, same trg_refit_info, same single wait.  A pointer
 *                           that hipPointerGetAttributes does not call device memory of that device (host memory, another device's) is
 *                           refused (TRG_ERR_INVALID) before anything is enqueued.  SIZES ARE THE CALLER'S RESPONSIBILITY: the buffers must hold
 *                           n_verts x 12, n_tris x 12 and n_tris x 36 bytes.  The call also refuses a buffer whose allocation, as
 *                           hipMemGetAddressRange reports it, is too small -- but that answer is the runtime's record of an allocation, not of
 *                           the caller's array (a tensor inside a caching allocator's 2 MiB block is vouched for to the end of the block, and
 *                           in a process with a history of allocations a buffer 4 bytes short has been seen to pass): best effort, no promise.
 *                           Whatever the buffers hold, indices are clamped and nothing is written before every check has passed.  A scene of
 *                           the LDS tier downloads the buffers and takes the REBUILD path.  The caller must not write the buffers until the
 *                           call returns.
 *
 *  trg_pose_*               bind: the REST geometry -- the arrays trg_load_scene was given -- and an object table; object j is triangles
 *                           [first[j], first[j + 1]), first[0] = 0, strictly ascending, first[n_objects] = n_tris (the loaded scene's).  A
 *                           vertex may be named by triangles of one object only; a vertex no triangle names belongs to none and never moves.
 *                           Checked on the host (indices, finite values, the table, shared vertices: TRG_ERR_INVALID names the first
 *                           offender).  The device keeps the rest positions and normals, the indices, the vertex-to-object and
 *                           triangle-to-object maps and posed copies: CURRENT and PREVIOUS, both the rest pose at first, and one to pose into.
 *                           Bind does not refit and does not touch the scene.
 *                           apply: n_objects x 12 floats, row-major [A | t] per object, finite (else TRG_ERR_INVALID, nothing enqueued).
 *                           48 bytes per object are uploaded, one streaming kernel poses every vertex (x' = A x + t) and every corner normal
 *                           (cofactor matrix of A, sign of det A, renormalised; a normal that cannot be renormalised keeps its rest value) into
 *                           the spare copy, and trg_refit_scene_device's path runs on it.  On success the copies rotate: current becomes
 *                           previous.  A refused refit (a collapsed quad, a box that is no parallelepiped any more: TRG_ERR_RANGE) leaves the
 *                           scene, the current and the previous pose exactly as they were.  With normals3 == NULL at bind normals are not
 *                           posed: the loaded ones stay.
 *                           A binding is stale after a trg_load_scene -- and, for a scene of the LDS tier, after a trg_refit_scene of the caller's
 *                           own, which rebuilds it --: every pose call then returns TRG_ERR_INVALID ("bind again").  This is detected by a
 *                           HEURISTIC, not a counter: the scene's memory, triangle count, layout (sizes and offsets of its sections) or
 *                           measured build time differs.  A reload that matches in all of them is not noticed -- then the rest geometry of the
 *                           old scene is posed into the new one's tree, whose checks still keep every read in bounds --: bind after every load.
 *                           (One prebuilt scene uploaded twice matches in all of them, build time included; it is the same scene.)
 *
 * The arithmetic, operation by operation, is toyraygun_amd/csrc/trg_pose_math.h.  Equal inputs give equal outputs: the copies of a shared corner stay
 * bitwise equal.  The identity gives values equal under == (a -0 becomes +0).
 *
 * Out of scope: per-vertex deformation (linear-blend skinning is include/trg_skin.h; the caller's own device buffers go through trg_refit_scene_device); changed
 * topology, colours or materials; the 8-wide experiments build.
 */
#ifndef TRG_POSE_H
#define TRG_POSE_H

#include "trg_refit.h"

#ifdef __cplusplus
extern "C" {
#endif

TRG_API int trg_refit_scene_device(trg_ctx *ctx, const void *positions3_dev, const void *normals3_dev, const void *indices_dev, uint32_t n_verts, uint32_t n_tris);

TRG_API int trg_pose_bind(trg_ctx *ctx, const float *positions3, const float *normals3, const uint32_t *indices, uint32_t n_verts, uint32_t n_tris,
                          const uint32_t *object_first_tri, uint32_t n_objects);
TRG_API int trg_pose_apply(trg_ctx *ctx, const float *xforms12);
/* the current pose, n_verts x 3 and (bound with normals) n_tris x 9 floats; waits */
TRG_API int trg_pose_read(trg_ctx *ctx, float *positions3_host, float *normals3_host);
/* the unit's device buffers: current positions / normals, indices, previous positions / normals (normals NULL when bound without).  Any out pointer
 * may be NULL.  They stay valid, and change roles, until the next apply, bind or release. */
TRG_API int trg_pose_buffers(trg_ctx *ctx, void **pos_dev, void **nrm_dev, void **idx_dev, void **prev_pos_dev, void **prev_nrm_dev);
/* frees the binding only (trg_refit_release and trg_destroy free it too) */
TRG_API int trg_pose_release(trg_ctx *ctx);
/* every context of the group binds / poses its own copy; the first failure is returned (trg_last_error of that context has the text) */
TRG_API int trg_group_pose_bind(trg_group *g, const float *positions3, const float *normals3, const uint32_t *indices, uint32_t n_verts, uint32_t n_tris,
                                const uint32_t *object_first_tri, uint32_t n_objects);
TRG_API int trg_group_pose_apply(trg_group *g, const float *xforms12);

#ifdef __cplusplus
}
#endif
#endif /* TRG_POSE_H */
